"""Curve functionals of a dose-response fit on simulated data: the area under every curve and its IC50 (the dose at which
the curve falls through 0.5) with 90 % bands, and the posterior probability that a curve is monotone - read off the
samples on the GPU, where doseresponse/feature_importance.py forms the (S,N,M,T) tensor on the host.

    python examples/curve_functionals.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import functionals  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def simulate(N=24, M=5, T=9, K=3, seed=0):
    """Monotone decreasing curves in (0, 1] of rank K: every row mixes the K basis curves of a column with convex weights."""
    rs = np.random.RandomState(seed)
    W = rs.gamma(1.0, 1.0, size=(N, K))
    W /= W.sum(axis=1, keepdims=True)
    dose = np.linspace(0.0, 1.0, T)
    steep = rs.uniform(0.3, 4.0, size=(M, 1, K))
    V = 1.0 / (1.0 + (dose[None, :, None] * steep) ** 2)                # (M, T, K): each falls from 1 with the dose
    truth = np.einsum("nk,mtk->nmt", W, V)
    Y = truth[..., None] + rs.normal(0, 0.05, size=truth.shape + (3,))
    return dose, truth, Y


def main():
    dose, truth, Y = simulate()
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(*Y.shape[:3], nembeds=3, rng="device")
    model.run_gibbs(Y, nburn=500, nthin=1, nsamples=500, verbose=False)
    # rise = the sum of the upward steps of a sampled curve: 0 (up to rounding) exactly when the sample is non-increasing
    out = model.posterior_functionals(which=("auc", "crossing", "rise"), q=(5, 50, 95), x=dose, level=0.5, exceed=1e-12)
    true = functionals.curve_functionals(truth, dose, level=0.5)
    auc, ic50 = out["auc"], out["crossing"]
    inside = (auc["quantiles"][0] <= true["auc"]) & (true["auc"] <= auc["quantiles"][2])
    print("AUC: mean abs error %.4f; the 90 %% band holds the truth for %d of %d curves"
          % (np.abs(auc["mean"] - true["auc"]).mean(), inside.sum(), inside.size))
    for i, j in [(0, 0), (5, 2), (11, 4)]:
        lo, med, hi = ic50["quantiles"][:, i, j]
        print("curve (%2d,%d): AUC %.3f [%.3f, %.3f] (true %.3f)   IC50 %.3f [%.3f, %.3f] (true %.3f; reached in %.0f %% of "
              "samples)   P(monotone) %.2f" % (i, j, auc["mean"][i, j], auc["quantiles"][0, i, j], auc["quantiles"][2, i, j],
                                               true["auc"][i, j], med, lo, hi, true["crossing"][i, j],
                                               100 * ic50["defined"][i, j], 1.0 - out["rise"]["prob_above"][i, j]))
    print("nan in an IC50 band: the percentile lies among the samples whose curve never falls to 0.5 inside the dose range")


if __name__ == "__main__":
    main()
