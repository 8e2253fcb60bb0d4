"""Monotone projection of an unconstrained posterior: a Gaussian fit of decreasing dose-response curves on simulated data
has no monotonicity constraint in its sampler, so few of its sampled curves are monotone.  posterior_monotone projects every
kept sample with factor_pav on the GPU (what doseresponse/fit.py:365-374 does on the host, sample by sample) and returns the
bands of the projected curves; in_place=True then makes every other analysis call read the projected posterior - the
btf_mono route of doseresponse/select_btf.py.

    python examples/monotone_posterior.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def simulate(N=24, M=5, T=9, K=3, seed=0, noise=0.08):
    """Monotone decreasing curves in (0, 1] of rank K, observed three times with noise."""
    rs = np.random.RandomState(seed)
    W = rs.gamma(1.0, 1.0, size=(N, K))
    W /= W.sum(axis=1, keepdims=True)
    dose = np.linspace(0.0, 1.0, T)
    steep = rs.uniform(0.3, 4.0, size=(M, 1, K))
    V = 1.0 / (1.0 + (dose[None, :, None] * steep) ** 2)
    truth = np.einsum("nk,mtk->nmt", W, V)
    return truth, truth[..., None] + rs.normal(0, noise, size=truth.shape + (3,))


def main(verbose=True, nburn=300, nsamples=300, **sim):
    truth, Y = simulate(**sim)
    T = truth.shape[2]
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(*Y.shape[:3], nembeds=3, rng="device")
    model.run_gibbs(Y, nburn=nburn, nthin=1, nsamples=nsamples, verbose=False)

    def p_monotone():                                  # rise = the sum of a sampled curve's upward steps
        return 1.0 - model.posterior_functionals(which=("rise",), q=None, exceed=1e-12)["rise"]["prob_above"]

    mean0, band0 = model.posterior_summary(q=(5, 95))
    pm0, ic0 = p_monotone(), model.information_criteria()
    out = model.posterior_monotone(q=(5, 95), in_place=True)          # from here on the collected samples ARE the projection
    mean1, band1 = out["mean"], out["quantiles"]
    pm1, ic1 = p_monotone(), model.information_criteria()
    rows = dict(p_monotone=(float(pm0.mean()), float(pm1.mean())), waic=(ic0["waic"], ic1["waic"]), dic=(ic0["dic"], ic1["dic"]),
                rmse=(float(np.sqrt(((mean0 - truth) ** 2).mean())), float(np.sqrt(((mean1 - truth) ** 2).mean()))),
                band_width=(float((band0[1] - band0[0]).mean()), float((band1[1] - band1[0]).mean())),
                band_upward_steps=(int((np.diff(band0, axis=3) > 0).sum()), int((np.diff(band1, axis=3) > 0).sum())),
                pools_mean=float(out["pools"].mean()), changed=out["changed"])
    if verbose:
        print("%d samples; a column block of %d depths keeps %.1f pools on average; share of samples that needed a merge, per "
              "column: %s" % (out["nsamples"], T, rows["pools_mean"], np.round(out["changed"], 2)))
        print("%-34s %12s %12s" % ("", "sampled", "projected"))
        for key, label, fmt in (("p_monotone", "P(curve is monotone), mean", "%12.3f"), ("rmse", "RMSE of the mean curve", "%12.4f"),
                                ("band_width", "mean width of the 90 % band", "%12.4f"),
                                ("band_upward_steps", "upward steps in the band curves", "%12d"), ("waic", "WAIC", "%12.1f"),
                                ("dic", "DIC", "%12.1f")):
            print("%-34s" % label + fmt % rows[key][0] + fmt % rows[key][1])
    return out, rows


if __name__ == "__main__":
    main()
