"""Simultaneous credible bands of a Gaussian fit on simulated data: the pointwise 95 % band of one curve next to the two
bands that hold the WHOLE curve with 95 %, and the share of kept curves that stay inside the pointwise band - read off the
samples on the GPU, where the host route forms the (S,N,M,T) tensor and loops.

    python examples/simultaneous_bands.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def simulate(N=24, M=5, T=32, K=3, seed=0):
    """Smooth curves of rank K over T depths, observed three times with noise."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    truth = np.einsum("nk,mtk->nmt", W, V)
    return truth, truth[..., None] + rs.normal(0, 0.5, size=truth.shape + (3,))


def main():
    truth, Y = simulate()
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(*Y.shape[:3], nembeds=3, rng="device")
    model.run_gibbs(Y, nburn=500, nthin=1, nsamples=1000, verbose=False)
    mean, (lo, hi) = model.posterior_summary(q=(2.5, 97.5))
    sup = model.posterior_bands(method="supt", level=95, truth=truth)
    rk = model.posterior_bands(method="rank", level=95, truth=truth)
    i, j = 5, 2
    print("curve (%d,%d): pointwise 95 %% band, sup-t band, rank band, truth" % (i, j))
    for t in range(0, Y.shape[2], 4):
        print("  t=%2d  [%6.3f, %6.3f]   [%6.3f, %6.3f]   [%6.3f, %6.3f]   %6.3f"
              % (t, lo[i, j, t], hi[i, j, t], sup["lower"][i, j, t], sup["upper"][i, j, t], rk["lower"][i, j, t],
                 rk["upper"][i, j, t], truth[i, j, t]))
    print("share of the %d kept curves wholly inside their band, curve (%d,%d): pointwise %.3f, sup-t %.3f, rank %.3f"
          % (rk["nsamples"], i, j, rk["pointwise_inside"][i, j], sup["inside"][i, j], rk["inside"][i, j]))
    print("over all curves: pointwise %.3f .. %.3f (mean %.3f); sup-t and rank at least %.3f"
          % (rk["pointwise_inside"].min(), rk["pointwise_inside"].max(), rk["pointwise_inside"].mean(),
             min(sup["inside"].min(), rk["inside"].min())))
    width = lambda b: float((b["upper"] - b["lower"]).mean())
    print("mean width: pointwise %.3f, sup-t %.3f (crit %.2f sd on average), rank %.3f (k = %d .. %d of k_pointwise = %d)"
          % (float((hi - lo).mean()), width(sup), sup["crit"].mean(), width(rk), rk["k"].min(), rk["k"].max(), rk["k_pointwise"]))
    from functionalmf_amd import bands
    print("true curves wholly inside: pointwise %.3f, sup-t %.3f, rank %.3f"
          % (bands.coverage(lo, hi, truth)[1], sup["coverage"], rk["coverage"]))


if __name__ == "__main__":
    main()
