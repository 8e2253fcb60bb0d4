"""Fold new weeks into a fitted series without another burn-in, and compare with the model's forecast.

A flu-like series: 50 regions, one column, smooth seasonal curves.  Fit a Gaussian model on the first T weeks, then H more
weeks arrive for half the regions.  fold_in_depth returns the curves at the new weeks for EVERY region; the same call without
data is the forecast.  Printed: the RMSE at the regions that did not report, against the noiseless truth, for both - and for
carrying the last fitted week forward.

    python examples/fold_in_depth.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main(N=50, T=60, H=8, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    weeks = np.arange(T + H)
    V = np.stack([np.sin(2 * np.pi * (weeks / 52.0 + p)) * a for p, a in zip(rs.uniform(size=K), 1 + rs.uniform(size=K))], axis=1)[None]
    truth = np.einsum("nk,mtk->nmt", W, V)                      # (N,1,T+H)
    Y = truth + rs.normal(0, 0.5, size=truth.shape)

    np.random.seed(seed)
    model = GaussianBayesianTensorFiltering(N, 1, T, nembeds=K, rng="device")
    res = model.run_gibbs(np.ascontiguousarray(Y[:, :, :T]), nburn=500, nsamples=200, verbose=False)

    reporting = rs.permutation(N)[:N // 2]                     # half the regions report the new weeks
    hidden = np.setdiff1d(np.arange(N), reporting)
    Y_new = np.full((N, 1, H), np.nan)                         # (N,M,H)
    Y_new[reporting] = Y[reporting, :, T:]
    out = model.fold_in_depth(Y_new, q=(5, 95))                # from the samples on the device: only Y_new is uploaded
    forecast = model.fold_in_depth(None, horizon=H, q=(5, 95))  # no data: the model's forecast (honest, weak, heavy-tailed)
    t = truth[hidden, :, T:]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    carry = np.repeat(model.posterior_summary()[0][hidden, :, -1:], H, axis=2)
    print("%d new weeks reported by %d of %d regions" % (H, len(reporting), N))
    print("RMSE at the other regions: folded in %.3f   forecast %.3f   last week carried forward %.3f"
          % (rmse(out["mean"][hidden]), rmse(forecast["mean"][hidden]), rmse(carry)))
    for name, o in (("folded in", out), ("forecast", forecast)):
        lo, hi = o["quantiles"][:, hidden]
        print("%-9s  share of the truth inside the 5-95 %% band: %.2f   mean band width %.2f"
              % (name, float(np.mean((t >= lo) & (t <= hi))), float(np.mean(hi - lo))))
    # the extended posterior goes straight into the other posterior tools
    V_all = np.concatenate([res["V"], out["V"]], axis=2)       # (S,1,T+H,K)
    peak = utils.posterior_functionals(res["W"], V_all, which=("max",))["max"]["mean"]
    print("posterior mean peak of the extended curves, first five regions:", np.round(peak[:5, 0], 2).tolist())


if __name__ == "__main__":
    main()
