"""Fold new weeks into a fitted count series under positivity, without another burn-in, and compare with the constrained forecast.

Weekly Poisson counts: 30 regions, 4 series, smooth positive curves.  Fit the constrained Poisson model (identity link, every
curve w_i . v_j(t) >= 0) on the first T weeks, then H more weeks arrive for half the regions.  slice_fold_in_depth returns the
curves at the new weeks for EVERY region; the same call without data is the constrained forecast - the prior continuation
truncated to the feasible set.  A constrained model must be told its constraints on the extended grid of T + H weeks: here
positivity of every new week.  Printed: the RMSE at the regions that did not report, against the true rates, for both - and
for carrying the last fitted week forward - and that every returned draw is feasible.

    python examples/slice_fold_in_depth.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import slice_fold_in_depth as sd  # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering  # noqa: E402


def positivity(ndepth):
    return np.concatenate([np.eye(ndepth), np.zeros((ndepth, 1))], axis=1)


def main(N=30, M=4, T=40, H=6, K=3, seed=0, sweeps=None):
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    weeks = np.arange(T + H)
    V = np.stack([4.0 + 3.0 * np.sin(2 * np.pi * (weeks / 52.0 + p)) for p in rs.uniform(size=M * K)], axis=1).reshape(T + H, M, K)
    V = np.ascontiguousarray(V.transpose(1, 0, 2))               # (M,T+H,K), positive
    truth = np.einsum("nk,mtk->nmt", W, V)                       # (N,M,T+H)
    Y = rs.poisson(truth).astype(float)

    np.random.seed(seed)
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", positivity(T), nembeds=K, tf_order=2,
                                                           W_init=np.full((N, K), 1.0), V_init=np.full((M, T, K), Y.mean() / K),
                                                           rng="device", device_seed=seed + 1)
    res = model.run_gibbs(np.ascontiguousarray(Y[:, :, :T]), nburn=300, nsamples=100, verbose=False)

    reporting = rs.permutation(N)[:N // 2]                      # half the regions report the new weeks
    hidden = np.setdiff1d(np.arange(N), reporting)
    Y_new = np.full((N, M, H), np.nan)                          # (N,M,H)
    Y_new[reporting] = Y[reporting, :, T:]
    Cons = positivity(T + H)                                    # the constraints on the extended grid: never stretched silently
    out = model.slice_fold_in_depth(Y_new, results=res, Constraints=Cons, sweeps=sweeps, q=(5, 95))
    forecast = model.slice_fold_in_depth(None, horizon=H, results=res, Constraints=Cons, sweeps=sweeps, q=(5, 95))
    t = truth[hidden, :, T:]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    carry = np.repeat((np.einsum("snk,smk->nm", res["W"], res["V"][:, :, -1]) / res["W"].shape[0])[hidden, :, None], H, axis=2)
    print("%d new weeks reported by %d of %d regions" % (H, len(reporting), N))
    print("RMSE at the other regions: folded in %.3f   constrained forecast %.3f   last week carried forward %.3f"
          % (rmse(out["mean"][hidden]), rmse(forecast["mean"][hidden]), rmse(carry)))
    for name, o in (("folded in", out), ("forecast", forecast)):
        lo, hi = o["quantiles"][:, hidden]
        rates = np.einsum("snk,smhk->snmh", res["W"], o["V"])
        print("%-9s  share of the truth inside the 5-95 %% band: %.2f   mean band width %.2f   every draw positive: %s   "
              "proposals per sweep %.2f   sweeps at the cap %d"
              % (name, float(np.mean((t >= lo) & (t <= hi))), float(np.mean(hi - lo)), bool(np.all(rates >= 0)),
                 float(o["rounds"].mean()) / float(sweeps or sd.DEFAULT_SWEEPS), int(o["unfinished"].sum())))
    model.shutdown()


if __name__ == "__main__":
    main()
