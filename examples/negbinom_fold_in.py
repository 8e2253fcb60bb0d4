#!/usr/bin/env python3
"""Fit a Negative-Binomial model to count series, then fold new weeks in without another burn-in.

Over-dispersed weekly counts for 40 regions and 3 series, three replicates each.  The model is fitted on the first T weeks;
then H more weeks arrive for half the regions.  negbin_fold_in_depth returns the curves at the new weeks for EVERY region,
with the sampled rate of every kept sample; the same call without data is the forecast.  Printed: the RMSE of the expected
counts R exp(w . v) at the regions that did not report, against the truth, for both - and for carrying the last fitted week
forward.  (Expected counts, not success probabilities: the rate and the level of the curves are only identified together.)
A new series (column) observed at some of the regions is folded in the same way by negbin_fold_in_cols(Y_cols, res).

    python examples/negbinom_fold_in.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils                                                   # noqa: E402
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering          # noqa: E402
from functionalmf_amd.utils import ilogit                                            # noqa: E402


def expected_counts(res, V):
    """Posterior median of R_s exp(w_i^s . v_jt^s) over the kept samples, (N,M,T): the draws of a fold-in are heavy-tailed
    (fresh horseshoe+ scales), and the exponential of a heavy tail has no useful mean."""
    R = np.asarray(res["R"], dtype=float).reshape(len(V), -1)[:, :1, None, None]      # (one shared rate per sample here)
    return np.median(R * np.exp(np.minimum(np.einsum("snk,smtk->snmt", res["W"], V), 50.0)), axis=0)


def main(N=40, M=3, T=48, H=6, K=3, nreps=3, seed=0, nburn=600, nthin=2, nsamples=150):
    rs = np.random.RandomState(seed)
    W = 0.8 * rs.normal(size=(N, K))
    weeks = np.arange(T + H)
    V = np.stack([np.stack([a * np.sin(2 * np.pi * (weeks / 52.0 + p)) for p, a in zip(rs.uniform(size=K), 0.5 + rs.uniform(size=K))], axis=1)
                  for _ in range(M + 1)])                        # (M + 1, T + H, K): one series more than is fitted (kept out)
    P = ilogit(np.einsum("nk,mtk->nmt", W, V))
    R_true = 4.0
    Y = rs.negative_binomial(R_true, 1 - P[..., None].repeat(nreps, -1)).astype(float)       # mean R p / (1 - p) = R exp(w . v)
    mean_true = R_true * P / (1 - P)

    np.random.seed(seed)
    # sigma2 and lam2 are held fixed.  With them sampled this chain lets the scale drift between W and V (only their product
    # is identified) and lam2 sink to its floor while the fitted local scales grow to make up for it; a fold-in draws FRESH
    # local scales of order one for the new penalty rows, which then cannot: it continues each sample's tail rigidly.
    model = NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_true=1.0, lam2_true=0.1, nmetropolis=10)
    res = model.run_gibbs(np.ascontiguousarray(Y[:, :M, :T]), nburn=nburn, nthin=nthin, nsamples=nsamples, verbose=False)
    print("sampled rate: mean %.2f (data simulated with %.1f)" % (float(np.mean(res["R"])), R_true))

    # ---- new weeks for half the regions
    reporting = rs.permutation(N)[:N // 2]
    hidden = np.setdiff1d(np.arange(N), reporting)
    Y_new = np.full((N, M, H, nreps), np.nan)
    Y_new[reporting] = Y[reporting, :M, T:]
    out = model.negbin_fold_in_depth(Y_new, res, transform="ilogit", q=(5, 95))       # the rate: res["R"], shared along the depths
    forecast = model.negbin_fold_in_depth(None, res, horizon=H, transform="ilogit", q=(5, 95))
    truth = mean_true[hidden, :M, T:]
    rmse = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    last = expected_counts(res, res["V"])[hidden, :, -1:]
    print("%d new weeks reported by %d of %d regions" % (H, len(reporting), N))
    print("RMSE of the expected counts at the other regions: folded in %.3f   forecast %.3f   last week carried forward %.3f"
          % (rmse(expected_counts(res, out["V"])[hidden]), rmse(expected_counts(res, forecast["V"])[hidden]), rmse(np.repeat(last, H, axis=2))))
    lo, hi = out["quantiles"][:, hidden]
    print("mean width of the 5-95 %% band of the success probabilities: folded in %.3f, forecast %.3f"
          % (float(np.mean(hi - lo)), float(np.mean(forecast["quantiles"][1, hidden] - forecast["quantiles"][0, hidden]))))
    # the extended posterior goes into the predictive with the sampled rate
    V_all = np.concatenate([res["V"], out["V"]], axis=2)
    pp = utils.posterior_predictive(res["W"], V_all, "negative_binomial", R=res["R"], seed=1)
    print("posterior predictive mean count, region %d, series 0, new weeks: %s" % (hidden[0], np.round(pp["mean"][hidden[0], 0, T:], 1).tolist()))

    return out, forecast


if __name__ == "__main__":
    main()
