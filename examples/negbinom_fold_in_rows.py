#!/usr/bin/env python3
"""Fit a Negative-Binomial model with one rate per row, then fold rows in that the chain never saw.

Over-dispersed weekly counts for 44 regions and 3 series, two replicates each; every region has its own rate
(rdims=(1, 2), the layout of the reference's own example).  The model is fitted on 40 regions.  The other four arrive
afterwards with half their cells observed: negbin_fold_in_rows returns their embeddings per kept sample and - since a new
region has no kept rate - SAMPLES one rate for each, by the model's own Metropolis step inside the short chain of every
(kept sample, new region).  Printed: the sampled rates against the ones the data were simulated with, and the coverage of
the hidden cells by the posterior predictive band, which reads the new rows' W and R.

    python examples/negbinom_fold_in_rows.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils                                                   # noqa: E402
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering          # noqa: E402
from functionalmf_amd.utils import ilogit                                            # noqa: E402


def main(N=40, Rnew=4, M=3, T=48, K=3, nreps=2, seed=0, nburn=600, nthin=2, nsamples=150):
    rs = np.random.RandomState(seed)
    W = 0.8 * rs.normal(size=(N + Rnew, K))
    weeks = np.arange(T)
    V = np.stack([np.stack([a * np.sin(2 * np.pi * (weeks / 52.0 + p)) for p, a in zip(rs.uniform(size=K), 0.5 + rs.uniform(size=K))], axis=1)
                  for _ in range(M)])                                                  # (M,T,K)
    P = ilogit(np.einsum("nk,mtk->nmt", W, V))
    R_true = rs.uniform(2.0, 8.0, size=N + Rnew)                                       # one rate per region
    Y = rs.negative_binomial(R_true[:, None, None, None], 1 - P[..., None].repeat(nreps, -1)).astype(float)

    np.random.seed(seed)
    # (sigma2 and lam2 held fixed: see examples/negbinom_fold_in.py)
    model = NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_true=1.0, lam2_true=0.1, nmetropolis=10,
                                                    rdims=(1, 2))
    res = model.run_gibbs(np.ascontiguousarray(Y[:N]), nburn=nburn, nthin=nthin, nsamples=nsamples, verbose=False)
    S = len(res["W"])
    res.setdefault("sigma2", np.ones(S))
    print("fitted rates %s: posterior mean of the first four %s (simulated with %s)"
          % (np.shape(res["R"]), np.round(np.mean(res["R"], axis=0).reshape(-1)[:4], 2).tolist(), np.round(R_true[:4], 2).tolist()))

    # ---- four new regions, half their cells observed
    Y_new = Y[N:].copy()
    hidden = rs.uniform(size=Y_new.shape[:3]) < 0.5
    Y_new[hidden] = np.nan
    out = model.negbin_fold_in_rows(Y_new, res, transform="ilogit", q=(5, 95), seed=1)
    print("new regions: sampled rate, posterior mean %s  5-95 %% %s / %s   (simulated with %s)"
          % (np.round(out["R"].mean(axis=0), 2).tolist(), np.round(np.percentile(out["R"], 5, axis=0), 2).tolist(),
             np.round(np.percentile(out["R"], 95, axis=0), 2).tolist(), np.round(R_true[N:], 2).tolist()))
    print("accepted share of the Metropolis steps: %.2f" % float(out["accept"].mean()))
    rmse = float(np.sqrt(np.mean((out["mean"] - P[N:]) ** 2)))
    print("RMSE of the success probabilities of the new regions against the truth: %.3f" % rmse)
    # the new rows go into the predictive with their own sampled rates; scored on the cells that were hidden
    held = np.where(hidden[..., None], Y[N:], np.nan)
    pp = utils.posterior_predictive(out["W"], res["V"], "negative_binomial", data=held, q=(5, 95), R=out["R"][:, :, None, None], seed=2)
    print("hidden cells of the new regions: coverage of the 5-95 %% predictive band %.3f (nominal %.2f), RMSE %.2f"
          % (pp["coverage"], pp["nominal"], float(np.nanmean(pp["rmse"]))))
    return out, pp


if __name__ == "__main__":
    main()
