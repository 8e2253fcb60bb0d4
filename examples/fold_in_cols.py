"""Fold a column the chain never saw into a fitted posterior.

Fit a Gaussian model with the last column left out, fold it in from the 30 % of the rows it was measured on, and print the
RMSE of the predicted curves on the other rows against the noiseless truth - next to that of predicting zero.

    python examples/fold_in_cols.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main(N=200, M=12, T=30, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    truth = np.einsum("nk,mtk->nmt", W, V)
    Y = truth + rs.normal(0, 0.5, size=truth.shape)

    np.random.seed(seed)
    model = GaussianBayesianTensorFiltering(N, M - 1, T, nembeds=K, rng="device")
    res = model.run_gibbs(np.ascontiguousarray(Y[:, :M - 1]), nburn=300, nsamples=200, verbose=False)

    observed = rs.permutation(N)[:(3 * N) // 10]               # the new drug was tested on 30 % of the cell lines
    hidden = np.setdiff1d(np.arange(N), observed)
    Y_new = np.full((1, N, T), np.nan)                         # (C,N,T): one new column
    Y_new[0, observed] = Y[observed, M - 1]
    out = model.fold_in_cols(Y_new, q=(5, 95))                 # from the samples on the device: no upload of W
    t = truth[hidden, M - 1]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    lo, hi = out["quantiles"][:, hidden, 0]
    print("new column observed on %d of %d rows" % (len(observed), N))
    print("RMSE on the unobserved rows: fold-in %.3f   predicting zero %.3f" % (rmse(out["mean"][hidden, 0]), rmse(np.zeros_like(t))))
    print("share of the truth inside the 5-95 %% band: %.2f" % float(np.mean((t >= lo) & (t <= hi))))
    # the draws go straight into the other posterior tools
    auc = utils.posterior_functionals(res["W"], out["V"], which=("auc",))["auc"]["mean"]
    print("posterior mean AUC of the new column, first five rows:", np.round(auc[:5, 0], 2).tolist())


if __name__ == "__main__":
    main()
