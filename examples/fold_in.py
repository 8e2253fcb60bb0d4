"""Fold rows the chain never saw into a fitted posterior.

Fit a Gaussian model with the last rows left out, fold them in from a few observed columns, and print the RMSE of the
predicted curves on their unobserved columns against the noiseless truth - next to that of the prior mean (zero).

    python examples/fold_in.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main(N=200, M=12, T=30, K=3, nnew=10, seed=0):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    truth = np.einsum("nk,mtk->nmt", W, V)
    Y = truth + rs.normal(0, 0.5, size=truth.shape)

    np.random.seed(seed)
    model = GaussianBayesianTensorFiltering(N - nnew, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y[:N - nnew], nburn=300, nsamples=200, verbose=False)

    observed = np.arange(0, M, 3)                              # the new rows were measured on 4 of the 12 columns
    hidden = np.setdiff1d(np.arange(M), observed)
    Y_new = Y[N - nnew:].copy()
    Y_new[:, hidden] = np.nan
    out = model.fold_in_rows(Y_new, q=(5, 95))                 # from the samples on the device: no upload of V
    t = truth[N - nnew:][:, hidden]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    lo, hi = out["quantiles"][:, :, hidden]
    print("new rows %d, observed columns %s" % (nnew, observed.tolist()))
    print("RMSE on the unobserved columns: fold-in %.3f   prior mean (zero) %.3f" % (rmse(out["mean"][:, hidden]), rmse(np.zeros_like(t))))
    print("share of the truth inside the 5-95 %% band: %.2f" % float(np.mean((t >= lo) & (t <= hi))))
    # the draws go straight into the other posterior tools
    auc = utils.posterior_functionals(out["W"], res["V"], which=("auc",))["auc"]["mean"]
    print("posterior mean AUC of the first new row, per column:", np.round(auc[0], 2).tolist())


if __name__ == "__main__":
    main()
