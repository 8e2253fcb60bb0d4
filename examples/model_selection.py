#!/usr/bin/env python3
"""Model selection on the GPU: synthetic Gaussian data with K = 3 latent factors, fitted with nembeds in {1, 2, 3, 5};
WAIC and DIC of each fit from the per-curve log-likelihood over the kept samples (model.information_criteria), plus
the held-out log predictive density of the examples' 3x3 block of curves.  Prints the table; lower WAIC / DIC is
better, higher held-out lppd is better.  No plotting."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import GaussianBayesianTensorFiltering   # noqa: E402


def main(seed=0, nburn=500, nsamples=200):
    nrows, ncols, ndepth, nreps, K_true = 40, 12, 20, 2, 3
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(nrows, K_true))
    V = 0.3 * np.cumsum(rs.normal(size=(ncols, ndepth, K_true)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.3, size=(nrows, ncols, ndepth, nreps))
    train = Y.copy()
    train[:3, :3] = np.nan                                     # hold out nine curves
    held = np.full_like(Y, np.nan)
    held[:3, :3] = Y[:3, :3]

    print("%8s %12s %10s %12s %10s %14s" % ("nembeds", "WAIC", "p_waic", "DIC", "p_dic", "held-out lppd"))
    for K in (1, 2, 3, 5):
        np.random.seed(seed + 1)
        model = GaussianBayesianTensorFiltering(nrows, ncols, ndepth, nembeds=K, tf_order=2, sigma2_init=0.5,
                                                lam2_init=0.1, nu2_init=1, rng="device", device_seed=seed)
        results = model.run_gibbs(train, nburn=nburn, nsamples=nsamples, verbose=False)
        ic = model.information_criteria()                      # the samples still on the GPU: no upload
        out = model.information_criteria(results, data=held)   # the held-out curves under the same samples
        print("%8d %12.1f %10.1f %12.1f %10.1f %14.1f" % (K, ic["waic"], ic["p_waic"], ic["dic"], ic["p_dic"], out["lppd"]))


if __name__ == "__main__":
    main()
