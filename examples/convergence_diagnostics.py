#!/usr/bin/env python3
"""Convergence diagnostics on the GPU: four rng="device" Gaussian chains with different seeds on synthetic data, then
split R-hat, bulk / tail ESS and the MCSE of every cell of W V' (diagnostics.convergence), and of the scalar parameters.
Prints the summary.  No plotting.  At this shape 1000 burn-in sweeps are not enough and the diagnostics say so (max R-hat
about 2.4, bulk ESS about 5); rerun with main(nburn=5000) to see the chains agree."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import diagnostics  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main(seed=0, nburn=1000, nsamples=500, nchains=4):
    nrows, ncols, ndepth, nreps, K = 40, 12, 20, 2, 3
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(nrows, K))
    V = 0.3 * np.cumsum(rs.normal(size=(ncols, ndepth, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.3, size=(nrows, ncols, ndepth, nreps))
    models = []
    for c in range(nchains):
        np.random.seed(seed + 1 + c)
        model = GaussianBayesianTensorFiltering(nrows, ncols, ndepth, nembeds=K, tf_order=2, sigma2_init=0.5,
                                                lam2_init=0.1, nu2_init=1, rng="device", device_seed=seed + 1 + c)
        model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
        models.append(model)
    d = models[0].convergence_diagnostics(*models[1:])          # the samples stay on the GPU
    print("%d chains x %d draws, %d cells" % (d["nchains"], d["ndraws"], d["rhat"].size))
    print("max R-hat %.4f (%d cells above %.2f), min bulk ESS %.0f, min tail ESS %.0f, median MCSE %.2e"
          % (d["max_rhat"], d["n_rhat_above"], diagnostics.RHAT_THRESHOLD, d["min_ess_bulk"], d["min_ess_tail"],
             np.nanmedian(d["mcse_mean"])))
    for name, s in d["scalars"].items():
        print("%8s: R-hat %.4f  bulk ESS %.0f  tail ESS %.0f" % (name, s["rhat"], s["ess_bulk"], s["ess_tail"]))


if __name__ == "__main__":
    main()
