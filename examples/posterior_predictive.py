"""Posterior predictive checks on simulated data, the flu benchmark's procedure (flutrends/benchmark.py): hold out blocks
of depth, fit, 95 % predictive band, in- and out-of-sample coverage, RMSE / MAE - for the Gaussian and the Poisson model.

    python examples/posterior_predictive.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import GaussianBayesianTensorFiltering, NonconjugateBayesianTensorFiltering  # noqa: E402


def simulate(kind, N=30, M=4, T=40, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W, V = rs.normal(0, 0.6, size=(N, K)), 0.25 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    eta = np.einsum("nk,mtk->nmt", W, V)
    Y = eta + rs.normal(0, 0.3, size=eta.shape) if kind == "gaussian" else rs.poisson(np.exp(eta)).astype(float)
    held = np.zeros(eta.shape, dtype=bool)
    for i in range(N):                                   # every row loses one block of depth in one column
        t0 = rs.randint(0, T - 8)
        held[i, rs.randint(M), t0:t0 + 8] = True
    return np.where(held, np.nan, Y), np.where(held, Y, np.nan)


def report(name, pp):
    print("  %-13s coverage %.3f of nominal %.2f over %d observations; RMSE %.3f  MAE %.3f (means over the samples)"
          % (name, pp["coverage"], pp["nominal"], int(pp["nobs"].sum()), pp["rmse"].mean(), pp["mae"].mean()))


def main():
    for kind in ("gaussian", "poisson"):
        Y_in, Y_out = simulate(kind)
        np.random.seed(1)
        if kind == "gaussian":
            model = GaussianBayesianTensorFiltering(*Y_in.shape, nembeds=3, rng="device")
            res = model.run_gibbs(Y_in, nburn=300, nthin=1, nsamples=300, verbose=False)
            res = None                                   # the samples are still on the device: nothing is uploaded
        else:
            model = NonconjugateBayesianTensorFiltering(*Y_in.shape, loglikelihood="poisson_log", nembeds=3)
            res = model.run_gibbs(Y_in, nburn=300, nthin=1, nsamples=300, verbose=False)
        print(kind)
        report("in-sample", model.posterior_predictive(results=res, draws_per_sample=4, seed=7))
        report("out-of-sample", model.posterior_predictive(results=res, data=Y_out, draws_per_sample=4, seed=7))


if __name__ == "__main__":
    main()
