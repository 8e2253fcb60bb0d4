#!/usr/bin/env python3
"""The dose-response application with binary row features end to end (doseresponse/fit.py:40-50, :86, :102-145): the
start (W0, V0, U0) from bounded_tensor_nmf(Y, K, monotone=True, max_entry=0.999, row_features=X), then a constrained
gamma-grid chain in which every row update of W carries the Bernoulli side likelihood of the features under
0 <= W U' <= 1, and every feature embedding u_f is resampled after each sweep - all on the GPU.  Prints the feature
fit mean |X - W U'| of the start and of the posterior mean.  The simulation and the likelihood are those of
examples/doseresponse_gamma_grid.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doseresponse_gamma_grid import gamma_grid, simulate                              # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # noqa: E402
from functionalmf_amd.utils import bounded_tensor_nmf, ep_from_mf                     # noqa: E402


def main(seed=42, nburn=100, nsamples=100, n=40, m=30, t=9, r=6, k=3, nembeds=3, nfeatures=8, verbose=True):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    obs, effects = simulate(rs, n, m, t, r, k)
    obs[rs.rand(*obs.shape) < 0.05] = np.nan
    likelihood = gamma_grid(obs[:, :, 0])
    Y = obs[:, :, 1:]
    # binary biomarkers: thresholds of random projections of the rows' mean response, 10 % unknown
    resp = np.nanmean(Y, axis=(2, 3))
    X = (resp @ rs.normal(size=(m, nfeatures)) > np.median(resp @ rs.normal(size=(m, nfeatures)), axis=0)).astype(float)
    X[rs.rand(*X.shape) < 0.1] = np.nan

    C_zero = np.concatenate([np.eye(t), np.zeros((t, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(t - i - 2), [-1e-2]]) for i in range(t - 1)])
    C_one = np.concatenate([np.eye(t) * -1, np.full((t, 1), -1)], axis=1)
    C = np.concatenate([C_zero, C_one, C_mono], axis=0)

    W0, V0, U0 = bounded_tensor_nmf(np.clip(Y, 0, 1), nembeds, max_entry=0.999, row_features=X, monotone=True)
    top = float((W0 @ U0.T).max())
    if top > 0.999:                    # the chain needs 0 <= W U' <= 1 from the start (non-negative factors: only the top)
        U0 = U0 * (0.999 / top)
    Mu_ep, Sigma_ep = ep_from_mf(Y, W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(n, m, t, "gamma_grid", C, likelihood_param=likelihood,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=2,
                                                           W_init=W0, V_init=V0, rng="device", device_seed=seed,
                                                           row_features=X, feature_embeddings=U0, sample_features=True)
    results = model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
    P = np.einsum("snk,sfk->snf", results["W"], results["U"])
    fit0 = float(np.nanmean(np.abs(X - W0 @ U0.T)))
    fit1 = float(np.nanmean(np.abs(X - P.mean(axis=0))))
    if verbose:
        print("U samples %s; W U' of the chain in [%.3f, %.3f]" % (results["U"].shape, P.min(), P.max()))
        print("feature fit mean |X - W U'|: start %.3f, posterior mean %.3f" % (fit0, fit1))
    return results, (fit0, fit1)


if __name__ == "__main__":
    main()
