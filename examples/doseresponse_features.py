#!/usr/bin/env python3
"""The start of the dose-response application's chains (doseresponse/fit.py:86,154): a monotone non-negative
factorisation with every curve bounded by max_entry=0.999 and binary row features (biomarkers per cell line) as side
information, bounded_tensor_nmf(Y, K, monotone=True, max_entry=0.999, row_features=X).  The start lies inside the [0, 1]
and monotone constraints of fit.py:58-61 as it is - no clipping or rescaling - and a short constrained gamma-grid chain
runs from it.  The simulation and the likelihood are those of examples/doseresponse_gamma_grid.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doseresponse_gamma_grid import gamma_grid, simulate                              # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # noqa: E402
from functionalmf_amd.utils import bounded_tensor_nmf, ep_from_mf, posterior_summary  # noqa: E402


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

    W0, V0, R0, info = bounded_tensor_nmf(np.clip(Y, 0, 1), nembeds, max_entry=0.999, row_features=X, monotone=True,
                                          return_info=True)
    Mu0 = np.einsum("nk,mtk->nmt", W0, V0)
    assert Mu0.min() >= -1e-9 and Mu0.max() <= 1.0, (Mu0.min(), Mu0.max())        # fit.py:161-163
    assert np.all(np.diff(Mu0, axis=-1) <= 1e-9)
    Mu_ep, Sigma_ep = ep_from_mf(Y, W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(n, m, t, "gamma_grid", C, likelihood_param=likelihood,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=2,
                                                           W_init=W0, V_init=V0, rng="device", device_seed=seed)
    results = model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
    mean, _ = posterior_summary(results['W'], results['V'], q=(5, 95))
    if verbose:
        print("start: %d ALS steps, %s systems projected per step, curves in [%.3f, %.3f]; feature fit |X - W R'| %.3f"
              % (info["steps"], list(info["projected"]), Mu0.min(), Mu0.max(), float(np.nanmean(np.abs(X - W0 @ R0.T)))))
        print("posterior mean curves in [%.3f, %.3f]; MAE against the true effects %.3f; log-likelihood %.1f"
              % (mean.min(), mean.max(), float(np.mean(np.abs(mean - effects))), model.log_likelihood(Y)))
    return mean, effects, (W0, V0, R0)


if __name__ == "__main__":
    main()
