#!/usr/bin/env python3
"""The constrained Poisson model with EP-centred proposals, as the reference's applications run it on real data
(doseresponse/fit.py, politics/benchmark.py): a monotone non-negative factorisation (utils.tensor_nmf) as the start,
a Gaussian fit of the likelihood around it (utils.ep_from_mf, mode='multiplier', multiplier=3), then
ConstrainedNonconjugateBayesianTensorFiltering(..., ep_approx=(Mu_ep, Sigma_ep)): every GASS ellipse is centred on
that fit and the likelihood is divided by it, so the target is unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # was: functionalmf.factor
from functionalmf_amd.utils import ep_from_mf, posterior_summary, tensor_nmf


def main(seed=1, nburn=300, nsamples=200, nrows=40, ncols=30, ndepth=16, nembeds=3):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    W_true = rs.gamma(1, 1, size=(nrows, nembeds))
    V_true = np.cumsum(rs.gamma(1, 0.3, size=(ncols, ndepth, nembeds)) * (rs.rand(ncols, ndepth, 1) < 0.3), axis=1)[:, ::-1] + 0.2
    rate = np.einsum('nk,mtk->nmt', W_true, V_true)
    Y = rs.poisson(np.repeat(rate[..., None], 2, axis=-1)).astype(float)
    Y[rs.rand(*Y.shape) < 0.05] = np.nan

    Constraints = np.concatenate([np.eye(ndepth), np.zeros((ndepth, 1))], axis=1)               # positive means
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(ndepth - i - 2), [-1e-2]]) for i in range(ndepth - 1)])
    Constraints = np.concatenate([Constraints, C_mono], axis=0)                                  # decreasing in t

    W0, V0 = tensor_nmf(Y, nembeds, monotone=True)
    Mu_ep, Sigma_ep = ep_from_mf(Y, W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(nrows, ncols, ndepth, "poisson_identity", Constraints,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=0,
                                                           sigma2_init=1.0, lam2_init=0.1, W_init=W0, V_init=V0,
                                                           rng="device", device_seed=seed)
    results = model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
    mean, _ = posterior_summary(results['W'], results['V'], q=(5, 95))
    rel = float(np.mean(np.abs(mean - rate)) / np.mean(rate))
    print("rate: relative MAE %.3f; final log-likelihood %.1f" % (rel, model.log_likelihood(Y)))
    model.shutdown()
    return rel


if __name__ == "__main__":
    main()
