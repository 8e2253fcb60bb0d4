#!/usr/bin/env python3
"""The dose-response application (doseresponse/fit.py) on the device: cell counts simulated as doseresponse/sim.py does,
an empirical-Bayes gamma grid over the initial population means (built with numpy here; the reference's
estimate_likelihood fits it from a pandas frame), the constraints of fit.py:58-61 (every curve in [0, 1] and
monotone), a monotone non-negative factorisation as the start, EP-centred proposals (ep_from_mf, multiplier 3), then
ConstrainedNonconjugateBayesianTensorFiltering(..., "gamma_grid", likelihood_param=...) and the posterior mean curves."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # was: functionalmf.factor
from functionalmf_amd.likelihoods import GammaGridLikelihood                         # was: empirical_bayes
from functionalmf_amd.utils import ep_from_mf, posterior_summary, tensor_nmf


def ilogit(x):
    return 1.0 / (1.0 + np.exp(-x))


def simulate(rs, n, m, t, r, k):
    """doseresponse/sim.py:33-55: embeddings, effects ilogit(3 - W V'), gamma cell counts per (cell line, drug, dose)
    around a population mean near 1, scaled by the effect; the first dose level is the control."""
    W = rs.gamma(3, 1, size=(n, k))
    V = np.cumsum((rs.random_sample(size=(m, t, 1)) <= np.linspace(0.05, 0.5, t)[None, :, None]) * rs.gamma(1, 0.15, size=(m, t, k)),
                  axis=1)
    effects = ilogit(-(W[:, None, None] * V[None]).sum(axis=-1) + 3)
    means = rs.normal(1, 0.1, size=(n, m, t + 1, 1))
    scales = np.exp(rs.normal(-7, 1, size=means.shape))
    obs = rs.gamma(means / scales, scales, size=(n, m, t + 1, r))
    obs[:, :, 1:] *= effects[..., None]
    return obs, effects


def gamma_grid(controls, nbins=20):
    """A grid of population means over the range of the controls, weights from their histogram, and the variance of
    the controls about their mean (the shape of estimate_likelihood's result, without its regression)."""
    c = controls[~np.isnan(controls)]
    edges = np.linspace(c.min(), c.max(), nbins + 1)
    counts, _ = np.histogram(c, bins=edges)
    probs = (counts + 1e-3) / (counts + 1e-3).sum()
    return GammaGridLikelihood((edges[1:] + edges[:-1]) / 2, probs, float(np.var(c)))


def main(seed=42, nburn=200, nsamples=200, n=40, m=30, t=9, r=6, k=3, nembeds=3, verbose=True):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    obs, effects = simulate(rs, n, m, t, r, k)
    obs[rs.rand(*obs.shape) < 0.05] = np.nan
    likelihood = gamma_grid(obs[:, :, 0])
    Y = obs[:, :, 1:]

    C_zero = np.concatenate([np.eye(t), np.zeros((t, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(t - i - 2), [-1e-2]]) for i in range(t - 1)])
    C_one = np.concatenate([np.eye(t) * -1, np.full((t, 1), -1)], axis=1)
    C = np.concatenate([C_zero, C_one, C_mono], axis=0)

    # fit.py:154 passes max_entry=0.999 (not supported by tensor_nmf yet): rescale W instead
    W0, V0 = tensor_nmf(np.clip(Y, 0, 1), nembeds, monotone=True)
    W0 *= min(1.0, 0.999 / np.einsum("nk,mtk->nmt", W0, V0).max())
    Mu_ep, Sigma_ep = ep_from_mf(Y, W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(n, m, t, "gamma_grid", C, likelihood_param=likelihood,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=2,
                                                           W_init=W0, V_init=V0, rng="device", device_seed=seed)
    results = model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
    mean, _ = posterior_summary(results['W'], results['V'], q=(5, 95))
    mae = float(np.mean(np.abs(mean - effects)))
    monotone = bool(np.all(np.diff(mean, axis=-1) <= 1e-2 + 1e-9))
    if verbose:
        print("posterior mean curves in [%.3f, %.3f], monotone: %s; MAE against the true effects %.3f; log-likelihood %.1f"
              % (mean.min(), mean.max(), monotone, mae, model.log_likelihood(Y)))
    return mean, effects


if __name__ == "__main__":
    main()
