#!/usr/bin/env python3
"""Hyper-parameter selection for the dose-response application (the loop of doseresponse/select_btf.py) on the device:
the simulated data and the gamma grid of examples/doseresponse_gamma_grid.py, one constrained gamma_grid fit per lam2,
each scored by DIC, WAIC and PSIS-LOO under the gamma-grid likelihood where its samples lie (gamma_grid_criteria /
gamma_grid_loo), and the candidates compared pairwise with criteria.compare.  select_btf.py computes the same DIC on the
host, one saved sample at a time; utils.gamma_grid_criteria(Ws, Vs, Y, likelihood) is that form, without a model."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from doseresponse_gamma_grid import gamma_grid, simulate                             # noqa: E402
from functionalmf_amd import criteria, utils                                         # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # noqa: E402  (was: functionalmf.factor)


def main(seed=42, lam2s=(1e-1, 1e-2), nburn=100, nsamples=100, n=30, m=20, t=9, r=6, k=3, nembeds=3, verbose=True):
    rs = np.random.RandomState(seed)
    obs, _ = simulate(rs, n, m, t, r, k)
    obs[rs.rand(*obs.shape) < 0.05] = np.nan
    likelihood = gamma_grid(obs[:, :, 0])
    Y = obs[:, :, 1:]
    C_zero = np.concatenate([np.eye(t), np.zeros((t, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(t - i - 2), [-1e-2]]) for i in range(t - 1)])
    C_one = np.concatenate([np.eye(t) * -1, np.full((t, 1), -1)], axis=1)
    C = np.concatenate([C_zero, C_one, C_mono], axis=0)
    W0, V0 = utils.tensor_nmf(np.clip(Y, 0, 1), nembeds, monotone=True)
    W0 *= min(1.0, 0.999 / np.einsum("nk,mtk->nmt", W0, V0).max())

    scores = {}
    for lam2 in lam2s:
        np.random.seed(seed)
        model = ConstrainedNonconjugateBayesianTensorFiltering(n, m, t, "gamma_grid", C, likelihood_param=likelihood, nembeds=nembeds,
                                                               tf_order=2, lam2_true=lam2, W_init=W0.copy(), V_init=V0.copy(),
                                                               rng="device", device_seed=seed)
        results = model.run_gibbs(Y, nburn=nburn, nsamples=nsamples, verbose=False)
        ic = model.gamma_grid_criteria()                   # the kept samples, read where they lie on the device
        loo = model.gamma_grid_loo()
        # the model-free form on the saved samples: the same numbers, bit for bit
        assert utils.gamma_grid_criteria(results["W"], results["V"], Y, likelihood)["dic"] == ic["dic"]
        scores[lam2] = (ic, loo)
        if verbose:
            print("lam2=%-6g DIC %.1f (p_dic %.1f)  WAIC %.1f (p_waic %.1f)  elpd_loo %.1f +- %.1f  curves with k-hat > %.2f: %d of %d"
                  % (lam2, ic["dic"], ic["p_dic"], ic["waic"], ic["p_waic"], loo["elpd_loo"], loo["se"], loo["good_k"], loo["n_bad"],
                     loo["n_curves"]))
    best = min(scores, key=lambda l: scores[l][0]["dic"])
    if verbose:
        print("selected by DIC: lam2=%g" % best)
        a, b = lam2s[0], lam2s[1]
        for name, idx in (("WAIC", 0), ("PSIS-LOO", 1)):
            cmp = criteria.compare(scores[a][idx], scores[b][idx])
            print("%s: elpd(lam2=%g) - elpd(lam2=%g) = %.1f +- %.1f over %d curves" % (name, a, b, cmp["elpd_diff"], cmp["se_diff"],
                                                                                     cmp["n_curves"]))
    return best, scores


if __name__ == "__main__":
    main()
