#!/usr/bin/env python3
"""A new drug in the dose-response application: the chain runs on all drugs but three, then the three are folded into
the fitted posterior on the GPU from a handful of the fitted cell lines (model.slice_fold_in_cols(Y_new)).  Prints the error
of the predicted curves on the cell lines nobody tested the new drugs on against the true effects, beside predicting the
average fitted drug (the start of every fold-in chain).  The simulation, the likelihood and the constraints are those of
examples/doseresponse_gamma_grid.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doseresponse_gamma_grid import gamma_grid, simulate                              # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # noqa: E402
from functionalmf_amd.slice_fold_in_cols import DEFAULT_SWEEPS                        # noqa: E402
from functionalmf_amd.utils import bounded_tensor_nmf, ep_from_mf                     # noqa: E402


def main(seed=42, nburn=100, nsamples=100, n=45, m=30, t=9, r=6, k=3, nembeds=3, nnew=3, ntested=12, sweeps=None, verbose=True):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    obs, effects = simulate(rs, n, m, t, r, k)
    obs[rs.rand(*obs.shape) < 0.05] = np.nan
    likelihood = gamma_grid(obs[:, :, 0])
    Y = obs[:, :, 1:]
    fit, new = slice(0, m - nnew), slice(m - nnew, m)

    C_zero = np.concatenate([np.eye(t), np.zeros((t, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(t - i - 2), [-1e-2]]) for i in range(t - 1)])
    C_one = np.concatenate([np.eye(t) * -1, np.full((t, 1), -1)], axis=1)
    C = np.concatenate([C_zero, C_one, C_mono], axis=0)

    Y_fit = np.ascontiguousarray(Y[:, fit])
    W0, V0 = bounded_tensor_nmf(np.clip(Y_fit, 0, 1), nembeds, max_entry=0.999, monotone=True)[:2]
    Mu_ep, Sigma_ep = ep_from_mf(Y_fit, W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(n, m - nnew, t, "gamma_grid", C, likelihood_param=likelihood,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=2,
                                                           W_init=W0, V_init=V0, rng="device", device_seed=seed)
    results = model.run_gibbs(Y_fit, nburn=nburn, nsamples=nsamples, verbose=False)

    # the new drugs: tested on `ntested` of the n cell lines
    tested = rs.choice(n, size=ntested, replace=False)
    hidden = np.setdiff1d(np.arange(n), tested)
    Y_new = np.full((nnew, n) + Y.shape[2:], np.nan)
    Y_new[:, tested] = Y[:, new].transpose(1, 0, 2, 3)[:, tested]
    out = model.slice_fold_in_cols(Y_new, results=results, seed=1, sweeps=sweeps)
    start = np.einsum("snk,sctk->nct", results["W"], out["V_start"]) / nsamples
    truth = effects[:, new][hidden]
    mae = lambda curves: float(np.mean(np.abs(curves[hidden] - truth)))
    err = {"the tested cell lines": mae(out["mean"]), "the average fitted drug": mae(start)}
    if verbose:
        print("fold-in of %d drugs over %d kept samples: %.1f likelihood evaluations per sweep, %d sweeps at the cap"
              % (nnew, nsamples, out["rounds"].mean() / (sweeps or DEFAULT_SWEEPS), int(out["unfinished"].sum())))
        for name, v in err.items():
            print("MAE on the %d untested cell lines, predicted from %s: %.3f" % (len(hidden), name, v))
    return out, err


if __name__ == "__main__":
    main()
