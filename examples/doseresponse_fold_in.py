#!/usr/bin/env python3
"""A new cell line in the dose-response application: the chain runs on all cell lines but five, then the five are folded
into the fitted posterior on the GPU - once from a handful of tested drugs and their biomarkers
(model.slice_fold_in_rows(Y_new, row_features=X_new)), once from the biomarkers alone (Y_new=None: the case the reference
leaves as commented-out code, doseresponse/fit.py:90-91).  Prints the error of the predicted curves on the drugs nobody
tested against the true effects, beside predicting the average fitted cell line (the start of every fold-in chain).  The
simulation, the likelihood and the model are those of examples/doseresponse_row_features.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doseresponse_gamma_grid import gamma_grid, simulate                              # noqa: E402
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering   # noqa: E402
from functionalmf_amd.utils import bounded_tensor_nmf, ep_from_mf                     # noqa: E402


def main(seed=42, nburn=100, nsamples=100, n=45, m=30, t=9, r=6, k=3, nembeds=3, nfeatures=8, nnew=5, ntested=6, verbose=True):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    obs, effects = simulate(rs, n, m, t, r, k)
    obs[rs.rand(*obs.shape) < 0.05] = np.nan
    likelihood = gamma_grid(obs[:, :, 0])
    Y = obs[:, :, 1:]
    resp = np.nanmean(Y, axis=(2, 3))
    proj = rs.normal(size=(m, nfeatures))
    X = (resp @ proj > np.median(resp @ proj, axis=0)).astype(float)             # binary biomarkers of every cell line
    fit, new = slice(0, n - nnew), slice(n - nnew, n)

    C_zero = np.concatenate([np.eye(t), np.zeros((t, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(t - i - 2), [-1e-2]]) for i in range(t - 1)])
    C_one = np.concatenate([np.eye(t) * -1, np.full((t, 1), -1)], axis=1)
    C = np.concatenate([C_zero, C_one, C_mono], axis=0)

    W0, V0, U0 = bounded_tensor_nmf(np.clip(Y[fit], 0, 1), nembeds, max_entry=0.999, row_features=X[fit], monotone=True)
    top = float((W0 @ U0.T).max())
    if top > 0.999:
        U0 = U0 * (0.999 / top)
    Mu_ep, Sigma_ep = ep_from_mf(Y[fit], W0, V0, mode='multiplier', multiplier=3)
    model = ConstrainedNonconjugateBayesianTensorFiltering(n - nnew, m, t, "gamma_grid", C, likelihood_param=likelihood,
                                                           ep_approx=(Mu_ep, Sigma_ep), nembeds=nembeds, tf_order=2,
                                                           W_init=W0, V_init=V0, rng="device", device_seed=seed,
                                                           row_features=X[fit], feature_embeddings=U0, sample_features=True)
    results = model.run_gibbs(Y[fit], nburn=nburn, nsamples=nsamples, verbose=False)

    # the new cell lines: `ntested` of the m drugs tested, all biomarkers known
    tested = rs.choice(m, size=ntested, replace=False)
    hidden = np.setdiff1d(np.arange(m), tested)
    Y_new = np.full((nnew,) + Y.shape[1:], np.nan)
    Y_new[:, tested] = Y[new][:, tested]
    both = model.slice_fold_in_rows(Y_new, results=results, row_features=X[new], seed=1)
    feats = model.slice_fold_in_rows(None, results=results, row_features=X[new], seed=1)
    start = np.einsum("srk,smtk->rmt", both["W_start"], results["V"]) / nsamples
    truth = effects[new][:, hidden]
    mae = lambda curves: float(np.mean(np.abs(curves[:, hidden] - truth)))
    out = {"tested drugs and biomarkers": mae(both["mean"]), "biomarkers alone": mae(feats["mean"]), "the average cell line": mae(start)}
    if verbose:
        print("fold-in of %d cell lines over %d kept samples: %.1f likelihood evaluations per chain, %d sweeps at the cap"
              % (nnew, nsamples, both["rounds"].mean(), int(both["unfinished"].sum())))
        for name, v in out.items():
            print("MAE on the %d untested drugs, predicted from %s: %.3f" % (len(hidden), name, v))
    return both, feats, out


if __name__ == "__main__":
    main()
