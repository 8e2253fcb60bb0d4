#!/usr/bin/env python3
"""Negative-Binomial or Poisson?  Over-dispersed count curves fitted with both models on the GPU and compared on the same
data by their per-curve elpd: model.negbin_criteria / negbin_loo (the Negative-Binomial likelihood with its sampled rate)
against information_criteria / loo of a poisson_log fit, through criteria.compare.  Prints the table and the paired
difference; a positive elpd_diff favours the Negative-Binomial model.  No plotting."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import criteria                                                                            # noqa: E402
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering  # noqa: E402
from functionalmf_amd.utils import ilogit                                                                        # noqa: E402


def main(seed=1, nburn=600, nthin=2, nsamples=200):
    nrows, ncols, ndepth, nembeds, nreps = 24, 10, 16, 3, 3
    rs = np.random.RandomState(seed)
    W = 0.8 * rs.normal(size=(nrows, nembeds))
    V = 0.25 * np.cumsum(rs.normal(size=(ncols, ndepth, nembeds)), axis=1)
    P = ilogit(np.einsum("nk,mtk->nmt", W, V))
    R_true = 3.0                                               # variance = mean (1 + mean / R): well above Poisson's
    Y = rs.negative_binomial(R_true, 1 - P[..., None].repeat(nreps, -1)).astype(float)
    Y[:2, :2] = np.nan                                         # four curves without observations: left out by both

    np.random.seed(seed)
    nb = NegativeBinomialBayesianTensorFiltering(nrows, ncols, ndepth, nembeds=nembeds, tf_order=2, sigma2_init=0.5,
                                                 lam2_init=0.1, nmetropolis=10)
    nb_fit = nb.run_gibbs(Y, nburn=nburn, nthin=nthin, nsamples=nsamples, verbose=False)
    nb_ic, nb_loo = nb.negbin_criteria(nb_fit), nb.negbin_loo(nb_fit)

    np.random.seed(seed)
    po = NonconjugateBayesianTensorFiltering(nrows, ncols, ndepth, "poisson_log", nembeds=nembeds, tf_order=2,
                                             sigma2_init=0.5, lam2_init=0.1)
    po_fit = po.run_gibbs(Y, nburn=nburn, nthin=nthin, nsamples=nsamples, verbose=False)
    po_ic, po_loo = po.information_criteria(po_fit, data=Y), po.loo(po_fit, data=Y)

    print("%20s %12s %10s %12s %12s %8s" % ("model", "WAIC", "p_waic", "DIC", "elpd_loo", "bad k"))
    for name, ic, lo in (("negative binomial", nb_ic, nb_loo), ("poisson (log link)", po_ic, po_loo)):
        print("%20s %12.1f %10.1f %12.1f %12.1f %8d" % (name, ic["waic"], ic["p_waic"], ic["dic"], lo["elpd_loo"], lo["n_bad"]))
    out = {"waic": criteria.compare(nb_ic, po_ic), "loo": criteria.compare(nb_loo, po_loo),
           "R_hat": float(nb_fit["R"].mean()), "R_true": R_true}
    for k in ("waic", "loo"):
        print("elpd(NB) - elpd(Poisson) by %-4s: %.1f +- %.1f over %d curves" % (k, out[k]["elpd_diff"], out[k]["se_diff"], out[k]["n_curves"]))
    print("sampled rate: mean %.2f (data simulated with %.1f)" % (out["R_hat"], R_true))
    return out


if __name__ == "__main__":
    main(seed=int(sys.argv[1]) if len(sys.argv) > 1 else 1)
