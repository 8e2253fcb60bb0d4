"""Posterior predictive checks of two Poisson fits: one of Poisson counts, one of over-dispersed (Negative-Binomial) counts
with the same means.  Cell by cell both look alike; the chi-square of whole replicated curves tells them apart.

    python examples/posterior_checks.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import checks  # noqa: E402
from functionalmf_amd.factor import NonconjugateBayesianTensorFiltering  # noqa: E402


def simulate(N=30, M=4, T=40, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W, V = rs.normal(0, 0.6, size=(N, K)), 0.25 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    lam = np.exp(np.einsum("nk,mtk->nmt", W, V))
    return {"Poisson counts": rs.poisson(lam).astype(float),
            "over-dispersed counts (Negative-Binomial, r = 1)": rs.poisson(rs.gamma(1.0, lam)).astype(float)}


def main():
    for name, Y in simulate().items():
        np.random.seed(1)
        model = NonconjugateBayesianTensorFiltering(*Y.shape, loglikelihood="poisson_log", nembeds=3)
        res = model.run_gibbs(Y, nburn=1000, nthin=1, nsamples=300, verbose=False)
        pc = model.posterior_checks(results=res, seed=7)
        print("a Poisson fit of %s" % name)
        for which in pc["which"]:
            o, c = pc["overall"][which], pc[which]
            two = checks.two_sided(c["p_ge"], c["p_gt"])
            print("  %-6s overall: T_obs %10.3f  T_rep %10.3f  P(T_rep >= T_obs) = %.3f;   curves with two-sided p < 0.05: %3d of %d"
                  % (which, np.mean(o["T_obs"]), np.mean(o["T_rep"]), o["p_ge"], int(np.sum(two < 0.05)), int(np.sum(~np.isnan(two)))))
        flagged = pc["overall"]["chisq"]["p_ge"] < 0.01
        print("  -> %s\n" % ("FLAGGED by the chi-square check: the data is more dispersed than the model's replicates" if flagged
                            else "not flagged by the chi-square check"))


if __name__ == "__main__":
    main()
