"""PSIS-LOO on the GPU: two nembeds compared on leave-one-curve-out and on WAIC, the Pareto k-hat table, and one
leave-curve-out fitted curve against its data.

    python examples/loo.py
"""
import numpy as np

from functionalmf_amd import criteria
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

if __name__ == "__main__":
    rs = np.random.RandomState(0)
    N, M, T, K_true = 40, 12, 16, 3
    W = rs.normal(size=(N, K_true))
    V = np.cumsum(rs.normal(0, 0.3, size=(M, T, K_true)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.3, size=(N, M, T, 2))

    loo, waic = {}, {}
    for K in (1, 3):
        np.random.seed(1)
        model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=2)
        model.run_gibbs(Y, nburn=300, nsamples=300, verbose=False)
        loo[K] = model.loo(mean=(K == 3))
        waic[K] = model.information_criteria()
        print("nembeds %d: elpd_loo %.1f (se %.1f), p_loo %.1f, looic %.1f | elpd_waic %.1f" % (
            K, loo[K]["elpd_loo"], loo[K]["se"], loo[K]["p_loo"], loo[K]["looic"], waic[K]["elpd_waic"]))

    for name, scores in (("LOO", loo), ("WAIC", waic)):
        c = criteria.compare(scores[3], scores[1])
        print("%s: nembeds 3 over 1: elpd_diff %.1f, se_diff %.1f (%d curves)" % (name, c["elpd_diff"], c["se_diff"], c["n_curves"]))

    # the k-hat table: which curves the estimate can be believed for
    k = loo[3]["curves"]["pareto_k"]
    edges = [-np.inf, 0.5, loo[3]["good_k"], 1.0, np.inf]
    labels = ["good", "ok", "bad", "very bad"]
    print("Pareto k-hat, nembeds 3 (good_k = %.3f):" % loo[3]["good_k"])
    for lo, hi, lab in zip(edges[:-1], edges[1:], labels):
        n = int(((k > lo) & (k <= hi)).sum())
        print("  (%5.2f, %5.2f]  %-8s %5d  %5.1f%%" % (lo, hi, lab, n, 100.0 * n / k.size))

    # what the model predicts for the curve with the largest k-hat, had it not seen it
    i, j = np.unravel_index(np.nanargmax(np.where(np.isfinite(k), k, np.nan)), k.shape)
    print("curve (%d,%d), k-hat %.2f: data mean / leave-curve-out fit" % (i, j, k[i, j]))
    for t in range(T):
        print("  t=%2d  %8.3f  %8.3f" % (t, Y[i, j, t].mean(), loo[3]["mean"][i, j, t]))
