"""Which drug is best for a cell line, and with what probability: the rank of every column within its row by the area under
the sampled curve, summarised over the kept samples on the GPU.  The mean AUC of posterior_functionals names a winner per
row; posterior_ranking says in what share of the joint posterior samples that column really is the lowest.

    python examples/ranking.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.curve_functionals import simulate  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main():
    dose, truth, Y = simulate()
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(*Y.shape[:3], nembeds=3, rng="device")
    model.run_gibbs(Y, nburn=500, nthin=1, nsamples=500, verbose=False)
    auc = model.posterior_functionals(which=("auc",), x=dose)["auc"]["mean"]
    best = auc.argmin(axis=1)                                           # the column with the lowest mean AUC of every row
    rows = np.arange(len(best))
    pairs = np.stack([rows, best, rows, (best + 1) % auc.shape[1]], axis=1)
    out = model.posterior_ranking("auc", along="cols", order="ascending", top=(1, 2), x=dose, pairs=pairs)
    p1 = out["p_top"][0]
    print("lowest mean AUC = most probable rank 1 in %d of %d rows" % ((p1.argmax(axis=1) == best).sum(), len(best)))
    for i in (0, 5, 11):
        j = best[i]
        print("row %2d: column %d has the lowest mean AUC (%.3f); it is the lowest in %.0f %% of the samples, among the two lowest "
              "in %.0f %%; expected rank %.2f (sd %.2f); P(AUC below column %d's) = %.2f"
              % (i, j, auc[i, j], 100 * p1[i, j], 100 * out["p_top"][1, i, j], out["expected_rank"][i, j],
                 np.sqrt(out["rank_var"][i, j]), pairs[i, 3], out["prob_less"][i]))
    ic50 = model.posterior_ranking("crossing", along="cols", transform=None, x=dose, level=0.5, top=(1,))
    print("row 0, P(column reaches 0.5 at the lowest dose):", np.round(ic50["p_top"][0, 0], 2),
          "(a curve that never reaches it in a sample ranks last there)")


if __name__ == "__main__":
    main()
