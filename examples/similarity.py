"""Which cell lines respond alike: the distance between the fitted surfaces of every two rows, summarised over the kept
samples on the GPU, the three nearest neighbours of a few rows with their probabilities, and a 2-D map of the rows by
multidimensional scaling of the posterior-mean distances.  The scatter of the embeddings themselves
(doseresponse/plot_embeddings.py) depends on a K x K map that differs from sample to sample; these distances do not.

    python examples/similarity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.curve_functionals import simulate  # noqa: E402
from functionalmf_amd import similarity  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def main():
    dose, truth, Y = simulate()
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(*Y.shape[:3], nembeds=3, rng="device")
    model.run_gibbs(Y, nburn=500, nthin=1, nsamples=500, verbose=False)
    out = model.posterior_similarity(along="rows", metric="rms", q=(5, 95), nearest=(1, 3))
    E = out["mean"].shape[0]
    print("%d rows over %d cells each, %d samples; rms distance between fitted surfaces" % (E, out["ncells"], out["nsamples"]))
    for i in (0, 5, 11):
        order = np.argsort(out["expected_rank"][i], kind="stable")[:3]
        print("row %2d: nearest " % i + "; ".join(
            "row %d (d = %.3f [%.3f, %.3f], nearest in %.0f %% of the samples, among the three nearest in %.0f %%)"
            % (f, out["mean"][i, f], out["quantiles"][0, i, f], out["quantiles"][1, i, f], 100 * out["p_nearest"][0, i, f],
               100 * out["p_nearest"][1, i, f]) for f in order))
    X, share = similarity.embed(out, dims=2)
    print("multidimensional scaling of the posterior-mean squared distances: two axes carry %.1f %% of the trace" % (100 * share))
    for i in range(min(E, 8)):
        print("row %2d: (%7.3f, %7.3f)" % (i, X[i, 0], X[i, 1]))
    cols = model.posterior_similarity(along="cols", metric="cosine", nearest=(1,))
    j = int(np.argmax(np.where(np.eye(len(cols["mean"]), dtype=bool), -1.0, cols["p_nearest"][0]).max(axis=1)))
    f = int(np.argmax(np.where(np.arange(len(cols["mean"])) == j, -1.0, cols["p_nearest"][0][j])))
    print("columns, cosine metric: column %d's nearest neighbour is column %d in %.0f %% of the samples (d = %.3f)"
          % (j, f, 100 * cols["p_nearest"][0, j, f], cols["mean"][j, f]))


if __name__ == "__main__":
    main()
