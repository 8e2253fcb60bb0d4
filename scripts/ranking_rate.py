"""Time posterior_ranking against the host route and against posterior_functionals on the same device-collected samples
(one run on the GPU).

S kept samples at C3 (512,256,64) and at the flu shape (50,1,370), K = 5.  Three calls, alternated:
    ranking      model.posterior_ranking("auc", along="cols")                       (downloads of its (N,M) outputs included)
    host route   model.posterior_functionals(("auc",), pointwise=True), then numpy: a stable argsort per group and the
                 counts - what there was before posterior_ranking (its (S,N,M) download included)
    functionals  model.posterior_functionals(("auc",)) alone: the same sweep, reduced per curve
Prints one JSON line per call: host wall clock around calls that end in a device synchronise.  The script also checks
that the two routes return the same numbers.

    python scripts/ranking_rate.py [--samples 1000] [--repeats 5] [--small] [--once] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import ranking  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402

TOP = (1, 5)


def case(name, N, M, T, R, K, S, repeats, once, out):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    print("# %s: %d samples collected" % (name, S), file=sys.stderr, flush=True)

    def host_route():
        f = model.posterior_functionals(which=("auc",), q=None, pointwise=True)["auc"]["pointwise"]
        return ranking.summarize(ranking.ranks(f, "cols", "ascending"), TOP)

    calls = [("posterior_ranking auc cols", lambda: model.posterior_ranking("auc", along="cols", top=TOP)),
             ("host route: functionals pointwise + numpy argsort", host_route),
             ("posterior_functionals auc", lambda: model.posterior_functionals(which=("auc",)))]
    if once:                               # under a profiler: one call each, no timing
        for _, fn in calls:
            fn()
        return
    got, ref = calls[0][1](), calls[1][1]()         # warm-up: code objects, allocations; and the two routes agree
    calls[2][1]()
    same = bool(np.array_equal(got["expected_rank"], ref[0]) and np.array_equal(got["rank_var"], ref[1]) and
                np.array_equal(got["p_top"], ref[2]))
    # alternate the three so that a drift of the shared host hits them alike
    ts = {what: [] for what, _ in calls}
    for _ in range(repeats):
        for what, fn in calls:
            t0 = time.perf_counter()
            fn()
            ts[what].append(time.perf_counter() - t0)
    t_rank = min(ts[calls[0][0]])
    for what, _ in calls:
        line = json.dumps(dict(case=name, what=what, seconds_min=min(ts[what]), seconds_median=float(np.median(ts[what])),
                               ratio_to_ranking=min(ts[what]) / t_rank, routes_agree=same, shape=[N, M, T, R], nembeds=K, nsamples=S,
                               repeats=repeats))
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a (32,16,16) rehearsal instead of C3")
    ap.add_argument("--once", action="store_true", help="one call of each, untimed (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    case("flu (50,1,370)", 50, 1, 370, 1, 5, a.samples, a.repeats, a.once, a.out)
    if a.small:
        case("small", 32, 16, 16, 1, 5, min(a.samples, 64), a.repeats, a.once, a.out)
    else:
        case("C3 (512,256,64)", 512, 256, 64, 1, 5, a.samples, a.repeats, a.once, a.out)


if __name__ == "__main__":
    main()
