"""Time posterior_functionals against posterior_summary on the same device-collected samples (one run on the GPU).

S kept samples at C3 (512,256,64) and at the flu shape (50,1,370), K = 5: which=("auc",) and all seven functionals next to
model.posterior_summary(q=(5, 95)), which reads the same states and sorts T times as many values per curve.  Prints one
JSON line per case: host wall clock around calls that end in a device synchronise (downloads of the outputs included).

    python scripts/functionals_rate.py [--samples 1000] [--repeats 5] [--small] [--once]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import functionals  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def case(name, N, M, T, R, K, S, repeats, once):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    q = (5, 95)
    calls = [("posterior_summary", lambda: model.posterior_summary(q=q)),
             ("posterior_functionals auc", lambda: model.posterior_functionals(which=("auc",), q=q)),
             ("posterior_functionals all seven", lambda: model.posterior_functionals(which=functionals.NAMES, q=q, level=0.0))]
    if once:                               # under a profiler: one call each, no timing
        for _, fn in calls:
            fn()
        return
    for _, fn in calls:                    # warm-up: code objects, allocations
        fn()
    # alternate the three so that a drift of the shared host hits them alike
    ts = {what: [] for what, _ in calls}
    for _ in range(repeats):
        for what, fn in calls:
            t0 = time.perf_counter()
            fn()
            ts[what].append(time.perf_counter() - t0)
    t_sum = min(ts["posterior_summary"])
    for what, _ in calls:
        print(json.dumps(dict(case=name, what=what, seconds_min=min(ts[what]), seconds_median=float(np.median(ts[what])),
                              ratio_to_summary=min(ts[what]) / t_sum, shape=[N, M, T, R], nembeds=K, nsamples=S, repeats=repeats)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a (32,16,16) rehearsal instead of C3")
    ap.add_argument("--once", action="store_true", help="one call of each, untimed (for a kernel trace)")
    a = ap.parse_args()
    case("flu (50,1,370)", 50, 1, 370, 1, 5, a.samples, a.repeats, a.once)
    if a.small:
        case("small", 32, 16, 16, 1, 5, min(a.samples, 64), a.repeats, a.once)
    else:
        case("C3 (512,256,64)", 512, 256, 64, 1, 5, a.samples, a.repeats, a.once)


if __name__ == "__main__":
    main()
