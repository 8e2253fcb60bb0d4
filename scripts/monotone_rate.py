"""Time posterior_monotone against the route that existed before it and against posterior_summary alone, on the same
uploaded samples (one run on the GPU).

S samples, with rs = RandomState(seed): Ws = rs.gamma(1, 1, (S,N,K)) and
Vs = 0.2 * rs.gamma(1, 1, (S,M,T,K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, noise, (S,M,T,K)), at noise 0.05 (few merges)
and 0.3 (many): the cost of a projection depends on its merges.  Shapes: C3 (512,256,64) K = 5, dose-response (1024,256,9)
K = 5, flu (50,1,370) K = 10.  Per shape and noise, alternated, host wall clock with all transfers:
    (a)  utils.posterior_monotone(Ws, Vs, q=(5, 95))               projected samples, pools, mean and percentile curves
    (a') utils.posterior_monotone(Ws, Vs, q=None)                  projected samples and pools, no summary
    (b') utils.factor_pav(Ws[s], Vs[s]) for every s                what a user could do before: S uploads, launches, downloads
    (b)  (b') and utils.posterior_summary(Ws, V', q=(5, 95))       ... and the summary of the result, uploaded again
    (c)  utils.posterior_summary(Ws, Vs, q=(5, 95))                the summary alone, on the unprojected samples
The outputs of (a) and (b) are compared bit for bit (`routes_agree`).  Prints one JSON line per call: minimum and median of
`--repeats` rounds after a warm-up, and the ratios of (a) to (b), of (a') to (b') and of (a) to (c).

    python scripts/monotone_rate.py [--samples 1000] [--repeats 3] [--small] [--once] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils  # noqa: E402

Q = (5, 95)


def emit(out, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def inputs(S, N, M, T, K, noise, seed):
    rs = np.random.RandomState(seed)
    Ws = rs.gamma(1, 1, (S, N, K))
    Vs = np.ascontiguousarray(0.2 * rs.gamma(1, 1, (S, M, T, K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, noise, (S, M, T, K)))
    return Ws, Vs


def case(name, N, M, T, K, S, noise, repeats, once, out):
    Ws, Vs = inputs(S, N, M, T, K, noise, seed=int(noise * 100))
    print("# %s noise %.2f: %d samples drawn" % (name, noise, S), file=sys.stderr, flush=True)
    if once:                                       # under a profiler: one call, no timing
        utils.posterior_monotone(Ws, Vs, q=Q)
        return
    keep = {}

    def a_full():
        keep["a"] = utils.posterior_monotone(Ws, Vs, q=Q)

    def a_project():
        keep["a'"] = utils.posterior_monotone(Ws, Vs, q=None)

    def b_project():
        keep["Vb"] = np.stack([utils.factor_pav(Ws[s], Vs[s]) for s in range(S)])

    def b_full():
        b_project()
        keep["b"] = utils.posterior_summary(Ws, keep["Vb"], Q)

    def c_summary():
        utils.posterior_summary(Ws, Vs, Q)

    calls = [("a: posterior_monotone with summary", a_full), ("a': posterior_monotone without summary", a_project),
             ("b: factor_pav per sample + posterior_summary", b_full), ("b': factor_pav per sample", b_project),
             ("c: posterior_summary alone", c_summary)]
    for _, fn in calls:                            # warm-up: code objects, allocations; and the routes agree
        fn()
    a, ap = keep["a"], keep["a'"]
    agree = bool(np.array_equal(a["V"], keep["Vb"]) and np.array_equal(ap["V"], keep["Vb"]) and np.array_equal(a["mean"], keep["b"][0])
                 and np.array_equal(a["quantiles"], keep["b"][1]) and np.array_equal(a["pools"], ap["pools"]))
    ts = {what: [] for what, _ in calls}
    for _ in range(repeats):                       # alternate them so that a drift of the shared host hits them alike
        for what, fn in calls:
            t0 = time.perf_counter()
            fn()
            ts[what].append(time.perf_counter() - t0)
    tmin = {what[:2].strip(":"): min(v) for what, v in ts.items()}
    common = dict(case=name, shape=[N, M, T], nembeds=K, nsamples=S, noise=noise, repeats=repeats, routes_agree=agree,
                  pools_mean=float(a["pools"].mean()), changed_mean=float(a["changed"].mean()))
    for what, _ in calls:
        emit(out, what=what, seconds_min=min(ts[what]), seconds_median=float(np.median(ts[what])), **common)
    emit(out, what="ratios", a_to_b=tmin["a"] / tmin["b"], a_project_to_b_project=tmin["a'"] / tmin["b'"], a_to_c=tmin["a"] / tmin["c"],
         a_beats_b=bool(tmin["a"] < tmin["b"] and tmin["a'"] < tmin["b'"]), **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (64,16,9) rehearsal instead of the three shapes")
    ap.add_argument("--once", action="store_true", help="one posterior_monotone call per case, untimed (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    shapes = [("small", 64, 16, 9, 5)] if a.small else [("C3 (512,256,64)", 512, 256, 64, 5), ("dose-response (1024,256,9)", 1024, 256, 9, 5),
                                                        ("flu (50,1,370)", 50, 1, 370, 10)]
    for name, N, M, T, K in shapes:
        for noise in (0.05, 0.3):
            case(name, N, M, T, K, min(a.samples, 64) if a.small else a.samples, noise, a.repeats, a.once, a.out)


if __name__ == "__main__":
    main()
