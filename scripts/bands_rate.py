"""Time posterior_bands against posterior_summary on the same device-collected samples (one run on the GPU).

S kept samples at C3 (512,256,64), K = 5, and at the flu shape (50,1,370), K = 10: method="supt" and method="rank" next to
model.posterior_summary(q=(2.5, 97.5)), the pointwise band of the same level from the same states.  At the flu shape also
the host route: the numpy definition (functionalmf_amd.bands) on the (S,N,M,T) tensor formed from the downloaded samples.
Prints one JSON line per case and call: host wall clock around calls that end in a device synchronise (downloads of the
outputs included), the minimum of `repeats`.

    python scripts/bands_rate.py [--samples 1000] [--repeats 3] [--small] [--once]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import bands  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def case(name, N, M, T, R, K, S, repeats, once, host):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    calls = [("posterior_summary", lambda: model.posterior_summary(q=(2.5, 97.5))),
             ("posterior_bands supt", lambda: model.posterior_bands(method="supt", level=95)),
             ("posterior_bands rank", lambda: model.posterior_bands(method="rank", level=95))]
    if host:                               # the route without the call: the tensor on the host, then numpy
        tensor = lambda: np.einsum("znk,zmtk->znmt", res["W"], res["V"])
        calls += [("numpy supt on downloaded samples", lambda: bands.supt_band(tensor(), 95)),
                  ("numpy rank on downloaded samples", lambda: bands.rank_band(tensor(), 95))]
    if once:                               # under a profiler: one call each, no timing
        for _, fn in calls[:3]:
            fn()
        return
    for _, fn in calls[:3]:                # warm-up: code objects, allocations
        fn()
    # alternate the calls so that a drift of the shared host hits them alike
    ts = {what: [] for what, _ in calls}
    for _ in range(repeats):
        for what, fn in calls:
            t0 = time.perf_counter()
            out = fn()
            ts[what].append(time.perf_counter() - t0)
            if what == "posterior_bands rank":
                shares = dict(pointwise_inside_mean=float(out["pointwise_inside"].mean()), inside_min=float(out["inside"].min()))
    t_sum = min(ts["posterior_summary"])
    for what, _ in calls:
        extra = shares if what == "posterior_bands rank" else {}
        print(json.dumps(dict(case=name, what=what, seconds_min=min(ts[what]), seconds_median=float(np.median(ts[what])),
                              ratio_to_summary=min(ts[what]) / t_sum, shape=[N, M, T, R], nembeds=K, nsamples=S, repeats=repeats,
                              **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (32,16,16) rehearsal instead of C3")
    ap.add_argument("--once", action="store_true", help="one call of each, untimed (for a kernel trace)")
    a = ap.parse_args()
    case("flu (50,1,370)", 50, 1, 370, 1, 10, a.samples, a.repeats, a.once, host=True)
    if a.small:
        case("small", 32, 16, 16, 1, 5, min(a.samples, 64), a.repeats, a.once, host=True)
    else:
        case("C3 (512,256,64)", 512, 256, 64, 1, 5, a.samples, a.repeats, a.once, host=False)


if __name__ == "__main__":
    main()
