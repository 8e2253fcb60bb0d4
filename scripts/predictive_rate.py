"""Time posterior_predictive against posterior_summary on the same device-collected samples (one run on the GPU).

Gaussian, draws_per_sample = 1, S kept samples at C3 (512,256,64) and at the flu shape (50,1,370); then the Binomial and
Poisson families at C3 on the same samples through predictive.evaluate.  The Gaussian predictive does the summary's work
(dot products, per-cell sort) plus one normal per value, so the summary is its yardstick.  Prints one JSON line per case:
host wall clock around calls that end in a device synchronise (uploads of Y and downloads of the outputs included).

    python scripts/predictive_rate.py [--samples 1000] [--repeats 3] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import predictive  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def best(fn, repeats):
    fn()                                   # warm-up: code objects, allocations
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def case(name, N, M, T, R, K, S, repeats, counts):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    shape = (N, M, T)
    q = (2.5, 97.5)
    rows = []
    t_sum = best(lambda: model.posterior_summary(q=q), repeats)
    rows.append(dict(case=name, what="posterior_summary", seconds_min=t_sum[0], seconds_median=t_sum[1]))
    t_pp = best(lambda: model.posterior_predictive(q=q, seed=1), repeats)
    rows.append(dict(case=name, what="posterior_predictive gaussian (with data: pit, coverage, rmse)", seconds_min=t_pp[0],
                     seconds_median=t_pp[1], ratio_to_summary=t_pp[0] / t_sum[0]))
    bare = lambda fam, **kw: predictive.evaluate(model._ctx, shape, K, fam, S, q=q, seed=1, **kw)
    t_b = best(lambda: bare(3, aux_flags=1), repeats)
    rows.append(dict(case=name, what="posterior_predictive gaussian (no data: mean, moments, band)", seconds_min=t_b[0],
                     seconds_median=t_b[1], ratio_to_summary=t_b[0] / t_sum[0]))
    if counts:
        tr = np.full(shape, 20.0)
        for fam, kw in (("poisson", {}), ("binomial", dict(trials=tr))):
            t = best(lambda: bare(predictive.family_code(fam), **kw), repeats)
            rows.append(dict(case=name, what="posterior_predictive %s (no data)" % fam, seconds_min=t[0], seconds_median=t[1],
                             ratio_to_summary=t[0] / t_sum[0]))
    for r in rows:
        r.update(shape=[N, M, T, R], nsamples=S)
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (32,16,16) rehearsal instead of C3")
    a = ap.parse_args()
    case("flu (50,1,370)", 50, 1, 370, 1, 5, a.samples, a.repeats, False)
    if a.small:
        case("small", 32, 16, 16, 1, 5, min(a.samples, 64), a.repeats, True)
    else:
        case("C3 (512,256,64)", 512, 256, 64, 1, 5, a.samples, a.repeats, True)


if __name__ == "__main__":
    main()
