"""Time posterior_checks against posterior_predictive (with data) on the same device-collected samples (one run on the GPU).

reps = 1, S kept samples: the large shape (512,256,64,4) K = 5, Gaussian through the model's methods and Poisson through
checks.evaluate / predictive.evaluate on the same samples; the flu shape (50,1,370) K = 10, Gaussian.  The check draws
nreps replicates per cell and sample where the predictive call draws one, and sorts nothing.  At the flu shape also the
host route: every draw downloaded (posterior_predictive(cells=all)["draws"]) and reduced by the numpy definition,
checks.reference.  Prints one JSON line per case: host wall clock around calls that end in a device
synchronise (uploads of Y and downloads of the outputs included), min and median of --repeats after a warm-up.

    python scripts/checks_rate.py [--samples 1000] [--repeats 3] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import checks, predictive  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def best(fn, repeats):
    fn()                                   # warm-up: code objects, allocations
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def fit(N, M, T, R, K, S):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    return model, Y, res


def case(name, N, M, T, R, K, S, repeats, poisson, host):
    model, Y, res = fit(N, M, T, R, K, S)
    shape = (N, M, T)
    rows = []
    t_pp = best(lambda: model.posterior_predictive(seed=1), repeats)
    rows.append(dict(case=name, what="posterior_predictive gaussian (with data)", seconds_min=t_pp[0], seconds_median=t_pp[1]))
    t_ck = best(lambda: model.posterior_checks(seed=1), repeats)
    rows.append(dict(case=name, what="posterior_checks gaussian (chisq, max, lag1, total)", seconds_min=t_ck[0], seconds_median=t_ck[1],
                     ratio_to_predictive=t_ck[0] / t_pp[0]))
    if poisson:
        Yc = np.round(np.abs(2 * Y))
        t_pp = best(lambda: predictive.evaluate(model._ctx, shape, K, 0, S, Y=Yc, seed=1), repeats)
        rows.append(dict(case=name, what="posterior_predictive poisson (with data)", seconds_min=t_pp[0], seconds_median=t_pp[1]))
        t_ck = best(lambda: checks.evaluate(model._ctx, shape, K, 0, S, Y=Yc, seed=1), repeats)
        rows.append(dict(case=name, what="posterior_checks poisson (all five)", seconds_min=t_ck[0], seconds_median=t_ck[1],
                         ratio_to_predictive=t_ck[0] / t_pp[0]))
    if host:
        def host_route():
            pp = model.posterior_predictive(draws_per_sample=R, seed=1, cells=np.arange(N * M * T, dtype=np.int32))
            eta = np.einsum("znk,zmtk->znmt", res["W"], res["V"])
            return checks.reference(Y, eta, np.broadcast_to(res["nu2"].reshape(-1, 1, 1, 1), eta.shape), pp["draws"], reps=1,
                                    which=checks.DISCREPANCIES[:4])
        t_host = best(host_route, 1)
        rows.append(dict(case=name, what="host route: every draw downloaded + the numpy definition", seconds_min=t_host[0],
                         seconds_median=t_host[1], ratio_to_checks=t_host[0] / t_ck[0]))
    for r in rows:
        r.update(shape=[N, M, T, R], nembeds=K, nsamples=S)
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (32,16,16,2) rehearsal instead of the large shape")
    a = ap.parse_args()
    case("flu (50,1,370)", 50, 1, 370, 1, 10, a.samples, a.repeats, False, True)
    if a.small:
        case("small", 32, 16, 16, 2, 5, min(a.samples, 64), a.repeats, True, False)
    else:
        case("large (512,256,64,4)", 512, 256, 64, 4, 5, a.samples, a.repeats, True, False)


if __name__ == "__main__":
    main()
