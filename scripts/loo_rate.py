"""Time BayesianTensorFiltering.loo() against information_criteria() and posterior_summary() on the same
device-collected samples, in one process: C3 (512,256,64) Gaussian and the flu shape (50,1,370), S = 1000.

    python scripts/loo_rate.py [--out profiles/r14_loo_rate.jsonl] [--repeats 5] [--samples 1000]

Every timed call ends in a device synchronise (the C entry points synchronise before they return).  One warm-up call of
each kind, then `repeats` alternating rounds; the median and the spread are written, one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import criteria                                             # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering              # noqa: E402


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def run(shape, K, S, repeats, host_curves):
    N, M, T = shape
    rs = np.random.RandomState(0)
    W0 = rs.normal(size=(N, K))
    V0 = 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W0, V0)[..., None] + rs.normal(0, 0.5, size=(N, M, T, 4))
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=1)
    m.run_gibbs(Y, nburn=20, nsamples=S, verbose=False)
    calls = {"information_criteria": lambda: m.information_criteria(), "loo": lambda: m.loo(),
             "loo_mean": lambda: m.loo(mean=True), "posterior_summary": lambda: m.posterior_summary()}
    for fn in calls.values():
        fn()
    ms = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    row = {"shape": [N, M, T], "nembeds": K, "nsamples": S, "repeats": repeats}
    for k, v in ms.items():
        row[k + "_ms"] = float(np.median(v))
        row[k + "_ms_min_max"] = [float(min(v)), float(max(v))]
    row["loo_over_information_criteria"] = row["loo_ms"] / row["information_criteria_ms"]
    row["loo_mean_over_posterior_summary"] = row["loo_mean_ms"] / row["posterior_summary_ms"]
    if host_curves:                       # the other route: download the matrix, loop over curves on the host
        t = time.perf_counter()
        ic = m.information_criteria(pointwise=True)
        row["download_ms"] = (time.perf_counter() - t) * 1e3
        n = min(host_curves, N * M)
        sub = np.ascontiguousarray(ic["loglik"].reshape(S, N * M)[:, :n]).reshape(S, n, 1)
        t = time.perf_counter()
        criteria.psis_loo_host(sub, np.ones((n, 1), dtype=bool))
        row["host_ms_per_curve"] = (time.perf_counter() - t) * 1e3 / n
        row["host_route_ms"] = row["download_ms"] + row["host_ms_per_curve"] * N * M
    res = m.loo()
    row["share_above_good_k"] = res["n_bad"] / max(res["n_curves"], 1)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1000)
    a = ap.parse_args()
    rows = [run((512, 256, 64), 5, a.samples, a.repeats, 200), run((50, 1, 370), 5, a.samples, a.repeats, 50)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
