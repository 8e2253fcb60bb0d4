"""Time of tensor_nmf on the GPU (csrc/btf_nmf.h): 30 ALS steps after a warm-up call.
python scripts/nmf_rate.py [c3_complete | c3_missing5 | c3_monotone | c5_complete ...]  - one JSON line per configuration.

  c3_complete  (512,256,64,4) nembeds 5, complete data
  c3_missing5  (512,256,64,4) nembeds 5, 5 % of the cells and 5 % of the replicates missing
  c3_monotone  (512,256,64,4) nembeds 5, complete data, monotone=True (factor_pav after every V step)
  c5_complete  (4096,1024,64,4) nembeds 8, complete data

stats_ms: building the statistics on the host and uploading them (btf_nmf_create), by the host clock;
call_ms: one run of `steps` ALS steps (tol = -1: every step runs) with the statistics resident, by the host clock
(upload of W0 / V0 and download of the result included); kernel_ms_per_step: device time of the queued steps (HIP events
around them) divided by the steps run."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import nmf  # noqa: E402

CONFIGS = {"c3_complete": (512, 256, 64, 4, 5, 0.0, False), "c3_missing5": (512, 256, 64, 4, 5, 0.05, False),
           "c3_monotone": (512, 256, 64, 4, 5, 0.0, True), "c5_complete": (4096, 1024, 64, 4, 8, 0.0, False)}
STEPS = 30


def run(name):
    N, M, T, R, K, miss, monotone = CONFIGS[name]
    rs = np.random.RandomState(0)
    Y = np.einsum("nk,mtk->nmt", rs.gamma(2.0, 0.5, (N, K)), rs.gamma(2.0, 0.5, (M, T, K)))[..., None] + \
        rs.normal(0, 0.5, size=(N, M, T, R))
    if miss:
        Y[rs.uniform(size=(N, M, T)) < miss] = np.nan
        Y[rs.uniform(size=Y.shape) < miss] = np.nan
    np.random.seed(1)
    W0 = np.random.gamma(1, 1, (N, K))
    W0[np.triu_indices(K, k=1)] = 0
    V0 = np.random.gamma(1, 1, (M, T, K))
    t0 = time.perf_counter()
    data = nmf.NMFData(Y, K)
    stats_ms = 1e3 * (time.perf_counter() - t0)
    del Y
    try:
        data.run(W0, V0, max_steps=STEPS, monotone=monotone, tol=-1.0)          # warm-up
        t0 = time.perf_counter()
        W, V, info = data.run(W0, V0, max_steps=STEPS, monotone=monotone, tol=-1.0, timing=True)
        call_ms = 1e3 * (time.perf_counter() - t0)
    finally:
        data.close()
    return {"config": name, "shape": [N, M, T, R], "nembeds": K, "missing": miss, "monotone": monotone,
            "steps": info["steps"], "call_ms": round(call_ms, 3), "stats_ms": round(stats_ms, 1),
            "kernel_ms_per_step": round(info["device_ms"] / max(info["steps"], 1), 4), "rmse_last": float(info["rmse"][-1])}


if __name__ == "__main__":
    for name in sys.argv[1:] or sorted(CONFIGS):
        print(json.dumps(run(name)), flush=True)
