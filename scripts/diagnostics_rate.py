"""Time of one convergence-diagnostics call (functionalmf_amd.diagnostics.convergence: csrc/btf_diag.h) after a warm-up
call, over 4 device-collected Gaussian chains (rng="device", no upload).
python scripts/diagnostics_rate.py [c3 | flu ...]  - one JSON line per configuration.

  c3   (512,256,64) nembeds 5, 4 chains x 1000 draws: 8.4 M cells of 4000 draws
  flu  (50,1,370) nembeds 5, 4 chains x 1000 draws

call_s: the whole call by the host clock (the kernel, the output download and the host summaries).
For the per-kernel breakdown run it under `rocprofv3 --kernel-trace --stats -- python scripts/diagnostics_rate.py`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import diagnostics  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402

CONFIGS = {"c3": (512, 256, 64, 5, 4, 1000), "flu": (50, 1, 370, 5, 4, 1000)}


def run(name):
    N, M, T, K, C, S = CONFIGS[name]
    rs = np.random.RandomState(0)
    W0 = rs.normal(size=(N, K))
    V0 = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1) / np.sqrt(T)
    Y = np.einsum("nk,mtk->nmt", W0, V0) + rs.normal(0, 0.3, size=(N, M, T))
    models = []
    for c in range(C):
        np.random.seed(c)
        m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=c)
        m.run_gibbs(Y, nburn=100, nsamples=S, verbose=False)
        models.append(m)
    diagnostics.convergence(models)              # warm-up
    t0 = time.perf_counter()
    res = diagnostics.convergence(models)
    dt = time.perf_counter() - t0
    return {"config": name, "shape": [N, M, T], "nembeds": K, "nchains": C, "ndraws": S, "call_s": round(dt, 4),
            "cells_per_s": round(N * M * T / dt), "max_rhat": res["max_rhat"], "n_rhat_above": res["n_rhat_above"],
            "min_ess_bulk": res["min_ess_bulk"], "min_ess_tail": res["min_ess_tail"]}


if __name__ == "__main__":
    for name in sys.argv[1:] or ["flu", "c3"]:
        print(json.dumps(run(name)), flush=True)
