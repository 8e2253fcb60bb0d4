"""Time of one model-selection criteria call (information_criteria: csrc/btf_criteria.h) after a warm-up call.
python scripts/criteria_rate.py [c3_gauss | c3_binom | c5_gauss ...]  - one JSON line per configuration.

  c3_gauss  (512,256,64,4) nembeds 5, Gaussian, S = 1000 device-collected samples (no upload)
  c3_binom  (512,256,64) nembeds 5, Binomial 4 trials per cell, S = 1000 uploaded samples (Vs alone is 655 MB)
  c5_gauss  (4096,1024,64,4) nembeds 8, Gaussian, S = 100 device-collected samples

kernel_ms: the criteria launches (main kernel + plug-in + per-sample totals), bracketed by HIP events (btf_set_profiling);
call_ms: the whole call by the host clock (statistics cached from the warm-up; upload of uploaded samples included)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering  # noqa: E402

CONFIGS = {"c3_gauss": (512, 256, 64, 4, 5, 1000), "c3_binom": (512, 256, 64, 1, 5, 1000), "c5_gauss": (4096, 1024, 64, 4, 8, 100)}


def timed(m, call):
    call()                                   # warm-up: statistics built and uploaded, code loaded
    m.sync()
    m._ctx.call("btf_set_profiling", 1)
    m._ctx.kernel_times()
    t0 = time.perf_counter()
    out = call()
    wall = time.perf_counter() - t0
    kt = m._ctx.kernel_times()
    m._ctx.call("btf_set_profiling", 0)
    return out, 1e3 * wall, kt["criteria"]


def run(name):
    N, M, T, R, K, S = CONFIGS[name]
    rs = np.random.RandomState(0)
    W0 = rs.normal(size=(N, K))
    V0 = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1) / np.sqrt(T)
    Mu = np.einsum("nk,mtk->nmt", W0, V0)
    np.random.seed(1)
    if name == "c3_binom":
        Nt = np.full((N, M, T), 4.0)
        Y = rs.binomial(4, 1.0 / (1.0 + np.exp(-Mu))).astype(float)
        data = (Y, Nt)
        m = BinomialBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=1)
        m.set_data(data)
        # S posterior-like states around the truth (the cost does not depend on the values)
        res = {"W": W0[None] + 0.05 * rs.normal(size=(S, N, K)), "V": V0[None] + 0.01 * rs.normal(size=(S, M, T, K))}
        call = lambda: m.information_criteria(res)
        bound = "fp64 VALU (softplus: exp + log1p per cell and sample); the call adds the 676 MB upload over PCIe"
    else:
        Y = Mu[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
        del Mu
        m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=1)
        m.run_gibbs(Y, nburn=10, nsamples=S, verbose=False)
        call = lambda: m.information_criteria()
        bound = "cache / HBM bytes: the statistics re-read once per 32 samples, w_i^s per sample and depth chunk"
    ic, wall, (kms, nl) = timed(m, call)
    cells = N * M * T
    return {"config": name, "shape": [N, M, T, R], "nembeds": K, "nsamples": S, "kernel_ms": round(kms, 3), "launches": nl,
            "call_ms": round(wall, 2), "cell_samples_per_s": round(cells * S / (kms * 1e-3), 1), "bound": bound,
            "waic": ic["waic"], "dic": ic["dic"]}


if __name__ == "__main__":
    for name in sys.argv[1:] or sorted(CONFIGS):
        print(json.dumps(run(name)), flush=True)
