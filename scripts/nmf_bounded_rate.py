"""Cost of bounded_tensor_nmf's max_entry projection and row features on the GPU (csrc/btf_nmf.h) against the plain call.
python scripts/nmf_bounded_rate.py [dose | c3 ...]  - one JSON line per configuration, appended to
profiles/r16_nmf_bounded_rate.jsonl.

  dose  (1024,256,9,6) nembeds 5   the dose-response shape
  c3    (512,256,64,4) nembeds 5

Data in [0, 1] near the upper plateau plus noise, so that some fits overshoot.  Per configuration three calls share one
NMFData handle (statistics resident) and run in one process, each after a warm-up and as the median of 5 rounds that
alternate between them: tensor_nmf(monotone=True), bounded (monotone=True, max_entry=0.999) and the same with F = 32
binary row features.  STEPS ALS steps with tol = -1 (every step runs).  device_ms: HIP events around the queued steps;
ratio: to the plain call; projected_share: systems projected per step / systems fitted per step (N + M*T [+ F])."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from functionalmf_amd import nmf  # noqa: E402

CONFIGS = {"dose": (1024, 256, 9, 6, 5), "c3": (512, 256, 64, 4, 5)}
STEPS, ROUNDS, F = 10, 5, 32


def run(name):
    N, M, T, R, K = CONFIGS[name]
    rs = np.random.RandomState(0)
    Vt = -np.sort(-rs.uniform(0.05, 1.0, size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", rs.dirichlet(0.5 * np.ones(K), size=N), Vt)[..., None] + rs.normal(0, 0.08, size=(N, M, T, R))
    X = (rs.uniform(size=(N, F)) < 0.5).astype(float)
    X[rs.uniform(size=X.shape) < 0.1] = np.nan
    np.random.seed(1)
    W0 = np.random.gamma(1, 1, (N, K))
    W0[np.triu_indices(K, k=1)] = 0
    V0 = np.random.gamma(1, 1, (M, T, K))
    R0 = np.random.gamma(1, 1, (F, K))
    calls = {"plain": {}, "bounded": {"max_entry": 0.999}, "bounded_features": {"max_entry": 0.999, "row_features": X, "R": R0}}
    data = nmf.NMFData(Y, K)
    del Y
    ms = {k: [] for k in calls}
    last = {}
    try:
        for rnd in range(ROUNDS + 1):                        # round 0 warms up
            for k, kw in calls.items():
                _, _, info = data.run(W0, V0, max_steps=STEPS, monotone=True, tol=-1.0, timing=True, **kw)
                if rnd:
                    ms[k].append(info["device_ms"])
                last[k] = info
    finally:
        data.close()
    out = {"config": name, "shape": [N, M, T, R], "nembeds": K, "steps": STEPS, "rounds": ROUNDS, "features": F}
    plain = float(np.median(ms["plain"]))
    for k in calls:
        med = float(np.median(ms[k]))
        out[k + "_device_ms"] = round(med, 3)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 3), round(max(ms[k]), 3)]
        if k != "plain":
            nsys = N + M * T + (F if k == "bounded_features" else 0)
            out[k + "_ratio"] = round(med / plain, 3)
            out[k + "_projected_share"] = [round(float(p) / nsys, 4) for p in last[k]["projected"]]
    return out


if __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r16_nmf_bounded_rate.jsonl"), "a") as fh:
        for name in sys.argv[1:] or sorted(CONFIGS):
            line = json.dumps(run(name))
            print(line, flush=True)
            fh.write(line + "\n")
