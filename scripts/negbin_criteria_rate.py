"""Time negbin_criteria / negbin_loo of the Negative-Binomial model (csrc/btf_nb_criteria.h) on S uploaded samples, for a
scalar rate and for one rate per row, beside information_criteria() of a BinomialBayesianTensorFiltering at the same shape
and S (the logit family: its main kernel does the same softplus work) and beside the host definition
criteria.negbin_loglik, in one process: (512,256,64,4) K = 5 and the flu shape (50,1,370) K = 10.

    python scripts/negbin_criteria_rate.py [--out profiles/r22_negbin_criteria_rate.jsonl] [--repeats 3] [--samples 1000]

Wall clock is the host's, transfers of the samples included (the C entry points synchronise before they return): one
warm-up call, then the minimum of `repeats`.  Kernel time is the sum of the call's BTF_K_CRITERIA launches by HIP events
(btf_set_profiling): for negbin_criteria the constant kernel, the main kernel, the plug-in and the totals together - the
Binomial call has the last three, so the difference is the constant kernel plus what the rate reads cost the main one.
The host route is timed on `--host-samples` samples and scaled to S.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import criteria                                                                        # noqa: E402
from functionalmf_amd.factor import BinomialBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering  # noqa: E402


def best(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(min(ms))


def kernel_ms(model, fn):
    """Sum of the BTF_K_CRITERIA launches of one call, by HIP events."""
    ctx = model._ctx
    ctx.call("btf_set_profiling", 1)
    ctx.kernel_times()
    fn()
    ms, n = ctx.kernel_times()["criteria"]
    ctx.call("btf_set_profiling", 0)
    return float(ms), int(n)


def run(shape, nreps, K, S, repeats, host_samples):
    N, M, T = shape
    rs = np.random.RandomState(0)
    W0 = 0.7 * rs.normal(size=(N, K)) / np.sqrt(K)
    V0 = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    P = 1 / (1 + np.exp(-np.clip(np.einsum("nk,mtk->nmt", W0, V0), -6, 6)))
    Y = rs.negative_binomial(5.0, 1 - P[..., None].repeat(nreps, -1)).astype(float)
    Ws = W0[None] + 0.02 * rs.normal(size=(S, N, K))
    Vs = V0[None] + 0.02 * rs.normal(size=(S, M, T, K)).astype(np.float64)
    row = {"shape": [N, M, T, nreps], "nembeds": K, "nsamples": S, "repeats": repeats,
           "counts_max": float(Y.max()), "counts_over_32": float((Y > 32).mean())}
    for tag, rdims, rshape in (("scalar", (0, 1, 2), (1, 1, 1)), ("per_row", (1, 2), (N, 1, 1))):
        np.random.seed(0)
        m = NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, rdims=rdims, R_init=np.full(rshape, 5.0))
        m.set_data(Y)
        res = {"W": Ws, "V": Vs, "R": 5.0 * np.exp(0.05 * rs.normal(size=(S,) + rshape))}
        print("%r %s" % (shape, tag), file=sys.stderr, flush=True)
        row[tag + "_criteria_ms"] = best(lambda: m.negbin_criteria(res), repeats)
        row[tag + "_loo_ms"] = best(lambda: m.negbin_loo(res), repeats)
        row[tag + "_criteria_kernels_ms"], row[tag + "_criteria_launches"] = kernel_ms(m, lambda: m.negbin_criteria(res))
        row[tag + "_loo_kernels_ms"], row[tag + "_loo_launches"] = kernel_ms(m, lambda: m.negbin_loo(res))
        if tag == "scalar":
            t = time.perf_counter()
            hs = min(host_samples, S)
            criteria.negbin_loglik(Y, Ws[:hs], Vs[:hs], res["R"][:hs])
            row["host_ms_per_sample"] = (time.perf_counter() - t) * 1e3 / hs
            row["host_route_ms"] = row["host_ms_per_sample"] * S
        del m
    # the yardstick: the logit family on Binomial data of the same shape and S
    Ntr = np.full((N, M, T), float(nreps))
    Yb = rs.binomial(nreps, P).astype(float)
    np.random.seed(0)
    b = BinomialBayesianTensorFiltering(N, M, T, nembeds=K)
    b.set_data((Yb, Ntr))
    resb = {"W": Ws, "V": Vs}
    row["binomial_criteria_ms"] = best(lambda: b.information_criteria(resb), repeats)
    row["binomial_criteria_kernels_ms"], row["binomial_criteria_launches"] = kernel_ms(b, lambda: b.information_criteria(resb))
    for tag in ("scalar", "per_row"):
        row[tag + "_kernels_over_binomial"] = row[tag + "_criteria_kernels_ms"] / row["binomial_criteria_kernels_ms"]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--host-samples", type=int, default=2)
    ap.add_argument("--label", default=None, help="written into every row as `build` (BTF_NB_CRIT_TABLE=0: the direct path alone)")
    a = ap.parse_args()
    rows = [run((512, 256, 64), 4, 5, a.samples, a.repeats, a.host_samples), run((50, 1, 370), 1, 10, a.samples, a.repeats, a.host_samples)]
    for r in rows:
        if a.label:
            r["build"] = a.label
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
