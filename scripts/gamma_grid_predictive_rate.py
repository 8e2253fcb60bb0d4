"""Time utils.gamma_grid_predictive against utils.posterior_predictive(..., "poisson_identity") on the same states (one run
on the GPU), and against the host route of the reference application.

Two shapes: (1024,256,9) K = 5, G = 50, S = 1000 and the dose-response size (256,128,10,3) K = 5, G = 50, S = 500; each with
draws_per_sample 1 and 10, with data (band, PIT, coverage, RMSE / MAE).  The Poisson identity-link call is the kernel the
gamma-grid family was instantiated from: the same launch geometry, the same sort, another sampler - so it is the yardstick.
The host route is doseresponse/fit.py:475-478: GammaGridLikelihood.sample at size [draws, S, T] and np.percentile per
curve, in a Python loop over the curves of a slab of rows; its time for the whole tensor is EXTRAPOLATED from the slab.
Host wall clock around calls that end in a device synchronise, uploads of the states and of Y and downloads of the outputs
included: the minimum of --repeats calls after a warm-up.  One JSON line per case, appended to --out when given
(profiles/rNN_gg_predictive_rate.jsonl).

    python scripts/gamma_grid_predictive_rate.py [--repeats 3] [--small] [--out profiles/rNN_gg_predictive_rate.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import utils  # noqa: E402
from functionalmf_amd.likelihoods import GammaGridLikelihood  # noqa: E402


def rate_table(G=50):
    """Means 0.5 .. 1.5, a bump of weights around 1, variance 0.01 (tests/test_gpu_gg_predictive.py checks the sampler on it)."""
    grid = np.linspace(0.5, 1.5, G)
    return GammaGridLikelihood(grid, np.exp(-0.5 * ((grid - 1.0) / 0.25) ** 2), 0.01)


def best(fn, repeats):
    fn()                                   # warm-up: code objects, allocations
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def host_route(lik, Ws, Vs, rows, draws, q):
    """fit.py:475-478 on the first `rows` rows: seconds."""
    rs = np.random.RandomState(0)
    M = Vs.shape[1]
    t0 = time.perf_counter()
    for i in range(rows):
        for j in range(M):
            mu = np.einsum("sk,stk->st", Ws[:, i], Vs[:, j])                   # (S, T)
            y = lik.sample(mu[None], size=(draws,) + mu.shape, rng=rs)
            np.percentile(y, q, axis=(0, 1))
    return time.perf_counter() - t0


def case(name, N, M, T, R, K, G, S, repeats, slab_rows, out):
    rs = np.random.RandomState(0)
    lik = rate_table(G)
    W = rs.uniform(0.2, 0.6, size=(N, K))
    V = np.cumsum(rs.uniform(0.0, 0.1, size=(M, T, K)), axis=1)[:, ::-1]       # decreasing curves, w.v in (0, 1.6)
    Ws = W[None] * np.exp(0.05 * rs.normal(size=(S, N, K)))
    Vs = np.ascontiguousarray(V)[None] * np.exp(0.05 * rs.normal(size=(S, M, T, K)))
    eta = np.einsum("nk,mtk->nmt", W, V)
    Y = lik.sample(eta[..., None], size=eta.shape + (R,), rng=rs)
    q = (5.0, 95.0)
    rows = []
    for dps in (1, 10):
        t_p = best(lambda: utils.posterior_predictive(Ws, Vs, "poisson_identity", data=np.ceil(Y), q=q, draws_per_sample=dps, seed=1), repeats)
        t_g = best(lambda: utils.gamma_grid_predictive(Ws, Vs, lik, data=Y, q=q, draws_per_sample=dps, seed=1), repeats)
        rows.append(dict(what="posterior_predictive poisson_identity", draws_per_sample=dps, seconds_min=t_p[0], seconds_median=t_p[1]))
        rows.append(dict(what="gamma_grid_predictive", draws_per_sample=dps, seconds_min=t_g[0], seconds_median=t_g[1],
                         ratio_to_poisson_identity=t_g[0] / t_p[0]))
    slab = min(slab_rows, N)
    t_h = host_route(lik, Ws, Vs, slab, 1, q)
    rows.append(dict(what="host route: GammaGridLikelihood.sample + np.percentile per curve, draws_per_sample 1", slab_rows=slab,
                     seconds_slab=t_h, seconds_extrapolated=t_h * N / slab, extrapolated=slab < N))
    for r in rows:
        r.update(case=name, shape=[N, M, T, R], nembeds=K, components=G, nsamples=S)
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (32,16,9) rehearsal instead of the two shapes")
    ap.add_argument("--slab-rows", type=int, default=2, help="rows of the host route's slab")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.small:
        case("small", 32, 16, 9, 2, 3, 50, 40, a.repeats, a.slab_rows, a.out)
        return
    case("dose-response (256,128,10,3)", 256, 128, 10, 3, 5, 50, 500, a.repeats, a.slab_rows, a.out)
    case("(1024,256,9)", 1024, 256, 9, 1, 5, 50, 1000, a.repeats, a.slab_rows, a.out)


if __name__ == "__main__":
    main()
