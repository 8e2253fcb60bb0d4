"""Time posterior_similarity against the host route and against posterior_ranking on the same device-collected samples
(one run on the GPU).

S kept samples, K = 5, at C3 (512,256,64) along the rows (E = 512) and the columns (E = 256), at the dose-response shape
(1024,256,9) along the rows (E = 1024) and at the flu shape (50,1,370) along the rows.  Three calls, alternated:
    similarity   model.posterior_similarity(along=...)                     (downloads of its (.,E,E) outputs included)
    host route   a download of the collected W and V, then numpy: the quadratic form per sample, np.percentile over the
                 (S,E,E) distances and a stable argsort per (sample, entity) with its counts - the steps of similarity.reference.  At the
                 large shapes that is minutes and gigabytes for S = 1000, so the numpy half runs on the first
                 `host_nsamples` samples only (as many as keep it to some seconds); the line reports the time measured for
                 those and `seconds_min_scaled`, the same scaled to all S (every step of it is linear in S).  The
                 download is that of all S samples.
    ranking      model.posterior_ranking("auc") within the other axis: the nearest existing analysis, as an observation
Prints one JSON line per call: host wall clock around calls that end in a device synchronise, min of `repeats`.  The
script also checks that the device and the host route agree on the samples the host route took.

    python scripts/similarity_rate.py [--samples 1000] [--repeats 3] [--small] [--once] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd import _native, similarity  # noqa: E402
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402

NEAREST = (1, 5)
Q = (5, 95)


def fit(N, M, T, R, K, S):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    return model


def case(name, model, R, S, along, repeats, once, out):
    N, M, T, K = model.nrows, model.ncols, model.ndepth, model.nembeds
    E, TT = (N, 1) if along == "rows" else (M, T)
    Sh = int(max(min(8, S), min(S, 2e9 // (E * E * TT * K), 3e7 // (E * E))))
    print("# %s %s: %d samples collected, host route on %d" % (name, along, S, Sh), file=sys.stderr, flush=True)

    def download():
        Ws, Vs = np.zeros((S, N, K)), np.zeros((S, M, T, K))
        model._ctx.call("btf_collect_end", int(S), _native.dptr(Ws), _native.dptr(Vs), None, None)
        model._ctx.call("btf_sync")
        return Ws, Vs

    def host_route():
        Ws, Vs = download()
        d2 = similarity.squared_distances(Ws[:Sh], Vs[:Sh], along)
        mean, var, quant = similarity.summarize(np.sqrt(d2), Q)
        d2[:, np.arange(E), np.arange(E)] = np.nan                          # the keys: e itself last
        e, v, p = similarity.neighbours(d2, NEAREST)
        return {"mean": mean, "var": var, "quantiles": quant, "expected_rank": e, "rank_var": v, "p_nearest": p}

    calls = [("posterior_similarity rms " + along, lambda: model.posterior_similarity(along=along, q=Q, nearest=NEAREST)),
             ("host route: download + numpy form, percentile, argsort", host_route),
             ("posterior_ranking auc", lambda: model.posterior_ranking("auc", along="cols" if along == "rows" else "rows"))]
    if once:                               # under a profiler: one device call each, no timing
        calls[0][1]()
        calls[2][1]()
        return
    calls[0][1]()                          # warm-up: code objects, allocations
    calls[2][1]()
    ref = calls[1][1]()
    sub = model.posterior_similarity(results=dict(zip("WV", (a[:Sh] for a in download()))), along=along, q=Q, nearest=NEAREST)
    agree = bool(np.abs(sub["mean"] ** 2 - ref["mean"] ** 2).max() <= 1e-9 * (ref["mean"] ** 2).max() and
                 np.abs(sub["expected_rank"] - ref["expected_rank"]).max() <= 0.05 * E)
    # alternate the three so that a drift of the shared host hits them alike
    ts = {what: [] for what, _ in calls}
    for _ in range(repeats):
        for what, fn in calls:
            t0 = time.perf_counter()
            fn()
            ts[what].append(time.perf_counter() - t0)
    t_sim = min(ts[calls[0][0]])
    t0 = time.perf_counter()
    download()
    t_down = time.perf_counter() - t0
    for what, _ in calls:
        t = min(ts[what])
        rec = dict(case=name, along=along, entities=E, what=what, seconds_min=t, seconds_median=float(np.median(ts[what])),
                   ratio_to_similarity=t / t_sim, routes_agree=agree, shape=[N, M, T, R], nembeds=K, nsamples=S, repeats=repeats)
        if what.startswith("host"):
            rec.update(host_nsamples=Sh, seconds_download=t_down, seconds_min_scaled=t_down + (t - t_down) * S / Sh,
                       ratio_scaled_to_similarity=(t_down + (t - t_down) * S / Sh) / t_sim)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (32,16,16) rehearsal instead of the large shapes")
    ap.add_argument("--once", action="store_true", help="one call of each, untimed (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    shapes = [("flu (50,1,370)", (50, 1, 370), ("rows",))]
    if a.small:
        shapes.append(("small", (32, 16, 16), ("rows", "cols")))
    else:
        shapes += [("C3 (512,256,64)", (512, 256, 64), ("rows", "cols")), ("dose-response (1024,256,9)", (1024, 256, 9), ("rows",))]
    for name, dims, alongs in shapes:
        S = min(a.samples, 64) if name == "small" else a.samples
        model = fit(*dims, 1, 5, S)
        for along in alongs:
            case(name, model, 1, S, along, a.repeats, a.once, a.out)
        del model


if __name__ == "__main__":
    main()
