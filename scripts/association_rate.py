"""Time posterior_feature_association against posterior_functionals and against the host route on the same
device-collected samples (one run on the GPU).

S kept samples of a Gaussian chain, K = 5, at the dose-response shape (1024,256,9) with F = 32 and F = 1024 features and at
C3 (512,256,64) with F = 32.  The feature embeddings are standard normal draws (S,F,K): the work does not depend on their
values.  Three calls, alternated:
    association  model.posterior_feature_association(U, "auc", stats=("r",))          (uploads U, downloads its outputs)
    functionals  model.posterior_functionals(("auc",)) alone: the floor, the association call contains that sweep
    host route   model.posterior_functionals(("auc",), pointwise=True), its (S,N,M) download, then per sample the numpy
                 correlation matrix of W_s U_s' (N,F) and the values (N,M) - what there was before.  Timed at F = 32 only;
                 at F = 1024 its numpy part is EXTRAPOLATED by F / 32 from the F = 32 measurement and marked so (an upper
                 estimate: the per-sample work that does not depend on F is scaled too; the F = 32 time is the lower one).
Prints one JSON line per call: host wall clock around calls that end in a device synchronise.  The script also checks that
the two routes return the same mean r to 1e-10.

    python scripts/association_rate.py [--samples 1000] [--repeats 3] [--small] [--once] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import GaussianBayesianTensorFiltering  # noqa: E402


def host_r_mean(f, Ws, Us):
    """mean_s of the (F,M) correlation matrix of W_s U_s' and f_s, every value defined (auc): one matmul per sample."""
    acc = 0.0
    for s in range(f.shape[0]):
        X, y = Ws[s] @ Us[s].T, f[s]
        X, y = X - X.mean(axis=0), y - y.mean(axis=0)
        acc = acc + (X.T @ y) / np.sqrt((X * X).sum(axis=0)[:, None] * (y * y).sum(axis=0)[None, :])
    return acc / f.shape[0]


def emit(out, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def case(name, N, M, T, K, S, features, repeats, once, out):
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.5, size=(N, M, T, 1))
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y, nburn=20, nthin=1, nsamples=S, verbose=False)
    print("# %s: %d samples collected" % (name, S), file=sys.stderr, flush=True)
    host_numpy = None                                  # seconds of the numpy part at the first (smallest) F
    for F in features:
        Us = rs.normal(size=(S, F, K))
        timed_host = host_numpy is None
        parts = {}

        def host_route():
            t0 = time.perf_counter()
            f = model.posterior_functionals(which=("auc",), q=None, pointwise=True)["auc"]["pointwise"]
            t1 = time.perf_counter()
            r = host_r_mean(f, res["W"], Us)
            parts["device"], parts["numpy"] = t1 - t0, time.perf_counter() - t1
            return r

        calls = [("posterior_feature_association auc r", lambda: model.posterior_feature_association(U=Us, which="auc", stats=("r",))),
                 ("posterior_functionals auc", lambda: model.posterior_functionals(which=("auc",)))]
        if timed_host:
            calls.append(("host route: functionals pointwise + numpy correlation per sample", host_route))
        if once:                               # under a profiler: one call each, no timing
            for _, fn in calls[:2]:
                fn()
            continue
        got = calls[0][1]()                    # warm-up: code objects, allocations; and the two routes agree
        calls[1][1]()
        agree = None
        if timed_host:
            agree = bool(np.abs(got["r"]["mean"] - host_route()).max() < 1e-10)
        ts = {what: [] for what, _ in calls}
        hp = []
        for _ in range(repeats):               # alternate them so that a drift of the shared host hits them alike
            for what, fn in calls:
                t0 = time.perf_counter()
                fn()
                ts[what].append(time.perf_counter() - t0)
            if timed_host:
                hp.append(dict(parts))
        t_assoc = min(ts[calls[0][0]])
        common = dict(case=name, shape=[N, M, T], nfeatures=F, nembeds=K, nsamples=S, repeats=repeats)
        for what, _ in calls:
            emit(out, what=what, seconds_min=min(ts[what]), seconds_median=float(np.median(ts[what])),
                 ratio_to_association=min(ts[what]) / t_assoc, routes_agree=agree, extrapolated=False, **common)
        if timed_host:
            host_numpy = (F, min(p["numpy"] for p in hp), min(p["device"] for p in hp))
        else:
            F0, t_np, t_dev = host_numpy
            t = t_dev + t_np * F / F0
            emit(out, what="host route: functionals pointwise + numpy correlation per sample", seconds_min=t, seconds_median=t,
                 ratio_to_association=t / t_assoc, routes_agree=None, extrapolated=True,
                 note="upper estimate: numpy part %.3f s at F = %d scaled by F / %d (its F-independent work too), pointwise call %.3f s as "
                      "measured; lower estimate: the F = %d route as measured" % (t_np, F0, F0, t_dev, F0), **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a (64,16,9) rehearsal instead of the three shapes")
    ap.add_argument("--once", action="store_true", help="one call of each, untimed (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if a.small:
        case("small", 64, 16, 9, 5, min(a.samples, 64), (8, 40), a.repeats, a.once, a.out)
        return
    case("dose-response (1024,256,9)", 1024, 256, 9, 5, a.samples, (32, 1024), a.repeats, a.once, a.out)
    case("C3 (512,256,64)", 512, 256, 64, 5, a.samples, (32,), a.repeats, a.once, a.out)


if __name__ == "__main__":
    main()
