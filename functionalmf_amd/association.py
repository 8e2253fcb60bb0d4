"""Posterior feature association: which row feature goes with which column's curve functional, with uncertainty.

The constrained model samples a feature embedding u_f for every binary row feature (a biomarker); w_i . u_f is the
probability that row i carries feature f.  What the reference application fits them for is
doseresponse/feature_importance.py:39-54: for every (feature, drug) pair it regresses the per-row AUC of the fitted curves
on the per-row feature probability and lists the strongest positive and negative associations - on posterior means only,
with no uncertainty, although the chain carries all of it.  Here the regression is formed per kept sample and summarised
over the samples; the plug-in table of the reference comes back beside it (`of_means`).  The data-sized work - the
functional of every (curve, sample), the moments of every (sample, column) and the reduction over the samples of every
(feature, column) pair - is the HIP of csrc/btf_assoc.h (btf_posterior_association / btf_collect_association); this module
holds the host halves in plain numpy (importable without a GPU): the DEFINITION (`statistics`, `summarize`, `plug_in_table`,
`reference`), the argument checks, and `evaluate`, the one caller of the C entry points.

For kept sample s, feature f, column j and one functional of functionals.py:
    y_i = functional(f(w_i^s . v_j,:^s))            x_i = w_i^s . u_f^s            I = {i : y_i is not nan},  n = |I|
    Sxx, Syy, Sxy  the centred sums over I           r = Sxy / sqrt(Sxx Syy)        slope = Sxy / Sxx
    intercept = ybar - slope xbar                    defined iff n >= 3, Sxx > 0 and Syy > 0; otherwise r, slope, intercept nan
An undefined `crossing` leaves that row out of that column's regression in that sample.  Over the samples, per (f, j) and
statistic: mean and var (ddof 1; 0 with one defined sample), np.nanpercentile's linear percentiles and prob_positive = the
share with a value > 0, all over the DEFINED samples (nan when there is none); defined = defined samples / S.

The device never forms x: it is linear in w, so with wbar, c = sum_I (w - wbar)(y - ybar) and C = sum_I (w - wbar)(w - wbar)'
per (sample, column):  xbar = u . wbar,  Sxy = u . c,  Sxx = u' C u  (`moments` / `from_moments` restate that route).
"""
import numpy as np

from . import functionals
from ._analysis import check_q, transform_code

STATS = ("r", "slope")                      # index = the code of csrc/btf_assoc.h
STAT_CODES = {n: k for k, n in enumerate(STATS)}
OF_MEANS = ("r", "slope", "intercept", "stderr", "n")      # the planes of the plug-in table, in the device's order
MAX_SAMPLES = functionals.MAX_SAMPLES       # the S values of a pair are sorted in LDS


def _regress(x, y):
    """(n, xbar, ybar, Sxx, Syy, Sxy) of x (F,n) and y (n,): centred sums."""
    n = y.shape[0]
    if n == 0:
        z = np.zeros(x.shape[0])
        return 0, z, 0.0, z, 0.0, z
    xbar, ybar = x.mean(axis=1), y.mean()
    dx, dy = x - xbar[:, None], y - ybar
    return n, xbar, ybar, (dx * dx).sum(axis=1), float(dy @ dy), dx @ dy


def _finish(n, xbar, ybar, sxx, syy, sxy):
    """(r, slope, intercept, ok) of the sums above; nan where the triple is undefined."""
    ok = (n >= 3) & (sxx > 0) & (syy > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ok, sxy / np.sqrt(sxx * syy), np.nan)
        slope = np.where(ok, sxy / sxx, np.nan)
    return r, slope, np.where(ok, ybar - slope * xbar, np.nan), ok


def statistics(y, Ws, Us):
    """{r, slope, intercept (S,F,M), n (S,M) int64} of the functional values y (S,N,M), Ws (S,N,K) and Us (S,F,K), in numpy,
    directly from x = W U': the definition the kernels are tested against."""
    y, Ws, Us = np.asarray(y, dtype=float), np.asarray(Ws, dtype=float), np.asarray(Us, dtype=float)
    S, N, M = y.shape
    F = Us.shape[1]
    out = {k: np.full((S, F, M), np.nan) for k in ("r", "slope", "intercept")}
    out["n"] = np.zeros((S, M), dtype=np.int64)
    for s in range(S):
        X = Us[s] @ Ws[s].T                                   # (F,N)
        for j in range(M):
            I = ~np.isnan(y[s, :, j])
            sums = _regress(X[:, I], y[s, I, j])
            out["n"][s, j] = sums[0]
            out["r"][s, :, j], out["slope"][s, :, j], out["intercept"][s, :, j], _ = _finish(*sums)
    return out


def moments(y, W):
    """(n, ybar, Syy, wbar (K), c (K), C (K,K)) of one sample's column y (N,) and W (N,K): what the device keeps per
    (sample, column)."""
    I = ~np.isnan(y)
    n = int(I.sum())
    K = W.shape[1]
    if n == 0:
        return 0, 0.0, 0.0, np.zeros(K), np.zeros(K), np.zeros((K, K))
    ybar, wbar = y[I].mean(), W[I].mean(axis=0)
    d, e = y[I] - ybar, W[I] - wbar
    return n, ybar, float(d @ d), wbar, e.T @ d, e.T @ e


def from_moments(mom, u):
    """(r, slope, intercept) of one feature embedding u (K,) from the moments of one (sample, column): the device's route."""
    n, ybar, syy, wbar, c, C = mom
    r, slope, icpt, _ = _finish(n, u @ wbar, ybar, u @ C @ u, syy, u @ c)
    return float(r), float(slope), float(icpt)


def summarize(v, q=(5, 95)):
    """{mean, var, quantiles, prob_positive, defined} of the per-sample statistics v (S,F,M), nan = undefined."""
    v = np.asarray(v, dtype=float)
    S = v.shape[0]
    ok = ~np.isnan(v)
    cnt = ok.sum(axis=0)
    z = np.where(ok, v, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(cnt > 0, z.sum(axis=0) / cnt, np.nan)
        dev = np.where(ok, v - mean, 0.0)
        var = np.where(cnt > 1, (dev * dev).sum(axis=0) / (cnt - 1), np.where(cnt == 1, 0.0, np.nan))
        prob = np.where(cnt > 0, (ok & (z > 0)).sum(axis=0) / cnt, np.nan)
    qs = np.atleast_1d(np.asarray(q, dtype=float))
    quant = np.full((len(qs),) + v.shape[1:], np.nan)
    some = cnt > 0
    if len(qs) and some.any():
        quant[:, some] = np.nanpercentile(v[:, some], qs, axis=0)
    return {"mean": mean, "var": var, "quantiles": quant, "prob_positive": prob, "defined": cnt / float(S)}


def plug_in_table(y, Ws, Us):
    """The reference's plug-in table (doseresponse/feature_importance.py:39-54) in numpy: the regression of
    gbar = mean over the defined samples of y (N,M) on Pbar = mean_s W_s U_s' (N,F) over the rows with a defined gbar.
    {r, slope, intercept, stderr, n (F,M); sd_x (F,), sd_y (M,) ddof 0 - the two filters of feature_importance.py:50}:
    scipy.stats.linregress's numbers; the p-value follows from r and n."""
    y, Ws, Us = np.asarray(y, dtype=float), np.asarray(Ws, dtype=float), np.asarray(Us, dtype=float)
    S, N, M = y.shape
    F = Us.shape[1]
    Pbar = np.einsum("snk,sfk->nf", Ws, Us) / S
    ok = ~np.isnan(y)
    cnt = ok.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        gbar = np.where(cnt > 0, np.where(ok, y, 0.0).sum(axis=0) / cnt, np.nan)
    out = {k: np.full((F, M), np.nan) for k in OF_MEANS}
    out["sd_x"], out["sd_y"] = Pbar.std(axis=0), np.full(M, np.nan)
    for j in range(M):
        I = ~np.isnan(gbar[:, j])
        n, xbar, ybar, sxx, syy, sxy = _regress(Pbar[I].T, gbar[I, j])
        r, slope, icpt, good = _finish(n, xbar, ybar, sxx, syy, sxy)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(good, np.sqrt(np.maximum(1.0 - r * r, 0.0) * syy / sxx / (n - 2.0)), np.nan)
        out["r"][:, j], out["slope"][:, j], out["intercept"][:, j], out["stderr"][:, j], out["n"][:, j] = r, slope, icpt, err, n
        if n:
            out["sd_y"][j] = np.sqrt(syy / n)
    return out


def reference(y, Ws, Us, which="auc", stats=("r",), q=(5, 95), pairs=None, of_means=True):
    """The dictionary posterior_feature_association returns, from the functional values y (S,N,M) in numpy."""
    st = statistics(y, Ws, Us)
    names = (stats,) if isinstance(stats, str) else tuple(stats)
    out = {"which": which, "stats": names, "nsamples": int(y.shape[0]), "n_mean": st["n"].mean(axis=0)}
    for k in names:
        r = summarize(st[k], q)
        out["defined"] = r.pop("defined")
        if pairs is not None:
            p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            r["values"] = np.ascontiguousarray(st[k][:, p[:, 0], p[:, 1]].T)
        out[k] = r
    if of_means:
        out["of_means"] = plug_in_table(y, Ws, Us)
    return out


def check_features(Us, S=None, K=None):
    """Us as a contiguous float64 (S,F,K) array of finite values; S, K: what the first and last extent must be."""
    if Us is None:
        raise ValueError("posterior feature association needs the feature embeddings U (S,F,nembeds): pass U= or a run_gibbs result "
                         "dict with 'U' (a model fitted with row_features= and sample_features=True returns it)")
    Us = np.ascontiguousarray(Us, dtype=np.float64)
    if Us.ndim != 3 or Us.shape[1] < 1 or (S is not None and Us.shape[0] != S) or (K is not None and Us.shape[2] != K):
        raise ValueError("U must be (S,F,nembeds) = (%s,F,%s) with F >= 1, got %r" % ("S" if S is None else S, "K" if K is None else K, Us.shape))
    if not np.all(np.isfinite(Us)):
        raise ValueError("U must be finite")
    return Us


def check_args(which, stats, q, transform, x, level, pairs, S, M, T, F):
    """Validate and normalise the arguments of posterior_feature_association; raises ValueError before any device call.
    Returns (name, functional code, stat names, stat codes int32, qs, transform code, x, level, pairs int32 (P,2) or None)."""
    if not isinstance(which, str) or which not in functionals.CODES:
        raise ValueError("unknown functional %r (one of %s)" % (which, functionals.NAMES))
    names = (stats,) if isinstance(stats, str) else tuple(stats)
    if not names or any(n not in STAT_CODES for n in names) or len(set(names)) != len(names):
        raise ValueError("stats must be a non-empty subset of %s without repeats, got %r" % (STATS, stats))
    qs = check_q(q, allow_none=True)
    tcode = transform_code(transform)
    if int(T) < 2:
        raise ValueError("posterior feature association needs ndepth >= 2 (a curve over depth)")
    if int(S) < 1:
        raise ValueError("posterior feature association: at least one sample")
    if int(S) > MAX_SAMPLES:
        raise ValueError("posterior feature association: %d samples exceed %d (the values of a pair are sorted in LDS); thin the samples"
                         % (S, MAX_SAMPLES))
    xs = functionals.default_x(T) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    if xs.shape != (int(T),):
        raise ValueError("x must hold ndepth = %d depth coordinates, got shape %r" % (T, xs.shape))
    if not np.all(np.isfinite(xs)) or not np.all(np.diff(xs) > 0):
        raise ValueError("x must be finite and strictly increasing")
    if which == "crossing" and (level is None or not np.isfinite(float(level))):
        raise ValueError("the crossing functional needs a finite level=")
    lev = float(level) if level is not None else float("nan")
    pr = None
    if pairs is not None:
        pr = np.asarray(pairs)
        if pr.dtype.kind not in "iu" or pr.ndim != 2 or pr.shape[1] != 2 or not len(pr):
            raise ValueError("pairs must be a non-empty (P,2) integer array of (feature, column)")
        pr = pr.astype(np.int64)
        if F is not None and (pr.min() < 0 or pr[:, 0].max() >= F or pr[:, 1].max() >= M):
            raise ValueError("pairs must hold (feature, column) inside (%d, %d)" % (F, M))
        pr = np.ascontiguousarray(pr, dtype=np.int32)
    return (which, functionals.CODES[which], names, np.array([STAT_CODES[n] for n in names], dtype=np.int32), qs, tcode, xs, lev, pr)


def evaluate(shape, K, S, Us, which="auc", stats=("r",), q=(5, 95), transform=None, x=None, level=None, pairs=None,
             of_means=True, ctx=None, Ws=None, Vs=None, device=0, _scratch_bytes=0):
    """Run the device evaluation and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (only Us is
    uploaded); otherwise Ws (S,N,K) / Vs (S,M,T,K) are uploaded too (stateless entry point).  _scratch_bytes: a cap of the
    staging buffer for this call (0: the default; the tests force several chunks of samples with it).  Returns the dictionary
    of utils.posterior_feature_association."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    Us = check_features(Us, S, K)
    F = Us.shape[1]
    name, code, names, scodes, qs, tcode, xs, lev, pr = check_args(which, stats, q, transform, x, level, pairs, S, M, T, F)
    if int(_scratch_bytes) < 0:
        raise ValueError("_scratch_bytes must be >= 0")
    ns, nq, P = len(names), len(qs), 0 if pr is None else len(pr)
    mean, var, prob = np.zeros((ns, F, M)), np.zeros((ns, F, M)), np.zeros((ns, F, M))
    quant = np.zeros((ns, nq, F, M))
    defined, nmean = np.zeros((F, M)), np.zeros(M)
    values = np.zeros((ns, P, S)) if P else None
    om, sdx, sdy = (np.zeros((len(OF_MEANS), F, M)), np.zeros(F), np.zeros(M)) if of_means else (None, None, None)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    d = _native.dptr
    tail = (d(Us), tcode, code, d(xs), lev, ip(scodes), ns, d(qs) if nq else None, nq, ip(pr), P, d(mean), d(var),
            d(quant) if nq else None, d(prob), d(defined), d(nmean), d(values), d(om), d(sdx), d(sdy), int(_scratch_bytes))
    if Ws is None and Vs is None:
        ctx.call("btf_collect_association", int(S), int(F), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_association(int(device), int(S), N, M, T, K, int(F), d(Ws), d(Vs), *tail), lib)
    out = {"which": name, "stats": names, "nsamples": int(S), "n_mean": nmean, "defined": defined}
    for k, n in enumerate(names):
        out[n] = {"mean": mean[k], "var": var[k], "quantiles": quant[k], "prob_positive": prob[k]}
        if P:
            out[n]["values"] = values[k]
    if of_means:
        out["of_means"] = dict(zip(OF_MEANS, om))
        out["of_means"]["sd_x"], out["of_means"]["sd_y"] = sdx, sdy
    return out
