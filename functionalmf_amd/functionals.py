"""Posterior curve functionals: area under the curve, peak, level crossing, over the kept samples.

What a fit is read for is per curve and nonlinear in the whole curve over depth: the AUC of a dose-response curve (the
reference application forms the (S,N,M,T) tensor on the host for it, doseresponse/feature_importance.py:40), the dose at
which it falls through a level (IC50), how far a sampled curve is from monotone, the peak week of a flu season.  None of
them follows from per-cell summaries.  The data-sized work - the T-long sweep per (curve, sample) and the reduction of the
S values of each curve - is the HIP of csrc/btf_functionals.h (btf_posterior_functionals / btf_collect_functionals); this
module holds the host halves in plain numpy (importable without a GPU): the DEFINITION of the functionals
(`curve_functionals`), the argument checks, and `evaluate`, the one caller of the C entry points.

For one sampled curve m (T,) over depth coordinates x (T, strictly increasing; default np.linspace(0, 1, T)):
    auc        np.trapz(m, x)
    max, min   m.max(), m.min()
    argmax, argmin   x[np.argmax(m)], x[np.argmin(m)]  (first occurrence)
    rise       np.clip(np.diff(m), 0, None).sum()      (0 for a non-increasing curve)
    crossing   with d = m - level: x[0] if d[0] == 0; otherwise at the first t with d[t] * d[t+1] < 0 or d[t+1] == 0:
               x[t] + (x[t+1] - x[t]) * d[t] / (d[t] - d[t+1]); nan (undefined) if there is none
"""
import numpy as np

from ._analysis import check_q, transform_code

NAMES = ("auc", "max", "min", "argmax", "argmin", "rise", "crossing")      # index = the code of csrc/btf_functionals.h
CODES = {n: k for k, n in enumerate(NAMES)}
MAX_SAMPLES = 8192          # FUNC_MAX_S of csrc/btf_functionals.h: the S values of a curve are sorted in 64 KiB of LDS

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def default_x(T):
    return np.linspace(0.0, 1.0, int(T))


def curve_functionals(m, x=None, level=None):
    """The seven functionals of the curves m (..., T) along the last axis, in numpy: the definition the kernels are
    tested against.  Returns {name: array of m.shape[:-1]}; `crossing` only with a level."""
    m = np.asarray(m, dtype=float)
    T = m.shape[-1]
    if T < 2:
        raise ValueError("a curve needs at least two depth points")
    x = default_x(T) if x is None else np.asarray(x, dtype=float)
    if x.shape != (T,) or not np.all(np.diff(x) > 0):
        raise ValueError("x must hold T strictly increasing depth coordinates")
    out = {"auc": _trapezoid(m, x, axis=-1), "max": m.max(axis=-1), "min": m.min(axis=-1),
           "argmax": x[np.argmax(m, axis=-1)], "argmin": x[np.argmin(m, axis=-1)],
           "rise": np.clip(np.diff(m, axis=-1), 0, None).sum(axis=-1)}
    if level is not None:
        d = m - float(level)
        d0, d1 = d[..., :-1], d[..., 1:]
        hit = (d0 * d1 < 0) | (d1 == 0)
        t = np.argmax(hit, axis=-1)                            # the first such step (0 if there is none)
        a = np.take_along_axis(d0, t[..., None], axis=-1)[..., 0]
        b = np.take_along_axis(d1, t[..., None], axis=-1)[..., 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            pos = x[t] + (x[t + 1] - x[t]) * (a / (a - b))
        cross = np.where(hit.any(axis=-1), pos, np.nan)
        out["crossing"] = np.where(d[..., 0] == 0, x[0], cross)
    return out


def censored_percentile(v, q, axis=0):
    """Percentiles (numpy's linear rule) with nan = undefined counted as +inf; nan where the interpolation touches a
    non-finite order statistic.  The rule the device applies to `crossing`."""
    v = np.asarray(v, dtype=float)
    with np.errstate(invalid="ignore"):
        r = np.percentile(np.where(np.isnan(v), np.inf, v), q, axis=axis)
    return np.where(np.isfinite(r), r, np.nan)


def check_args(which, q, transform, x, level, exceed, curves, S, N, M, T):
    """Validate and normalise the arguments of posterior_functionals; raises ValueError before any device call.
    Returns (names, codes int32, transform code, qs, x, level, exceed, curves int32 (ncurves, 2) or None)."""
    if isinstance(which, str):
        which = (which,)
    names = tuple(which)
    if not names:
        raise ValueError("which must name at least one functional of %s" % (NAMES,))
    for n in names:
        if n not in CODES:
            raise ValueError("unknown functional %r (one of %s)" % (n, NAMES))
    if len(set(names)) != len(names):
        raise ValueError("which names a functional twice")
    tcode = transform_code(transform)
    if int(T) < 2:
        raise ValueError("posterior functionals need ndepth >= 2 (a curve over depth)")
    if int(S) < 1:
        raise ValueError("posterior functionals: at least one sample")
    if int(S) > MAX_SAMPLES:
        raise ValueError("posterior functionals: %d samples exceed %d (the values of a curve are sorted in LDS); thin the samples"
                         % (S, MAX_SAMPLES))
    qs = check_q(q, allow_none=True)
    xs = default_x(T) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    if xs.shape != (int(T),):
        raise ValueError("x must hold ndepth = %d depth coordinates, got shape %r" % (T, xs.shape))
    if not np.all(np.isfinite(xs)) or not np.all(np.diff(xs) > 0):
        raise ValueError("x must be finite and strictly increasing")
    if "crossing" in names:
        if level is None or not np.isfinite(float(level)):
            raise ValueError("the crossing functional needs a finite level=")
    lev = float(level) if level is not None else float("nan")
    exc = None if exceed is None else float(exceed)
    cv = None
    if curves is not None:
        cv = np.ascontiguousarray(np.asarray(curves, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        if len(cv) and (cv.min() < 0 or cv[:, 0].max() >= N or cv[:, 1].max() >= M):
            raise ValueError("curves must be (i, j) pairs inside (%d, %d)" % (N, M))
        if not len(cv):
            cv = None
    return names, np.array([CODES[n] for n in names], dtype=np.int32), tcode, qs, xs, lev, exc, cv


def evaluate(shape, K, S, which=("auc",), q=(5, 95), transform=None, x=None, level=None, exceed=None, curves=None,
             pointwise=False, ctx=None, Ws=None, Vs=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (no
    upload); otherwise Ws (S,N,K) / Vs (S,M,T,K) are uploaded (stateless entry point).  Returns {name: {"mean", "var" (N,M),
    "quantiles" (len(q),N,M), and where asked "prob_above" (N,M), "curves" (ncurves,S), "pointwise" (S,N,M); crossing:
    "defined" (N,M)}}."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    names, codes, tcode, qs, xs, lev, exc, cv = check_args(which, q, transform, x, level, exceed, curves, S, N, M, T)
    nw, nq, ncv = len(names), len(qs), 0 if cv is None else len(cv)
    mean, var = np.zeros((nw, N, M)), np.zeros((nw, N, M))
    quant = np.zeros((nw, nq, N, M)) if nq else None
    defined = np.zeros((N, M)) if "crossing" in names else None
    prob = np.zeros((nw, N, M)) if exc is not None else None
    cvals = np.zeros((nw, ncv, S)) if ncv else None
    pw = np.zeros((nw, S, N, M)) if pointwise else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    d = _native.dptr
    tail = (tcode, ip(codes), nw, d(xs), lev, exc if exc is not None else float("nan"), d(qs) if nq else None, nq, ip(cv), ncv,
            d(mean), d(var), d(quant), d(defined), d(prob), d(cvals), d(pw))
    if Ws is None and Vs is None:
        ctx.call("btf_collect_functionals", int(S), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_functionals(int(device), int(S), N, M, T, K, d(Ws), d(Vs), *tail), lib)
    out = {}
    for k, n in enumerate(names):
        r = {"mean": mean[k], "var": var[k], "quantiles": quant[k] if nq else np.zeros((0, N, M))}
        if n == "crossing":
            r["defined"] = defined
        if prob is not None:
            r["prob_above"] = prob[k]
        if ncv:
            r["curves"] = cvals[k]
        if pointwise:
            r["pointwise"] = pw[k]
        out[n] = r
    return out
