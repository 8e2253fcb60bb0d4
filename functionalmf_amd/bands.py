"""Simultaneous credible bands per curve: a band that holds the WHOLE fitted curve with the nominal probability.

The percentiles of posterior_summary and the band of posterior_predictive are pointwise: each cell's interval holds that
cell's value with probability level / 100, and the curve as a whole leaves the band somewhere far more often.  What is drawn
around a dose-response curve or a flu season should answer "does the whole curve lie in here with 95 % probability".  The
data-sized work - S N M T values, a sort over the S samples per curve or per cell - is the HIP of csrc/btf_bands.h
(btf_posterior_bands / btf_collect_bands); this module holds the host halves in plain numpy (importable without a GPU): the
DEFINITION of the two bands (`supt_band`, `rank_band`), the argument checks, and `evaluate`, the one caller of the C entry
points.

With m_s(t) = f(w_i^s . v_jt^s) the S kept curves of one (i,j), `depths` the depths the band is simultaneous over (default
all) and need = ceil(level / 100 * S):

    supt   center, scale = mean and sd (ddof 1) over s per cell; D_s = max over the used depths with scale > 0 of
           |m_s - center| / scale (0 if there is none); crit = np.sort(D)[need - 1], an order statistic; the band is
           center -+ crit * scale at every depth; inside = share of samples with D_s <= crit.
    rank   distribution-free, for ilogit curves near 0 or 1.  Per cell lo_s = #{s' : m_s' < m_s}, hi_s = #{s' : m_s' > m_s};
           depth_s = min over the used depths of min(lo_s, hi_s); k = the largest integer with #{s : depth_s >= k} >= need;
           the band is the k-th and the (S-1-k)-th order statistic (0-based) of every cell; inside = #{s : depth_s >= k} / S;
           pointwise_inside = the same with k_pw = floor((1 - level / 100) / 2 * S): the share of kept curves wholly inside
           the pointwise band of the same nominal level.

Either way at least `need` of the S kept curves lie wholly inside the band over the used depths, by construction.
"""
import numpy as np

from ._analysis import transform_code

METHODS = {"supt": 0, "rank": 1}                  # the method codes of csrc/btf_bands.h
MAX_SAMPLES = {"supt": 8192,                      # FUNC_MAX_S of csrc/btf_functionals.h: a curve's D_s are sorted in 64 KiB of LDS
               "rank": 4096}                      # BAND_RANK_MAX_S of csrc/btf_bands.h: key, sample index and depth, 16 B a sample


def need_of(level, S):
    """The number of kept curves the band must hold: ceil(level / 100 * S)."""
    return int(np.ceil(float(level) / 100.0 * int(S)))


def pointwise_k(level, S):
    """k_pw = floor((1 - level / 100) / 2 * S): the order statistics k_pw and S-1-k_pw are the pointwise band."""
    return int(np.floor((1.0 - float(level) / 100.0) / 2.0 * int(S)))


def _used(depths, T):
    use = np.ones(T, dtype=bool) if depths is None else np.asarray(depths)
    if use.dtype != bool or use.shape != (T,):
        raise ValueError("depths must be a boolean mask of the ndepth = %d depths, got %s %r" % (T, use.dtype, use.shape))
    if not use.any():
        raise ValueError("depths selects no depth: the band must be simultaneous over at least one")
    return use


def _check_curves_level(m, level):
    m = np.asarray(m, dtype=float)
    if m.ndim < 2 or m.shape[0] < 2 or m.shape[-1] < 1:
        raise ValueError("m must be (S, ..., T) with S >= 2 sampled curves of T >= 1 depths")
    if not 0.0 < float(level) < 100.0:
        raise ValueError("level must lie in (0, 100)")
    return m


def supt_band(m, level=95, depths=None):
    """The sup-t band of the sampled curves m (S, ..., T) in numpy: the definition the kernels are tested against.
    Returns center, scale, lower, upper (..., T); crit, inside (...); stat (S, ...) = D_s; need."""
    m = _check_curves_level(m, level)
    S, T = m.shape[0], m.shape[-1]
    use, need = _used(depths, T), need_of(level, S)
    center, scale = m.mean(axis=0), m.std(axis=0, ddof=1)
    ok = use & (scale > 0)
    D = np.where(ok, np.abs(m - center) / np.where(ok, scale, 1.0), 0.0).max(axis=-1)
    crit = np.sort(D, axis=0)[need - 1]
    half = crit[..., None] * scale
    return {"center": center, "scale": scale, "lower": center - half, "upper": center + half, "crit": crit,
            "inside": (D <= crit).sum(axis=0) / S, "stat": D, "need": need}


def strict_counts(m):
    """(lo, hi) of the samples m (S, ...) along axis 0: lo_s = #{s' : m_s' < m_s}, hi_s = #{s' : m_s' > m_s}."""
    m = np.asarray(m, dtype=float)
    S = m.shape[0]
    order = np.argsort(m, axis=0, kind="stable")
    sv = np.take_along_axis(m, order, axis=0)
    pos = np.arange(S).reshape((S,) + (1,) * (m.ndim - 1))
    new = np.ones(m.shape, dtype=bool)
    new[1:] = sv[1:] != sv[:-1]                                    # a run of equal values starts here
    first = np.maximum.accumulate(np.where(new, pos, 0), axis=0)   # the start of each position's run
    end = np.ones(m.shape, dtype=bool)
    end[:-1] = new[1:]
    last = np.minimum.accumulate(np.where(end, pos, S - 1)[::-1], axis=0)[::-1]
    lo, hi = np.empty(m.shape, dtype=np.int64), np.empty(m.shape, dtype=np.int64)
    np.put_along_axis(lo, order, first, axis=0)
    np.put_along_axis(hi, order, S - 1 - last, axis=0)
    return lo, hi


def rank_band(m, level=95, depths=None):
    """The rank (depth) band of the sampled curves m (S, ..., T) in numpy: the definition the kernels are tested against.
    Returns lower, upper (..., T); k (int), inside, pointwise_inside (...); stat (S, ...) = depth_s (int); need, k_pointwise."""
    m = _check_curves_level(m, level)
    S, T = m.shape[0], m.shape[-1]
    use, need, kpw = _used(depths, T), need_of(level, S), pointwise_k(level, S)
    lo, hi = strict_counts(m)
    depth = np.minimum(lo, hi)[..., use].min(axis=-1)
    k = np.sort(depth, axis=0)[S - need]               # the need-th largest: #{depth >= k} >= need, and no larger k does
    srt = np.sort(m, axis=0)
    kk = np.broadcast_to(k[None, ..., None], (1,) + m.shape[1:])
    lower = np.take_along_axis(srt, kk, axis=0)[0]
    upper = np.take_along_axis(srt, S - 1 - kk, axis=0)[0]
    return {"lower": lower, "upper": upper, "k": k, "inside": (depth >= k).sum(axis=0) / S,
            "pointwise_inside": (depth >= kpw).sum(axis=0) / S, "stat": depth, "need": need, "k_pointwise": kpw}


def coverage(lower, upper, truth, depths=None):
    """Whether the band holds the known curve: covered (...) = 1 if lower <= truth <= upper at every used depth where truth
    is known, 0 if not, nan where no used depth is known; coverage = the mean of covered over the curves that are not nan
    (nan if there is none).  truth (..., T), NaN = unknown."""
    lower, upper = np.asarray(lower, dtype=float), np.asarray(upper, dtype=float)
    truth = np.asarray(truth, dtype=float)
    if truth.shape != lower.shape:
        raise ValueError("truth must have the band's shape %r, got %r" % (lower.shape, truth.shape))
    known = _used(depths, lower.shape[-1]) & ~np.isnan(truth)
    with np.errstate(invalid="ignore"):
        out = known & ((truth < lower) | (truth > upper))
    covered = np.where(known.any(axis=-1), 1.0 - out.any(axis=-1), np.nan)
    seen = ~np.isnan(covered)
    return covered, float(covered[seen].mean()) if seen.any() else float("nan")


def check_args(method, level, depths, transform, curves, truth, S, N, M, T):
    """Validate and normalise the arguments of posterior_bands; raises ValueError before any device call.
    Returns (method code, level, depth flags int32 (T,), transform code, curves int32 (ncurves, 2) or None, truth or None)."""
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError("unknown method %r (one of %s)" % (method, tuple(METHODS)))
    tcode = transform_code(transform)
    try:
        lev = float(level)
    except (TypeError, ValueError):
        raise ValueError("level must be a number in (0, 100)")
    if not 0.0 < lev < 100.0:
        raise ValueError("level must lie in (0, 100), got %r" % (level,))
    if int(T) < 1:
        raise ValueError("posterior bands need ndepth >= 1")
    if int(S) < 2:
        raise ValueError("posterior bands need at least two samples")
    if int(S) > MAX_SAMPLES[method]:
        raise ValueError("posterior bands: %d samples exceed %d for method %r (the values of a curve are sorted in LDS); thin the samples"
                         % (S, MAX_SAMPLES[method], method))
    use = _used(depths, int(T))
    cv = None
    if curves is not None:
        cv = np.ascontiguousarray(np.asarray(curves, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        if len(cv) and (cv.min() < 0 or cv[:, 0].max() >= N or cv[:, 1].max() >= M):
            raise ValueError("curves must be (i, j) pairs inside (%d, %d)" % (N, M))
        if not len(cv):
            cv = None
    if truth is not None:
        truth = np.asarray(truth, dtype=float)
        if truth.shape != (N, M, T):
            raise ValueError("truth must be (%d, %d, %d), got %r" % (N, M, T, truth.shape))
    return METHODS[method], lev, np.ascontiguousarray(use, dtype=np.int32), tcode, cv, truth


def evaluate(shape, K, S, method="supt", level=95, depths=None, transform=None, curves=None, truth=None, ctx=None, Ws=None,
             Vs=None, device=0, _scratch_bytes=0):
    """Run the device evaluation and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (no
    upload); otherwise Ws (S,N,K) / Vs (S,M,T,K) are uploaded (stateless entry point).  Returns a dict: lower, upper (N,M,T),
    inside (N,M), method, level, need, nsamples; supt: center, scale (N,M,T), crit (N,M); rank: k (N,M) int,
    pointwise_inside (N,M), k_pointwise; with curves "stat" (ncurves,S); with truth "covered" (N,M) and "coverage"."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    mcode, lev, use, tcode, cv, truth = check_args(method, level, depths, transform, curves, truth, S, N, M, T)
    supt = method == "supt"
    ncv = 0 if cv is None else len(cv)
    lower, upper = np.zeros((N, M, T)), np.zeros((N, M, T))
    center, scale = (np.zeros((N, M, T)), np.zeros((N, M, T))) if supt else (None, None)
    crit, inside = np.zeros((N, M)), np.zeros((N, M))
    pw = None if supt else np.zeros((N, M))
    stat = np.zeros((ncv, S)) if ncv else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    d = _native.dptr
    tail = (tcode, mcode, lev, ip(use), ip(cv), ncv, d(center), d(scale), d(lower), d(upper), d(crit), d(inside), d(pw), d(stat),
            int(_scratch_bytes))
    if Ws is None and Vs is None:
        ctx.call("btf_collect_bands", int(S), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_bands(int(device), int(S), N, M, T, K, d(Ws), d(Vs), *tail), lib)
    out = {"method": method, "level": lev, "need": need_of(lev, S), "nsamples": int(S), "lower": lower, "upper": upper,
           "inside": inside}
    if supt:
        out.update(center=center, scale=scale, crit=crit)
    else:
        out.update(k=crit.astype(np.int64), pointwise_inside=pw, k_pointwise=pointwise_k(lev, S))
    if ncv:
        out["stat"] = stat if supt else stat.astype(np.int64)
    if truth is not None:
        out["covered"], out["coverage"] = coverage(lower, upper, truth, use.astype(bool))
    return out
