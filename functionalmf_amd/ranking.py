"""Posterior ranking: which column is best for a row (or which row for a column), and with what probability.

What a dose-response or flu fit is read for is comparative: which drug has the lowest AUC for this cell line, which reaches
the IC50 at the lowest dose, which state peaks first.  That is a property of the JOINT posterior across curves - a drug whose
AUC mean is lowest may be best in only 30 % of the samples - so the per-curve means and bands of posterior_functionals cannot
give it.  The data-sized work - the functional of every (curve, sample), the sort of every group of every sample and the
integer sums over the samples - is the HIP of csrc/btf_ranking.h (btf_posterior_ranking / btf_collect_ranking); this module
holds the host halves in plain numpy (importable without a GPU): the DEFINITION (`ranks`, `summarize`, `pair_probabilities`,
`reference`), the argument checks, and `evaluate`, the one caller of the C entry points.

Let f_s(i,j) be one functional of functionals.py for kept sample s and curve (i,j).  along="cols" ranks the M columns within
each row i (a group is (s, i), L = M members), along="rows" the N rows within each column j (L = N).  Within a group
    order="ascending":   rank = 1 + #{members with a smaller value} + #{members with an equal value and a smaller index}
                         = 1 + the member's position in np.argsort(values, kind="stable")
    order="descending":  "smaller value" becomes "larger value"; ties still go to the smaller index
    an undefined value (nan: a crossing that never happens) ranks after every defined value in both orders; undefined
    members are ordered among themselves by index.
With r_s(i,j) the rank and the integer sums A = sum_s r_s, B = sum_s r_s^2, C_k = #{s : r_s <= k}:
    expected_rank = A / S       rank_var = (S B - A A) / (S (S - 1))  (0 when S = 1)       p_top[k] = C_k / S
Numerator and denominator of rank_var are exact 64-bit integers (L <= 4096 and S <= 8192 keep them below 2^53) and one
fp64 division follows, so the device and this module agree exactly given the same f values.
"""
import numpy as np

from . import functionals
from ._analysis import transform_code

ALONG = {"cols": 0, "rows": 1}              # the code of csrc/btf_ranking.h
ORDER = {"ascending": 0, "descending": 1}
MAX_GROUP = 4096                            # RANK_MAX_L of csrc/btf_ranking.h: a group is sorted in one workgroup's LDS
MAX_TOP = 8                                 # RANK_MAX_TOP
MAX_SAMPLES = functionals.MAX_SAMPLES


def ranks(f, along="cols", order="ascending"):
    """The ranks (S,N,M) int64 of the values f (S,N,M) within every group, in numpy: the definition the kernels are tested
    against."""
    f = np.asarray(f, dtype=float)
    if f.ndim != 3:
        raise ValueError("f must be (S,N,M)")
    if along not in ALONG or order not in ORDER:
        raise ValueError("along must be one of %s and order one of %s" % (tuple(ALONG), tuple(ORDER)))
    axis = 2 if along == "cols" else 1
    undefined = np.isnan(f)
    key = np.where(undefined, 0.0, f if order == "ascending" else -f) + 0.0          # (+ 0.0: -0 and +0 are one value)
    pos = np.lexsort((key, undefined), axis=axis)         # stable: by undefined, then value, then index
    L = f.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = L
    r = np.empty(f.shape, dtype=np.int64)
    np.put_along_axis(r, pos, np.arange(1, L + 1, dtype=np.int64).reshape(shape), axis=axis)
    return r


def summarize(r, top=(1, 5)):
    """(expected_rank (N,M), rank_var (N,M), p_top (len(top),N,M)) of the ranks r (S,N,M): integer sums, one division each."""
    r = np.asarray(r, dtype=np.int64)
    S = r.shape[0]
    A, B = r.sum(0), (r * r).sum(0)
    var = (S * B - A * A).astype(np.float64) / float(S * (S - 1)) if S > 1 else np.zeros(A.shape)
    p_top = np.stack([(r <= int(k)).sum(0).astype(np.float64) / float(S) for k in top])
    return A.astype(np.float64) / float(S), var, p_top


def pair_probabilities(f, pairs):
    """(prob_less, prob_defined), each (P,), of the values f (S,N,M) and the (P,4) pairs (i, j, i2, j2): the share of samples
    with f(i,j) < f(i2,j2), and with both defined; a sample with an undefined value counts for neither."""
    f = np.asarray(f, dtype=float)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    a, b = f[:, p[:, 0], p[:, 1]], f[:, p[:, 2], p[:, 3]]
    ok = ~(np.isnan(a) | np.isnan(b))
    with np.errstate(invalid="ignore"):
        less = ok & (a < b)
    S = float(f.shape[0])
    return less.sum(0) / S, ok.sum(0) / S


def reference(f, which="auc", along="cols", order="ascending", top=(1, 5), pairs=None, pointwise=False):
    """The dictionary posterior_ranking returns, from the values f (S,N,M) in numpy."""
    r = ranks(f, along, order)
    e, v, p = summarize(r, top)
    out = {"expected_rank": e, "rank_var": v, "p_top": p, "top": tuple(int(k) for k in top), "along": along, "order": order,
           "which": which, "nsamples": int(r.shape[0])}
    if pointwise:
        out["ranks"] = r.astype(np.int32)
    if pairs is not None:
        out["prob_less"], out["prob_defined"] = pair_probabilities(f, pairs)
    return out


def check_args(which, along, order, top, transform, x, level, pairs, S, N, M, T):
    """Validate and normalise the arguments of posterior_ranking; raises ValueError before any device call.
    Returns (name, functional code, along code, order code, top int32, transform code, x, level, pairs int32 (P,4) or None)."""
    if not isinstance(which, str) or which not in functionals.CODES:
        raise ValueError("unknown functional %r (one of %s)" % (which, functionals.NAMES))
    if not isinstance(along, str) or along not in ALONG:
        raise ValueError("along must be one of %s, not %r" % (tuple(ALONG), along))
    if not isinstance(order, str) or order not in ORDER:
        raise ValueError("order must be one of %s, not %r" % (tuple(ORDER), order))
    tp = np.atleast_1d(np.asarray(top))
    if tp.ndim != 1 or tp.dtype.kind not in "iu" or not 1 <= tp.size <= MAX_TOP or tp.min() < 1 or len(set(tp.tolist())) != tp.size:
        raise ValueError("top must hold 1 to %d distinct integers >= 1, got %r" % (MAX_TOP, top))
    tcode = transform_code(transform)
    if int(T) < 2:
        raise ValueError("posterior ranking needs ndepth >= 2 (a curve over depth)")
    if int(S) < 1:
        raise ValueError("posterior ranking: at least one sample")
    if int(S) > MAX_SAMPLES:
        raise ValueError("posterior ranking: %d samples exceed %d; thin the samples" % (S, MAX_SAMPLES))
    L = int(N) if along == "rows" else int(M)
    if L > MAX_GROUP:
        raise ValueError("posterior ranking: a group of %d members along %r exceeds %d (a group is sorted in LDS)"
                         % (L, along, MAX_GROUP))
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
        if pr.dtype.kind not in "iu" or pr.ndim != 2 or pr.shape[1] != 4:
            raise ValueError("pairs must be a (P,4) integer array of (i, j, i2, j2)")
        pr = pr.astype(np.int64)
        if len(pr) and (pr.min() < 0 or pr[:, ::2].max() >= N or pr[:, 1::2].max() >= M):
            raise ValueError("pairs must hold (i, j, i2, j2) with curves inside (%d, %d)" % (N, M))
        pr = np.ascontiguousarray(pr, dtype=np.int32)
    # every entry above MAX_GROUP is certain whatever its value: the device gets distinct stand-ins above MAX_GROUP for them
    # (the library refuses repeated entries, and an entry need not fit 32 bits)
    big = np.array([int(k) > MAX_GROUP for k in tp.tolist()])
    tdev = np.where(big, MAX_GROUP + np.cumsum(big), np.where(big, 0, tp)).astype(np.int32)
    return (which, functionals.CODES[which], ALONG[along], ORDER[order], np.ascontiguousarray(tdev), tcode, xs, lev, pr)


def evaluate(shape, K, S, which="auc", along="cols", order="ascending", top=(1, 5), transform=None, x=None, level=None,
             pairs=None, pointwise=False, ctx=None, Ws=None, Vs=None, device=0, _scratch_bytes=0):
    """Run the device evaluation and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (no
    upload); otherwise Ws (S,N,K) / Vs (S,M,T,K) are uploaded (stateless entry point).  _scratch_bytes: a cap of the staging
    buffer for this call (0: the default; the tests force several chunks of samples with it).  Returns the dictionary of
    utils.posterior_ranking."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    name, code, acode, ocode, tp, tcode, xs, lev, pr = check_args(which, along, order, top, transform, x, level, pairs, S, N, M, T)
    if int(_scratch_bytes) < 0:
        raise ValueError("_scratch_bytes must be >= 0")
    ntop, P = len(tp), 0 if pr is None else len(pr)
    expected, var, ptop = np.zeros((N, M)), np.zeros((N, M)), np.zeros((ntop, N, M))
    rk = np.zeros((S, N, M), dtype=np.int32) if pointwise else None
    less, defined = (np.zeros(P), np.zeros(P)) if pr is not None else (None, None)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    d = _native.dptr
    tail = (tcode, code, d(xs), lev, acode, ocode, ip(tp), ntop, ip(pr) if P else None, P, d(expected), d(var), d(ptop), ip(rk),
            d(less) if P else None, d(defined) if P else None, int(_scratch_bytes))
    if Ws is None and Vs is None:
        ctx.call("btf_collect_ranking", int(S), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_ranking(int(device), int(S), N, M, T, K, d(Ws), d(Vs), *tail), lib)
    out = {"expected_rank": expected, "rank_var": var, "p_top": ptop, "top": tuple(int(k) for k in np.atleast_1d(np.asarray(top))),
           "along": along, "order": order, "which": name, "nsamples": int(S)}
    if pointwise:
        out["ranks"] = rk
    if pr is not None:
        out["prob_less"], out["prob_defined"] = less, defined
    return out
