"""Monotone projection of the posterior: every kept sample's V through factor_pav, and the summary of the projected curves.

The dose-response application projects its posterior to monotone curves before it reports anything
(doseresponse/fit.py:365-374): factor_pav(W_s, V_s[j]) for every kept sample s and column j, then the mean and the 5 % / 95 %
curves of the projected W V', and the projected samples themselves (btf_mono.npy, what select_btf.py scores).  The data-sized
work - the S x M independent projections and the summary of the projected states - is the HIP of csrc/btf_monotone.h
(btf_posterior_monotone / btf_collect_monotone); this module holds the host halves in plain numpy (importable without a
GPU): the DEFINITION (`project_host`), the argument checks, and `evaluate`, the one caller of the C entry points.

The projection of one column block V (T,K) under W (N,K), decreasing (the reference's direction):
    every depth starts as a pool of its own.  A sweep visits the pairs (t, t+1) from t = 0.  The pair violates when
    w_i . v_t - w_i . v_{t+1} < 0 for ANY row i.  A violation merges the pool of t (w0 depths) and the pool of t+1 (w1 depths):
    every depth of both becomes (w0 v_t + w1 v_{t+1}) / (w0 + w1), and the sweep goes on at the merged pool's last depth,
    t + w1; otherwise it goes on at t + 1.  Sweeps repeat until one merges nothing.
increasing=True is the same with the difference taken the other way round, which is -project(W, -V) exactly.  W is never
changed.  pools = T minus the merges made: T says the block was monotone already.
"""
import numpy as np

from ._analysis import check_q, transform_code

MAX_SUMMARY_SAMPLES = 16384                 # the summary kernel sorts a cell's values in LDS
LDS_BYTES = 64 * 1024                       # a column block and one word per depth: pav_fits of csrc/btf_nmf.hip
MAX_K = 10


def pav_fits(T, K):
    """Whether a (T,K) column block fits the PAV kernels' LDS: 8 T K + 4 T <= 65536 bytes."""
    return 8 * int(T) * int(K) + 4 * int(T) <= LDS_BYTES


def _project_block(W, V, increasing):
    """One column block V (T,K) under W (N,K): (projected copy, number of merges)."""
    V = np.array(V, dtype=np.float64)
    T = V.shape[0]
    first = np.arange(T)                     # the first depth of every depth's pool
    merges = 0
    while True:
        merged_in_sweep = False
        t = 0
        while t < T - 1:
            left, right = W @ V[t], W @ V[t + 1]
            step = (right - left) if increasing else (left - right)
            if np.any(step < 0):
                mine, next_ = first == first[t], first == first[t + 1]
                w0, w1 = int(mine.sum()), int(next_.sum())
                V[mine | next_] = (w0 * V[t] + w1 * V[t + 1]) / (w0 + w1)
                first[next_] = first[t]
                merges += 1
                merged_in_sweep = True
                t += w1
            else:
                t += 1
        if not merged_in_sweep:
            return V, merges


def project_host(Ws, Vs, increasing=False):
    """(V' (S,M,T,K), pools (S,M) int32) of Ws (S,N,K) and Vs (S,M,T,K) in numpy: the definition the kernel is tested
    against.  A host loop over S x M blocks - for checks, not for work."""
    Ws, Vs = np.asarray(Ws, dtype=np.float64), np.asarray(Vs, dtype=np.float64)
    if Ws.ndim != 3 or Vs.ndim != 4 or Ws.shape[0] != Vs.shape[0] or Ws.shape[2] != Vs.shape[3]:
        raise ValueError("Ws must be (S,N,K) and Vs (S,M,T,K), got %r / %r" % (Ws.shape, Vs.shape))
    S, M, T, _ = Vs.shape
    out = np.empty_like(Vs)
    pools = np.empty((S, M), dtype=np.int32)
    for s in range(S):
        for j in range(M):
            out[s, j], merges = _project_block(Ws[s], Vs[s, j], bool(increasing))
            pools[s, j] = T - merges
    return out, pools


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be True or False, not %r" % (name, v))
    return bool(v)


def check_args(q, transform, increasing, return_V, in_place, T, K, uploaded=False):
    """Validate and normalise the arguments of posterior_monotone; raises ValueError before any device call.
    Returns (percentiles or None when there is no summary, transform code, increasing, return_V, in_place)."""
    qs = None if q is None else check_q(q)
    tcode = transform_code(transform)
    inc, ret, inp = _flag("increasing", increasing), _flag("return_V", return_V), _flag("in_place", in_place)
    if inp and uploaded:
        raise ValueError("in_place=True projects the samples collected on the device: it cannot be combined with results=")
    if not 1 <= int(K) <= MAX_K:
        raise ValueError("posterior monotone: nembeds must be 1..%d" % MAX_K)
    if not pav_fits(T, K):
        raise ValueError("posterior monotone: ndepth * nembeds = %d * %d exceeds the PAV kernels' LDS bound (pav_fits: "
                         "8 T K + 4 T <= %d bytes)" % (T, K, LDS_BYTES))
    return qs, tcode, inc, ret, inp


def evaluate(shape, K, S, q=(5, 95), transform=None, increasing=False, return_V=False, in_place=False, ctx=None, Ws=None,
             Vs=None, device=0):
    """Run the device projection and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (no
    upload; in_place overwrites their V); ctx with Ws / Vs: those states, uploaded on the context's device; no ctx: the
    stateless entry point.  Returns the dictionary of utils.posterior_monotone."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    uploaded = Ws is not None or Vs is not None
    qs, tcode, inc, ret, inp = check_args(q, transform, increasing, return_V, in_place, T, K, uploaded=uploaded or ctx is None)
    if int(S) < 1:
        raise ValueError("posterior monotone: at least one sample")
    if qs is not None and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("posterior monotone: %d samples exceed %d with a summary; pass q=None or thin the samples"
                         % (S, MAX_SUMMARY_SAMPLES))
    pools = np.zeros((S, M), dtype=np.int32)
    Vout = np.zeros((S, M, T, K)) if ret else None
    mean = quant = None
    if qs is not None:
        mean, quant = np.zeros((N, M, T)), np.zeros((len(qs), N, M, T))
    d = _native.dptr
    tail = (tcode, d(qs) if qs is not None and len(qs) else None, 0 if qs is None else len(qs), d(Vout),
            pools.ctypes.data_as(C.POINTER(C.c_int32)), d(mean), d(quant) if qs is not None and len(qs) else None)
    if ctx is not None:
        ctx.call("btf_collect_monotone", int(S), d(Ws), d(Vs), int(inc), int(inp), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_monotone(int(device), int(S), N, M, T, K, d(Ws), d(Vs), int(inc), *tail), lib)
    out = {"pools": pools, "changed": (pools < T).mean(axis=0), "nsamples": int(S)}
    if qs is not None:
        out["mean"], out["quantiles"] = mean, quant
    if ret:
        out["V"] = Vout
    return out
