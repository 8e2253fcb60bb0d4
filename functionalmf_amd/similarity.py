"""Posterior similarity: which rows (or columns) are alike, as distances between their fitted surfaces, with neighbours.

"Which cell lines respond alike, which drugs act alike, which states' flu seasons move together" is usually answered with a
scatter of the embeddings (doseresponse/plot_embeddings.py, the PCA of Ws.mean(axis=0) at the end of flutrends/benchmark.py).
That is not a posterior quantity: W is identified only up to an invertible K x K map shared with V, and the map differs
from kept sample to kept sample.  The distance between two entities' fitted SURFACES mu = W V' is invariant under the map; it
is computed per kept sample and summarised over the samples.  The data-sized work - the K x K metric of every sample, the
distance of every (pair, sample), the sort of every neighbour group and the reductions over the samples - is the HIP of
csrc/btf_similarity.h (btf_posterior_similarity / btf_collect_similarity); this module holds the host halves in plain numpy
(importable without a GPU): the DEFINITION (`squared_distances`, `distances`, `keys`, `neighbours`, `reference`), the
argument checks, `evaluate`, the one caller of the C entry points, and `embed`, multidimensional scaling of the result.

For kept sample s let mu_ijt = w_i . v_jt, the linear predictor.  (No transform= is offered: under a non-linear transform the
distance stops being a quadratic form in the embeddings, and the surfaces themselves, (S,N,M,T), would have to be formed.)
    along="rows"   the E = N entities are the rows; entity i's surface is mu_i.. over the columns in `over` (default: all)
                   and all depths: n = len(over) * T cells.
    along="cols"   the E = M entities are the columns; entity j's surface is mu_.j. over the rows in `over` and all depths.
    metric="rms"   d2_s(e,f) = (1/n) sum_cells (mu_e - mu_f)^2, d_s = sqrt(d2_s): the root-mean-square gap between the two
                   surfaces, in the units of the linear predictor.
    metric="cosine"  d_s = 1 - <mu_e, mu_f> / sqrt(|mu_e|^2 |mu_f|^2), the ratio clamped to [-1, 1].  A surface that is
                   identically zero has cosine 0 with everything (distance 1); d_s(e,e) = 0 by definition, the zero surface
                   included: there is no undefined value anywhere.
The surfaces are linear in the embeddings, so a pair costs a small quadratic form:
    rows   Q_s = sum_{j in over, t} v_jt v_jt'   and   n d2_s(i,i') = delta' Q_s delta,          delta = w_i - w_i'
    cols   Q_s = sum_{i in over} w_i w_i'        and   n d2_s(j,j') = sum_t delta_t' Q_s delta_t,  delta_t = v_jt - v_j't
with the difference of the embeddings taken first (the expanded form g_ee + g_ff - 2 g_ef cancels and can go negative under
the root) and d2 clamped at 0: two entities with identical embeddings are at exactly 0.0, d_s(e,f) and d_s(f,e) are the same
bits, the diagonal is exactly 0.
Neighbours: the group of (s, e) is all E entities ordered by ascending key, ties to the smaller index; the key is d2 for rms
(so that no root decides a tie) and d for cosine, and e itself ranks last: `ranking.ranks` of the keys with a nan diagonal.
Over the samples the summaries are those of `ranking.summarize`: expected_rank, rank_var, p_nearest[k] = P(rank <= k).
"""
import numpy as np

from . import functionals, ranking
from ._analysis import check_q

ALONG = {"rows": 0, "cols": 1}              # the codes of csrc/btf_similarity.h
METRIC = {"rms": 0, "cosine": 1}
MAX_ENTITIES = ranking.MAX_GROUP            # SIM_MAX_E: a neighbour group is sorted in one workgroup's LDS
MAX_NEAREST = ranking.MAX_TOP               # SIM_MAX_NEAREST
MAX_SAMPLES = functionals.MAX_SAMPLES
MAX_K = 10
MAX_POINTWISE_BYTES = 1 << 30               # pointwise=True: the (S,E,E) array of distances may take this much


def _coordinates(Ws, Vs, along, over):
    """(X (S,E,TT,K) the entities' coordinates, Q (S,K,K) the metric, n the cells of a surface)."""
    Ws, Vs = np.asarray(Ws, dtype=float), np.asarray(Vs, dtype=float)
    if along not in ALONG:
        raise ValueError("along must be one of %s, not %r" % (tuple(ALONG), along))
    T = Vs.shape[2]
    if along == "rows":
        Y = Vs if over is None else Vs[:, np.asarray(over, dtype=np.int64)]
        return Ws[:, :, None, :], np.einsum("sjtk,sjtl->skl", Y, Y), Y.shape[1] * T
    Y = Ws if over is None else Ws[:, np.asarray(over, dtype=np.int64)]
    return Vs, np.einsum("sik,sil->skl", Y, Y), Y.shape[1] * T


def squared_distances(Ws, Vs, along="rows", over=None):
    """d2 (S,E,E) of the rms metric, in numpy: the difference of the embeddings first, then the form; clamped at 0."""
    X, Q, n = _coordinates(Ws, Vs, along, over)
    out = np.empty((X.shape[0], X.shape[1], X.shape[1]))
    for s in range(X.shape[0]):
        delta = X[s][:, None] - X[s][None]                                    # (E,E,TT,K)
        out[s] = np.maximum(np.einsum("eftk,eftk->ef", delta, delta @ Q[s]), 0.0) / n
    return out


def distances(Ws, Vs, along="rows", metric="rms", over=None):
    """The distances d (S,E,E) in numpy: the definition the kernels are tested against."""
    if metric not in METRIC:
        raise ValueError("metric must be one of %s, not %r" % (tuple(METRIC), metric))
    if metric == "rms":
        return np.sqrt(squared_distances(Ws, Vs, along, over))
    X, Q, _ = _coordinates(Ws, Vs, along, over)
    out = np.empty((X.shape[0], X.shape[1], X.shape[1]))
    for s in range(X.shape[0]):
        dot = np.einsum("etk,ftk->ef", X[s], X[s] @ Q[s])
        dot = np.triu(dot) + np.triu(dot, 1).T                                # one value for (e,f) and (f,e)
        nn = np.multiply.outer(np.diag(dot), np.diag(dot))
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(nn > 0, np.clip(dot / np.sqrt(nn), -1.0, 1.0), 0.0)
        out[s] = 1.0 - c
        np.fill_diagonal(out[s], 0.0)
    return out


def keys(Ws, Vs, along="rows", metric="rms", over=None):
    """What the neighbours are ordered by, (S,E,E): d2 for rms, d for cosine; nan on the diagonal (e itself ranks last)."""
    k = squared_distances(Ws, Vs, along, over) if metric == "rms" else distances(Ws, Vs, along, metric, over)
    k[:, np.arange(k.shape[1]), np.arange(k.shape[1])] = np.nan
    return k


def neighbours(key, nearest=(1, 5)):
    """(expected_rank (E,E), rank_var (E,E), p_nearest (len(nearest),E,E)) of the keys (S,E,E) with a nan diagonal."""
    return ranking.summarize(ranking.ranks(key, "cols", "ascending"), nearest)


def summarize(d, q=(5, 95)):
    """(mean, var (ddof 1; nan for a single sample), quantiles (len(q),E,E)) of the distances d (S,E,E)."""
    d = np.asarray(d, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = d.var(axis=0, ddof=1) if d.shape[0] > 1 else np.full(d.shape[1:], np.nan)
    return d.mean(axis=0), var, np.percentile(d, np.atleast_1d(q), axis=0)


def reference(Ws, Vs, along="rows", metric="rms", over=None, q=(5, 95), nearest=(1, 5), pairs=None, pointwise=False):
    """The dictionary posterior_similarity returns, in numpy."""
    d = distances(Ws, Vs, along, metric, over)
    mean, var, quant = summarize(d, q)
    e, v, p = neighbours(keys(Ws, Vs, along, metric, over), nearest)
    T = np.asarray(Vs).shape[2]
    nover = (np.asarray(Vs).shape[1] if along == "rows" else np.asarray(Ws).shape[1]) if over is None else len(over)
    out = {"mean": mean, "var": var, "quantiles": quant, "expected_rank": e, "rank_var": v, "p_nearest": p, "along": along,
           "metric": metric, "nearest": tuple(int(k) for k in nearest), "nsamples": int(d.shape[0]), "ncells": int(nover * T)}
    if pairs is not None:
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        out["pair_values"] = d[:, pr[:, 0], pr[:, 1]]
    if pointwise:
        out["distances"] = d
    return out


def embed(out, dims=2):
    """Classical multidimensional scaling of a posterior_similarity result (metric="rms"): (coordinates (E,dims), share).

    The posterior mean of d2 is mean**2 + var * (S - 1) / S (the second moment of d over the samples); it is double-centred,
    B = -J D2 J / 2, and the coordinates are the eigenvectors of the `dims` largest non-negative eigenvalues of B scaled by
    their roots (numpy.linalg.eigh).  share: the part of the trace of B those eigenvalues carry.  The sound form of the
    reference's embedding scatter: the configuration is fixed up to a rigid motion, whatever map each sample's W carries."""
    mean, S = np.asarray(out["mean"], dtype=float), int(out["nsamples"])
    d2 = mean ** 2
    if S > 1:
        d2 = d2 + np.asarray(out["var"], dtype=float) * (S - 1) / S
    E = d2.shape[0]
    dims = int(dims)
    if not 1 <= dims <= E:
        raise ValueError("dims must lie in 1..%d" % E)
    J = np.eye(E) - 1.0 / E
    B = -0.5 * J @ ((d2 + d2.T) / 2) @ J
    lam, vec = np.linalg.eigh((B + B.T) / 2)
    top = np.argsort(lam)[::-1][:dims]
    l = np.maximum(lam[top], 0.0)
    trace = np.maximum(lam, 0.0).sum()
    return vec[:, top] * np.sqrt(l), (float(l.sum() / trace) if trace > 0 else 1.0)


def check_args(along, metric, over, q, nearest, pairs, pointwise, S, N, M, T, K):
    """Validate and normalise the arguments of posterior_similarity; raises ValueError before any device call.
    Returns (along code, metric code, over int32 or None, q, nearest as given (tuple), nearest int32 for the device,
    pairs int32 (P,2) or None, E, ncells)."""
    if not isinstance(along, str) or along not in ALONG:
        raise ValueError("along must be one of %s, not %r" % (tuple(ALONG), along))
    if not isinstance(metric, str) or metric not in METRIC:
        raise ValueError("metric must be one of %s, not %r" % (tuple(METRIC), metric))
    E, YN = (int(N), int(M)) if along == "rows" else (int(M), int(N))
    ov = None
    if over is not None:
        ov = np.atleast_1d(np.asarray(over))
        if ov.ndim != 1 or ov.dtype.kind not in "iu" or ov.size < 1 or ov.min() < 0 or ov.max() >= YN or len(set(ov.tolist())) != ov.size:
            raise ValueError("over must hold distinct integer indices in 0..%d, at least one, got %r" % (YN - 1, over))
        ov = np.ascontiguousarray(ov, dtype=np.int32)
    qs = check_q(q)
    tp = np.atleast_1d(np.asarray(nearest))
    if tp.ndim != 1 or tp.dtype.kind not in "iu" or not 1 <= tp.size <= MAX_NEAREST or tp.min() < 1 or len(set(tp.tolist())) != tp.size:
        raise ValueError("nearest must hold 1 to %d distinct integers >= 1, got %r" % (MAX_NEAREST, nearest))
    pr = None
    if pairs is not None:
        pr = np.asarray(pairs)
        if pr.dtype.kind not in "iu" or pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be a (P,2) integer array of (e, f)")
        if len(pr) and (pr.min() < 0 or pr.max() >= E):
            raise ValueError("pairs must hold (e, f) with both inside 0..%d" % (E - 1))
        pr = np.ascontiguousarray(pr, dtype=np.int32)
    if not 1 <= int(K) <= MAX_K:
        raise ValueError("posterior similarity: nembeds must lie in 1..%d, got %d" % (MAX_K, K))
    if int(S) < 1:
        raise ValueError("posterior similarity: at least one sample")
    if int(S) > MAX_SAMPLES:
        raise ValueError("posterior similarity: %d samples exceed %d; thin the samples" % (S, MAX_SAMPLES))
    if E > MAX_ENTITIES:
        raise ValueError("posterior similarity: %d entities along %r exceed %d (a neighbour group is sorted in LDS)"
                         % (E, along, MAX_ENTITIES))
    if pointwise and int(S) * E * E * 8 > MAX_POINTWISE_BYTES:
        raise ValueError("posterior similarity: pointwise=True would return %d bytes of distances, above the limit of %d; "
                         "ask for the pairs you need with pairs=" % (int(S) * E * E * 8, MAX_POINTWISE_BYTES))
    # entries above MAX_ENTITIES are certain whatever their value: distinct stand-ins, as ranking.check_args
    big = np.array([int(k) > MAX_ENTITIES for k in tp.tolist()])
    tdev = np.where(big, MAX_ENTITIES + np.cumsum(big), np.where(big, 0, tp)).astype(np.int32)
    ncells = (YN if ov is None else int(ov.size)) * int(T)
    return (ALONG[along], METRIC[metric], ov, qs, tuple(int(k) for k in tp.tolist()), np.ascontiguousarray(tdev), pr, E, ncells)


def evaluate(shape, K, S, along="rows", metric="rms", over=None, q=(5, 95), nearest=(1, 5), pairs=None, pointwise=False,
             ctx=None, Ws=None, Vs=None, device=0, _scratch_bytes=0):
    """Run the device evaluation and unpack it.  ctx with Ws = Vs = None: the context's first S collected samples (no
    upload); otherwise Ws (S,N,K) / Vs (S,M,T,K) are uploaded (stateless entry point).  _scratch_bytes: a cap of the staging
    buffer for this call (0: the default; the tests force several tiles of entities with it).  Returns the dictionary of
    utils.posterior_similarity."""
    import ctypes as C
    from . import _native
    N, M, T = shape
    acode, mcode, ov, qs, near, tdev, pr, E, ncells = check_args(along, metric, over, q, nearest, pairs, pointwise, S, N, M, T, K)
    if int(_scratch_bytes) < 0:
        raise ValueError("_scratch_bytes must be >= 0")
    nq, ntop, P = len(qs), len(tdev), 0 if pr is None else len(pr)
    mean, var, quant = np.zeros((E, E)), np.zeros((E, E)), np.zeros((nq, E, E))
    expected, rvar, pnear = np.zeros((E, E)), np.zeros((E, E)), np.zeros((ntop, E, E))
    pv = np.zeros((S, P)) if pr is not None else None
    dist = np.zeros((S, E, E)) if pointwise else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    d = _native.dptr
    tail = (acode, mcode, ip(ov), 0 if ov is None else len(ov), d(qs) if nq else None, nq, ip(tdev), ntop, ip(pr) if P else None, P,
            d(mean), d(var), d(quant) if nq else None, d(expected), d(rvar), d(pnear), d(pv) if P else None, d(dist),
            int(_scratch_bytes))
    if Ws is None and Vs is None:
        ctx.call("btf_collect_similarity", int(S), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_posterior_similarity(int(device), int(S), N, M, T, K, d(Ws), d(Vs), *tail), lib)
    out = {"mean": mean, "var": var, "quantiles": quant, "expected_rank": expected, "rank_var": rvar, "p_nearest": pnear,
           "along": along, "metric": metric, "nearest": near, "nsamples": int(S), "ncells": int(ncells)}
    if pr is not None:
        out["pair_values"] = pv
    if pointwise:
        out["distances"] = dist
    return out
