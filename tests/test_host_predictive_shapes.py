"""The case lists of tests/test_gpu_predictive_shapes.py, their inputs and numpy references, on the CPU alone.

The predictive kernels (csrc/btf_predict.h: pred_kernel<FAM>, pred_score_kernel<FAM>, pred_score_total_kernel,
pred_batch_kernel<FAM>, launched by predict_run of csrc/btf_analysis.hip) and posterior_summary_kernel<K>
(csrc/btf_kernels.h, launch_summary) sort the n values of a cell in a row of LDS.  This module enumerates the shapes at which
they are compared with numpy ("Shape passes", the predictive entry), builds the inputs of every case and holds the
references; the GPU file imports all three.  Here every list is shown to be the enumeration it claims and every case
admissible - its LDS fits, its states are dyadic so that w . v is exact in any order, and its (eta, aux) put cells on both
sides of every sampler switch: a case that is not fails here, it is never dropped.  Inputs are the first seed of a fixed
sequence for which the sampler branches are met.  No GPU.

Geometry the cases are derived from (sort_geom of csrc/btf_ctx.h): a row of P doubles, P the power of two >= max(2, n);
cells per workgroup = max(1, min(16, budget // (8 P))), budget 64 KiB for the predictive (n = S R draws) and 128 KiB for the
summary (n = S); PRED_THREADS = 256, four waves of WAVE = 64 lanes, wave w taking the cells w, w + 4, ... of its workgroup;
PRED_SCORE_CELLS = 4096 cells per workgroup of pred_score_kernel; 256 samples per workgroup of pred_score_total_kernel.
"""
import collections
import functools
import os
import zlib

import numpy as np
import pytest

from functionalmf_amd import _native, predictive
from functionalmf_amd.likelihoods import GammaGridLikelihood

WAVE, PRED_THREADS, PRED_WAVES, PRED_SCORE_CELLS = 64, 256, 4, 4096
PRED_SORT_LDS, SUMMARY_SORT_LDS, SORT_CAP, CU_LDS = 64 * 1024, 128 * 1024, 16, 160 * 1024
MAX_DRAWS, TOTAL_THREADS = 16384, 256
NSEEDS = 200                     # length of every seed sequence below
FAMILIES = ("poisson", "poisson_identity", "binomial", "gaussian", "negbin", "gamma_grid")
COUNT_FAMILIES = ("poisson", "poisson_identity", "binomial", "negbin")
POSITIVE = ("poisson_identity", "gamma_grid")            # families whose eta has to be > 0
KS = tuple(range(1, 11))
SEED = 21                        # the device seed of every call
# percentiles of every case outside list 3: unsorted, with the three integral positions 0, 50 (odd n), 100
Q5 = (2.5, 0.0, 50.0, 100.0, 97.5)
GG_TABLE = GammaGridLikelihood.from_table([0.5, 2.0, 9.0, 1.0], [0.25, 0.5, 0.125, 1.0], [1.0, 3.0, 2.0, 0.0])


def sort_geom(n, budget, cap=SORT_CAP):
    """(P, cells, lds bytes) of sort_geom(n, budget, cap) in csrc/btf_ctx.h"""
    P = 2
    while P < n:
        P <<= 1
    cells = max(1, min(cap, budget // (8 * P)))
    return P, cells, cells * P * 8


def pred_geom(n):
    return sort_geom(n, PRED_SORT_LDS)


def summary_geom(S):
    return sort_geom(S, SUMMARY_SORT_LDS)


def workgroup_cells(MT, cells):
    """nc of every workgroup of one row"""
    return [min(cells, MT - j0) for j0 in range(0, MT, cells)]


# (M, T) of a cell count per row, T >= 2 (a context needs it)
MT_SHAPES = {2: (1, 2), 3: (1, 3), 5: (1, 5), 6: (2, 3), 11: (1, 11), 17: (1, 17), 35: (5, 7)}
# M T per cells value: a partial last workgroup, and nc = 2, 3, 5, (16, 1), (16, 16, 3) at 16 cells
MT_OF_CELLS = {16: (2, 3, 5, 17, 35), 8: (11,), 4: (6,), 2: (3,), 1: (3,)}

Case = collections.namedtuple("Case", "fam S R N M T K q nreps data param listed", defaults=(Q5, 2, "mixed", "default", None))


def case_id(c):
    if not isinstance(c, Case):
        return None
    s = "%s-S%dxR%d-%dx%dx%d-K%d" % (c.fam, c.S, c.R, c.N, c.M, c.T, c.K)
    if c.q != Q5:
        s += "-nq%d" % len(c.q)
    if c.nreps != 2:
        s += "-reps%d" % c.nreps
    for v in (c.data, c.param):
        if v not in ("mixed", "default"):
            s += "-" + "".join(str(int(x)) if isinstance(x, bool) else str(x) for x in (v if isinstance(v, tuple) else (v,)))
    if c.listed is not None:
        s += "-list%d" % c.listed
    return s


# ------------------------------------------------------------------------------------------- 1. sort geometry of pred_kernel
SORT_N_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16383, 16384)
SORT_N = tuple(sorted(SORT_N_EDGES + (5, 9, 17)))      # and P = 8, 16, 32, which the edges above leave out
# n = S R with R > 1 (a prime n: S = 1)
SORT_SR = {2: (1, 2), 3: (1, 3), 5: (1, 5), 9: (3, 3), 17: (1, 17), 63: (21, 3), 64: (32, 2), 65: (13, 5), 127: (1, 127),
           128: (64, 2), 129: (43, 3), 511: (73, 7), 512: (256, 2), 513: (171, 3), 1024: (512, 2), 1025: (205, 5), 2048: (1024, 2), 2049: (683, 3), 4096: (2048, 2),
           4097: (241, 17), 8192: (4096, 2), 8193: (2731, 3), 16383: (5461, 3), 16384: (8192, 2)}


def _sort_geometries():
    """(S, R, (M, T)) of list 1: every n as S x 1 and as S x R; M T cycles through the values of its cells class"""
    out, seen = [], collections.Counter()
    for n in SORT_N:
        for S, R in ((n, 1),) + ((SORT_SR[n],) if n in SORT_SR else ()):
            cells = pred_geom(n)[1]
            choices = MT_OF_CELLS[cells]
            out.append((S, R, MT_SHAPES[choices[seen[cells] % len(choices)]]))
            seen[cells] += 1
    return out


SORT_GEOMETRIES = _sort_geometries()
SORT_CASES = [Case(f, S, R, 2, M, T, 3) for S, R, (M, T) in SORT_GEOMETRIES for f in FAMILIES]

# ------------------------------------------------------------------------------------------- 2. nembeds
K_CASES = [Case(f, 13, 5, 2, 1, 5, K) for K in KS for f in ("gaussian", "poisson")]

# ------------------------------------------------------------------------------------------- 3. percentiles
NQS = (0, 1, 2, 63, 64, 65, 128, 129)


def percentile_list(nq):
    """nq percentiles in shuffled order, 0 and 100 among them from nq = 2 on"""
    if nq < 2:
        return (37.5,)[:nq]
    return tuple(float(v) for v in np.random.RandomState(nq).permutation(np.linspace(0.0, 100.0, nq)))


Q_CASES = [Case(f, 37, 3, 2, 5, 7, 3, q=percentile_list(nq)) for nq in NQS for f in FAMILIES]

# ------------------------------------------------------------------------------------------- 4. listed cells
LIST_LENGTHS = (1, 63, 64, 65, 129)
LIST_SHAPE = (4, 5, 7)           # 140 cells
LIST_TWICE = {65: (3, 64), 129: (10, 128)}      # positions of the index given twice: different blocks of 64
LIST_CASES = [Case(f, 37, 3, *LIST_SHAPE, 3, listed=L) for L in LIST_LENGTHS for f in FAMILIES]


def listed_cells(L, ncell):
    cells = np.random.RandomState(400 + L).permutation(ncell)[:L].astype(np.int32)
    if L in LIST_TWICE:
        a, b = LIST_TWICE[L]
        cells[b] = cells[a]
    return cells


# ------------------------------------------------------------------------------------------- 5. data
NREPS = (1, 2, 5)
DATA_CASES = [Case(f, 37, 3, 2, 5, 7, 3, nreps=r) for r in NREPS for f in FAMILIES]
# a missing trial count inside a workgroup of 16 cells (n = 111) and one of 8 (n = 1000): (case, the poisoned flat cell)
POISON_CASES = [Case("binomial", 37, 3, 2, 5, 7, 3, param=("poison", 40)), Case("binomial", 500, 2, 2, 1, 11, 3, param=("poison", 16))]

# ------------------------------------------------------------------------------------------- 6. parameters
LAYOUTS = tuple((a, b, d) for a in (False, True) for b in (False, True) for d in (False, True))
PARAM_SHAPE = (3, 4, 5)
PARAM_CASES = [Case("negbin", 37, 3, *PARAM_SHAPE, 3, param=lay) for lay in LAYOUTS] + \
              [Case("negbin", 37, 3, *PARAM_SHAPE, 3, param=p) for p in ("shared", ("const", 0.5), ("const", 3.0))] + \
              [Case("gaussian", 37, 3, *PARAM_SHAPE, 3, param=p) for p in ("default", ("const", 2.25))] + \
              [Case("binomial", 37, 3, *PARAM_SHAPE, 3, param="none")]

# ------------------------------------------------------------------------------------------- 7. scores
SCORE_SHAPES = {2: (1, 1, 2), 255: (3, 5, 17), 256: (4, 8, 8), 257: (1, 1, 257), 4095: (5, 9, 91), 4096: (16, 16, 16),
                4097: (241, 1, 17), 8193: (2731, 1, 3)}
SCORE_CASES = [Case(f, 2, 1, *shape, 3) for shape in SCORE_SHAPES.values() for f in FAMILIES]
SCORE_CHUNK_MISSING = [Case(f, 2, 1, *SCORE_SHAPES[8193], 3, data="chunk_missing") for f in ("gaussian", "negbin")]
SCORE_ALL_MISSING = [Case(f, 2, 1, *SCORE_SHAPES[257], 3, data="all_missing") for f in ("gaussian", "poisson")]
TOTAL_S = (1, 255, 256, 257)
TOTAL_CASES = [Case(f, S, 1, 2, 2, 3, 3) for S in TOTAL_S for f in ("gaussian", "binomial")]

# ------------------------------------------------------------------------------------------- 8. pred_batch_kernel
BATCH_FULL, BATCH_PREFIXES = 1000, (1, 255, 256, 257)

# ------------------------------------------------------------------------------------------- 9. posterior_summary_kernel
TRANSFORMS = (None, "ilogit", "square")
SUMMARY_Q = (5.0, 50.0, 95.0, 0.0, 100.0, 33.3)
SUMMARY_S = (1, 2, 3, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16383, 16384)
SUMMARY_NQ = (0, 1, 16, 17, 40)
# (S, N, (M, T), K, transform, q)
SUMMARY_K = [(37, 3, (1, 17), K, tr, SUMMARY_Q) for K in KS for tr in TRANSFORMS]


def _summary_geometries():
    out, seen = [], collections.Counter()
    for S in SUMMARY_S:
        for K, tr in ((1, None), (7, "square")):
            cells = summary_geom(S)[1]
            choices = MT_OF_CELLS[cells]
            out.append((S, 2, MT_SHAPES[choices[seen[cells] % len(choices)]], K, tr, SUMMARY_Q))
            seen[cells] += 1
    return out


SUMMARY_GEOMETRIES = _summary_geometries()


def summary_percentiles(nq):
    if nq < 2:
        return (50.0,)[:nq]
    return tuple(float(v) for v in np.random.RandomState(900 + nq).permutation(np.linspace(0.0, 100.0, nq)))


SUMMARY_NQ_CASES = [(37, 3, (1, 17), 3, None, summary_percentiles(nq)) for nq in SUMMARY_NQ]
SUMMARY_CASES = SUMMARY_K + SUMMARY_GEOMETRIES + SUMMARY_NQ_CASES
SUMMARY_LIMIT = 16384

# the two largest cases, run twice (D)
REPEAT_PRED = Case("negbin", 8192, 2, 2, 1, 3, 3)
REPEAT_SUMMARY = (16384, 2, (1, 3), 7, "square", SUMMARY_Q)

ALL_PRED_CASES = SORT_CASES + K_CASES + Q_CASES + LIST_CASES + DATA_CASES + POISON_CASES + PARAM_CASES + SCORE_CASES + \
    SCORE_CHUNK_MISSING + SCORE_ALL_MISSING + TOTAL_CASES


# ------------------------------------------------------------------------------------------------------------------ inputs
def dyadic(rs, shape, positive):
    """multiples of 1/4 with |entries| <= 2, strictly positive on demand"""
    return (rs.randint(1, 9, size=shape) if positive else rs.randint(-8, 9, size=shape)) / 4.0


def family_inputs(c):
    """(keyword arguments of the public call, aux broadcastable against (S,N,M,T) or None) - passed through unchanged"""
    S, N, M, T = c.S, c.N, c.M, c.T
    const = c.param[1] if isinstance(c.param, tuple) and c.param[0] == "const" else None
    if c.fam == "gaussian":
        if const is not None:
            return dict(param=const), np.full((1, 1, 1, 1), const)
        nu2 = np.array([0.25, 1.0, 2.25])[np.arange(S) % 3]
        return dict(nu2=nu2), nu2[:, None, None, None]
    if c.fam == "negbin":
        if const is not None:
            return dict(param=const), np.full((1, 1, 1, 1), const)
        lay = (False, False, False) if c.param == "shared" else ((True, False, True) if c.param == "default" else c.param)
        ext = tuple(full if on else 1 for full, on in zip((N, M, T), lay))
        s, i, j, t = np.ogrid[:S, :ext[0], :ext[1], :ext[2]]
        R = 0.5 + 0.25 * ((7 * s + 3 * i + 5 * j + 11 * t) % 13)         # 0.5 .. 3.5: different along every axis
        return dict(R=R[:, 0, 0, 0] if c.param == "shared" else R), R
    if c.fam == "binomial":
        if c.param == "none":
            return {}, np.ones((1, 1, 1, 1))
        tr = np.array([0.0, 400.0, 3.0, 40.0, 1.0, 400.0, 7.0])[np.arange(N * M * T) % 7].reshape(N, M, T)
        if isinstance(c.param, tuple) and c.param[0] == "poison":
            tr[np.unravel_index(c.param[1], (N, M, T))] = np.nan
        return dict(trials=tr), tr[None]
    return {}, None


def mean_of(c, eta, aux):
    with np.errstate(invalid="ignore", over="ignore"):
        if c.fam == "gamma_grid":
            return predictive.gamma_grid_mean(GG_TABLE, eta)
        return predictive.mean_function(c.fam, eta, aux)


def branches(c, eta, aux):
    """{switch side: present} of the count samplers for the (eta, aux) of a case; empty where the family has no switch"""
    if c.fam in ("poisson", "poisson_identity"):
        with np.errstate(over="ignore"):
            lam = np.exp(eta) if c.fam == "poisson" else eta
        return {"inversion": bool((lam < predictive.POISSON_SWITCH).any()), "ptrs": bool((lam >= predictive.POISSON_SWITCH).any())}
    if c.fam == "binomial":
        tr = np.broadcast_to(aux, eta.shape)
        with np.errstate(invalid="ignore"):
            small = tr / (1.0 + np.exp(np.abs(eta)))                   # n min(p, 1 - p)
        live = tr > 0
        return {"binv": bool((small[live] < predictive.BINOMIAL_SWITCH).any()), "btrs": bool((small[live] >= predictive.BINOMIAL_SWITCH).any()),
                "eta<0": bool((eta[live] < 0).any()), "eta>0": bool((eta[live] > 0).any()), "no trials": bool((tr == 0).any())}
    if c.fam == "negbin":
        return {"rate<1": bool((aux < 1).any()), "rate>1": bool((aux > 1).any())}
    return {}


def branches_demanded(c):
    """The sides a case can reach at all: a constant rate has one side, one trial per cell stays under the Binomial
    switch, and eta = w . v <= 4 K stays under the Poisson switch of the identity link below K = 3."""
    if c.fam == "negbin" and isinstance(c.param, tuple) and c.param[0] == "const":
        return ()
    if c.fam == "binomial" and c.param == "none":
        return ("binv", "eta<0", "eta>0")
    if c.fam == "poisson_identity" and c.K < 3:
        return ("inversion",)
    return None                  # all of them


def observations(c, rs, Mu0):
    """Y (N,M,T,nreps) around the mean of sample 0: dyadic for the Gaussian family, > 0 for the gamma grid, counts within 2
    of round(E y) otherwise (so that a count equals a draw); then the patterns of `data`."""
    N, M, T = Mu0.shape
    size, ncell = (N, M, T, c.nreps), N * M * T
    if c.fam == "gaussian":
        Y = Mu0[..., None] + rs.randint(-8, 9, size=size) / 4.0
    elif c.fam == "gamma_grid":
        Y = Mu0[..., None] * rs.randint(1, 9, size=size) / 4.0
    else:
        Y = np.round(np.nan_to_num(Mu0))[..., None] + rs.randint(0, 3, size=size)
    Y = Y.reshape(ncell, c.nreps)
    complete = Y.copy()
    if ncell > 8:
        Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    if ncell >= 4:
        Y[0, 0] = complete[0, 0]
        Y[ncell - 1] = np.nan                                         # every replicate missing
        Y[ncell - 2] = np.nan
        Y[ncell - 2, -1] = complete[ncell - 2, -1]                    # observed in its last replicate only
    if c.data == "all_missing":
        Y[:] = np.nan
    elif c.data == "chunk_missing":
        Y[PRED_SCORE_CELLS:2 * PRED_SCORE_CELLS] = np.nan             # the second chunk of pred_score_kernel
        Y[ncell - 1] = complete[ncell - 1]                            # (and the last chunk, of one cell, observed)
    return Y.reshape(size)


@functools.lru_cache(maxsize=None)
def build(c):
    """The inputs of a predictive case: the first seed of its sequence whose (eta, aux) meet every demanded sampler branch."""
    S, N, M, T, K = c.S, c.N, c.M, c.T, c.K
    positive = c.fam in POSITIVE
    kw, aux = family_inputs(c)
    want = branches_demanded(c)
    base = zlib.crc32(repr(c).encode()) & 0x3fffffff
    for k in range(NSEEDS):
        rs = np.random.RandomState(base + 7919 * k)
        Ws, Vs = dyadic(rs, (S, N, K), positive), dyadic(rs, (S, M, T, K), positive)
        if positive and K >= 3:
            Ws[0, 0], Vs[0, 0, 0] = 2.0, 2.0                          # eta = 4 K >= 12 in one cell of sample 0
        eta = np.einsum("znk,zmtk->znmt", Ws, Vs)
        have = branches(c, eta, aux)
        if all(v for name, v in have.items() if want is None or name in want):
            break
    else:
        raise AssertionError("no seed with every sampler branch: %r" % (have,))
    Mu = mean_of(c, eta, aux)
    Y = observations(c, rs, Mu[0])
    ncell = N * M * T
    cells = np.arange(ncell, dtype=np.int32) if c.listed is None else listed_cells(c.listed, ncell)
    for a in (Ws, Vs, eta, Mu, Y, cells):
        a.setflags(write=False)
    return dict(Ws=Ws, Vs=Vs, eta=eta, aux=aux, kw=kw, Mu=Mu, Y=Y, cells=cells, branches=have, seed=base + 7919 * k, tries=k + 1)


def batch_inputs(c, b, cells=None):
    """(eta, aux, idx): the inputs of predictive.batch / gamma_grid_batch that restate the draws of `cells` (default: the
    listed ones) at their global indices g = (cell S + s) R + r; idx (len(cells), S R) are those indices.  Indices no draw
    uses hold a valid value (eta = 1, the aux of cell 0 in sample 0)."""
    S, R = c.S, c.R
    cells = b["cells"] if cells is None else np.asarray(cells)
    idx = (cells.astype(np.int64)[:, None, None] * S + np.arange(S)[None, :, None]) * R + np.arange(R)[None, None, :]
    size = int(idx.max()) + 1
    eta2 = b["eta"].reshape(S, -1)
    full = np.ones(size)
    full[idx.ravel()] = np.repeat(eta2[:, cells].T, R, axis=1).ravel()
    aux = None
    if b["aux"] is not None:
        aux2 = np.broadcast_to(b["aux"], b["eta"].shape).reshape(S, -1)
        aux = np.full(size, aux2[0, 0])
        aux[idx.ravel()] = np.repeat(aux2[:, cells].T, R, axis=1).ravel()
    return full, aux, idx.reshape(len(cells), S * R)


def reference(c, b, d):
    """The reductions of pred_kernel in numpy from the draws d (ncell, n) of every cell, and the scores from E[y]."""
    N, M, T, n = c.N, c.M, c.T, c.S * c.R
    shape = (N, M, T)
    d = d.reshape(shape + (n,))
    Y, Mu, q = b["Y"], b["Mu"], np.asarray(c.q, dtype=float)
    nanc = np.isnan(d).any(axis=-1)
    ref = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        ref["quantiles"] = np.percentile(d, q, axis=-1) if len(q) else np.zeros((0,) + shape)
        ref["y_mean"] = d.mean(-1)
        ref["y_var"] = d.var(-1, ddof=1) if n > 1 else np.full(shape, np.nan)
        ref["mean"] = Mu.mean(axis=0)
        obs = ~np.isnan(Y)
        nobs = obs.sum(-1).astype(float)
        lt = np.where(obs, (d[..., None, :] < Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
        le = np.where(obs, (d[..., None, :] <= Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
        lt[nanc], le[nanc] = np.nan, np.nan
        if len(q) >= 2:
            ins = (obs & (Y >= ref["quantiles"][0][..., None]) & (Y <= ref["quantiles"][-1][..., None])).sum(-1).astype(float)
            ins[nanc] = np.nan
            ok = ~nanc
            ref["coverage"] = ins[ok].sum() / nobs[ok].sum() if nobs[ok].sum() > 0 else np.nan
        else:
            ins, ref["coverage"] = np.full(shape, np.nan), np.nan
        res = (Y[None] - Mu[..., None])[:, obs]                       # (S, n_obs): politics/benchmark.py:158-164
        ref["rmse"] = np.sqrt((res ** 2).mean(axis=1)) if obs.any() else np.full(c.S, np.nan)
        ref["mae"] = np.abs(res).mean(axis=1) if obs.any() else np.full(c.S, np.nan)
    ref.update(pit_lo=lt, pit_hi=le, inside=ins, nobs=nobs)
    return ref


@functools.lru_cache(maxsize=None)
def summary_inputs(S, N, MT, K):
    rs = np.random.RandomState(zlib.crc32(repr((S, N, MT, K)).encode()) & 0x3fffffff)
    Ws, Vs = dyadic(rs, (S, N, K), False), dyadic(rs, (S,) + MT + (K,), False)
    for a in (Ws, Vs):
        a.setflags(write=False)
    return Ws, Vs


def summary_reference(Ws, Vs, transform, q):
    Mu = np.einsum("znk,zmtk->znmt", Ws, Vs)
    if transform == "ilogit":
        Mu = 1.0 / (1.0 + np.exp(-Mu))
    elif transform == "square":
        Mu = Mu ** 2
    quant = np.percentile(Mu, q, axis=0) if len(q) else np.zeros((0,) + Mu.shape[1:])
    return Mu, Mu.mean(axis=0), quant


@functools.lru_cache(maxsize=None)
def batch_case(fam):
    """eta, aux of BATCH_FULL draws of a family, both sides of its switches among them"""
    rs = np.random.RandomState(800 + FAMILIES.index(fam))
    eta = (dyadic(rs, (BATCH_FULL, 3), fam in POSITIVE) * dyadic(rs, (BATCH_FULL, 3), fam in POSITIVE)).sum(axis=1)
    eta[0] = 12.0
    aux = {"binomial": np.array([0.0, 400.0, 3.0, 40.0])[np.arange(BATCH_FULL) % 4], "gaussian": np.full(BATCH_FULL, 2.25),
           "negbin": np.array([0.5, 3.0])[np.arange(BATCH_FULL) % 2]}.get(fam)
    return eta, aux


# ------------------------------------------------------------------------------------------------------------------- tests
def test_the_geometry_is_the_headers():
    """The constants restated above, in the sources they come from."""
    src = lambda name: open(os.path.join(_native.CSRC, name)).read()
    ctx, pred, ana = src("btf_ctx.h"), src("btf_predict.h"), src("btf_analysis.hip")
    assert "constexpr size_t SUMMARY_SORT_LDS = 128 * 1024, PRED_SORT_LDS = 64 * 1024;" in ctx
    assert "constexpr int SUMMARY_SORT_CELLS = %d, PRED_SORT_CELLS = %d;" % (SORT_CAP, SORT_CAP) in ctx
    assert "g.cells = std::max(1, std::min(cap, (int)(budget / ((size_t)g.P * sizeof(double)))));" in ctx
    assert "constexpr int PRED_THREADS = %d;" % PRED_THREADS in pred and "constexpr int PRED_SCORE_CELLS = %d;" % PRED_SCORE_CELLS in pred
    assert "constexpr int PRED_MAX_DRAWS = %d;" % MAX_DRAWS in pred and predictive.MAX_DRAWS == MAX_DRAWS
    assert "c += PRED_THREADS / WAVE" in pred and PRED_THREADS // WAVE == PRED_WAVES
    assert "constexpr size_t PRED_CU_LDS = 160 * 1024;" in ana and "dim3((S + 255) / 256), dim3(256)" in ana
    assert "nsamples > %d" % SUMMARY_LIMIT in ana
    assert pred_geom(1) == (2, 16, 256) and pred_geom(512) == (512, 16, 65536) and pred_geom(513) == (1024, 8, 65536)
    assert pred_geom(8192) == (8192, 1, 65536) and pred_geom(16384) == (16384, 1, 131072)       # twice the documented budget
    assert summary_geom(1024) == (1024, 16, 131072) and summary_geom(1025) == (2048, 8, 131072) and summary_geom(16384) == (16384, 1, 131072)


def test_list_1_is_every_sort_geometry():
    assert len(SORT_N_EDGES) == 22 and len(SORT_N) == len(set(SORT_N)) == 25 and max(SORT_N) == MAX_DRAWS
    geoms = {n: pred_geom(n) for n in SORT_N}
    assert {g[0] for g in geoms.values()} == {2 ** k for k in range(1, 15)}                   # every P from 2 to 16384
    assert {g[1] for g in geoms.values()} == {16, 8, 4, 2, 1}
    for cells in (16, 8, 4, 2, 1):
        assert any(n == geoms[n][0] for n in SORT_N if geoms[n][1] == cells)                    # n == P: no pad
        assert any(n == geoms[n][0] // 2 + 1 for n in SORT_N if geoms[n][1] == cells)           # the longest pad
    for cells in (16, 1):                                                                       # one pad: n == P - 1
        assert any(n == geoms[n][0] - 1 for n in SORT_N if geoms[n][1] == cells)
    assert all(g[2] <= CU_LDS for g in geoms.values())
    # every n as S x 1 and once as S x R, R > 1 (n = 1 has no such form)
    assert len(SORT_GEOMETRIES) == len(set(SORT_GEOMETRIES)) == 25 + 24
    assert sorted(S * R for S, R, _ in SORT_GEOMETRIES if R == 1) == sorted(SORT_N)
    assert sorted(S * R for S, R, _ in SORT_GEOMETRIES if R > 1) == sorted(n for n in SORT_N if n > 1)
    assert all(S * R == n and R > 1 for n, (S, R) in SORT_SR.items())
    assert (1, 2) in {(S, R) for S, R, _ in SORT_GEOMETRIES}
    # M T per cells class: a partial last workgroup; at 16 cells every nc the wave loop distinguishes
    by_cells = collections.defaultdict(set)
    for S, R, (M, T) in SORT_GEOMETRIES:
        assert T >= 2 and MT_SHAPES[M * T] == (M, T)
        by_cells[pred_geom(S * R)[1]].add(M * T)
    assert {k: tuple(sorted(v)) for k, v in by_cells.items()} == MT_OF_CELLS
    nc16 = [tuple(workgroup_cells(MT, 16)) for MT in MT_OF_CELLS[16]]
    assert nc16 == [(2,), (3,), (5,), (16, 1), (16, 16, 3)]            # idle waves; a wave with two cells; one cell; full
    assert tuple(workgroup_cells(11, 8)) == (8, 3) and tuple(workgroup_cells(6, 4)) == (4, 2) and tuple(workgroup_cells(3, 2)) == (2, 1)
    assert tuple(workgroup_cells(3, 1)) == (1, 1, 1)
    assert len(SORT_CASES) == len(set(SORT_CASES)) == 49 * 6
    assert {(c.fam, c.S, c.R, (c.M, c.T)) for c in SORT_CASES} == {(f, S, R, MT) for S, R, MT in SORT_GEOMETRIES for f in FAMILIES}
    assert {c.N for c in SORT_CASES} == {2} and {c.q for c in SORT_CASES} == {Q5} and {c.listed for c in SORT_CASES} == {None}


def test_lists_2_to_8_are_their_enumerations():
    assert {(c.fam, c.K) for c in K_CASES} == {(f, K) for f in ("gaussian", "poisson") for K in KS} and len(K_CASES) == 20
    assert {c.S * c.R for c in K_CASES} == {65}
    # 3. percentiles: one pass of the q0 loop, exactly one, two, exactly two, three
    assert {(c.fam, len(c.q)) for c in Q_CASES} == {(f, nq) for f in FAMILIES for nq in NQS} and len(Q_CASES) == 48
    assert {c.S * c.R for c in Q_CASES} == {111}
    assert sorted({-(-nq // WAVE) for nq in NQS}) == [0, 1, 2, 3] and {WAVE, 2 * WAVE} <= set(NQS) and {WAVE + 1, 2 * WAVE + 1} <= set(NQS)
    for nq in NQS:
        q = percentile_list(nq)
        assert len(q) == nq and all(0 <= v <= 100 for v in q)
        if nq >= 2:
            assert 0.0 in q and 100.0 in q and list(q) != sorted(q)
        if nq > WAVE:
            assert (nq - 1) - WAVE * ((nq - 1) // WAVE) != nq - 1       # the lane of qhi differs with and without q0
    # 4. listed cells: one and two passes of the l0 loop, three at 129
    assert {(c.fam, c.listed) for c in LIST_CASES} == {(f, L) for f in FAMILIES for L in LIST_LENGTHS} and len(LIST_CASES) == 30
    ncell = LIST_SHAPE[0] * LIST_SHAPE[1] * LIST_SHAPE[2]
    assert ncell == 140 and sorted({-(-L // WAVE) for L in LIST_LENGTHS}) == [1, 2, 3]
    for L in LIST_LENGTHS:
        cells = listed_cells(L, ncell)
        assert len(cells) == L and cells.min() >= 0 and cells.max() < ncell and (L < 3 or list(cells) != sorted(cells))
        if L in LIST_TWICE:
            a, b = LIST_TWICE[L]
            assert cells[a] == cells[b] and a // WAVE != b // WAVE and len(set(cells.tolist())) == L - 1
        else:
            assert len(set(cells.tolist())) == L
        assert len(set(range(ncell)) - set(cells.tolist())) > 0        # unlisted cells exist
    # 5. data
    assert {(c.fam, c.nreps) for c in DATA_CASES} == {(f, r) for f in FAMILIES for r in NREPS}
    assert [pred_geom(c.S * c.R)[1] for c in POISON_CASES] == [16, 8]
    for c in POISON_CASES:
        cells, flat = pred_geom(c.S * c.R)[1], c.param[1]
        jt = flat % (c.M * c.T)
        nc = workgroup_cells(c.M * c.T, cells)[jt // cells]
        assert 0 < jt % cells < nc - 1                                  # neighbours on both sides in its workgroup
    # 6. parameters
    assert len(LAYOUTS) == len(set(LAYOUTS)) == 8 and min(PARAM_SHAPE) > 1 and len(set(PARAM_SHAPE)) == 3
    nb = [c.param for c in PARAM_CASES if c.fam == "negbin"]
    assert set(nb) == set(LAYOUTS) | {"shared", ("const", 0.5), ("const", 3.0)} and len(nb) == 11
    assert [c.param for c in PARAM_CASES if c.fam == "gaussian"] == ["default", ("const", 2.25)]
    assert [c.param for c in PARAM_CASES if c.fam == "binomial"] == ["none"]
    # 7. scores: one, two, three chunks; a last chunk of one cell; fewer cells than threads
    assert {s[0] * s[1] * s[2]: s for s in SCORE_SHAPES.values()} == SCORE_SHAPES and all(s[2] >= 2 for s in SCORE_SHAPES.values())
    assert sorted(SCORE_SHAPES) == [2, 255, 256, 257, 4095, 4096, 4097, 8193]
    assert sorted({-(-n // PRED_SCORE_CELLS) for n in SCORE_SHAPES}) == [1, 2, 3]
    assert 4097 % PRED_SCORE_CELLS == 1 and 8193 % PRED_SCORE_CELLS == 1 and min(SCORE_SHAPES) < PRED_THREADS
    assert {(c.fam, c.N * c.M * c.T) for c in SCORE_CASES} == {(f, n) for f in FAMILIES for n in SCORE_SHAPES} and {c.S for c in SCORE_CASES} == {2}
    assert all(c.N * c.M * c.T == 8193 and c.data == "chunk_missing" for c in SCORE_CHUNK_MISSING) and SCORE_CHUNK_MISSING
    assert all(c.data == "all_missing" for c in SCORE_ALL_MISSING) and SCORE_ALL_MISSING
    assert {(c.fam, c.S) for c in TOTAL_CASES} == {(f, S) for f in ("gaussian", "binomial") for S in TOTAL_S}
    assert {c.N * c.M * c.T for c in TOTAL_CASES} == {12} and {TOTAL_THREADS - 1, TOTAL_THREADS, TOTAL_THREADS + 1} <= set(TOTAL_S)
    # 8. batch
    assert {PRED_THREADS - 1, PRED_THREADS, PRED_THREADS + 1, 1} == set(BATCH_PREFIXES) and BATCH_FULL > 3 * PRED_THREADS
    assert len(ALL_PRED_CASES) == len(set(ALL_PRED_CASES))


def test_list_9_is_every_summary_geometry():
    assert {(c[3], c[4]) for c in SUMMARY_K} == {(K, tr) for K in KS for tr in TRANSFORMS} and len(SUMMARY_K) == 30
    assert {c[:3] for c in SUMMARY_K} == {(37, 3, (1, 17))}
    geoms = {S: summary_geom(S) for S in SUMMARY_S}
    assert {g[1] for g in geoms.values()} == {16, 8, 4, 2, 1} and max(SUMMARY_S) == SUMMARY_LIMIT
    for cells in (16, 8, 4, 2, 1):
        assert any(S == geoms[S][0] for S in SUMMARY_S if geoms[S][1] == cells)
        assert any(S == geoms[S][0] // 2 + 1 for S in SUMMARY_S if geoms[S][1] == cells)
    assert all(g[2] <= CU_LDS for g in geoms.values())
    assert {(c[0], c[3]) for c in SUMMARY_GEOMETRIES} == {(S, K) for S in SUMMARY_S for K in (1, 7)} and len(SUMMARY_GEOMETRIES) == 28
    by_cells = collections.defaultdict(set)
    for S, N, (M, T), K, tr, q in SUMMARY_GEOMETRIES:
        assert T >= 2 and tr in (None, "square") and N == 2
        by_cells[geoms[S][1]].add(M * T)
        assert workgroup_cells(M * T, geoms[S][1])[-1] < geoms[S][1] or geoms[S][1] == 1       # a partial last workgroup
    assert by_cells[16] == set(MT_OF_CELLS[16]) and all(by_cells[k] == set(MT_OF_CELLS[k]) for k in (8, 4, 2, 1))
    # the nc * nq loop: under one pass of 256 threads, exactly one, more than one
    assert [len(c[5]) for c in SUMMARY_NQ_CASES] == list(SUMMARY_NQ)
    nc = workgroup_cells(17, summary_geom(37)[1])
    assert nc == [16, 1] and 16 * 16 == 256 and 16 * 17 > 256 and 16 * 1 < 256 and 16 * 40 > 2 * 256
    for nq in SUMMARY_NQ:
        q = summary_percentiles(nq)
        assert len(q) == nq and (nq < 2 or (0.0 in q and 100.0 in q and list(q) != sorted(q)))
    assert REPEAT_PRED in SORT_CASES and REPEAT_PRED.S * REPEAT_PRED.R == MAX_DRAWS
    assert REPEAT_SUMMARY in SUMMARY_GEOMETRIES and REPEAT_SUMMARY[0] == SUMMARY_LIMIT
    assert len(SUMMARY_CASES) == len(set(SUMMARY_CASES)) == 30 + 28 + 5


@pytest.mark.parametrize("c", ALL_PRED_CASES, ids=case_id)
def test_predictive_cases_are_admissible(c):
    n, ncell = c.S * c.R, c.N * c.M * c.T
    P, cells, lds = pred_geom(n)
    assert 1 <= n <= MAX_DRAWS and lds <= CU_LDS and c.T >= 2 and 1 <= c.K <= 10
    b = build(c)
    Ws, Vs, eta = b["Ws"], b["Vs"], b["eta"]
    assert Ws.shape == (c.S, c.N, c.K) and Vs.shape == (c.S, c.M, c.T, c.K)
    for a in (Ws, Vs):
        assert np.array_equal(4 * a, np.round(4 * a)) and np.abs(a).max() <= 2
    assert np.array_equal(16 * eta, np.round(16 * eta)) and np.abs(eta).max() <= 4 * c.K       # every partial sum exact
    if c.fam in POSITIVE:
        assert Ws.min() > 0 and Vs.min() > 0 and eta.min() > 0
    want = branches_demanded(c)
    for name, present in b["branches"].items():
        assert present or (want is not None and name not in want), (name, b["branches"])
    if c.fam in COUNT_FAMILIES:
        assert b["branches"]
    Y = b["Y"]
    assert Y.shape == (c.N, c.M, c.T, c.nreps)
    obs = ~np.isnan(Y).reshape(ncell, c.nreps)
    if c.data == "all_missing":
        assert not obs.any()
    elif ncell >= 4 and c.data == "mixed":
        assert not obs[ncell - 1].any() and obs[ncell - 2, -1] and not obs[ncell - 2, :-1].any() and obs[0, 0]
    if c.data == "chunk_missing":
        assert not obs[PRED_SCORE_CELLS:2 * PRED_SCORE_CELLS].any() and obs[:PRED_SCORE_CELLS].any() and obs[2 * PRED_SCORE_CELLS:].any()
    if c.fam == "gamma_grid":
        assert np.nanmin(Y) > 0
    elif c.fam != "gaussian" and obs.any():
        assert np.array_equal(Y[~np.isnan(Y)], np.floor(Y[~np.isnan(Y)])) and np.nanmin(Y) >= 0
    if isinstance(c.param, tuple) and c.param[0] == "poison":
        tr = b["kw"]["trials"].reshape(-1)
        assert np.isnan(tr[c.param[1]]) and np.isnan(tr).sum() == 1
    # the batch that restates the draws covers every index exactly once when all cells are listed
    full, aux, idx = batch_inputs(c, b)
    assert idx.shape == (len(b["cells"]), n) and idx.max() < ncell * n
    if c.listed is None:
        assert np.array_equal(np.sort(idx.ravel()), np.arange(ncell * n))
    assert aux is None or aux.shape == full.shape


def test_rate_layouts_differ_along_every_axis():
    """A swap of two extents in pred_aux reads another rate: under every layout the rates differ along each kept axis."""
    for c in PARAM_CASES:
        if c.fam != "negbin" or not isinstance(c.param, tuple) or c.param[0] == "const":
            continue
        R = family_inputs(c)[0]["R"]
        rates, flags = predictive.rate_layout(R, c.S, PARAM_SHAPE)
        assert R.shape == (c.S,) + tuple(full if on else 1 for full, on in zip(PARAM_SHAPE, c.param))
        assert rates.shape == (c.S, int(np.prod(R.shape[1:])))
        for axis, on in enumerate(c.param):
            if on:
                assert np.all(np.diff(R, axis=axis + 1) != 0)
        assert bool(flags & _native.PRED_AUX_ROWS) == c.param[0] and bool(flags & _native.PRED_AUX_COLS) == c.param[1] and \
            bool(flags & _native.PRED_AUX_DEPTH) == c.param[2]


@pytest.mark.parametrize("case", SUMMARY_CASES, ids=lambda c: "S%d-N%d-%dx%d-K%d-%s-nq%d" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4], len(c[5])))
def test_summary_cases_are_admissible(case):
    S, N, MT, K, transform, q = case
    assert 1 <= S <= SUMMARY_LIMIT and summary_geom(S)[2] <= CU_LDS and MT[1] >= 2
    Ws, Vs = summary_inputs(S, N, MT, K)
    Mu, mean, quant = summary_reference(Ws, Vs, transform, q)
    assert quant.shape == (len(q), N) + MT and np.all(np.isfinite(Mu))
    if transform != "ilogit":                                          # dyadic: the values, their sums and the mean's numerator exact
        scale = 16 if transform is None else 256
        assert np.array_equal(scale * Mu, np.round(scale * Mu)) and np.abs(scale * Mu).sum(axis=0).max() < 2.0 ** 53


@pytest.mark.parametrize("fam", FAMILIES)
def test_batch_cases_hold_both_sides(fam):
    eta, aux = batch_case(fam)
    assert eta.shape == (BATCH_FULL,) and np.array_equal(16 * eta, np.round(16 * eta))
    c = Case(fam, 1, 1, 1, 1, 2, 3)
    have = branches(c, eta, aux)
    assert all(have.values()), have
    if fam in POSITIVE:
        assert eta.min() > 0
