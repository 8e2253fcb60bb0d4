"""Posterior ranking on the GPU at every tile geometry of rank_kernel (csrc/btf_ranking.h, launched by ranking_run of
csrc/btf_analysis.hip), next to tests/test_gpu_ranking.py, which holds one shape.

Every comparison is exact (np.array_equal).  The device's ranks, expected_rank, rank_var, p_top and pair probabilities are
compared with ranking.reference applied to the device's own posterior_functionals(pointwise=True) values; ranking.ranks
itself is checked against a second definition written here (`_count_ranks`: 1 + #{strictly before in value} + #{equal value
and smaller index} by O(L^2) comparison counts, nan last), so that the definition module is not its own judge.  (The
from-scratch comparison against host-formed curves stays with the small shape of test_gpu_ranking.py: at L in the thousands
the smallest gap between normal draws falls below its 1e-9 guard.)

The geometry, from ranking_run:  L = members of a group (M along="cols", N along="rows"), Lp = the power of two >= L,
G = max(1, min(groups, 4096 / Lp, 64)) groups per workgroup, tiles = ceil(groups / G), E = G Lp <= 4096 LDS slots of which a
thread owns E / 512 (at most RANK_EPT = 8), ys = min(sc, ceil(1024 / tiles)) sample slices of a chunk of sc samples: a
workgroup takes the samples blockIdx.y, blockIdx.y + ys, ... of its tile.  `_geom` restates it and GROUPS lists
(L, groups) -> (Lp, G, tiles).

A slice of 256 samples (N = 2048 along cols, M = 2, S = 8192: 32 tiles x 32 slices) is run without the pointwise ranks:
2.6 s on an MI355X, of which 1.7 s form and fetch the 268 MB of functional values the reference needs.  The 16-bit p_top
counters cannot overflow while a chunk holds at most 8192 samples, which ranking_check enforces."""
import ctypes as C
import functools

import numpy as np
import pytest

from functionalmf_amd import _native, functionals, ranking
from functionalmf_amd.utils import posterior_functionals, posterior_ranking

pytestmark = pytest.mark.gpu

LEVEL = 1.0
ORDERS = ("ascending", "descending")
ALONGS = ("cols", "rows")


def _geom(L, groups):
    """(Lp, G, tiles) of ranking_run."""
    Lp = 1
    while Lp < L:
        Lp <<= 1
    G = max(1, min(groups, min(4096 // Lp, 64)))
    return Lp, G, -(-groups // G)


def _ys(sc, tiles):
    return max(1, min(sc, -(-1024 // tiles)))


# L -> groups: more than one tile, and a last tile with fewer groups than G wherever G > 1
#   L      groups   Lp    G   tiles  E = G Lp (slots a thread owns)
#   1        65      1   64     2      64   (1)   no sort at all
#   2        65      2   64     2     128   (1)   no padding
#   3        65      4   64     2     256   (1)
#   4        65      4   64     2     256   (1)   no padding
#   5        65      8   64     2     512   (1)
#   8        65      8   64     2     512   (1)   no padding
#   9        65     16   64     2    1024   (2)
#   63       65     64   64     2    4096   (8)
#   64       65     64   64     2    4096   (8)   no padding, every register slot, last tile of one group
#   65       33    128   32     2    4096   (8)   G limited by 4096 / Lp
#   128      33    128   32     2    4096   (8)
#   129      17    256   16     2    4096   (8)
#   1024      5   1024    4     2    4096   (8)
#   1025      3   2048    2     2    4096   (8)
#   2049      2   4096    1     2    4096   (8)
#   4096      2   4096    1     2    4096   (8)   no padding
GROUPS = {1: 65, 2: 65, 3: 65, 4: 65, 5: 65, 8: 65, 9: 65, 63: 65, 64: 65, 65: 33, 128: 33, 129: 17, 1024: 5, 1025: 3,
          2049: 2, 4096: 2}
GEOM = {1: (1, 64, 2), 2: (2, 64, 2), 3: (4, 64, 2), 4: (4, 64, 2), 5: (8, 64, 2), 8: (8, 64, 2), 9: (16, 64, 2),
        63: (64, 64, 2), 64: (64, 64, 2), 65: (128, 32, 2), 128: (128, 32, 2), 129: (256, 16, 2), 1024: (1024, 4, 2),
        1025: (2048, 2, 2), 2049: (4096, 1, 2), 4096: (4096, 1, 2)}
LENGTHS = sorted(GROUPS)
CROSSING = set(LENGTHS[1::2])               # every other length ranks `crossing`, the others `auc`
S_SMALL, T, K = 3, 3, 2


def _count_ranks(f, along, order):
    """The second definition: comparison counts within every group of f (S,N,M); int64 ranks."""
    g = np.asarray(f, dtype=float)
    if along == "rows":
        g = np.swapaxes(g, 1, 2)                                   # groups along the last axis
    a, b = g[..., :, None], g[..., None, :]                        # the member, the others
    na, nb = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        before = ((b < a) if order == "ascending" else (b > a)) | (na & ~nb)       # a defined value before an undefined one
        equal = (b == a) | (na & nb)
    idx = np.arange(g.shape[-1])
    r = 1 + before.sum(axis=-1) + (equal & (idx[None, :] < idx[:, None])).sum(axis=-1)
    return np.swapaxes(r, 1, 2) if along == "rows" else r


def _same(got, ref, what=""):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (what, k, got[k].dtype, got[k].shape)
            assert np.array_equal(got[k], v), (what, k, np.abs(got[k].astype(float) - v).max())
        else:
            assert got[k] == v, (what, k, got[k], v)


def _shape(L, along):
    return (GROUPS[L], L) if along == "cols" else (L, GROUPS[L])


def _corner_pairs(N, M):
    """(i, j, i2, j2) pairs that span the first and the last tile."""
    return np.array([(0, 0, N - 1, M - 1), (N - 1, M - 1, 0, 0), (N - 1, 0, 0, M - 1), (0, 0, 0, 0), (N // 2, M // 2, N - 1, 0)])


@functools.lru_cache(maxsize=None)
def _length_case(L, along):
    """(Ws, Vs, which, the device's own values (S,N,M)) of one group length, formed once.  The `crossing` cases hold, in
    sample 0, one group that never crosses (a zero row / column of factors) and one in which exactly one member does (a
    tiny row / column against one large member whose curve is (0, 2, 0))."""
    N, M = _shape(L, along)
    rs = np.random.RandomState(1000 * L + (along == "rows"))
    Ws, Vs = rs.normal(size=(S_SMALL, N, K)), rs.normal(size=(S_SMALL, M, T, K))
    which = "crossing" if L in CROSSING else "auc"
    if which == "crossing":
        bump, last = np.array([0.0, 2.0, 0.0]), GROUPS[L] - 1      # in sample 0 only: the other samples stay random
        if along == "cols":                                        # a group is a row
            Ws[0, 0] = 0.0
            Ws[0, last] = (1e-3, 0.0)
            Vs[0, M - 1, :, 0] = 1e3 * bump
        else:                                                      # a group is a column
            Vs[0, 0] = 0.0
            Vs[0, last] = 0.0
            Vs[0, last, :, 0] = 1e-3 * bump
            Ws[0, N - 1, 0] = 1e3
    out = posterior_functionals(Ws, Vs, which=(which,), level=LEVEL, pointwise=True)
    f = out[which]["pointwise"]
    for a in (Ws, Vs, f):
        a.setflags(write=False)
    return Ws, Vs, which, f


def test_the_geometry_table_is_the_formula():
    for L in LENGTHS:
        Lp, G, tiles = _geom(L, GROUPS[L])
        assert (Lp, G, tiles) == GEOM[L], L
        assert tiles > 1 and (G == 1 or GROUPS[L] % G != 0), L     # more than one tile; the last one is partial
    assert _geom(64, 65) == (64, 64, 2) and _geom(65, 33)[1] == 32 and _geom(1025, 3)[1] == 2 and _geom(4096, 2)[1] == 1
    assert len(CROSSING) == len(LENGTHS) // 2


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("along", ALONGS)
@pytest.mark.parametrize("L", LENGTHS, ids=["L%d-Lp%d-G%d-tiles%d" % ((L,) + GEOM[L]) for L in LENGTHS])
def test_group_lengths(L, along, order):
    Ws, Vs, which, f = _length_case(L, along)
    N, M = _shape(L, along)
    axis = 2 if along == "cols" else 1
    if which == "crossing":
        undefined = np.isnan(f)
        assert undefined.any() and not undefined.all()
        assert undefined.all(axis=axis).any()                                  # a group with no defined member
        assert ((~undefined).sum(axis=axis) == 1).any()                        # a group with exactly one
        assert (undefined.any(axis=0) & ~undefined.all(axis=0)).any()          # undefined in some samples only
    pairs = _corner_pairs(N, M)
    top = (1, 2, L) if L > 2 else (1, 2)
    got = posterior_ranking(Ws, Vs, which=which, along=along, order=order, top=top, level=LEVEL, pairs=pairs, pointwise=True)
    ref = ranking.reference(f, which=which, along=along, order=order, top=top, pairs=pairs, pointwise=True)
    _same(got, ref, (L, along, order))
    assert got["ranks"].min() == 1 and got["ranks"].max() == L
    if L <= 129:
        assert np.array_equal(ranking.ranks(f, along, order), _count_ranks(f, along, order)), (L, along, order)
    elif L == 4096:                                                            # one group: sample 1, the last group
        one = f[1:2, -1:, :] if along == "cols" else f[1:2, :, -1:]
        assert np.array_equal(ranking.ranks(one, along, order), _count_ranks(one, along, order))
        assert np.array_equal(got["ranks"][1:2, -1:, :] if along == "cols" else got["ranks"][1:2, :, -1:],
                              _count_ranks(one, along, order))


# ---------------------------------------------------------------- several samples per workgroup
# name -> (S, N, M, T, K), along, samples per chunk of the chunked call
MANY = {
    "S8192": ((8192, 3, 2, 2, 1), "cols", 3000),     # one tile, ys = 1024: eight samples a slice; chunks 3000, 3000, 2192
    "N2048": ((70, 2048, 2, 2, 1), "cols", 48),      # tiles = 32, ys = 32: three samples in slices 0..5, two in the others
}


@functools.lru_cache(maxsize=None)
def _many_case(name):
    (S, N, M, T_, K_), along, _ = MANY[name]
    rs = np.random.RandomState(len(name) + S)
    Ws, Vs = rs.normal(size=(S, N, K_)), rs.normal(size=(S, M, T_, K_))
    out = posterior_functionals(Ws, Vs, which=("auc", "crossing"), level=0.3, pointwise=True)
    f = {k: out[k]["pointwise"] for k in ("auc", "crossing")}
    for a in (Ws, Vs) + tuple(f.values()):
        a.setflags(write=False)
    return Ws, Vs, f


def test_the_sample_slices_are_the_ones_meant():
    (S, N, M, _, _), _, chunk = MANY["S8192"]
    Lp, G, tiles = _geom(M, N)
    assert tiles == 1 and _ys(S, tiles) == 1024 and S // 1024 == 8
    assert S % chunk not in (0, chunk) and _ys(chunk, tiles) == 1024 and _ys(S % chunk, tiles) == 1024
    (S, N, M, _, _), _, chunk = MANY["N2048"]
    Lp, G, tiles = _geom(M, N)
    assert (G, tiles) == (64, 32) and _ys(S, tiles) == 32 and S % 32 == 6 and S // 32 == 2
    assert 0 < S % chunk < chunk and _ys(chunk, tiles) == 32 and _ys(S % chunk, tiles) == S % chunk


@pytest.mark.parametrize("which,order", [("auc", "descending"), ("crossing", "ascending")])
@pytest.mark.parametrize("name", sorted(MANY))
def test_several_samples_per_workgroup(name, which, order):
    (S, N, M, _, _), along, chunk = MANY[name]
    Ws, Vs, f = _many_case(name)
    if which == "crossing":
        undefined = np.isnan(f[which])
        assert undefined.any() and not undefined.all()
    pairs = _corner_pairs(N, M)
    kw = dict(which=which, along=along, order=order, top=(1, 2), level=0.3, pairs=pairs, pointwise=True)
    got = posterior_ranking(Ws, Vs, **kw)
    ref = ranking.reference(f[which], which=which, along=along, order=order, top=(1, 2), pairs=pairs, pointwise=True)
    _same(got, ref, (name, which))
    if which == "auc":                                              # the order of a row's two columns varies over the samples
        assert 1 < got["expected_rank"].min() and got["expected_rank"].max() < 2 and got["rank_var"].min() > 0
    chunked = posterior_ranking(Ws, Vs, _scratch_bytes=chunk * N * M * 8, **kw)
    _same(chunked, got, (name, which, "chunked against unchunked"))
    _same(chunked, ref, (name, which, "chunked against the reference"))
    assert np.array_equal(ranking.ranks(f[which][:64], along, order), _count_ranks(f[which][:64], along, order))


def test_a_slice_of_256_samples():
    """N = 2048 along cols, M = 2, S = 8192: every workgroup adds 256 samples into its registers before the atomics (the
    16-bit p_top counts pass 255)."""
    S, N, M = 8192, 2048, 2
    Lp, G, tiles = _geom(M, N)
    assert tiles == 32 and _ys(S, tiles) == 32 and S // 32 == 256
    rs = np.random.RandomState(1)
    Ws, Vs = rs.normal(size=(S, N, 1)), rs.normal(size=(S, M, 2, 1))
    f = posterior_functionals(Ws, Vs, which=("auc",), pointwise=True)["auc"]["pointwise"]
    got = posterior_ranking(Ws, Vs, which="auc", along="cols", order="descending", top=(1, 2))
    _same(got, ranking.reference(f, which="auc", along="cols", order="descending", top=(1, 2)), "256 samples a slice")
    assert 0.4 < got["p_top"][0].min() and got["p_top"][0].max() < 0.6 and (got["p_top"][1] == 1).all()


# ---------------------------------------------------------------- top
@pytest.mark.parametrize("along", ALONGS)
@pytest.mark.parametrize("L", [5, 64])
def test_eight_top_entries_up_to_the_clamp(L, along):
    Ws, Vs, which, f = _length_case(L, along)
    top = (L + 1, 1, 100000, L - 1, 4096, L, 4097, 2)               # eight distinct entries, in no order
    assert len(set(top)) == ranking.MAX_TOP == 8
    for order in ORDERS:
        got = posterior_ranking(Ws, Vs, which=which, along=along, order=order, top=top, level=LEVEL)
        ref = ranking.reference(f, which=which, along=along, order=order, top=top)
        _same(got, ref, (L, along, order))
        for k, t in enumerate(top):
            if t >= L:
                assert (got["p_top"][k] == 1.0).all(), (L, along, t)
            else:
                assert (got["p_top"][k] < 1.0).any(), (L, along, t)
        counts = np.rint(got["p_top"] * S_SMALL)
        groups_axis = 1 if along == "cols" else 0
        for k, t in enumerate(top):                                 # min(t, L) members of every group are in its top t
            assert np.array_equal(counts[k].sum(axis=groups_axis), np.full(counts[k].shape[1 - groups_axis], float(S_SMALL * min(t, L))))


def test_nine_top_entries_are_refused_by_the_library():
    lib = _native.load()
    d, ip = _native.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, buf = np.linspace(0, 1, 3), np.zeros(64)
    top = np.arange(1, 10, dtype=np.int32)

    def call(ntop):
        tail = (0, 0, d(x), float("nan"), 0, 0, ip(top), ntop, None, 0, None, None, None, None, None, None, 0)
        return lib.btf_posterior_ranking(0, 1, 1, 1, 3, 1, d(buf), d(buf), *tail)     # refused before anything is read

    assert call(9) == _native.BTF_EINVAL and call(0) == _native.BTF_EINVAL
    with pytest.raises(ValueError, match="top"):
        posterior_ranking(np.zeros((1, 1, 1)), np.zeros((1, 1, 3, 1)), top=tuple(range(1, 10)))


# ---------------------------------------------------------------- infinities, zeros and exact ties
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("along", ALONGS)
def test_infinite_values_rank_as_values_and_tie_by_index(along, order):
    """`square` of factors scaled until w v overflows: the max of such a curve is +inf.  Rows 1, 4 and columns 0, 3 are
    scaled, so every group holds several equal infinities beside finite values (K = 1: no inf - inf inside a curve)."""
    S, N, M = 6, 9, 7
    rs = np.random.RandomState(11)
    Ws, Vs = rs.normal(size=(S, N, 1)), rs.normal(size=(S, M, 3, 1))
    Ws[:, [1, 4]] *= 1e160
    Vs[:, [0, 3]] *= 1e160
    f = posterior_functionals(Ws, Vs, which=("max",), transform="square", pointwise=True)["max"]["pointwise"]
    inf = np.isposinf(f)
    assert not np.isnan(f).any() and inf[:, [1, 4]].all() and inf[:, :, [0, 3]].all() and np.isfinite(f[:, 0, 1:3]).all()
    axis = 2 if along == "cols" else 1
    assert (inf.sum(axis=axis) >= 2).all() and (~inf).any(axis=axis).any()
    top = (1, 2, 3)
    got = posterior_ranking(Ws, Vs, which="max", transform="square", along=along, order=order, top=top, pointwise=True,
                            pairs=_corner_pairs(N, M))
    ref = ranking.reference(f, which="max", along=along, order=order, top=top, pointwise=True, pairs=_corner_pairs(N, M))
    _same(got, ref, (along, order))
    assert np.array_equal(got["ranks"], _count_ranks(f, along, order))
    r = got["ranks"]
    if along == "rows":                                             # rows 1 and 4 are the two infinities of such a column
        mixed = [j for j in range(M) if j not in (0, 3)]
        assert np.array_equal(r[:, 4][:, mixed], r[:, 1][:, mixed] + 1)
        assert (r[:, 1][:, mixed] == (1 if order == "descending" else N - 1)).all()
        assert np.array_equal(r[:, :, 0], np.tile(np.arange(1, N + 1), (S, 1)))      # a column of nothing but +inf: by index
    else:
        mixed = [i for i in range(N) if i not in (1, 4)]           # columns 0 and 3 are the two infinities of such a row
        assert np.array_equal(r[:, mixed, 3], r[:, mixed, 0] + 1)
        assert (r[:, mixed, 0] == (1 if order == "descending" else M - 1)).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("along", ALONGS)
def test_exact_ties_and_zeros_with_integer_factors(along, order):
    """Integer factors: every curve value is an exact small integer, so `min` takes few distinct values, many of them 0."""
    S, N, M = 7, 40, 9
    rs = np.random.RandomState(5)
    Ws = rs.randint(-2, 3, size=(S, N, 2)).astype(float)
    Vs = rs.randint(-1, 2, size=(S, M, 3, 2)).astype(float)
    f = posterior_functionals(Ws, Vs, which=("min",), pointwise=True)["min"]["pointwise"]
    assert np.array_equal(f, np.rint(f)) and (f == 0).mean() > 0.1 and len(np.unique(f)) <= 12
    got = posterior_ranking(Ws, Vs, which="min", along=along, order=order, top=(1, 3), pointwise=True)
    _same(got, ranking.reference(f, which="min", along=along, order=order, top=(1, 3), pointwise=True), (along, order))
    assert np.array_equal(got["ranks"], _count_ranks(f, along, order))
    # -0.0 and +0.0 are one value in both definitions (the device's keys map -0 to +0 before the bit pattern is read)
    z = np.array([[[0.0, -0.0, 1.0, -0.0, np.nan, 0.0, -np.inf, np.inf, np.nan]]])
    for zz, al in ((z, "cols"), (np.swapaxes(z, 1, 2), "rows")):
        rr = ranking.ranks(zz, al, order)
        assert np.array_equal(rr, _count_ranks(zz, al, order))
        assert np.array_equal(np.sort(rr.ravel()[[0, 1, 3, 5]]), rr.ravel()[[0, 1, 3, 5]])       # the four zeros: by index


# ---------------------------------------------------------------- nembeds
@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds(nembeds):
    S, N, M = 5, 70, 5
    rs = np.random.RandomState(40 + nembeds)
    Ws, Vs = rs.normal(size=(S, N, nembeds)), rs.normal(size=(S, M, 3, nembeds))
    f = posterior_functionals(Ws, Vs, which=("auc",), pointwise=True)["auc"]["pointwise"]
    pairs = _corner_pairs(N, M)
    got = posterior_ranking(Ws, Vs, which="auc", along="cols", order="descending", top=(1, 2, 5), pairs=pairs, pointwise=True)
    _same(got, ranking.reference(f, along="cols", order="descending", top=(1, 2, 5), pairs=pairs, pointwise=True), nembeds)
    assert np.array_equal(got["ranks"], _count_ranks(f, "cols", "descending"))
    # the values are this nembeds' curves: against host-formed curves, to the tolerance of tests/test_gpu_functionals.py
    Mu = np.einsum("znk,zmtk->znmt", Ws, Vs)
    host = functionals.curve_functionals(Mu)["auc"]
    assert np.abs(f - host).max() <= 1e-12 * max(1.0, np.abs(Mu).max())
