"""Posterior ranking on the GPU (csrc/btf_ranking.h via utils.posterior_ranking and BayesianTensorFiltering.posterior_ranking)
against the numpy definition of functionalmf_amd/ranking.py.

Everything after the functional values is an integer count followed by one division, so every comparison here is exact
(np.array_equal): against the definition applied to the values posterior_functionals(pointwise=True) returns on the same
samples, and - on inputs whose gaps the test checks first - against the definition applied to curves formed on the host.

One shape throughout: N = 70 (a full 64-row block and a partial one), M = 5 (not a power of two), T = 7, K = 3, S = 37.
Rows 3 and 9 of every W_s are identical: along="rows" has a bit-equal pair in every group."""
import ctypes as C

import numpy as np
import pytest

from functionalmf_amd import _native, functionals, ranking
from functionalmf_amd.factor import GaussianBayesianTensorFiltering
from functionalmf_amd.utils import posterior_functionals, posterior_ranking

pytestmark = pytest.mark.gpu

S, N, M, T, K = 37, 70, 5, 7, 3
LEVEL = 2.0                      # of `crossing`: some of the curves (sd about sqrt(3) per point) never reach it
TOP = (1, 2, 5, 9)               # 9 > M: certain along="cols"
PAIRS = np.array([(0, 0, 0, 1), (3, 2, 9, 2), (9, 4, 3, 4), (69, 4, 0, 0), (5, 1, 5, 1), (64, 3, 12, 0)])
SAMPLE_BYTES = N * M * 8         # of staging scratch per sample
SEED = 3


def _states(seed=SEED):
    rs = np.random.RandomState(seed)
    Ws, Vs = rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K))
    Ws[:, 9] = Ws[:, 3]
    return Ws, Vs


@pytest.fixture(scope="module")
def states():
    return _states()


@pytest.fixture(scope="module")
def values(states):
    """{name: (S,N,M)}: the device's own functional values, computed once."""
    out = posterior_functionals(*states, which=("auc", "crossing"), level=LEVEL, pointwise=True)
    f = {k: out[k]["pointwise"] for k in ("auc", "crossing")}
    for v in f.values():
        v.setflags(write=False)
    return f


def _same(got, ref, what=""):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (what, k, got[k].dtype, got[k].shape)
            assert np.array_equal(got[k], v), (what, k, np.abs(got[k].astype(float) - v).max())
        else:
            assert got[k] == v, (what, k, got[k], v)


@pytest.mark.parametrize("which", ["auc", "crossing"])
@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("along", ["cols", "rows"])
def test_exact_agreement_with_the_definition(states, values, along, order, which):
    f = values[which]
    if which == "crossing":
        undefined = np.isnan(f)
        assert undefined.any() and not undefined.all()
        assert (undefined.any(axis=0) & ~undefined.all(axis=0)).any()       # some curves cross in some samples only
    kw = dict(which=which, along=along, order=order, top=TOP, level=LEVEL if which == "crossing" else None, pairs=PAIRS,
              pointwise=True)
    got = posterior_ranking(*states, **kw)
    ref = ranking.reference(f, which=which, along=along, order=order, top=TOP, pairs=PAIRS, pointwise=True)
    _same(got, ref, (along, order, which))
    assert got["ranks"].min() == 1 and got["ranks"].max() == (M if along == "cols" else N)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_ties_go_to_the_smaller_index(states, values, order):
    for which in ("auc", "crossing"):
        f = values[which]
        assert np.array_equal(f[:, 3], f[:, 9], equal_nan=True)              # bit-equal values in every along="rows" group
        r = posterior_ranking(*states, which=which, along="rows", order=order, level=LEVEL, pointwise=True)["ranks"]
        assert (r[:, 3] < r[:, 9]).all(), which
        ok = ~np.isnan(f[:, 3])                                               # equal defined values are neighbours
        assert ok.any() and np.array_equal(r[:, 9][ok], r[:, 3][ok] + 1), which


@pytest.mark.parametrize("along", ["cols", "rows"])
def test_from_scratch_against_host_formed_curves(states, along):
    Ws, Vs = states
    Mu = np.einsum("znk,zmtk->znmt", Ws, Vs)
    f = functionals.curve_functionals(Mu)["auc"]
    # the inputs' own condition: apart from the deliberate tie (row 9 = row 3) the smallest gap between two values of a
    # group exceeds 1e-9 of the values' scale, so that rounding (about 1e-16 of it) cannot reorder them
    g = np.delete(f, 9, axis=1) if along == "rows" else f
    gaps = np.diff(np.sort(g, axis=2 if along == "cols" else 1), axis=2 if along == "cols" else 1)
    assert gaps.min() > 1e-9 * np.abs(f).max(), gaps.min()
    for order in ("ascending", "descending"):
        got = posterior_ranking(Ws, Vs, which="auc", along=along, order=order, top=TOP, pointwise=True)
        ref = ranking.reference(f, along=along, order=order, top=TOP, pointwise=True)
        _same(got, ref, (along, order))


@pytest.mark.parametrize("nchunk_samples", [13, 5, 1])
def test_chunking_is_pure_geometry(states, nchunk_samples):
    assert -(-S // nchunk_samples) >= 3
    for along, which in (("cols", "crossing"), ("rows", "auc")):
        kw = dict(which=which, along=along, order="descending", top=TOP, level=LEVEL, pairs=PAIRS, pointwise=True)
        _same(posterior_ranking(*states, _scratch_bytes=nchunk_samples * SAMPLE_BYTES, **kw), posterior_ranking(*states, **kw),
              (along, nchunk_samples))


@pytest.mark.parametrize("along", ["cols", "rows"])
def test_invariants(states, along):
    out = posterior_ranking(*states, which="crossing", level=LEVEL, along=along, top=TOP)
    axis, L = (1, M) if along == "cols" else (0, N)
    counts = np.rint(out["p_top"] * S)
    assert np.array_equal(counts / S, out["p_top"])
    for k, c in zip(TOP, counts):
        assert np.array_equal(c.sum(axis=axis), np.full(c.shape[1 - axis], S * min(k, L)))
    total = out["expected_rank"].sum(axis=axis)
    assert np.abs(total - L * (L + 1) / 2).max() <= 1e-12 * L * (L + 1) / 2
    assert (out["rank_var"] >= 0).all()


def test_groups_of_one(states):
    Ws, Vs = states
    out = posterior_ranking(Ws, Vs[:, :1], which="auc", along="cols", top=(1, 3), pointwise=True)
    assert np.array_equal(out["ranks"], np.ones((S, N, 1), dtype=np.int32))
    assert np.array_equal(out["expected_rank"], np.ones((N, 1))) and np.array_equal(out["rank_var"], np.zeros((N, 1)))
    assert np.array_equal(out["p_top"], np.ones((2, N, 1)))
    one = posterior_ranking(Ws[:1], Vs[:1], which="max", along="rows", order="descending")       # a single sample
    assert np.array_equal(one["rank_var"], np.zeros((N, M))) and one["nsamples"] == 1
    assert np.array_equal(np.sort(one["expected_rank"], axis=0), np.tile(np.arange(1.0, N + 1)[:, None], (1, M)))


@pytest.fixture(scope="module")
def fitted():
    rs = np.random.RandomState(1)
    W, V = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.4, size=(N, M, T, 2))
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=5)
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        m.posterior_ranking()
    res = m.run_gibbs(Y, nburn=5, nsamples=S, verbose=False)
    return m, res


def test_entry_points_agree_bit_for_bit(fitted):
    m, res = fitted
    for along, which in (("cols", "auc"), ("rows", "crossing")):
        kw = dict(which=which, along=along, top=TOP, level=0.1, pairs=PAIRS, pointwise=True)
        a = m.posterior_ranking(**kw)
        _same(m.posterior_ranking(results=res, **kw), a, along)
        _same(posterior_ranking(res["W"], res["V"], **kw), a, along)
        f = m.posterior_functionals(which=(which,), level=0.1, pointwise=True)[which]["pointwise"]
        _same(a, ranking.reference(f, which=which, along=along, top=TOP, pairs=PAIRS, pointwise=True), along)
        assert a["nsamples"] == S


def test_pairs(states, values):
    for which in ("auc", "crossing"):
        out = posterior_ranking(*states, which=which, level=LEVEL, pairs=PAIRS)
        less, defined = ranking.pair_probabilities(values[which], PAIRS)
        assert np.array_equal(out["prob_less"], less) and np.array_equal(out["prob_defined"], defined)
        assert out["prob_less"][1] == 0 and out["prob_less"][2] == 0 and out["prob_less"][4] == 0      # identical rows; itself
        assert "ranks" not in out
    assert less.max() > 0 and 0 < defined.min() < 1                             # (crossing: undefined in some samples)
    assert "prob_less" not in posterior_ranking(*states)


def test_error_codes_of_the_c_entry_points(fitted):
    lib = _native.load()
    d, ip = _native.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, top, buf = np.linspace(0, 1, T), np.array([1], dtype=np.int32), np.zeros(8)

    def stateless(S_, N_, M_, along):
        tail = (0, 0, d(x), float("nan"), along, 0, ip(top), 1, None, 0, None, None, None, None, None, None, 0)
        return lib.btf_posterior_ranking(0, S_, N_, M_, T, 1, d(buf), d(buf), *tail)     # refused before anything is read

    assert stateless(1, 1, 4097, 0) == _native.BTF_EINVAL and b"4096" in lib.btf_last_error(None)
    assert stateless(1, 4097, 1, 1) == _native.BTF_EINVAL
    assert stateless(8193, 1, 1, 0) == _native.BTF_EINVAL and b"8192" in lib.btf_last_error(None)
    m, _ = fitted
    e, v, p = np.zeros((N, M)), np.zeros((N, M)), np.zeros((1, N, M))
    tail = (0, 0, d(x), float("nan"), 0, 0, ip(top), 1, None, 0, d(e), d(v), d(p), None, None, None, 0)
    assert lib.btf_collect_ranking(m._ctx.h, S + 1, *tail) == _native.BTF_ESTATE
    assert lib.btf_collect_ranking(m._ctx.h, S, *tail) == _native.BTF_OK and e.min() >= 1
