"""Posterior feature association on the GPU (csrc/btf_assoc.h via utils.posterior_feature_association and
BayesianTensorFiltering.posterior_feature_association) against the numpy definition of functionalmf_amd/association.py.

The definition is applied to the values posterior_functionals(pointwise=True) returns on the same samples (the staged
values are those bit for bit).  The device takes the moment route (Sxx = u' C u, ...), the definition forms x = W U'
directly: r agrees to 1e-12 absolute (the identity itself holds to 6.7e-16 at this shape), slope and intercept to 1e-11 of
the largest magnitude; the sets and counts - where a sample is defined, `defined`, `prob_positive`, n - agree exactly, which
the test makes sure of by first asserting that no defined sample has Sxx or Syy within 1e-8 of its scale.

The base shape: S = 37 (no power of two for the sort), N = 70 (a full 64-row block and a partial one), M = 5, T = 7, K = 3,
F = 6.  Standard normal inputs with: feature 4 all zero (a constant x: Sxx = 0, undefined in every sample); level = 2.0 for
`crossing` (about half of the values undefined); column 0 of V scaled by 1e-3 in ten samples (it never crosses there: n = 0
and `defined` below 1 for a whole column)."""
import numpy as np
import pytest

from functionalmf_amd import association
from functionalmf_amd.factor import GaussianBayesianTensorFiltering
from functionalmf_amd.utils import posterior_feature_association, posterior_functionals

pytestmark = pytest.mark.gpu

S, N, M, T, K, F = 37, 70, 5, 7, 3, 6
LEVEL = 2.0
PAIRS = np.array([(0, 0), (4, 1), (5, 4), (2, 0), (3, 3)])
SAMPLE_BYTES = N * M * 8         # of staging scratch per sample
STATS = ("r", "slope")
R_TOL, REL_TOL = 1e-12, 1e-11


def _states(seed=3, S=S, N=N, M=M, T=T, K=K, F=F):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K)), rs.normal(size=(S, F, K))


@pytest.fixture(scope="module")
def states():
    Ws, Vs, Us = _states()
    Us[:, 4] = 0.0
    Vs[:10, 0] *= 1e-3
    for a in (Ws, Vs, Us):
        a.setflags(write=False)
    return Ws, Vs, Us


@pytest.fixture(scope="module")
def values(states):
    """{name: (S,N,M)}: the device's own functional values, computed once."""
    out = posterior_functionals(states[0], states[1], which=("auc", "crossing"), level=LEVEL, pointwise=True)
    f = {k: out[k]["pointwise"] for k in ("auc", "crossing")}
    for v in f.values():
        v.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def default_call(states):
    return posterior_feature_association(*states, which="crossing", stats=STATS, level=LEVEL, pairs=PAIRS)


def _same(got, ref, what=""):
    """Bit for bit: the same keys, shapes and values (nan in the same places)."""
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k, v in ref.items():
        if isinstance(v, dict):
            _same(got[k], v, (what, k))
        elif isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (what, k, got[k].dtype, got[k].shape)
            assert np.array_equal(got[k], v, equal_nan=True), (what, k)
        else:
            assert got[k] == v, (what, k, got[k], v)


def _close(got, ref, tol, what):
    """nan in the same places; elsewhere |got - ref| <= tol."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print("%s: max error %.3g (tolerance %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _well_conditioned(y, Ws, Us):
    """No defined sample has Sxx or Syy within 1e-8 of its scale (the uncentred sum of squares): rounding cannot flip the
    defined set."""
    for s in range(y.shape[0]):
        X = Us[s] @ Ws[s].T
        for j in range(y.shape[2]):
            I = ~np.isnan(y[s, :, j])
            if I.sum() < 3:
                continue
            n, xbar, ybar, sxx, syy, sxy = association._regress(X[:, I], y[s, I, j])
            xs, ys = (X[:, I] ** 2).sum(axis=1), (y[s, I, j] ** 2).sum()
            assert syy > 1e-8 * ys, (s, j, syy, ys)
            assert ((sxx == 0) | (sxx > 1e-8 * xs)).all(), (s, j, sxx, xs)      # exactly constant (feature 4) or far from it


def _check_summaries(got, ref, what):
    assert got["which"] == ref["which"] and got["stats"] == ref["stats"] and got["nsamples"] == ref["nsamples"]
    assert np.array_equal(got["defined"], ref["defined"]), what
    assert np.array_equal(got["n_mean"], ref["n_mean"]), what
    for k in ref["stats"]:
        g, r = got[k], ref[k]
        scale = 1.0 if k == "r" else float(np.nanmax(np.abs(r["values"] if "values" in r else r["quantiles"])))
        tol = R_TOL if k == "r" else REL_TOL * scale
        assert np.array_equal(g["prob_positive"], r["prob_positive"], equal_nan=True), (what, k)
        _close(g["mean"], r["mean"], tol, (what, k, "mean"))
        _close(g["var"], r["var"], 2 * tol * max(scale, 1.0), (what, k, "var"))      # d var = 2 sd d value, sd <= scale
        _close(g["quantiles"], r["quantiles"], tol, (what, k, "quantiles"))
        if "values" in r:
            _close(g["values"], r["values"], tol, (what, k, "values"))


def _check_of_means(got, ref, what):
    assert set(got) == set(ref)
    assert np.array_equal(got["n"], ref["n"]), what
    _close(got["r"], ref["r"], R_TOL, (what, "of_means r"))
    scale = max(float(np.nanmax(np.abs(ref["slope"]))), float(np.nanmax(np.abs(ref["intercept"]))))
    for k in ("slope", "intercept", "stderr"):
        _close(got[k], ref[k], REL_TOL * scale, (what, "of_means", k))
    for k in ("sd_x", "sd_y"):
        _close(got[k], ref[k], REL_TOL * float(np.nanmax(ref[k])), (what, "of_means", k))


@pytest.mark.parametrize("which", ["auc", "crossing"])
def test_agreement_with_the_definition(states, values, which):
    Ws, Vs, Us = states
    y = values[which]
    if which == "crossing":
        undefined = np.isnan(y)
        assert 0.3 < undefined.mean() < 0.8 and undefined[:10, :, 0].all()
    _well_conditioned(y, Ws, Us)
    allpairs = np.array([(f, j) for f in range(F) for j in range(M)])
    got = posterior_feature_association(Ws, Vs, Us, which=which, stats=STATS, level=LEVEL if which == "crossing" else None,
                                        q=(0, 5, 50, 95, 100), pairs=allpairs)
    ref = association.reference(y, Ws, Us, which=which, stats=STATS, q=(0, 5, 50, 95, 100), pairs=allpairs)
    _check_summaries(got, ref, which)
    # the set patterns: feature 4 is constant; crossing: column 0 has no defined row in ten samples
    assert np.isnan(got["r"]["values"].reshape(F, M, S)[4]).all() and (got["defined"][4] == 0).all()
    assert np.isnan(got["r"]["mean"][4]).all() and np.isnan(got["slope"]["quantiles"][:, 4]).all()
    if which == "crossing":
        assert (got["defined"][[0, 1, 2, 3, 5], 0] <= (S - 10) / S).all() and got["n_mean"][0] < got["n_mean"][1:].min()
        st = association.statistics(y, Ws, Us)
        assert st["n"][st["n"] >= 3].min() <= 6 and (st["n"] == 0).sum() >= 10         # small n is covered, and n = 0
    else:
        assert (got["defined"][[0, 1, 2, 3, 5]] == 1).all() and (got["n_mean"] == N).all()
    assert np.nanmax(np.abs(got["r"]["values"])) <= 1 + 1e-12


@pytest.mark.parametrize("which", ["auc", "crossing"])
def test_of_means_against_the_definition(states, values, which):
    Ws, Vs, Us = states
    got = posterior_feature_association(Ws, Vs, Us, which=which, level=LEVEL, q=None)
    ref = association.plug_in_table(values[which], Ws, Us)
    _check_of_means(got["of_means"], ref, which)
    assert np.isnan(got["of_means"]["r"][4]).all() and not np.isnan(got["of_means"]["r"][:4]).any()
    assert got["r"]["quantiles"].shape == (0, F, M) and "slope" not in got
    assert "of_means" not in posterior_feature_association(Ws, Vs, Us, of_means=False)


@pytest.mark.parametrize("nchunk_samples", [1, 3])
def test_chunking_is_pure_geometry(states, default_call, nchunk_samples):
    got = posterior_feature_association(*states, which="crossing", stats=STATS, level=LEVEL, pairs=PAIRS,
                                        _scratch_bytes=nchunk_samples * SAMPLE_BYTES)
    _same(got, default_call, nchunk_samples)


def test_two_calls_return_identical_bits(states, default_call):
    _same(posterior_feature_association(*states, which="crossing", stats=STATS, level=LEVEL, pairs=PAIRS), default_call)
    a = posterior_feature_association(*states, which="auc", stats=("slope",))
    _same(posterior_feature_association(*states, which="auc", stats=("slope",)), a)
    # one statistic alone is the same statistic of the pair (another tile shape, the same sums)
    both = posterior_feature_association(*states, which="auc", stats=STATS)
    _same(a["slope"], both["slope"], "slope alone")


def test_entry_points_agree_bit_for_bit():
    rs = np.random.RandomState(1)
    W, V = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.4, size=(N, M, T, 2))
    Us = rs.normal(size=(S, F, K))
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=5)
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        m.posterior_feature_association(U=Us)
    res = m.run_gibbs(Y, nburn=5, nsamples=S, verbose=False)
    W0, V0 = np.array(m.W, copy=True), np.array(m.V, copy=True)
    for which in ("auc", "crossing"):                            # (this short chain's curves hardly ever cross: mostly undefined)
        kw = dict(which=which, stats=STATS, level=0.1, pairs=PAIRS)
        a = m.posterior_feature_association(U=Us, **kw)
        _same(posterior_feature_association(res["W"], res["V"], Us, **kw), a, "stateless")
        _same(m.posterior_feature_association(results=dict(res, U=Us), **kw), a, "results")
        assert a["nsamples"] == S
        assert np.array_equal(m.W, W0) and np.array_equal(m.V, V0)
        f = m.posterior_functionals(which=(which,), level=0.1, pointwise=True)[which]["pointwise"]
        ref = association.reference(f, res["W"], Us, which=which, stats=STATS, pairs=PAIRS)
        assert np.array_equal(a["defined"], ref["defined"]) and np.array_equal(a["n_mean"], ref["n_mean"])
        if which == "auc":
            assert np.isfinite(a["r"]["mean"]).all() and (a["defined"] == 1).all()
            _check_summaries(a, ref, "collected")
    # the C entry points refuse before anything is read or launched
    import ctypes as C
    from functionalmf_amd import _native
    lib = _native.load()
    d, ip = _native.dptr, lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    x, st, buf = np.linspace(0, 1, T), np.array([0], dtype=np.int32), np.zeros(8)
    tail = (0, 0, d(x), float("nan"), ip(st), 1, None, 0, None, 0) + (None,) * 10 + (0,)
    assert lib.btf_posterior_association(0, 8193, 1, 1, T, 1, 1, d(buf), d(buf), d(buf), *tail) == _native.BTF_EINVAL
    assert b"8192" in lib.btf_last_error(None)
    assert lib.btf_posterior_association(0, 1, 1, 1, T, 1, 1, d(buf), d(buf), None, *tail) == _native.BTF_EINVAL
    assert lib.btf_collect_association(m._ctx.h, S + 1, F, d(Us), *tail) == _native.BTF_ESTATE
    assert lib.btf_collect_association(m._ctx.h, S, F, d(Us), *tail) == _native.BTF_OK


EDGES = [
    ("K10", dict(S=8, N=130, M=3, T=5, K=10, F=4)),          # the 55-sum Gram; two full row blocks and a partial one
    ("S1", dict(S=1, N=70, M=2, T=4, K=3, F=3)),             # one sample: var 0, every quantile the value
    ("S64", dict(S=64, N=20, M=2, T=4, K=2, F=3)),           # a sort with no padding
    ("F1", dict(S=5, N=70, M=3, T=4, K=3, F=1)),
    ("N2", dict(S=4, N=2, M=3, T=4, K=2, F=2)),              # n < 3: everything undefined
]


@pytest.mark.parametrize("name,dims", EDGES, ids=[e[0] for e in EDGES])
def test_edge_shapes(name, dims):
    Ws, Vs, Us = _states(seed=3, **dims)
    s, f, m = dims["S"], dims["F"], dims["M"]
    allpairs = np.array([(a, b) for a in range(f) for b in range(m)])
    y = posterior_functionals(Ws, Vs, which=("auc",), pointwise=True)["auc"]["pointwise"]
    got = posterior_feature_association(Ws, Vs, Us, stats=STATS, q=(5, 50, 95), pairs=allpairs)
    ref = association.reference(y, Ws, Us, stats=STATS, q=(5, 50, 95), pairs=allpairs)
    if name == "N2":
        assert (got["defined"] == 0).all() and (got["n_mean"] == 2).all()
        for k in STATS:
            for key in ("mean", "var", "quantiles", "prob_positive", "values"):
                assert np.isnan(got[k][key]).all(), (k, key)
        assert np.isnan(got["of_means"]["r"]).all() and (got["of_means"]["n"] == 2).all()
        return
    _well_conditioned(y, Ws, Us)
    _check_summaries(got, ref, name)
    _check_of_means(got["of_means"], ref["of_means"], name)
    assert (got["defined"] == 1).all()
    if name == "S1":
        for k in STATS:
            v = got[k]["values"].reshape(f, m)
            assert (got[k]["var"] == 0).all() and np.array_equal(got[k]["mean"], v)
            assert all(np.array_equal(qv, v) for qv in got[k]["quantiles"])


def test_the_example_lists_the_top_associations_of_a_chain_that_samples_U():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("feature_importance", os.path.join(ROOT, "examples", "feature_importance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, rows = mod.main(ntop=3, verbose=False, seed=3, nburn=10, nsamples=10, n=16, m=8, nfeatures=4)
    assert out["nsamples"] == 10 and out["r"]["mean"].shape == (4, 8) and out["of_means"]["r"].shape == (4, 8)
    assert (out["n_mean"] == 16).all()
    for title, f, j, mean, lo, hi, p, plug, slope in rows:
        assert title in ("resistant", "sensitive") and lo <= mean <= hi and 0 <= p <= 1 and abs(plug) <= 1 + 1e-12
