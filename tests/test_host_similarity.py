"""Host halves of the posterior similarity (functionalmf_amd/similarity.py): the numpy definition against a from-scratch
einsum of the surfaces, its exact rules (identical entities, the zero surface, self last), `embed` on a planted
configuration, the argument checks made before any device call and their order, the ABI symbols, and the register and LDS
budget of the new kernels.  No GPU."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, ranking, similarity, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

# (S,N,M,T,K): the shapes of tests/test_gpu_similarity.py
SHAPES = [(3, 7, 5, 4, 3), (2, 70, 3, 9, 10), (4, 5, 66, 6, 1), (2, 3, 1, 1, 5), (5, 130, 2, 64, 5), (2, 9, 130, 3, 10)]


class _NoDevice:
    """Stands in for the native library and the context: any call into them fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def _states(S, N, M, T, K, seed=0):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K))


def _direct(Ws, Vs, along, over=None):
    """(d2, cosine distance) from the surfaces themselves."""
    mu = np.einsum("snk,smtk->snmt", Ws, Vs)
    if along == "cols":
        mu = mu.transpose(0, 2, 1, 3)
    if over is not None:
        mu = mu[:, :, list(over)]
    flat = mu.reshape(mu.shape[0], mu.shape[1], -1)                         # (S,E,n)
    diff = flat[:, :, None] - flat[:, None]
    d2 = (diff ** 2).mean(-1)
    dot = np.einsum("sen,sfn->sef", flat, flat)
    nrm = np.sqrt(np.einsum("sen,sen->se", flat, flat))
    cos = 1.0 - dot / (nrm[:, :, None] * nrm[:, None])
    cos[:, np.arange(cos.shape[1]), np.arange(cos.shape[1])] = 0.0
    return d2, cos


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("along", ["rows", "cols"])
def test_the_quadratic_form_is_the_distance_between_the_surfaces(shape, along):
    """|d2 - d2_direct| <= 1e-11 max(d2_direct): about M T K accumulated products times the fp64 unit, at most 4e-12 here."""
    Ws, Vs = _states(*shape)
    d2_ref, cos_ref = _direct(Ws, Vs, along)
    d2 = similarity.squared_distances(Ws, Vs, along)
    err = np.abs(d2 - d2_ref).max()
    print("%s %s: d2 err %.3e of scale %.3e" % (shape, along, err, d2_ref.max()))
    assert err <= 1e-11 * d2_ref.max()
    assert np.array_equal(similarity.distances(Ws, Vs, along), np.sqrt(d2))
    cos = similarity.distances(Ws, Vs, along, "cosine")
    assert np.abs(cos - cos_ref).max() <= 1e-12
    assert np.array_equal(cos, cos.transpose(0, 2, 1)) and np.array_equal(d2, d2.transpose(0, 2, 1))
    E = d2.shape[1]
    assert (d2[:, np.arange(E), np.arange(E)] == 0).all() and (cos[:, np.arange(E), np.arange(E)] == 0).all()
    over = [shape[2] - 1] if along == "rows" else list(range(shape[1]))[::-1][:-1] or [0]
    assert np.abs(similarity.squared_distances(Ws, Vs, along, over) - _direct(Ws, Vs, along, over)[0]).max() <= 1e-11 * d2_ref.max()


def test_identical_entities_are_at_exactly_zero():
    Ws, Vs = _states(4, 6, 5, 3, 4, seed=1)
    Ws[:, 4] = Ws[:, 1]
    Vs[:, 3] = Vs[:, 0]
    for along, (e, f) in (("rows", (1, 4)), ("cols", (0, 3))):
        d2 = similarity.squared_distances(Ws, Vs, along)
        assert (d2[:, e, f] == 0.0).all() and (d2[:, f, e] == 0.0).all() and (d2 >= 0).all()
        assert (similarity.distances(Ws, Vs, along, "cosine")[:, e, f] == 0.0).all()


def test_the_zero_surface_of_the_cosine_metric():
    Ws, Vs = _states(3, 5, 4, 3, 2, seed=2)
    Ws[:, 2] = 0.0
    d = similarity.distances(Ws, Vs, "rows", "cosine")
    assert np.isfinite(d).all()
    other = [0, 1, 3, 4]
    assert (d[:, 2, other] == 1.0).all() and (d[:, other, 2] == 1.0).all() and (d[:, 2, 2] == 0.0).all()
    Ws[:] = 0.0                                                              # every surface zero: still nothing undefined
    d = similarity.distances(Ws, Vs, "cols", "cosine")
    assert np.array_equal(d, np.broadcast_to(1.0 - np.eye(4), d.shape))


def test_self_ranks_last_and_ties_go_to_the_smaller_index():
    Ws, Vs = _states(5, 6, 3, 4, 2, seed=3)
    Ws[:, 5] = Ws[:, 2]
    key = similarity.keys(Ws, Vs, "rows")
    E = key.shape[1]
    assert np.isnan(key[:, np.arange(E), np.arange(E)]).all()
    r = ranking.ranks(key, "cols", "ascending")
    assert (r[:, np.arange(E), np.arange(E)] == E).all()
    assert (r[:, 2, 5] == 1).all() and (r[:, 5, 2] == 1).all()              # the twin is the nearest
    assert (r[:, 0, 2] < r[:, 0, 5]).all() and (r[:, 0, 5] == r[:, 0, 2] + 1).all()   # equal keys: the smaller index first
    e, v, p = similarity.neighbours(key, nearest=(1, E - 1, E))
    assert (p[0, 2, 5], p[0, 5, 2]) == (1.0, 1.0) and (p[2] == 1.0).all() and (p[1][np.eye(E, dtype=bool)] == 0.0).all()
    one = similarity.reference(Ws[:, :1], Vs)                               # E = 1: nothing to rank
    assert one["expected_rank"].tolist() == [[1.0]] and one["p_nearest"][:, 0, 0].tolist() == [1.0, 1.0]
    assert one["ncells"] == 12 and one["nsamples"] == 5 and one["nearest"] == (1, 5)


def test_embed_recovers_a_planted_configuration():
    rs = np.random.RandomState(4)
    P = rs.normal(size=(9, 2)) * [3.0, 1.0]
    D = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
    out = {"mean": D, "var": np.zeros_like(D), "nsamples": 7}
    X, share = similarity.embed(out, dims=2)
    assert X.shape == (9, 2) and abs(share - 1.0) < 1e-12
    assert np.abs(np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)) - D).max() < 1e-10      # up to a rigid motion
    Pc = P - P.mean(0)
    U, _, Vt = np.linalg.svd(X.T @ Pc)
    assert np.abs(X @ (U @ Vt) - Pc).max() < 1e-10                          # the best orthogonal map lands on the plant
    X1, share1 = similarity.embed(out, dims=1)
    assert X1.shape == (9, 1) and 0 < share1 < 1
    # the posterior mean of d2 is the second moment: mean^2 + var (S - 1) / S
    d = np.abs(rs.normal(size=(6, 4, 4)))
    d = d + d.transpose(0, 2, 1)
    d[:, np.arange(4), np.arange(4)] = 0
    o = {"mean": d.mean(0), "var": d.var(0, ddof=1), "nsamples": 6}
    assert np.allclose(o["mean"] ** 2 + o["var"] * 5 / 6, (d ** 2).mean(0), rtol=1e-12)
    with pytest.raises(ValueError, match="dims"):
        similarity.embed(out, dims=10)


BAD = [
    (dict(along="depth"), "along"),
    (dict(metric="l1"), "metric"),
    (dict(over=()), "over"),
    (dict(over=(0, 0)), "over"),
    (dict(over=(4,)), "over"),
    (dict(over=(-1,)), "over"),
    (dict(over=(0.5,)), "over"),
    (dict(along="cols", over=(5,)), "over"),
    (dict(q=(101,)), "percentiles"),
    (dict(nearest=()), "nearest"),
    (dict(nearest=(0, 1)), "nearest"),
    (dict(nearest=(1, 1)), "nearest"),
    (dict(nearest=(1.5,)), "nearest"),
    (dict(nearest=tuple(range(1, 10))), "nearest"),
    (dict(pairs=[(0, 5)]), "pairs"),
    (dict(pairs=[(-1, 0)]), "pairs"),
    (dict(pairs=[(0, 0, 1)]), "pairs"),
    (dict(pairs=[(0.0, 1.0)]), "pairs"),
    (dict(along="cols", pairs=[(0, 4)]), "pairs"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_argument_checks_raise_before_the_library_is_loaded(no_device, kw, msg):
    Ws, Vs = np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 2))
    with pytest.raises(ValueError, match=msg):
        utils.posterior_similarity(Ws, Vs, **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_similarity(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)))
    with pytest.raises(ValueError, match="nembeds"):
        utils.posterior_similarity(np.zeros((1, 2, 11)), np.zeros((1, 2, 2, 11)))
    S = similarity.MAX_SAMPLES + 1
    with pytest.raises(ValueError, match="exceed %d" % similarity.MAX_SAMPLES):
        utils.posterior_similarity(np.zeros((S, 1, 1)), np.zeros((S, 1, 1, 1)))
    E = similarity.MAX_ENTITIES + 1
    with pytest.raises(ValueError, match="exceed %d" % similarity.MAX_ENTITIES):
        utils.posterior_similarity(np.zeros((1, E, 1)), np.zeros((1, 2, 1, 1)))
    with pytest.raises(ValueError, match="exceed %d" % similarity.MAX_ENTITIES):
        utils.posterior_similarity(np.zeros((1, 2, 1)), np.zeros((1, E, 1, 1)), along="cols")
    utils_E = 2048                                                           # 32 x 2048 x 2048 x 8 bytes = 1 GiB exactly: allowed
    assert 32 * utils_E * utils_E * 8 == similarity.MAX_POINTWISE_BYTES
    with pytest.raises(ValueError, match="pairs="):
        utils.posterior_similarity(np.zeros((33, utils_E, 1)), np.zeros((33, 1, 1, 1)), pointwise=True)
    assert similarity.MAX_SAMPLES == 8192 and similarity.MAX_ENTITIES == 4096 and similarity.MAX_NEAREST == 8
    # the argument order: along before metric before over before q before nearest before pairs
    Ws, Vs = np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 2))
    order = [("along", "x"), ("metric", "x"), ("over", ()), ("q", (101,)), ("nearest", ()), ("pairs", [(9, 9)])]
    for k in range(len(order)):
        with pytest.raises(ValueError, match="percentiles" if order[k][0] == "q" else order[k][0]):
            utils.posterior_similarity(Ws, Vs, **dict(order[k:]))


def test_nearest_entries_above_the_largest_group_reach_the_library_distinct():
    near = (similarity.MAX_ENTITIES + 1, 1, 100000, 4, similarity.MAX_ENTITIES, 5, 2 ** 40, 2)
    got = similarity.check_args("rows", "rms", None, (5,), near, None, False, 3, 4, 5, 3, 2)
    dev = got[5]
    assert got[4] == near and dev.dtype == np.int32 and len(set(dev.tolist())) == len(near)
    small = np.array(near) <= similarity.MAX_ENTITIES
    assert np.array_equal(dev[small], np.array(near)[small]) and (dev[~small] > similarity.MAX_ENTITIES).all()


def _model_without_a_device(N=5, M=4, T=4, K=2, world=1):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds = N, M, T, K
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    return m


@pytest.mark.parametrize("kw,msg", BAD)
def test_the_model_method_checks_its_arguments_before_its_samples(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model_without_a_device().posterior_similarity(**kw)               # (no samples collected: the arguments come first)


def test_refusal_order_of_the_model_method():
    good = dict(W=np.zeros((3, 5, 2)), V=np.zeros((3, 4, 4, 2)))
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(world=2).posterior_similarity(along="x", results=good)
    with pytest.raises(ValueError, match="along"):
        _model_without_a_device().posterior_similarity(along="x", results={"V": good["V"]})
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device().posterior_similarity()
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_similarity(results={"V": good["V"]})
    with pytest.raises(ValueError, match="Ws must be"):
        _model_without_a_device().posterior_similarity(results=dict(good, W=np.zeros((3, 6, 2))))


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_similarity", "btf_collect_similarity"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_similarity") and hasattr(lib, "btf_collect_similarity")
    assert len(_native.SIGNATURES["btf_posterior_similarity"][1]) == 27
    assert len(_native.SIGNATURES["btf_collect_similarity"][1]) == 21
    assert any(src == os.path.join(_native.CSRC, "btf_similarity.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_similarity.h") in _native.HEADERS
    # the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    abi = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    assert abi.count("sim_run(s, ") == 2 and abi.count("sim_check(") == 3  # one of each, behind both entry points


def test_no_spills_or_scratch_in_the_similarity_kernels():
    """Code-object notes (scripts/kernel_notes.py): no sim_ kernel spills VGPRs or uses scratch memory; the static LDS of the
    metric kernel and the dynamic LDS of the distance kernel fit 64 KiB with room for several workgroups per CU."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"sim_(metric|dist|root|pairs|finish)_kernel", r["mangled"])]
    assert len(rows) == 10 + 20 + 3, sorted(r["mangled"] for r in rows)
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for r in rows:
        assert r["lds"] <= 64 * 1024 and r["vgpr"] <= 256, r
    K, waves, tb = 10, 4, 4                                                 # SIM_WAVES, SIM_TB of csrc/btf_similarity.h
    assert 64 * (tb * K + 1) * 8 <= 64 * 1024                               # the distance kernel's dynamic block
    metric = [r for r in rows if "sim_metric_kernel" in r["mangled"]]
    assert max(r["lds"] for r in metric) == (waves * K * (K + 1) // 2 + K * K) * 8
