"""Host halves of the monotone projection of the posterior (functionalmf_amd/monotone.py): the numpy definition against the
reference's factor_pav (tests/golden/g17_monotone.npz) and against a brute-force check of the monotone property, the
argument checks made before any device call, the refusal order of the model method, the ABI symbols and the register budget
of the new kernel.  No GPU."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, monotone, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_monotone.npz")
NCASES = 5


class _NoDevice:
    """Stands in for the native library and the context: any call into them fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert int(g["ncases"]) == NCASES
    return g


@pytest.mark.parametrize("c", range(NCASES))
@pytest.mark.parametrize("inc", [False, True], ids=["dec", "inc"])
def test_definition_against_the_reference_fixture(golden, c, inc):
    p = "c%d_" % c
    Ws, Vs = golden[p + "Ws"], golden[p + "Vs"]
    S, N, M, T, K = golden[p + "shape"]
    assert Ws.shape == (S, N, K) and Vs.shape == (S, M, T, K)
    W0 = Ws.copy()
    V, pools = monotone.project_host(Ws, Vs, increasing=inc)
    ref = golden[p + ("Pinc" if inc else "P")]
    assert np.abs(V - ref).max() <= 1e-12 * np.abs(ref).max()
    assert pools.dtype == np.int32 and np.array_equal(pools, golden[p + ("pools_inc" if inc else "pools")])
    assert np.array_equal(Ws, W0)
    if not inc:
        # the pool structures the fixture was chosen for: c0 6..9 of 12, c2 7..13 of 20, c3 an untouched column, c4 several
        lo, hi = {0: (6, 9), 1: (5, 7), 2: (7, 13), 3: (1, 2), 4: (14, 16)}[c]
        assert pools.min() == lo and pools.max() == hi
        if c in (3, 4):
            assert (pools == T).any()


@pytest.mark.parametrize("inc", [False, True], ids=["dec", "inc"])
def test_definition_against_a_brute_force_check_of_the_property(inc):
    """Every projected curve is monotone for every row; the pools are runs of equal depths and `pools` counts them; a pool's
    value lies within the range of its own input depths, per embedding; a pool of one depth keeps its input bits."""
    rs = np.random.RandomState(21)
    S, N, M, T, K = 3, 9, 4, 14, 3
    Ws = rs.gamma(1, 1, (S, N, K))
    Vs = 0.2 * rs.gamma(1, 1, (S, M, T, K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, 0.4, (S, M, T, K))
    Vs[0, 0] = np.sort(Vs[0, 0], axis=0)[::-1] if not inc else np.sort(Vs[0, 0], axis=0)       # one block monotone already
    V, pools = monotone.project_host(Ws, Vs, increasing=inc)
    assert pools[0, 0] == T and np.array_equal(V[0, 0], Vs[0, 0])
    assert (pools < T).any() and (pools >= 1).all()
    for s in range(S):
        for j in range(M):
            curves = Ws[s] @ V[s, j].T
            for i in range(N):
                for t in range(T - 1):
                    step = curves[i, t + 1] - curves[i, t]
                    assert (step >= -1e-12 * np.abs(curves).max()) if inc else (step <= 1e-12 * np.abs(curves).max())
            # pools are runs of equal depths; their count is `pools`; each holds values inside its inputs' range
            edges = [0] + [t + 1 for t in range(T - 1) if np.any(V[s, j, t + 1] != V[s, j, t])] + [T]
            assert len(edges) - 1 == pools[s, j]
            for a, b in zip(edges[:-1], edges[1:]):
                lo, hi = Vs[s, j, a:b].min(axis=0), Vs[s, j, a:b].max(axis=0)
                assert np.all(V[s, j, a] >= lo - 1e-12) and np.all(V[s, j, a] <= hi + 1e-12)
                if b - a == 1:
                    assert np.array_equal(V[s, j, a], Vs[s, j, a])
    # increasing is the negated projection of the negated input, exactly
    Vn, pn = monotone.project_host(Ws, -Vs, increasing=not inc)
    assert np.array_equal(-Vn, V) and np.array_equal(pn, pools)


def test_a_merge_by_hand():
    W = np.array([[1.0]])
    V = np.array([[3.0], [1.0], [2.0], [2.5], [0.5]])
    # decreasing: (1, 2) violates -> 1.5, 1.5; then (1.5, 2.5) violates -> pool of 3: (2 * 1.5 + 2.5) / 3
    out, pools = monotone.project_host(W[None], V[None, None])
    m = (2 * 1.5 + 2.5) / 3
    assert out[0, 0, :, 0].tolist() == [3.0, m, m, m, 0.5] and pools.tolist() == [[3]]
    out, pools = monotone.project_host(W[None], V[None, None], increasing=True)
    # increasing: (3, 1) -> 2, 2; (2.5, 0.5) -> 1.5, 1.5; next sweep (2, 1.5 x 2) -> 5/3 x 3; then (2 x 2, 5/3 x 3) -> 1.8 x 5
    assert pools.tolist() == [[1]] and np.abs(out[0, 0, :, 0] - 1.8).max() < 1e-15


BAD = [
    (dict(q=(5, 101)), "percentiles"),
    (dict(q=(-1,)), "percentiles"),
    (dict(transform="log"), "transform"),
    (dict(transform=1), "transform"),
    (dict(increasing=1), "increasing"),
    (dict(increasing="yes"), "increasing"),
    (dict(return_V=None), "return_V"),
]
GOOD = dict(Ws=np.zeros((3, 5, 2)), Vs=np.zeros((3, 4, 4, 2)))


@pytest.mark.parametrize("kw,msg", BAD)
def test_argument_checks_raise_before_the_library_is_loaded(no_device, kw, msg):
    with pytest.raises(ValueError, match=msg):
        utils.posterior_monotone(GOOD["Ws"], GOOD["Vs"], **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_monotone(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)))
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_monotone(np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 3)))
    big = monotone.MAX_SUMMARY_SAMPLES + 1
    with pytest.raises(ValueError, match="exceed %d" % monotone.MAX_SUMMARY_SAMPLES):
        utils.posterior_monotone(np.zeros((big, 1, 1)), np.zeros((big, 1, 2, 1)))
    with pytest.raises(ValueError, match="pav_fits"):
        utils.posterior_monotone(np.zeros((1, 2, 10)), np.zeros((1, 1, 1000, 10)))
    with pytest.raises(ValueError, match="nembeds must be 1..10"):
        utils.posterior_monotone(np.zeros((1, 2, 11)), np.zeros((1, 1, 4, 11)))
    assert monotone.MAX_SUMMARY_SAMPLES == 16384
    # the bound is the NMF path's: 8 T K + 4 T <= 64 KiB
    assert monotone.pav_fits(780, 10) and not monotone.pav_fits(781, 10) and monotone.pav_fits(5461, 1) and not monotone.pav_fits(5462, 1)


def _model_without_a_device(N=5, M=4, T=4, K=2, world=1):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds = N, M, T, K
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    return m


@pytest.mark.parametrize("kw,msg", BAD + [(dict(in_place=1), "in_place")])
def test_the_model_method_checks_its_arguments_before_its_samples(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model_without_a_device().posterior_monotone(**kw)            # (no samples collected: the arguments come first)


def test_refusal_order_of_the_model_method():
    good = dict(W=GOOD["Ws"], V=GOOD["Vs"])
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(world=2).posterior_monotone(q=(5, 101), results=good)
    with pytest.raises(ValueError, match="percentiles"):
        _model_without_a_device().posterior_monotone(q=(5, 101), results={"V": good["V"]})
    with pytest.raises(ValueError, match="in_place=True projects the samples collected on the device"):
        _model_without_a_device().posterior_monotone(results=good, in_place=True)
    with pytest.raises(ValueError, match="pav_fits"):
        _model_without_a_device(T=1000, K=10).posterior_monotone()
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device().posterior_monotone()
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device().posterior_monotone(in_place=True)
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_monotone(results={"V": good["V"]})
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_monotone(results=dict(W=np.zeros((3, 6, 2)), V=good["V"]))
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_monotone(results=7)


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_monotone", "btf_collect_monotone"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_monotone") and hasattr(lib, "btf_collect_monotone")
    assert len(_native.SIGNATURES["btf_posterior_monotone"][1]) == 16
    assert len(_native.SIGNATURES["btf_collect_monotone"][1]) == 13
    assert any(src == os.path.join(_native.CSRC, "btf_monotone.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_monotone.h") in _native.HEADERS
    # the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    abi = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    assert abi.count("return mono_run(s, ") == 3 and abi.count("mono_check(") == 3       # one run function behind both entry points
    nmf = open(os.path.join(_native.CSRC, "btf_nmf.h")).read()
    assert "void nmf_pav_kernel(" in nmf                                                # the chain-start kernel stays


def test_no_spills_or_scratch_in_the_monotone_kernel():
    """Code-object notes (scripts/kernel_notes.py): no instantiation of mono_project_kernel spills VGPRs or uses scratch; at
    most 128 VGPRs (4 waves per SIMD: four 256-thread workgroups per CU), which the header states; the static LDS (the
    block-wide vote's) beside the 64 KiB bound of the dynamic part leaves room for two workgroups in a CU's 160 KiB."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if "mono_project_kernel" in r["mangled"]]
    assert len(rows) == 10, [r["mangled"] for r in rows]
    bad = [(r["mangled"], r["vgpr_spill"], r["sgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for r in rows:
        assert r["vgpr"] + r["agpr"] <= 128, r
        assert r["lds"] % 16 == 0 and 2 * (r["lds"] + 64 * 1024) <= 160 * 1024, r
