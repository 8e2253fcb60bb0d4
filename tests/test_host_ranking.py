"""Host halves of the posterior ranking (functionalmf_amd/ranking.py): the numpy definition against hand-made values (ties,
nan, both orders, a group of one, k above the group), the argument checks made before any device call, the refusal of a
sharded model, the ABI symbols, and the register budget of the new kernels.  No GPU."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, ranking, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

nan = np.nan


class _NoDevice:
    """Stands in for the native library and the context: any call into them fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def test_ranks_of_one_group_by_hand():
    v = np.array([[[3.0, 1.0, 2.0, 1.0, nan, 0.5, nan]]])                 # S = N = 1, one group of 7 columns
    assert ranking.ranks(v, "cols", "ascending")[0, 0].tolist() == [5, 2, 4, 3, 6, 1, 7]
    assert ranking.ranks(v, "cols", "descending")[0, 0].tolist() == [1, 3, 2, 4, 6, 5, 7]
    # the same values as a column: along="rows"
    w = v.transpose(0, 2, 1)
    assert ranking.ranks(w, "rows", "ascending")[0, :, 0].tolist() == [5, 2, 4, 3, 6, 1, 7]
    assert ranking.ranks(w, "rows", "descending")[0, :, 0].tolist() == [1, 3, 2, 4, 6, 5, 7]
    # along="cols" on (1,7,1): seven groups of one member
    assert np.array_equal(ranking.ranks(w, "cols", "ascending"), np.ones((1, 7, 1), dtype=np.int64))


def test_ascending_is_the_position_in_a_stable_argsort_and_zero_signs_tie():
    rs = np.random.RandomState(0)
    f = rs.randint(0, 4, size=(6, 5, 9)).astype(float)                    # many ties
    r = ranking.ranks(f, "cols", "ascending")
    pos = np.argsort(np.argsort(f, axis=2, kind="stable"), axis=2, kind="stable")
    assert np.array_equal(r, pos + 1)
    r = ranking.ranks(f, "rows", "descending")
    pos = np.argsort(np.argsort(-f, axis=1, kind="stable"), axis=1, kind="stable")
    assert np.array_equal(r, pos + 1)
    z = np.array([[[0.0, -0.0, 0.0, -1.0]]])
    assert ranking.ranks(z, "cols", "ascending")[0, 0].tolist() == [2, 3, 4, 1]
    assert ranking.ranks(z, "cols", "descending")[0, 0].tolist() == [1, 2, 3, 4]
    inf = np.array([[[np.inf, nan, -np.inf, 1.0]]])                        # infinities are defined values
    assert ranking.ranks(inf, "cols", "ascending")[0, 0].tolist() == [3, 4, 1, 2]
    assert ranking.ranks(inf, "cols", "descending")[0, 0].tolist() == [1, 4, 3, 2]


def test_summaries_by_hand():
    # one curve pair (M = 2) over S = 4 samples: column 0 is first in 3 of 4
    f = np.array([[[1.0, 2.0]], [[1.0, 2.0]], [[5.0, 2.0]], [[2.0, 2.0]]])
    out = ranking.reference(f, top=(1, 2, 7), pointwise=True, pairs=[(0, 0, 0, 1), (0, 1, 0, 0)])
    assert out["ranks"].dtype == np.int32 and out["ranks"][:, 0, 0].tolist() == [1, 1, 2, 1]
    assert out["expected_rank"].tolist() == [[1.25, 1.75]]
    assert out["rank_var"].tolist() == [[0.25, 0.25]]                      # (4 * 7 - 25) / 12, (4 * 13 - 49) / 12
    assert out["p_top"].tolist() == [[[0.75, 0.25]], [[1.0, 1.0]], [[1.0, 1.0]]]      # k = 7 > L = 2 gives 1
    assert out["prob_less"].tolist() == [0.5, 0.25] and out["prob_defined"].tolist() == [1.0, 1.0]
    assert (out["top"], out["along"], out["order"], out["which"], out["nsamples"]) == ((1, 2, 7), "cols", "ascending", "auc", 4)
    one = ranking.reference(f[:1])
    assert one["rank_var"].tolist() == [[0.0, 0.0]]                        # a single sample: 0, not nan
    g = np.array([[[1.0, nan]], [[nan, nan]], [[3.0, 2.0]]])
    less, defined = ranking.pair_probabilities(g, [(0, 0, 0, 1), (0, 1, 0, 0)])
    assert less.tolist() == [0.0, 1 / 3] and defined.tolist() == [1 / 3, 1 / 3]
    assert ranking.ranks(g, "cols", "descending")[:, 0].tolist() == [[1, 2], [1, 2], [1, 2]]


def test_top_entries_above_the_largest_group_reach_the_library_distinct():
    """4097, 100000 and 2**40 all mean "certain"; the library refuses repeated entries, so each gets a stand-in of its own
    above MAX_GROUP (they used to be clamped to one value, and the call was refused)."""
    top = (ranking.MAX_GROUP + 1, 1, 100000, 4, ranking.MAX_GROUP, 5, 2 ** 40, 2)
    dev = ranking.check_args("auc", "cols", "ascending", top, None, None, None, None, 3, 4, 5, 3)[4]
    assert dev.dtype == np.int32 and len(set(dev.tolist())) == len(top)
    small = np.array(top) <= ranking.MAX_GROUP
    assert np.array_equal(dev[small], np.array(top)[small]) and (dev[~small] > ranking.MAX_GROUP).all()


def test_integer_sums_stay_exact_at_the_limits():
    S, L = ranking.MAX_SAMPLES, ranking.MAX_GROUP
    assert S * S * L * L < 2 ** 53
    r = np.full((S, 1, 1), L, dtype=np.int64)
    e, v, p = ranking.summarize(r, top=(L - 1, L))
    assert e[0, 0] == L and v[0, 0] == 0.0 and p[:, 0, 0].tolist() == [0.0, 1.0]


BAD = [
    (dict(which="area"), "unknown functional"),
    (dict(which=("auc",)), "unknown functional"),
    (dict(along="depth"), "along"),
    (dict(order="up"), "order"),
    (dict(top=()), "top"),
    (dict(top=(0, 1)), "top"),
    (dict(top=(1, 1)), "top"),
    (dict(top=(1.5,)), "top"),
    (dict(top=tuple(range(1, 10))), "top"),
    (dict(which="crossing"), "level"),
    (dict(which="crossing", level=np.inf), "level"),
    (dict(transform="log"), "transform"),
    (dict(x=np.array([0.0, 0.5, 0.5, 1.0])), "strictly increasing"),
    (dict(x=np.linspace(0, 1, 5)), "ndepth"),
    (dict(pairs=[(0, 0, 5, 0)]), "pairs"),
    (dict(pairs=[(0, 0, 0, 4)]), "pairs"),
    (dict(pairs=[(-1, 0, 0, 0)]), "pairs"),
    (dict(pairs=[(0, 0, 1)]), "pairs"),
    (dict(pairs=[(0.0, 0.0, 1.0, 1.0)]), "pairs"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_argument_checks_raise_before_the_library_is_loaded(no_device, kw, msg):
    Ws, Vs = np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 2))
    with pytest.raises(ValueError, match=msg):
        utils.posterior_ranking(Ws, Vs, **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    with pytest.raises(ValueError, match="ndepth >= 2"):
        utils.posterior_ranking(np.zeros((3, 5, 2)), np.zeros((3, 4, 1, 2)))
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_ranking(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)))
    S = ranking.MAX_SAMPLES + 1
    with pytest.raises(ValueError, match="exceed %d" % ranking.MAX_SAMPLES):
        utils.posterior_ranking(np.zeros((S, 1, 1)), np.zeros((S, 1, 2, 1)))
    L = ranking.MAX_GROUP + 1
    with pytest.raises(ValueError, match="exceeds %d" % ranking.MAX_GROUP):
        utils.posterior_ranking(np.zeros((1, 2, 1)), np.zeros((1, L, 2, 1)), along="cols")
    with pytest.raises(ValueError, match="exceeds %d" % ranking.MAX_GROUP):
        utils.posterior_ranking(np.zeros((1, L, 1)), np.zeros((1, 2, 2, 1)), along="rows")
    assert ranking.MAX_SAMPLES == 8192 and ranking.MAX_GROUP == 4096 and ranking.MAX_TOP == 8


def _model_without_a_device(N=5, M=4, T=4, K=2, world=1):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds = N, M, T, K
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    return m


@pytest.mark.parametrize("kw,msg", BAD)
def test_the_model_method_checks_its_arguments_before_its_samples(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model_without_a_device().posterior_ranking(**kw)                 # (no samples collected: the arguments come first)


def test_refusal_order_of_the_model_method():
    good = dict(W=np.zeros((3, 5, 2)), V=np.zeros((3, 4, 4, 2)))
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(world=2).posterior_ranking(which="area", results=good)
    with pytest.raises(ValueError, match="along"):
        _model_without_a_device().posterior_ranking(along="x", results={"V": good["V"]})
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device().posterior_ranking()
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_ranking(results={"V": good["V"]})
    with pytest.raises(ValueError, match="Ws must be"):
        _model_without_a_device().posterior_ranking(results=dict(good, W=np.zeros((3, 6, 2))))


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_ranking", "btf_collect_ranking"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_ranking") and hasattr(lib, "btf_collect_ranking")
    assert len(_native.SIGNATURES["btf_posterior_ranking"][1]) == 25
    assert len(_native.SIGNATURES["btf_collect_ranking"][1]) == 19
    assert any(src == os.path.join(_native.CSRC, "btf_ranking.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_ranking.h") in _native.HEADERS
    # the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    abi = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    assert abi.count("ranking_run(s, ") == 2 and abi.count("ranking_check(") == 3    # one of each, behind both entry points


def test_no_spills_or_scratch_in_the_ranking_kernels():
    """Code-object notes (scripts/kernel_notes.py): the two rank kernels, the pair count and the finish kernel neither spill
    VGPRs nor use scratch; the rank kernel has no static LDS beside its (at most 49.7 KB of) dynamic rows, and stays at or
    under 128 VGPRs: two workgroups of 512 threads per CU."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"rank_(pairs_|finish_)?kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    rank = [r for r in rows if re.search(r"rank_kernelILb[01]E", r["mangled"])]
    assert len(rank) == 2 and len(rows) == 4, [r["mangled"] for r in rows]
    for r in rank:
        assert r["lds"] == 0 and r["vgpr"] <= 128, r
    G, Lp = 64, 64                                                         # the geometry with the largest LDS
    assert G * (Lp + 1) * 8 + G * Lp * 4 <= 64 * 1024
    assert (ranking.MAX_GROUP + 1) * 8 + ranking.MAX_GROUP * 4 <= 64 * 1024
