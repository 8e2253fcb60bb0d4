"""Host halves of the simultaneous credible bands (functionalmf_amd/bands.py): the numpy definitions against their own
contracts and a plain loop, tie handling, every refusal before any native call, the ABI symbols, coverage of a known curve,
and the register budget of the new kernels.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, bands, utils


class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def _smooth(rs, S, shape, T):
    """Smooth sampled curves: a random walk over depth per sample, (S,) + shape + (T,)."""
    return np.cumsum(rs.normal(size=(S,) + shape + (T,)), axis=-1) + rs.normal(size=(S,) + shape + (1,))


def _depth_by_loop(col):
    """depth contributions (lo, hi) of one cell's S values by the definition's plain counts."""
    lo = np.array([(col < v).sum() for v in col])
    hi = np.array([(col > v).sum() for v in col])
    return lo, hi


@pytest.mark.parametrize("S,T,level", [(2, 1, 95), (7, 3, 50), (40, 9, 95), (200, 12, 80), (63, 5, 99.9)])
def test_definitions_keep_their_contracts(S, T, level):
    rs = np.random.RandomState(S + T)
    m = _smooth(rs, S, (3, 2), T)
    use = np.ones(T, dtype=bool)
    if T > 2:
        use[rs.choice(T, T // 3, replace=False)] = False
    need = bands.need_of(level, S)
    assert 1 <= need <= S and need == int(np.ceil(level / 100.0 * S))
    for depths in (None, use):
        u = np.ones(T, dtype=bool) if depths is None else depths
        sup = bands.supt_band(m, level, depths)
        assert sup["need"] == need and np.all(sup["inside"] >= need / S) and np.all(sup["inside"] <= 1)
        keep = sup["stat"] <= sup["crit"]                                            # (S,3,2)
        tol = 1e-12 * np.abs(m).max()                                                # |m - c| / sd * sd is not |m - c| to the bit
        ok = (m >= sup["lower"] - tol) & (m <= sup["upper"] + tol)
        assert np.all(ok[..., u][keep])
        assert np.array_equal(sup["crit"], np.sort(sup["stat"], axis=0)[need - 1])
        rk = bands.rank_band(m, level, depths)
        assert np.all(rk["inside"] >= need / S) and np.all(rk["pointwise_inside"] <= 1) and np.all(rk["k"] >= 0)
        keep = rk["stat"] >= rk["k"]
        ok = (m >= rk["lower"]) & (m <= rk["upper"])
        assert np.all(ok[..., u][keep])                                              # exact: order statistics of m itself
        assert np.array_equal(rk["inside"], keep.sum(0) / S)
        assert np.all((rk["stat"] >= rk["k"] + 1).sum(0) < need)                     # k is the largest that qualifies
        # the pointwise share, computed directly from the cell-wise order statistics k_pw and S-1-k_pw
        kpw = bands.pointwise_k(level, S)
        assert kpw == rk["k_pointwise"] and 0 <= kpw <= (S - 1) // 2
        srt = np.sort(m, axis=0)
        inside_pw = ((m >= srt[kpw]) & (m <= srt[S - 1 - kpw]))[..., u].all(-1)
        assert np.array_equal(rk["pointwise_inside"], inside_pw.sum(0) / S)
        # the depth by the definition's plain counts
        for idx in np.ndindex(3, 2):
            d = np.full(S, S)
            for t in np.flatnonzero(u):
                lo, hi = _depth_by_loop(m[(slice(None),) + idx + (t,)])
                d = np.minimum(d, np.minimum(lo, hi))
            assert np.array_equal(rk["stat"][(slice(None),) + idx], d)


def test_rank_band_at_k_zero_is_the_envelope():
    rs = np.random.RandomState(1)
    m = _smooth(rs, 20, (4,), 30)                    # 20 curves over 30 depths: the deepest curves cannot number 19
    rk = bands.rank_band(m, 95)
    assert np.all(rk["k"] == 0) and np.all(rk["inside"] == 1.0)
    assert np.array_equal(rk["lower"], m.min(0)) and np.array_equal(rk["upper"], m.max(0))


def test_pointwise_band_does_not_hold_the_curve():
    """What the call exists for: the share of smooth curves wholly inside their pointwise band is far below the level, the
    simultaneous bands hold it."""
    rs = np.random.RandomState(2)
    m = _smooth(rs, 400, (5,), 48)
    rk, sup = bands.rank_band(m, 95), bands.supt_band(m, 95)
    assert np.all(rk["pointwise_inside"] < 0.9) and np.all(rk["inside"] >= 0.95) and np.all(sup["inside"] >= 0.95)
    assert np.all(rk["k"] < rk["k_pointwise"])


def test_ties_with_integer_values():
    rs = np.random.RandomState(3)
    S, T = 30, 6
    m = rs.randint(-2, 3, size=(S, 4, 3, T)).astype(float)
    m[:, 0, 0, 2] = 1.0                                                  # a cell with scale == 0
    m[:, 1, 1, :] = -2.0                                                 # a curve with scale == 0 everywhere
    lo, hi = bands.strict_counts(m)
    for idx in np.ndindex(4, 3, T):
        l, h = _depth_by_loop(m[(slice(None),) + idx])
        assert np.array_equal(lo[(slice(None),) + idx], l) and np.array_equal(hi[(slice(None),) + idx], h)
    rk = bands.rank_band(m, 80)
    assert np.all(rk["stat"][:, 1, 1] == 0) and rk["k"][1, 1] == 0 and rk["inside"][1, 1] == 1.0
    assert np.all(rk["lower"][1, 1] == -2.0) and np.all(rk["upper"][1, 1] == -2.0)
    sup = bands.supt_band(m, 80)
    assert sup["scale"][0, 0, 2] == 0 and np.all(np.isfinite(sup["stat"]))
    assert np.all(sup["stat"][:, 1, 1] == 0) and sup["crit"][1, 1] == 0 and sup["inside"][1, 1] == 1.0
    only = np.zeros(T, dtype=bool)
    only[2] = True                                                       # the only used depth is skipped: D = 0
    sup = bands.supt_band(m, 80, only)
    assert np.all(sup["stat"][:, 0, 0] == 0) and sup["crit"][0, 0] == 0
    assert np.array_equal(sup["lower"][0, 0], sup["center"][0, 0])


def test_coverage_from_truth_with_nans():
    lower, upper = np.zeros((2, 2, 3)), np.ones((2, 2, 3))
    truth = np.full((2, 2, 3), 0.5)
    truth[0, 1, 1] = 1.5                              # outside at one depth
    truth[1, 0, :] = np.nan                           # unknown everywhere
    truth[1, 1, 0], truth[1, 1, 1] = np.nan, 2.0      # outside at a known depth, unknown at another
    covered, cov = bands.coverage(lower, upper, truth)
    assert np.array_equal(covered, [[1.0, 0.0], [np.nan, 0.0]], equal_nan=True) and cov == pytest.approx(1 / 3)
    use = np.array([True, False, True])               # the offending depths are not used
    covered, cov = bands.coverage(lower, upper, truth, use)
    assert np.array_equal(covered, [[1.0, 1.0], [np.nan, 1.0]], equal_nan=True) and cov == 1.0
    covered, cov = bands.coverage(lower, upper, np.full((2, 2, 3), np.nan))
    assert np.isnan(covered).all() and np.isnan(cov)
    assert bands.coverage(lower, upper, np.ones((2, 2, 3)))[1] == 1.0          # the edges belong to the band


@pytest.mark.parametrize("kw,msg", [
    (dict(method="bonferroni"), "unknown method"),
    (dict(method=None), "unknown method"),
    (dict(level=0), r"\(0, 100\)"),
    (dict(level=100), r"\(0, 100\)"),
    (dict(level=float("nan")), r"\(0, 100\)"),
    (dict(level=-5), r"\(0, 100\)"),
    (dict(depths=np.zeros(4, dtype=bool)), "no depth"),
    (dict(depths=np.ones(5, dtype=bool)), "mask"),
    (dict(depths=[0, 1, 2, 3]), "mask"),
    (dict(curves=[(0, 4)]), "curves"),
    (dict(curves=[(5, 0)]), "curves"),
    (dict(curves=[(-1, 0)]), "curves"),
    (dict(transform="log"), "transform"),
    (dict(truth=np.zeros((5, 4, 3))), "truth"),
])
@pytest.mark.parametrize("method", ["supt", "rank"])
def test_argument_checks_raise_before_the_library_is_loaded(no_device, method, kw, msg):
    Ws, Vs = np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 2))
    kw = dict(dict(method=method), **kw)
    with pytest.raises(ValueError, match=msg):
        utils.posterior_bands(Ws, Vs, **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    with pytest.raises(ValueError, match="at least two samples"):
        utils.posterior_bands(np.zeros((1, 5, 2)), np.zeros((1, 4, 4, 2)))
    with pytest.raises(ValueError, match="ndepth >= 1"):
        utils.posterior_bands(np.zeros((3, 5, 2)), np.zeros((3, 4, 0, 2)))
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_bands(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)))
    for method in ("supt", "rank"):
        S = bands.MAX_SAMPLES[method] + 1
        with pytest.raises(ValueError, match="exceed %d" % bands.MAX_SAMPLES[method]):
            utils.posterior_bands(np.zeros((S, 1, 1)), np.zeros((S, 1, 2, 1)), method=method)


def test_sharded_models_are_refused_first(no_device):
    from functionalmf_amd._analysis import PosteriorAnalysis

    class Plan:
        world = 2

    class Sharded(PosteriorAnalysis):
        _plan = Plan()
    with pytest.raises(NotImplementedError, match="unsharded"):
        Sharded().posterior_bands(method="nonsense")


def test_max_samples_mirror_the_headers():
    from conftest import ROOT
    csrc = os.path.join(ROOT, "functionalmf_amd", "csrc")
    func = open(os.path.join(csrc, "btf_functionals.h")).read()
    band = open(os.path.join(csrc, "btf_bands.h")).read()
    lds = eval(re.search(r"FUNC_SORT_LDS = ([0-9* ]+);", func).group(1))
    assert re.search(r"FUNC_MAX_S = FUNC_SORT_LDS / 8;", func) and bands.MAX_SAMPLES["supt"] == lds // 8
    rank_lds = eval(re.search(r"BAND_RANK_LDS = ([0-9* ]+);", band).group(1))
    per = int(re.search(r"BAND_RANK_BYTES = (\d+);", band).group(1))
    assert re.search(r"BAND_RANK_MAX_S = BAND_RANK_LDS / BAND_RANK_BYTES;", band)
    assert bands.MAX_SAMPLES["rank"] == rank_lds // per >= 4096 and rank_lds <= 64 * 1024
    text = open(os.path.join(csrc, "btf_analysis.hip")).read()
    assert "method == BAND_SUPT ? FUNC_MAX_S : BAND_RANK_MAX_S" in text
    assert set(bands.METHODS.items()) == {("supt", int(re.search(r"BAND_SUPT = (\d)", band).group(1))),
                                          ("rank", int(re.search(r"BAND_RANK = (\d)", band).group(1)))}


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_bands", "btf_collect_bands"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_bands") and hasattr(lib, "btf_collect_bands")
    assert len(_native.SIGNATURES["btf_posterior_bands"][1]) == 23
    assert len(_native.SIGNATURES["btf_collect_bands"][1]) == 17
    # no new compilation unit, and the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert not os.path.exists(os.path.join(_native.CSRC, "btf_bands.hip"))
    assert re.search(r"BTF_K_COUNT = %d\b" % len(_native.KERNEL_NAMES), text)


def test_no_spills_or_scratch_in_the_band_kernels():
    """Code-object notes (scripts/kernel_notes.py): the moments, sweep and rank kernels at every nembeds 1..10 and transform
    and the supt reduction neither spill VGPRs nor use scratch; the static LDS of the sorting kernels leaves room for
    their 64 KiB of rows twice per CU."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"band_(moments|sweep|rank_depth|rank_write|rank_k|supt)_kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    every = {(k, t) for k in range(1, 11) for t in range(3)}
    for kind in ("moments", "sweep", "rank_depth", "rank_write"):
        inst = {(int(k), int(t)) for r in rows for k, t in re.findall(r"band_%s_kernelILi(\d+)ELi(\d+)E" % kind, r["mangled"])}
        assert inst == every, (kind, inst)
    assert len(rows) == 4 * 30 + 2
    assert all(r["lds"] + 64 * 1024 <= 80 * 1024 for r in rows if "band_moments_kernel" not in r["mangled"])
