"""Host halves of the posterior curve functionals (functionalmf_amd/functionals.py): the numpy definition against
hand-worked curves, the argument checks made before any device call, the ABI symbols, and the register budget of the new
kernels.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, functionals, utils

trapezoid = getattr(np, "trapezoid", None) or np.trapz


class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def test_straight_line():
    x = np.linspace(0, 1, 5)
    f = functionals.curve_functionals(1.0 - 2.0 * x, level=0.5)          # falls from 1 to -1
    assert f["auc"] == pytest.approx(0.0, abs=1e-15)
    assert (f["max"], f["min"], f["argmax"], f["argmin"], f["rise"]) == (1.0, -1.0, 0.0, 1.0, 0.0)
    assert f["crossing"] == pytest.approx(0.25, abs=1e-15)
    g = functionals.curve_functionals(2.0 * x, level=0.25)               # rises from 0 to 2
    assert g["auc"] == pytest.approx(1.0) and g["rise"] == pytest.approx(2.0) and g["crossing"] == pytest.approx(0.125)
    assert (g["argmax"], g["argmin"]) == (1.0, 0.0)


def test_constant_curve():
    x = np.array([2.0, 3.0, 5.0, 9.0])
    m = np.full(4, 0.7)
    f = functionals.curve_functionals(m, x, level=0.7)
    assert f["crossing"] == 2.0                                          # the level itself: crossed at x[0]
    assert f["rise"] == 0.0 and f["argmax"] == 2.0 and f["argmin"] == 2.0 and f["max"] == 0.7 and f["min"] == 0.7
    assert f["auc"] == pytest.approx(0.7 * 7.0)
    for level in (0.6, 0.8, 0.0):
        assert np.isnan(functionals.curve_functionals(m, x, level=level)["crossing"])


def test_touching_the_level_at_a_grid_point_and_ties_in_the_maximum():
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    f = functionals.curve_functionals(np.array([3.0, 2.0, 1.0, 2.0, 3.0]), x, level=1.0)
    assert f["crossing"] == 2.0                                          # touches the level exactly at x[2], never below
    assert f["argmax"] == 0.0 and f["argmin"] == 2.0                     # the maximum 3 is taken at x[0] and x[4]: first
    assert f["rise"] == 2.0 and f["auc"] == 8.0
    f = functionals.curve_functionals(np.array([0.0, 5.0, 5.0, 1.0, 5.0]), x, level=5.0)
    assert f["argmax"] == 1.0 and f["crossing"] == 1.0 and f["rise"] == 9.0
    f = functionals.curve_functionals(np.array([4.0, 4.0, 6.0, 6.0, 0.0]), x, level=5.0)     # strict crossing between points
    assert f["crossing"] == 1.5 and f["argmax"] == 2.0 and f["argmin"] == 4.0


def test_non_uniform_x_and_batches_equal_np_trapz():
    rs = np.random.RandomState(0)
    x = np.cumsum(rs.uniform(0.1, 2.0, size=9))
    m = rs.normal(size=(4, 3, 9))
    f = functionals.curve_functionals(m, x, level=0.1)
    assert np.array_equal(f["auc"], trapezoid(m, x, axis=-1))
    assert np.array_equal(f["argmax"], x[m.argmax(-1)]) and np.array_equal(f["argmin"], x[m.argmin(-1)])
    assert np.allclose(f["rise"], np.clip(np.diff(m, axis=-1), 0, None).sum(-1), rtol=0, atol=0)
    for idx in np.ndindex(4, 3):                                         # the crossing by a plain loop over the definition
        d, want = m[idx] - 0.1, np.nan
        if d[0] == 0:
            want = x[0]
        else:
            for t in range(8):
                if d[t] * d[t + 1] < 0 or d[t + 1] == 0:
                    want = x[t] + (x[t + 1] - x[t]) * d[t] / (d[t] - d[t + 1])
                    break
        got = f["crossing"][idx]
        assert (np.isnan(want) and np.isnan(got)) or got == pytest.approx(want, rel=1e-15, abs=1e-15)
    # default x: the reference's dx = 1 / (T - 1)
    assert np.allclose(functionals.curve_functionals(m)["auc"], trapezoid(m, dx=1.0 / 8, axis=-1), rtol=1e-15, atol=1e-15)


def test_censored_percentile_rule():
    v = np.array([1.0, np.nan, 2.0, 3.0, np.nan])                        # sorted: 1 2 3 inf inf
    got = functionals.censored_percentile(v, [0, 25, 50, 60, 100])
    assert got[0] == 1.0 and got[1] == 2.0 and np.all(np.isnan(got[2:]))


@pytest.mark.parametrize("kw,msg", [
    (dict(which=("auc", "area")), "unknown functional"),
    (dict(which=("crossing",)), "level"),
    (dict(which=()), "at least one"),
    (dict(which=("auc", "auc")), "twice"),
    (dict(x=np.array([0.0, 0.5, 0.5, 1.0])), "strictly increasing"),
    (dict(x=np.array([0.0, 1.0, 0.5, 2.0])), "strictly increasing"),
    (dict(x=np.linspace(0, 1, 5)), "ndepth"),
    (dict(q=(5, 101)), r"\[0, 100\]"),
    (dict(q=(-1,)), r"\[0, 100\]"),
    (dict(transform="log"), "transform"),
    (dict(curves=[(0, 9)]), "curves"),
])
def test_argument_checks_raise_before_the_library_is_loaded(no_device, kw, msg):
    Ws, Vs = np.zeros((3, 5, 2)), np.zeros((3, 4, 4, 2))
    with pytest.raises(ValueError, match=msg):
        utils.posterior_functionals(Ws, Vs, **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    with pytest.raises(ValueError, match="ndepth >= 2"):
        utils.posterior_functionals(np.zeros((3, 5, 2)), np.zeros((3, 4, 1, 2)))
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_functionals(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)))
    S = functionals.MAX_SAMPLES + 1
    with pytest.raises(ValueError, match="exceed %d" % functionals.MAX_SAMPLES):
        utils.posterior_functionals(np.zeros((S, 1, 1)), np.zeros((S, 1, 2, 1)))
    assert functionals.MAX_SAMPLES >= 8192


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_functionals", "btf_collect_functionals"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_functionals") and hasattr(lib, "btf_collect_functionals")
    assert len(_native.SIGNATURES["btf_posterior_functionals"][1]) == 25
    assert len(_native.SIGNATURES["btf_collect_functionals"][1]) == 19
    assert os.path.join(_native.CSRC, "btf_functionals.hip") in _native.SOURCES
    # the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert re.search(r"BTF_K_COUNT = %d\b" % len(_native.KERNEL_NAMES), text)


def test_no_spills_or_scratch_in_the_functionals_kernels():
    """Code-object notes (scripts/kernel_notes.py): the sweep at every nembeds 1..10 and transform, the sort and the gather
    neither spill VGPRs nor use scratch; the sort's static LDS leaves room for its 64 KiB of rows twice per CU."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"func_(sweep|sort|gather)_kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    inst = {(int(k), int(t)) for r in rows for k, t in re.findall(r"func_sweep_kernelILi(\d+)ELi(\d+)E", r["mangled"])}
    assert inst == {(k, t) for k in range(1, 11) for t in range(3)}, inst
    sort = [r for r in rows if "func_sort_kernel" in r["mangled"]]
    assert len(sort) == 1 and len([r for r in rows if "func_gather_kernel" in r["mangled"]]) == 1
    assert sort[0]["lds"] + 64 * 1024 <= 80 * 1024, sort[0]["lds"]
