"""Host halves of tensor_nmf / factor_pav (functionalmf_amd/nmf.py): the seeded starting point, the statistics, the
argument checks made before any device call, and the register budget of the nmf_* kernels.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from functionalmf_amd import _native, nmf, utils


class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


class _Started(Exception):
    pass


def test_seeded_starting_point_equals_the_references(golden, monkeypatch):
    """np.random.seed(s) gives the reference's W0 / V0 (utils.py:283-292); a given W or V is passed on unchanged."""
    g = golden("g12_nmf.npz")
    seen = {}

    def fake_run(self, W, V, **kw):
        seen["W"], seen["V"] = np.array(W), np.array(V)
        raise _Started

    monkeypatch.setattr(nmf.NMFData, "__init__", lambda self, Y, K, device=0: None)
    monkeypatch.setattr(nmf.NMFData, "run", fake_run)
    monkeypatch.setattr(nmf.NMFData, "close", lambda self: None)
    for case in g["cases"]:
        p = str(case) + "_"
        np.random.seed(int(g[p + "seed"]))
        kw = {k: g[p + k] for k in ("W_in", "V_in") if p + k in g}
        with pytest.raises(_Started):
            utils.tensor_nmf(g[p + "Y"], int(g[p + "K"]), W=kw.get("W_in"), V=kw.get("V_in"))
        assert np.array_equal(seen["W"], g[p + "W0"]), case
        assert np.array_equal(seen["V"], g[p + "V0"]), case


def test_statistics_reproduce_the_residual_sum_of_squares():
    """RSS = ssw + sum (S - C m)^2 / C equals sum over the observed entries of (y - m)^2; counts only with gaps."""
    rs = np.random.RandomState(0)
    Y = rs.gamma(2.0, 1.0, size=(6, 5, 4, 3))
    S, cnt, ssw = nmf.nmf_statistics(Y)
    assert cnt is None and S.shape == (6, 20)
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    Y[:2, :2] = np.nan
    S, cnt, ssw = nmf.nmf_statistics(Y)
    assert cnt.dtype == np.uint8 and cnt.shape == (6, 20) and S.flags.c_contiguous
    Mu = rs.gamma(1.0, 1.0, size=(6, 5, 4))
    want = np.nansum((Y - Mu[..., None]) ** 2)
    m = Mu.reshape(6, 20)
    c = cnt.astype(float)
    got = ssw + np.sum(np.where(c > 0, (S - c * m) ** 2 / np.maximum(c, 1), 0.0))
    assert abs(got - want) <= 1e-12 * want
    S3, cnt3, ssw3 = nmf.nmf_statistics(Y[..., 0])
    assert ssw3 == 0.0 and np.array_equal(S3, np.nan_to_num(Y[..., 0]).reshape(6, 20))


def test_unsupported_and_bad_arguments_raise_before_any_device_call(no_device):
    Y = np.ones((4, 3, 5, 2))
    with pytest.raises(NotImplementedError):
        utils.tensor_nmf(Y, 2, max_entry=3.0)
    with pytest.raises(NotImplementedError):
        utils.tensor_nmf(Y, 2, row_features=np.ones((4, 2)))
    for k in (0, 11, -1, 2.5, True):
        with pytest.raises(ValueError):
            utils.tensor_nmf(Y, k)
    with pytest.raises(ValueError):
        utils.tensor_nmf(np.ones((4, 3)), 2)
    with pytest.raises(ValueError):
        utils.tensor_nmf(np.ones((4, 3, 5, 2, 1)), 2)
    with pytest.raises(ValueError):
        utils.tensor_nmf(Y, 2, W=np.ones((4, 3)))
    with pytest.raises(ValueError):
        utils.tensor_nmf(Y, 2, V=np.ones((3, 4, 2)))
    with pytest.raises(ValueError):
        utils.tensor_nmf(np.ones((4, 3, 5, 300)), 2)
    with pytest.raises(ValueError):
        utils.factor_pav(np.ones((4, 3)), np.ones((5, 2)))
    with pytest.raises(ValueError):
        utils.factor_pav(np.ones((4, 11)), np.ones((5, 11)))
    with pytest.raises(ValueError):
        utils.factor_pav(np.ones(4), np.ones((5, 1)))
    # non-finite input: a given factor with nan or inf, +-inf in the data (nan there is a missing entry)
    for bad in (np.nan, np.inf, -np.inf):
        Wb, Vb = np.ones((4, 2)), np.ones((3, 5, 2))
        Wb[3, 1] = bad
        Vb[2, 4, 0] = bad
        with pytest.raises(ValueError, match="W must be finite"):
            utils.tensor_nmf(Y, 2, W=Wb)
        with pytest.raises(ValueError, match="V must be finite"):
            utils.tensor_nmf(Y, 2, V=Vb, fit_V=False)
        if np.isinf(bad):
            Yb = Y.copy()
            Yb[1, 2, 3, 0] = bad
            with pytest.raises(ValueError, match="Y must be finite"):
                utils.tensor_nmf(Yb, 2)
            with pytest.raises(ValueError, match="Y must be finite"):
                utils.tensor_nmf(Yb[..., 0], 2, W=np.ones((4, 2)), V=np.ones((3, 5, 2)))
            with pytest.raises(ValueError, match="Y must be finite"):
                nmf.NMFData(Yb, 2)
            with pytest.raises(ValueError, match="Y must be finite"):
                nmf.nmf_statistics(Yb)


def test_a_handle_refuses_non_finite_factors_before_any_device_call(monkeypatch):
    """NMFData.run checks its own arguments: the handle's library is never called."""
    data = nmf.NMFData.__new__(nmf.NMFData)
    data.shape, data.nembeds, data.lib, data.h, data._bounded = (4, 3, 5, 2), 2, _NoDevice(), None, False
    W, V = np.ones((4, 2)), np.ones((3, 5, 2))
    for bad in (np.nan, np.inf, -np.inf):
        for name, idx in (("W", (0, 0)), ("V", (1, 2, 1))):
            a = {"W": W.copy(), "V": V.copy()}
            a[name][idx] = bad
            with pytest.raises(ValueError, match=name + " must be finite"):
                data.run(a["W"], a["V"], max_steps=1)
        Rb = np.ones((2, 2))
        Rb[1, 0] = bad
        with pytest.raises(ValueError, match="R must be finite"):
            data.run(W, V, max_steps=1, row_features=np.ones((4, 2)), R=Rb)


def test_nmf_entry_points_are_declared():
    for name in ("btf_nmf_create", "btf_nmf_run", "btf_nmf_destroy", "btf_nmf_pav"):
        assert name in _native.SIGNATURES
    assert any(s.endswith("btf_nmf.hip") for s in _native.SOURCES)


def test_no_vgpr_spills_in_the_nmf_kernels():
    """Code-object notes of the built library (scripts/kernel_notes.py): no nmf_* kernel spills VGPRs or uses scratch,
    for every nembeds 1..10 (the per-lane NNLS keeps its factor in registers and its system in LDS)."""
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if "nmf_" in r["mangled"]]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for kern in ("nmf_wsolve_kernel", "nmf_vsolve_kernel", "nmf_wpart_kernel", "nmf_vpart_kernel", "nmf_rss_kernel",
                 "nmf_gram_kernel", "nmf_pav_kernel"):
        ks = {int(m) for r in rows for m in __import__("re").findall(kern + r"ILi(\d+)E", r["mangled"])}
        assert ks == set(range(1, 11)), (kern, ks)
    assert not any("accum_kernel" in r["mangled"] for r in rows)
