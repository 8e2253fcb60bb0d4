"""Host halves of the EP-centred GASS updates (ep_approx): utils.ep_from_mf against the reference's outputs, the
argument checks made before any device call, the ABI symbol, and the register budget of the new kernels.  No GPU."""
import contextlib
import importlib.util
import io
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, utils


class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def test_ep_from_mf_equals_the_references(golden):
    """utils.py:423-438 run by the reference (tests/golden/make_golden_gass_ep.py): both modes, 3-D and 4-D Y with NaNs,
    the same arrays bit for bit and the same printed line."""
    g = golden("g13_gass_ep.npz")
    W, V, Y = g["s0_W"], g["s0_V"], g["Y"]
    for mode in ("max", "multiplier"):
        for nd, Yx in ((3, Y[..., 0]), (4, Y)):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                mu, sg = utils.ep_from_mf(Yx, W, V, mode=mode, multiplier=3)
            np.testing.assert_array_equal(mu, g["epmf_%s_%dd_mu" % (mode, nd)])
            np.testing.assert_array_equal(sg, g["epmf_%s_%dd_sigma" % (mode, nd)])
            assert buf.getvalue() == "Estimated stdev: {}\n".format(sg.flat[0])
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError):
            utils.ep_from_mf(Y, W, V, mode="median")


def _make(ep, **kw):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    N, M, T = 4, 3, 5
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    return ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", Cons, ep_approx=ep, nembeds=2, **kw)


@pytest.mark.parametrize("ep", [
    np.ones((4, 3, 5)),                                       # not a pair
    (np.ones((4, 3, 5)),),                                    # one array
    (np.ones((4, 3, 5)), np.ones((4, 3, 5)), np.ones(1)),      # three
    (np.ones((4, 3, 4)), np.ones((4, 3, 5))),                 # Mu_ep of the wrong shape
    (np.ones((4, 3, 5)), np.ones((2, 5))),                    # Sigma_ep does not broadcast
    (np.full((4, 3, 5), np.nan), np.ones((4, 3, 5))),         # NaN in Mu_ep
    (np.full((4, 3, 5), np.inf), np.ones((4, 3, 5))),
    (np.ones((4, 3, 5)), np.zeros((4, 3, 5))),                # Sigma_ep <= 0
    (np.ones((4, 3, 5)), -np.ones((4, 3, 5))),
    (np.ones((4, 3, 5)), np.full((4, 3, 5), np.nan)),
    (np.ones((4, 3, 5)), np.full((4, 3, 5), np.inf)),
])
def test_bad_ep_approx_raises_before_any_device_call(no_device, ep):
    with pytest.raises(ValueError):
        _make(ep)


@pytest.mark.parametrize("T, K, tf", [(5, 11, 0), (5, 2, 5), (200, 10, 2)])
def test_ep_limits_are_checked_up_front(no_device, T, K, tf):
    """nembeds > 10, ndepth < tf_order + 1, and column systems whose vectors and blocks do not fit on chip raise ValueError
    in the constructor, before any device call."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    with pytest.raises(ValueError):
        ConstrainedNonconjugateBayesianTensorFiltering(4, 3, T, "poisson_identity", Cons, nembeds=K, tf_order=tf,
                                                       ep_approx=(np.ones((4, 3, T)), np.ones((4, 3, T))))


def test_callable_likelihood_still_raises(no_device):
    """(a regression guard: the constrained model's likelihood must name a device likelihood, with or without EP)"""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    Cons = np.concatenate([np.eye(5), np.zeros((5, 1))], axis=1)
    with pytest.raises(NotImplementedError):
        ConstrainedNonconjugateBayesianTensorFiltering(4, 3, 5, lambda *a, **k: 0.0, Cons, nembeds=2,
                                                       ep_approx=(np.ones((4, 3, 5)), np.ones((4, 3, 5))))


def test_set_ep_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    assert re.search(r"int btf_gass_set_ep\(btf_ctx\* ctx, const double\* mu, const double\* sigma\);", text)
    assert "btf_gass_set_ep" in _native.SIGNATURES
    assert any(s.endswith("btf_gass_ep.hip") for s in _native.SOURCES)
    _native.build()
    assert hasattr(_native.load(), "btf_gass_set_ep")
    assert len(_native.KERNEL_NAMES) == 15


def test_no_spills_or_scratch_in_the_ep_and_changed_gass_kernels():
    """Code-object notes (scripts/kernel_notes.py): the gass_ep_* kernels (every nembeds 1..10) and the GASS kernels
    the EP path changed neither spill VGPRs nor use scratch."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"gass_(ep_|analyse|eval_kernel|select)", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for kern in ("gass_ep_rows_kernel", "gass_ep_cols_kernel"):
        ks = {int(m) for r in rows for m in re.findall(kern + r"ILi(\d+)E", r["mangled"])}
        assert ks == set(range(1, 11)), (kern, ks)
    assert any(re.search(r"gass_eval_kernelILi\d+ELb[01]ELb1E", r["mangled"]) for r in rows)
    assert any(re.search(r"gass_analyse_cols_kernelILb1E", r["mangled"]) for r in rows)
