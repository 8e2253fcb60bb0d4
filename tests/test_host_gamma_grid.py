"""Host halves of the gamma-grid likelihood (loglikelihood="gamma_grid"): the host class against the reference's own
logpdf (tests/golden/g14_gamma_grid.npz), the table and data checks made before any device call, the ABI symbols, and
the register budget of the new kernels.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, likelihoods


class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def test_logpdf_equals_the_references(golden):
    g = golden("g14_gamma_grid.npz")
    lik = likelihoods.GammaGridLikelihood(g["mean_grid"], g["mean_probs"], float(g["variance"]))
    v = lik.logpdf(g["logpdf_y"], g["logpdf_effect"])
    np.testing.assert_allclose(v, g["logpdf"], rtol=1e-12, atol=1e-12)
    # the fully missing row: log sum p (the reference's nansum)
    assert np.all(np.isnan(g["logpdf_y"][5]))
    assert v[5] == pytest.approx(np.log(g["mean_probs"].sum()), rel=1e-14)


def test_logpdf_edge_cases():
    lik = likelihoods.GammaGridLikelihood(np.array([0.8, 1.2]), np.array([0.3, 0.7]), 0.05)
    y = np.array([[0.9, np.nan], [np.nan, np.nan], [1.1, 0.7]])
    v = lik.logpdf(y, np.array([[0.0], [0.0], [-1.0]]))
    assert v[0] == -np.inf and v[2] == -np.inf           # observed cells at eta <= 0 (documented deviation)
    assert v[1] == pytest.approx(0.0, abs=1e-15)          # no observations, normalised weights


def _make(param, **kw):
    from functionalmf_amd.factor import NonconjugateBayesianTensorFiltering
    return NonconjugateBayesianTensorFiltering(4, 3, 5, "gamma_grid", likelihood_param=param, nembeds=2, **kw)


GOOD = (np.array([0.8, 1.0, 1.2]), np.array([0.2, 0.5, 0.3]), 0.02)


@pytest.mark.parametrize("param", [
    None,
    (np.array([0.8, 1.0]),),                                          # not a triple
    (np.array([0.8, np.nan]), np.array([0.5, 0.5]), 0.02),            # non-finite shape / scale
    (np.array([0.8, 1.0]), np.array([0.5, np.inf]), 0.02),            # non-finite weight
    (np.array([0.8, -1.0]), np.array([0.5, 0.5]), 0.02),              # scale <= 0
    (np.array([0.8, 0.0]), np.array([0.5, 0.5]), 0.02),               # scale = inf
    (np.array([0.8, 1.0]), np.array([0.5, 0.5]), -0.02),              # shape <= 0 (negative variance)
    (np.array([0.8, 1.0]), np.array([0.5, -0.1]), 0.02),              # p < 0
    (np.array([0.8, 1.0]), np.array([0.0, 0.0]), 0.02),               # all p = 0
    (np.array([0.8, 1.0]), np.array([0.5, 0.5, 0.1]), 0.02),          # lengths differ
    (np.linspace(0.5, 1.5, 129), np.ones(129), 0.02),                 # G > 128
    (np.zeros(0), np.zeros(0), 0.02),                                 # G = 0
])
def test_bad_tables_raise_before_any_device_call(no_device, param):
    with pytest.raises(ValueError):
        _make(param)


def test_table_by_duck_typing_and_triple_agree():
    lik = likelihoods.GammaGridLikelihood(*GOOD)
    a = likelihoods.gamma_grid_table(lik)
    b = likelihoods.gamma_grid_table(GOOD)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(ValueError):
        likelihoods.gamma_grid_table(object())


def test_constrained_model_checks_the_table_first(no_device):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    Cons = np.concatenate([np.eye(5), np.zeros((5, 1))], axis=1)
    with pytest.raises(ValueError):
        ConstrainedNonconjugateBayesianTensorFiltering(4, 3, 5, "gamma_grid", Cons, nembeds=2,
                                                       likelihood_param=(np.ones(2), np.zeros(2), 0.1))


def test_nonpositive_observation_raises_before_the_data_reach_the_device():
    """_upload checks every observed y > 0 before its first device call (the context itself is not touched)."""
    from functionalmf_amd.factor import NonconjugateBayesianTensorFiltering
    model = NonconjugateBayesianTensorFiltering.__new__(NonconjugateBayesianTensorFiltering)
    model._link, model.nrows, model.ncols, model.ndepth = 5, 2, 2, 3
    model._ctx = _NoDevice()
    model._plan = _NoDevice()
    Y = np.full((2, 2, 3, 2), 0.5)
    Y[0, 0, 0, 1] = np.nan
    Y[1, 1, 2, 0] = 0.0
    with pytest.raises(ValueError):
        model._upload(Y)
    Y[1, 1, 2, 0] = -0.3
    with pytest.raises(ValueError):
        model._upload(Y)


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    assert re.search(r"int btf_set_likelihood_table\(btf_ctx\* ctx, int link, const double\* shape, const double\* scale, "
                     r"const double\* prob, int G\);", text)
    assert re.search(r"int btf_set_data_logsum\(btf_ctx\* ctx, const double\* y_rows, const double\* y_cols, int nreps\);", text)
    assert "link 5" in text
    for name in ("btf_set_likelihood_table", "btf_set_data_logsum"):
        assert name in _native.SIGNATURES
    assert any(s.endswith("btf_gamma_grid.hip") for s in _native.SOURCES)
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_set_likelihood_table") and hasattr(lib, "btf_set_data_logsum")
    assert len(_native.KERNEL_NAMES) == 15


def test_no_spills_or_scratch_in_the_gamma_grid_kernels():
    """Code-object notes (scripts/kernel_notes.py): every gg_* kernel (the whole-state passes at every nembeds 1..10, the
    four candidate evaluations, the log-sum statistic) neither spills VGPRs nor uses scratch."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"gg_(ll_rows|ll_cols|eval|logsum)_kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for kern in ("gg_ll_rows_kernel", "gg_ll_cols_kernel"):
        ks = {int(m) for r in rows for m in re.findall(kern + r"ILi(\d+)E", r["mangled"])}
        assert ks == set(range(1, 11)), (kern, ks)
    evals = {m for r in rows for m in re.findall(r"gg_eval_kernelILb([01])ELb([01])E", r["mangled"])}
    assert evals == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}, evals
