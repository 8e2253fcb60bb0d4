"""Host halves of the posterior predictive (functionalmf_amd/predictive.py): the family table, the mean function, the
argument checks, the rate layout and the registration of the native entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
from scipy.special import expit, gammaln

from functionalmf_amd import _native, predictive
from functionalmf_amd.factor import (BayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)

CSRC = os.path.join(os.path.dirname(predictive.__file__), "csrc")


def test_family_table_matches_the_criteria_codes():
    from functionalmf_amd import criteria
    assert predictive.family_code("poisson") == criteria.FAMILY_POISSON_LOG == 0
    assert predictive.family_code("poisson_identity") == criteria.FAMILY_POISSON_IDENTITY == 1
    assert predictive.family_code("binomial") == predictive.family_code("bernoulli") == criteria.FAMILY_LOGIT == 2
    assert predictive.family_code("gaussian") == criteria.FAMILY_GAUSSIAN == 3
    assert predictive.family_code("negative_binomial") == criteria.FAMILY_NEGBIN == 4
    assert predictive.family_code(3) == 3
    for bad in ("gamma_grid", 5, -1):
        with pytest.raises(ValueError):
            predictive.family_code(bad)


def test_mean_function():
    eta = np.array([-2.0, -0.5, 0.0, 0.7, 3.0])
    np.testing.assert_array_equal(predictive.mean_function("gaussian", eta), eta)
    np.testing.assert_allclose(predictive.mean_function("poisson", eta), np.exp(eta), rtol=1e-15)
    m = predictive.mean_function("poisson_identity", eta)
    assert np.isnan(m[:3]).all() and np.array_equal(m[3:], eta[3:])
    np.testing.assert_allclose(predictive.mean_function("binomial", eta, 7.0), 7.0 * expit(eta), rtol=1e-15)
    np.testing.assert_allclose(predictive.mean_function("bernoulli", eta), expit(eta), rtol=1e-15)
    r, p = 2.5, expit(eta)
    np.testing.assert_allclose(predictive.mean_function("negbin", eta, r), r * p / (1 - p), rtol=1e-13)     # politics/benchmark.py:147-148
    with pytest.raises(ValueError):
        predictive.mean_function("negbin", eta)


def test_draw_limit_and_argument_checks():
    assert predictive.check_draws(4096, 4) == (4096, 4)
    with pytest.raises(ValueError, match="16384"):
        predictive.check_draws(4097, 4)
    with pytest.raises(ValueError):
        predictive.check_draws(10, 0)
    with pytest.raises(ValueError):
        predictive.check_draws(0, 1)
    with pytest.raises(ValueError):
        predictive.check_q([2.5, 101.0])
    shape = (3, 4, 5)
    with pytest.raises(ValueError):
        predictive.check_states(np.zeros((2, 3, 2)), np.zeros((2, 4, 6, 2)), shape, 2)
    with pytest.raises(ValueError):
        predictive.check_states(np.zeros((2, 3, 2)), np.zeros((3, 4, 5, 2)), shape, 2)
    with pytest.raises(ValueError):
        predictive.check_observations(np.zeros((3, 4, 6)), shape)
    assert predictive.check_observations(np.zeros(shape), shape).shape == (3, 4, 5, 1)
    with pytest.raises(ValueError):
        predictive.check_trials(np.zeros((3, 4)), shape)
    np.testing.assert_array_equal(predictive.check_cells([(0, 0, 1), (2, 3, 4)], shape), [1, 59])
    np.testing.assert_array_equal(predictive.check_cells(np.array([0, 59]), shape), [0, 59])
    assert predictive.check_cells(None, shape) is None
    for bad in ([60], [-1], [(0, 4, 0)], [0.5]):
        with pytest.raises(ValueError):
            predictive.check_cells(bad, shape)


def test_rate_layout():
    shape = (3, 4, 5)
    a, f = predictive.rate_layout(np.arange(6.0), 6, shape)
    assert a.shape == (6, 1) and f == _native.PRED_AUX_PER_SAMPLE
    a, f = predictive.rate_layout(np.ones((6, 1, 1, 1)), 6, shape)
    assert a.shape == (6, 1) and f == _native.PRED_AUX_PER_SAMPLE
    a, f = predictive.rate_layout(np.ones((6, 3, 1, 5)), 6, shape)
    assert a.shape == (6, 15) and f == _native.PRED_AUX_PER_SAMPLE | _native.PRED_AUX_ROWS | _native.PRED_AUX_DEPTH
    for bad in (np.ones((5, 1, 1, 1)), np.ones((6, 2, 1, 1)), np.ones((6, 3, 4))):
        with pytest.raises(ValueError):
            predictive.rate_layout(bad, 6, shape)


def test_summarise():
    inside = np.array([1.0, 2.0, np.nan, 0.0])
    nobs = np.array([1.0, 2.0, 3.0, 1.0])
    s = predictive.summarise(inside, nobs, np.array([2.5, 50.0, 97.5]))
    assert s["coverage"] == 3.0 / 4.0 and abs(s["nominal"] - 0.95) < 1e-15
    assert np.isnan(predictive.summarise(None, None, np.array([50.0]))["nominal"])


def test_native_registration_and_constants():
    assert any(os.path.basename(p) == "btf_predict.hip" for p in _native.SOURCES)
    for name in ("btf_predict_batch", "btf_predict_eval"):
        assert name in _native.SIGNATURES
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "btf.h")).read()
    assert "int btf_predict_batch(" in header and "int btf_predict_eval(" in header
    nargs = header.split("int btf_predict_eval(")[1].split(");")[0].count(",") + 1
    assert nargs == len(_native.SIGNATURES["btf_predict_eval"][1])
    src = open(os.path.join(CSRC, "btf_predict.h")).read()
    const = lambda name: float(re.search(name + r"\s*=\s*([0-9.]+)", src).group(1))
    assert const("PRED_MAX_DRAWS") == predictive.MAX_DRAWS
    assert const("PRED_POIS_SWITCH") == predictive.POISSON_SWITCH
    assert const("PRED_BINOM_SWITCH") == predictive.BINOMIAL_SWITCH
    flags = re.search(r"BTF_PRED_AUX_PER_SAMPLE = (\d+), BTF_PRED_AUX_ROWS = (\d+), BTF_PRED_AUX_COLS = (\d+), BTF_PRED_AUX_DEPTH = (\d+)", header)
    assert tuple(int(x) for x in flags.groups()) == (_native.PRED_AUX_PER_SAMPLE, _native.PRED_AUX_ROWS, _native.PRED_AUX_COLS,
                                                     _native.PRED_AUX_DEPTH)


def test_stirling_tail_table_of_the_samplers():
    """pred_fc(k) = log k! - [(k + 1/2) log(k + 1) - (k + 1) + log(2 pi) / 2]: the ten tabulated values and the series above."""
    src = open(os.path.join(CSRC, "btf_predict.h")).read()
    body = src.split("inline double pred_fc(double k)")[1].split("const double x =")[0]
    table = [float(x) for x in re.findall(r"return ([0-9.]+);", body)]
    assert len(table) == 10
    k = np.arange(10.0)
    exact = gammaln(k + 1) - ((k + 0.5) * np.log(k + 1) - (k + 1) + 0.5 * np.log(2 * np.pi))
    np.testing.assert_allclose(table, exact, atol=2e-15)
    k = np.array([10.0, 11.0, 50.0, 1e3])
    x = 1.0 / (k + 1)
    series = x * (1 / 12.0 - x**2 * (1 / 360.0 - x**2 * (1 / 1260.0 - x**2 / 1680.0)))
    exact = gammaln(k + 1) - ((k + 0.5) * np.log(k + 1) - (k + 1) + 0.5 * np.log(2 * np.pi))
    assert np.abs(series - exact).max() < 1e-12


def test_models_expose_the_method_and_refuse_what_has_no_sampler():
    assert callable(BayesianTensorFiltering.posterior_predictive)
    assert NegativeBinomialBayesianTensorFiltering._pred_family is not BayesianTensorFiltering._pred_family
    assert NonconjugateBayesianTensorFiltering._pred_family is not BayesianTensorFiltering._pred_family
    from functionalmf_amd import utils
    assert callable(utils.posterior_predictive)
    with pytest.raises(ValueError):
        utils.posterior_predictive(np.zeros((2, 3, 2)), np.zeros((3, 4, 5, 2)), "gaussian", param=1.0)
    with pytest.raises(ValueError, match="16384"):
        utils.posterior_predictive(np.zeros((9000, 3, 2)), np.zeros((9000, 4, 5, 2)), "poisson", draws_per_sample=2)
    with pytest.raises(ValueError):
        utils.posterior_predictive(np.zeros((2, 3, 2)), np.zeros((2, 4, 5, 2)), "gaussian")
