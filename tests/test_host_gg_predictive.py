"""Host halves of the gamma-grid posterior predictive (predictive.gamma_grid_*, GammaGridLikelihood.sample,
NonconjugateBayesianTensorFiltering.gamma_grid_predictive, utils.gamma_grid_predictive): the registration of the native
entry points, the mean, the host sampler, and every refusal made before any device call.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
from scipy import stats

from functionalmf_amd import _native, likelihoods, predictive, utils
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering, NonconjugateBayesianTensorFiltering

PFLOOR = 1e-6           # the p-value floor of tests/test_gpu_predictive.py
N, M, T, K, S = 5, 3, 4, 2, 6


def test_registration():
    assert os.path.join(_native.CSRC, "btf_gg_predict.hip") in _native.SOURCES
    assert os.path.exists(os.path.join(_native.CSRC, "btf_gg_predict.h"))
    header = open(os.path.join(_native.ROOT, "include", "btf.h")).read()
    analysis = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    abi = open(os.path.join(_native.CSRC, "btf_abi.hip")).read()
    for name in ("btf_predict_gg_eval", "btf_predict_gg_batch"):
        assert name in _native.SIGNATURES
        nargs = header.split("int %s(" % name)[1].split(");")[0].count(",") + 1
        assert nargs == len(_native.SIGNATURES[name][1]), name
        definition = re.compile(r"^int %s\(" % name, re.M)
        assert len(definition.findall(analysis)) == 1 and not definition.search(abi), name
    # the outputs of the two eval entries: the same eleven arrays in the same order
    outs = lambda name: [a.split()[-1] for a in header.split("int %s(" % name)[1].split(");")[0].split(",")][-11:]
    assert outs("btf_predict_gg_eval") == outs("btf_predict_eval")
    # the old family table is as it was
    assert "gamma_grid" not in predictive.FAMILIES and max(predictive.FAMILIES.values()) == 4
    with pytest.raises(ValueError):
        predictive.family_code(5)
    lib_path = _native.LIB_PATH
    if os.path.exists(lib_path):
        lib = _native.load()
        assert hasattr(lib, "btf_predict_gg_eval") and hasattr(lib, "btf_predict_gg_batch")


def test_gamma_grid_mean_against_a_direct_sum():
    rs = np.random.RandomState(0)
    a, s, p = rs.uniform(0.3, 30, size=17), rs.uniform(0.01, 2, size=17), rs.gamma(2.0, 1.0, size=17)
    p[[0, 5, 16]] = 0.0                                # zero-weight components, the first and the last among them
    eta = np.array([-1.0, 0.0, np.nan, 1e-3, 0.7, 40.0])
    for scale in (1.0, 7.0, 1.0 / p.sum()):            # unnormalised weights: the mean does not move
        lik = likelihoods.GammaGridLikelihood.from_table(a, s, p * scale)
        got = predictive.gamma_grid_mean(lik, eta)
        mbar = float(np.sum(p / p.sum() * a * s))
        assert np.isnan(got[:3]).all()
        np.testing.assert_allclose(got[3:], eta[3:] * mbar, rtol=1e-13)
    # the reference's triple: mean of component g is mean_grid[g] * eta
    grid, probs = np.linspace(0.6, 1.4, 5), np.array([1.0, 2.0, 0.0, 4.0, 1.0])
    np.testing.assert_allclose(predictive.gamma_grid_mean((grid, probs, 0.03), 2.0), 2.0 * (grid * probs).sum() / probs.sum(), rtol=1e-13)
    # the cumulative weights: ascending, ending at 1, flat over a zero weight
    _, _, w, c, _ = predictive.gamma_grid_weights(likelihoods.GammaGridLikelihood.from_table(a, s, p))
    assert np.all(np.diff(c) >= 0) and abs(c[-1] - 1.0) < 1e-14 and c[0] == 0.0 and c[5] == c[4] and w[5] == 0.0
    with pytest.raises(ValueError):
        predictive.gamma_grid_mean((grid, -probs, 0.03), 1.0)


def test_host_sample_one_component_is_a_gamma():
    lik = likelihoods.GammaGridLikelihood.from_table([2.5], [0.4], [3.0])
    x = lik.sample(1.7, size=50000, rng=np.random.RandomState(1))
    assert x.shape == (50000,)
    p = stats.kstest(x, stats.gamma(2.5, scale=0.4 * 1.7).cdf).pvalue
    print("host sample KS p", p)
    assert p >= PFLOOR
    # the shape of fit.py:476: effect (1, T) against size [100, S, T]
    y = lik.sample(np.full((1, 4), 0.5), size=[10, 3, 4], rng=np.random.RandomState(2))
    assert y.shape == (10, 3, 4) and np.all(y > 0)
    assert np.isnan(lik.sample(np.array([-1.0, 0.0, np.nan]), size=3, rng=np.random.RandomState(3))).all()


def test_host_sample_never_draws_a_zero_weight_component():
    # three components far apart: a draw tells its component
    lik = likelihoods.GammaGridLikelihood.from_table([4e4, 4e4, 4e4], [1.0 / 4e4, 10.0 / 4e4, 100.0 / 4e4], [1.0, 0.0, 3.0])
    x = lik.sample(1.0, size=40000, rng=np.random.RandomState(4))
    near = lambda m: np.abs(x / m - 1.0) < 0.1
    assert near(10.0).sum() == 0 and near(1.0).sum() + near(100.0).sum() == x.size
    # weighted, not uniform: 1/4 and 3/4 (a binomial count within 5.5 sd)
    assert abs(near(1.0).sum() - 0.25 * x.size) <= 5.5 * np.sqrt(x.size * 0.25 * 0.75)


# ---- a model with no device behind it: every refusal comes before any device call
class _NoDevice:
    def call(self, name, *args):
        raise AssertionError("device entry point %s called" % name)


def _model_without_a_device(cls=NonconjugateBayesianTensorFiltering, link=5, world=1, collected=S):
    m = object.__new__(cls)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.device = N, M, T, K, 0
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    m._link, m._callback = link, False
    m.loglikelihood = {5: "gamma_grid", 1: "poisson_identity"}[link]
    m._collected, m._draws, m._device_seed = collected, 0, 1
    return m


RES = dict(W=np.ones((S, N, K)), V=np.ones((S, M, T, K)))
Y = np.full((N, M, T), 0.5)


@pytest.mark.parametrize("cls", [NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering])
def test_model_refusals_come_before_any_device_call(cls):
    assert cls.gamma_grid_predictive is NonconjugateBayesianTensorFiltering.gamma_grid_predictive       # inherited
    with pytest.raises(ValueError, match="use posterior_predictive"):
        _model_without_a_device(cls, link=1).gamma_grid_predictive(RES, data=Y)
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(cls, world=2).gamma_grid_predictive(RES, data=Y)
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device(cls, collected=0).gamma_grid_predictive(data=Y)
    m = _model_without_a_device(cls)
    with pytest.raises(ValueError, match="16384"):
        m.gamma_grid_predictive(RES, data=Y, draws_per_sample=16384 // S + 1)
    with pytest.raises(ValueError, match="16384"):
        m.gamma_grid_predictive(data=Y, draws_per_sample=16384 // S + 1)               # the collected samples
    for bad in ([N * M * T], [-1], [(0, M, 0)], [0.5]):
        with pytest.raises(ValueError, match="cells"):
            m.gamma_grid_predictive(RES, data=Y, cells=bad)
    for y0 in (0.0, -0.3):
        Yb = Y.copy()
        Yb[1, 2, 3] = y0
        with pytest.raises(ValueError, match="y > 0"):
            m.gamma_grid_predictive(RES, data=Yb)
    with pytest.raises(ValueError, match="pair"):
        m.gamma_grid_predictive(RES, data=(Y, Y))
    with pytest.raises(ValueError):
        m.gamma_grid_predictive(RES, data=np.zeros((N, M, T + 1)))
    with pytest.raises(ValueError, match=r"\[0, 100\]"):
        m.gamma_grid_predictive(RES, data=Y, q=(5, 101))
    with pytest.raises(ValueError):
        m.gamma_grid_predictive(dict(W=RES["W"], V=RES["V"][:, :, :3]), data=Y)
    assert m._draws == 0                               # no refusal took a seed
    # the old refusal still names the likelihood, and now the way out
    with pytest.raises(NotImplementedError, match="gamma_grid") as err:
        m.posterior_predictive(RES)
    assert "gamma_grid_predictive" in str(err.value)


def test_stateless_refusals_come_before_any_device_call(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(_native, "Context", no_context)
    monkeypatch.setattr(_native, "load", no_context)
    lik = (np.linspace(0.6, 1.4, 5), np.ones(5), 0.03)
    Ws, Vs = RES["W"], RES["V"]
    bad_tables = [(np.linspace(0.6, 1.4, 5), np.zeros(5), 0.03), (np.linspace(0.6, 1.4, 5), -np.ones(5), 0.03),
                  (np.linspace(0.0, 1.4, 5), np.ones(5), 0.03), (np.linspace(0.6, 1.4, 129), np.ones(129), 0.03),
                  (np.linspace(0.6, 1.4, 5), np.ones(4), 0.03), "gamma"]
    for bad in bad_tables:
        with pytest.raises(ValueError, match="gamma.grid|likelihood_param"):
            utils.gamma_grid_predictive(Ws, Vs, bad, data=Y)
        with pytest.raises(ValueError, match="gamma.grid|likelihood_param"):
            predictive.gamma_grid_batch(np.ones(3), bad)
    with pytest.raises(ValueError, match="16384"):
        utils.gamma_grid_predictive(Ws, Vs, lik, draws_per_sample=3000)
    with pytest.raises(ValueError, match="cells"):
        utils.gamma_grid_predictive(Ws, Vs, lik, cells=[N * M * T])
    Yb = Y.copy()
    Yb[0, 0, 0] = 0.0
    with pytest.raises(ValueError, match="y > 0"):
        utils.gamma_grid_predictive(Ws, Vs, lik, data=Yb)
    with pytest.raises(ValueError, match="pair"):
        utils.gamma_grid_predictive(Ws, Vs, lik, data=(Y, Y))
    with pytest.raises(ValueError, match="Ws must be"):
        utils.gamma_grid_predictive(Ws, Vs[:, :, :, :1], lik)


def test_evaluate_refuses_on_its_own():
    ctx = _NoDevice()
    with pytest.raises(ValueError, match="y > 0"):
        predictive.gamma_grid_evaluate(ctx, (N, M, T), K, S, RES["W"], RES["V"], Y=-Y)
    with pytest.raises(ValueError, match="pair"):
        predictive.gamma_grid_evaluate(ctx, (N, M, T), K, S, RES["W"], RES["V"], Y=(Y, Y))
    with pytest.raises(ValueError, match="both Ws and Vs"):
        predictive.gamma_grid_evaluate(ctx, (N, M, T), K, S, RES["W"], None)
    with pytest.raises(AssertionError, match="btf_predict_gg_eval"):                    # and then makes its one call
        predictive.gamma_grid_evaluate(ctx, (N, M, T), K, S, RES["W"], RES["V"], Y=Y)
