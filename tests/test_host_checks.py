"""The written definition of the posterior predictive checks (functionalmf_amd/checks.py): the discrepancies on
hand-computed curves, the variance function against closed forms, the two-sided p-value, every refusal of
posterior_checks made before any device call, and the statistical property the GPU test asserts, shown here for the numpy
reference alone (replicates drawn by numpy).  No GPU."""
import types

import numpy as np
import pytest
from scipy import stats

from functionalmf_amd import _native, checks, predictive
from functionalmf_amd.factor import GaussianBayesianTensorFiltering, NonconjugateBayesianTensorFiltering

NAN = np.nan


# ---- the discrepancies
def test_complete_curve_by_hand():
    y, mu, v = np.array([3.0, 0.0, 5.0, 2.0]), np.array([1.0, 2.0, 4.0, 2.0]), np.array([4.0, 1.0, 0.25, 2.0])
    # residuals 2, -2, 1, 0; standardised e = 1, -2, 2, 0
    d = checks.discrepancies(y, mu, v)
    assert d.shape == (5,)
    assert d[0] == 1.0 + 4.0 + 4.0 + 0.0
    assert d[1] == 2.0
    assert d[2] == (1.0 * -2.0 + -2.0 * 2.0 + 2.0 * 0.0) / (1.0 + 4.0 + 4.0 + 0.0)
    assert d[3] == 10.0 and d[4] == 1.0
    assert checks.DISCREPANCIES == ("chisq", "max", "lag1", "total", "zeros")


def test_replicates_by_hand():
    # T = 3, nreps = 2; depth 1 has one replicate missing
    y = np.array([[1.0, 3.0], [NAN, 0.0], [0.0, 0.0]])
    mu, v = np.array([1.0, 2.0, 1.0]), np.array([2.0, 1.0, 0.5])
    d = checks.discrepancies(y, mu, v)
    # residuals: (0, 2), (-, -2), (-1, -1)
    assert d[0] == (0.0 + 4.0 / 2.0) + 4.0 / 1.0 + (1.0 / 0.5 + 1.0 / 0.5)
    assert d[1] == max(2.0 / np.sqrt(2.0), 2.0, 1.0 / np.sqrt(0.5))
    e = np.array([(0.0 + 2.0) / np.sqrt(2.0 * 2), -2.0 / np.sqrt(1.0 * 1), (-1.0 + -1.0) / np.sqrt(0.5 * 2)])
    assert d[2] == (e[0] * e[1] + e[1] * e[2]) / (e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    assert d[3] == 4.0 and d[4] == 3.0            # total and zeros over the five observed slots


def test_a_gap_breaks_adjacency():
    # depth 2 has every replicate missing, between observed depths: (1,2) and (2,3) are no pairs, (0,1) and (3,4) are
    y = np.array([[1.0, 2.0], [3.0, NAN], [NAN, NAN], [0.0, 1.0], [2.0, 2.0]])
    mu, v = np.full(5, 1.0), np.full(5, 1.0)
    e = np.array([1.0 / np.sqrt(2.0), 2.0, NAN, -1.0 / np.sqrt(2.0), 2.0 / np.sqrt(2.0)])
    d = checks.discrepancies(y, mu, v)
    assert d[2] == (e[0] * e[1] + e[3] * e[4]) / (e[0] ** 2 + e[1] ** 2 + e[3] ** 2 + e[4] ** 2)
    assert d[3] == 11.0 and d[4] == 1.0
    # without the gap the pair (1,3) would count: a different value
    closed = checks.discrepancies(np.delete(y, 2, axis=0), mu[:4], v[:4])
    assert closed[2] != d[2]


def test_alternating_depths_have_no_lag1():
    y = np.array([1.0, NAN, 2.0, NAN, 0.0])
    d = checks.discrepancies(y, np.ones(5), np.ones(5))
    assert np.isnan(d[2])
    assert d[0] == 0.0 + 1.0 + 1.0 and d[1] == 1.0 and d[3] == 3.0 and d[4] == 1.0


def test_one_and_two_depths():
    d1 = checks.discrepancies(np.array([[2.0, 4.0]]), np.array([1.0]), np.array([1.0]))
    assert np.isnan(d1[2]) and d1[0] == 10.0 and d1[1] == 3.0 and d1[3] == 6.0 and d1[4] == 0.0
    d2 = checks.discrepancies(np.array([3.0, 0.0]), np.array([1.0, 1.0]), np.array([1.0, 4.0]))
    # e = 2, -1/2: one pair
    assert d2[2] == (2.0 * -0.5) / (4.0 + 0.25) and d2[0] == 4.0 + 0.25
    # a residual-free curve: the denominator is 0
    assert np.isnan(checks.discrepancies(np.array([1.0, 1.0]), np.ones(2), np.ones(2))[2])
    # no observation at all
    d0 = checks.discrepancies(np.array([NAN, NAN]), np.ones(2), np.ones(2))
    assert d0[0] == 0.0 and d0[1] == 0.0 and np.isnan(d0[2]) and d0[3] == 0.0 and d0[4] == 0.0


def test_zero_variance_slot():
    # v == 0 at depth 1: out of chisq, max and lag1 (and it breaks the adjacency), kept in total and zeros
    y, mu, v = np.array([2.0, 0.0, 3.0, 1.0]), np.array([1.0, 0.0, 1.0, 2.0]), np.array([1.0, 0.0, 4.0, 1.0])
    d = checks.discrepancies(y, mu, v)
    assert d[0] == 1.0 + 1.0 + 1.0 and d[1] == 1.0
    assert d[2] == (1.0 * -1.0) / (1.0 + 1.0 + 1.0)             # e = 1, -, 1, -1: the pair (2,3) only
    assert d[3] == 6.0 and d[4] == 1.0


def test_batched_curves_equal_single_ones():
    rs = np.random.RandomState(0)
    y = rs.poisson(2.0, size=(3, 4, 6, 2)).astype(float)
    y[rs.uniform(size=y.shape) < 0.3] = NAN
    mu, v = rs.uniform(0.5, 3.0, size=(3, 4, 6)), rs.uniform(0.5, 3.0, size=(3, 4, 6))
    v[1, 2, 3] = 0.0
    got = checks.discrepancies(y, mu, v)
    assert got.shape == (3, 4, 5)
    for a in range(3):
        for b in range(4):
            np.testing.assert_array_equal(got[a, b], checks.discrepancies(y[a, b], mu[a, b], v[a, b]))


# ---- the variance function, the two-sided p-value
def test_variance_function_closed_forms():
    eta = np.array([-3.0, -0.2, 0.0, 1.5, 40.0])
    np.testing.assert_array_equal(checks.variance_function("gaussian", eta, 0.3), np.full(5, 0.3))
    np.testing.assert_array_equal(checks.variance_function("poisson", eta), np.exp(eta))
    vi = checks.variance_function("poisson_identity", eta)
    assert np.isnan(vi[:3]).all() and vi[3] == 1.5 and vi[4] == 40.0
    p = 1.0 / (1.0 + np.exp(-eta))
    n = np.array([1.0, 7.0, 0.0, 20.0, 3.0])
    vb = checks.variance_function("binomial", eta, n)
    np.testing.assert_allclose(vb[:4], (n * p * (1 - p))[:4], rtol=1e-14)
    assert vb[2] == 0.0 and abs(vb[4] - 3.0 * np.exp(-40.0)) <= 1e-14 * vb[4]         # the far tail, where 1 - p rounds to 0
    np.testing.assert_allclose(checks.variance_function("binomial", eta)[:4], (p * (1 - p))[:4], rtol=1e-14)    # one trial
    r = 2.5
    q = 1.0 / (1.0 + np.exp(eta[:4]))                    # 1 - p: Var = r p / (1 - p)^2
    np.testing.assert_allclose(checks.variance_function("negbin", eta[:4], r), r * (1 - q) / q ** 2, rtol=1e-13)
    m = predictive.mean_function("negbin", eta[:4], r)
    np.testing.assert_allclose(checks.variance_function("negbin", eta[:4], r), m + m * m / r, rtol=1e-13)
    for fam in ("gaussian", "negbin"):
        with pytest.raises(ValueError):
            checks.variance_function(fam, eta)
    with pytest.raises(ValueError, match="unknown predictive family"):
        checks.variance_function("gamma_grid", eta)


def test_two_sided():
    assert checks.two_sided(0.5, 0.5) == 1.0
    assert checks.two_sided(0.01, 0.0) == 0.02                 # T far in the upper tail
    assert checks.two_sided(1.0, 0.99) == pytest.approx(0.02)  # far in the lower tail
    assert checks.two_sided(1.0, 0.0) == 1.0                   # every replicate ties
    got = checks.two_sided(np.array([0.3, NAN]), np.array([0.2, 0.5]))
    assert got[0] == 0.6 and np.isnan(got[1])


# ---- the argument checks
def test_check_which():
    assert checks.check_which(None, "poisson").tolist() == [0, 1, 2, 3, 4]
    assert checks.check_which(None, "gaussian").tolist() == [0, 1, 2, 3]
    assert checks.check_which("lag1", "gaussian").tolist() == [2]
    got = checks.check_which(("zeros", 0), "gaussian")
    assert got.tolist() == [4, 0] and got.dtype == np.int32
    with pytest.raises(ValueError, match="unknown discrepancy 'deviance'.*chisq, max, lag1, total, zeros"):
        checks.check_which(["chisq", "deviance"], "poisson")
    for bad in ([5], [-1], [1.5]):
        with pytest.raises(ValueError, match="unknown discrepancy"):
            checks.check_which(bad, "poisson")
    with pytest.raises(ValueError, match="'max' is repeated"):
        checks.check_which(["max", "chisq", 1], "poisson")
    with pytest.raises(ValueError, match="at least one"):
        checks.check_which([], "poisson")


def test_check_reps_curves_and_data():
    assert checks.check_reps(7, 3) == (7, 3)
    for bad in (0, -2, 1.5, None):
        with pytest.raises(ValueError, match="reps must be an integer >= 1"):
            checks.check_reps(7, bad)
    with pytest.raises(ValueError, match=r"exceeds 2\^31 - 1"):
        checks.check_reps(70000, 70000)
    shape = (5, 3, 4)
    assert checks.check_curves(None, shape) is None and checks.check_curves([], shape) is None
    assert checks.check_curves([(0, 0), (4, 2), (1, 1)], shape).tolist() == [0, 14, 4]
    assert checks.check_curves([14, 0, 14], shape).tolist() == [14, 0, 14]
    for bad in ([(5, 0)], [(0, 3)], [15], [-1], [0.5], [(0, 0, 0)]):
        with pytest.raises(ValueError, match="curves"):
            checks.check_curves(bad, shape)
    with pytest.raises(ValueError, match="pass data="):
        checks.check_data(None, shape)
    for bad in (np.zeros((5, 3)), np.zeros((5, 3, 5)), np.zeros((4, 3, 4, 2))):
        with pytest.raises(ValueError, match=r"does not match the model's \(5, 3, 4\)"):
            checks.check_data(bad, shape)
    assert checks.check_data(np.zeros(shape), shape).shape == shape + (1,)


# ---- a model with no device behind it: every refusal comes before any device call (the pattern of test_host_analysis.py)
class _NoDevice:
    def call(self, name, *args):
        raise AssertionError("device entry point %s called" % name)


N, M, T, K, S = 5, 3, 4, 2, 6
Y = np.zeros((N, M, T))


def _model_without_a_device(world=1, collected=None, cls=GaussianBayesianTensorFiltering):
    m = object.__new__(cls)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.device = N, M, T, K, 0
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    if collected is not None:
        m._collected = collected
    return m


def test_the_entry_point_is_declared():
    assert "btf_predict_check" in _native.SIGNATURES
    assert len(_native.UNITS) + _native.INST_PARTS == 32             # the kernel lives in the predictive unit: no new compilation
    header = open(_native.HEADERS[-1]).read()
    assert "int btf_predict_check(" in header


def test_nothing_collected_sharded_and_malformed_results():
    for collected in (None, 0):
        with pytest.raises(RuntimeError, match="no samples collected on the device"):
            _model_without_a_device(collected=collected).posterior_checks(data=Y)
    good = dict(W=np.zeros((S, N, K)), V=np.zeros((S, M, T, K)), nu2=np.ones((S, 1)))
    for collected in (0, S):
        with pytest.raises(NotImplementedError, match="unsharded"):
            _model_without_a_device(world=2, collected=collected).posterior_checks(data=Y)
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(world=2, collected=S).posterior_checks(good, data=Y)
    one = np.ones((S, 1))
    for bad in (dict(W=np.zeros((S, N, K + 1)), V=np.zeros((S, M, T, K + 1)), nu2=one),
                dict(W=np.zeros((S, N, K)), V=np.zeros((S - 1, M, T, K)), nu2=one), {},
                dict(W=np.zeros((S, N, K)), V=np.zeros((S, M, T, K)))):                    # (the last: no nu2)
        with pytest.raises(ValueError):
            _model_without_a_device(collected=S).posterior_checks(bad, data=Y)


def test_bad_arguments_are_refused_with_the_limit_named():
    m = lambda: _model_without_a_device(collected=S)
    with pytest.raises(ValueError, match="pass data="):
        m().posterior_checks()                                       # no data bound
    with pytest.raises(ValueError, match=r"data shape \(5, 3, 5\) does not match the model's \(5, 3, 4\)"):
        m().posterior_checks(data=np.zeros((N, M, T + 1)))
    with pytest.raises(ValueError, match=r"does not match the model's"):
        m().posterior_checks(data=(np.zeros((N, M)), np.ones((N, M))))
    for reps in (0, -1, 2.5):
        with pytest.raises(ValueError, match="reps must be an integer >= 1"):
            m().posterior_checks(data=Y, reps=reps)
    with pytest.raises(ValueError, match="unknown discrepancy 'rmse'"):
        m().posterior_checks(data=Y, which=["rmse"])
    with pytest.raises(ValueError, match="'chisq' is repeated"):
        m().posterior_checks(data=Y, which=["chisq", "chisq"])
    with pytest.raises(ValueError, match="curves"):
        m().posterior_checks(data=Y, curves=[(N, 0)])


def test_gamma_grid_and_callable_likelihoods_are_refused():
    for link, callback, name in ((5, False, "gamma_grid"), (0, True, "Python-callable")):
        m = _model_without_a_device(collected=S, cls=NonconjugateBayesianTensorFiltering)
        m._link, m._callback = link, callback
        with pytest.raises(NotImplementedError, match=name):
            m.posterior_checks(data=Y)


# ---- the statistical property of the GPU test, for the numpy reference alone
Z, PFLOOR = 5.5, 1e-6            # the thresholds of tests/test_gpu_predictive.py


def _randomised_rank(res, name, rs):
    """(count_gt + u (count_ge - count_gt + 1)) / (n + 1): uniform when T_obs is exchangeable with its n replicates."""
    d = res[name]
    n = d["defined"]
    gt, ge = d["p_gt"] * n, d["p_ge"] * n
    ok = n > 0
    u = rs.uniform(size=n.shape)
    return ((gt + u * (ge - gt + 1.0)) / (n + 1.0))[ok]


@pytest.mark.parametrize("fam", ["gaussian", "poisson"])
def test_well_specified_ranks_are_uniform_with_numpy_replicates(fam):
    Nw, Mw, Tw, n = 40, 30, 12, 199
    rs = np.random.RandomState(3 if fam == "gaussian" else 4)
    eta = 0.3 * np.cumsum(rs.normal(size=(Nw, Mw, Tw)), axis=2) + (1.0 if fam == "poisson" else 0.0)
    if fam == "gaussian":
        Mu, Var = eta[None], np.full((1, Nw, Mw, Tw), 0.5)
        draw = lambda size: Mu[0][..., None] + np.sqrt(0.5) * rs.normal(size=size)
    else:
        Mu = Var = np.exp(eta)[None]
        draw = lambda size: rs.poisson(np.broadcast_to(Mu[0][..., None], size)).astype(float)
    Yw = draw((Nw, Mw, Tw, 1))[..., 0]
    res = checks.reference(Yw, Mu, Var, draw((Nw, Mw, Tw, n)), reps=n, which=("chisq", "lag1"))
    assert res["nsets"] == n and res["chisq"]["p_ge"].shape == (Nw, Mw)
    for name in ("chisq", "lag1"):
        r = _randomised_rank(res, name, rs)
        assert r.size == Nw * Mw
        p = stats.kstest(r, "uniform").pvalue
        print(fam, name, "KS p", p)
        assert p > PFLOOR


def test_misspecified_fits_are_flagged_with_numpy_replicates():
    Nw, Mw, Tw, n = 40, 30, 12, 199
    rs = np.random.RandomState(5)
    eta = 0.3 * np.cumsum(rs.normal(size=(Nw, Mw, Tw)), axis=2) + 1.0
    lam = np.exp(eta)
    # Negative-Binomial data with r = 0.5 at the Poisson truth's mean, scored as Poisson
    Ynb = rs.poisson(rs.gamma(0.5, lam / 0.5)).astype(float)
    res = checks.reference(Ynb, lam[None], lam[None], rs.poisson(np.broadcast_to(lam[..., None], lam.shape + (n,))).astype(float),
                           reps=n, which=("chisq",))
    assert res["overall"]["chisq"]["p_ge"] < 0.01
    # Gaussian data with AR(1) noise, coefficient 0.8, scored as independent noise of the same marginal variance
    z = rs.normal(size=(Nw, Mw, Tw))
    for t in range(1, Tw):
        z[..., t] = 0.8 * z[..., t - 1] + np.sqrt(1 - 0.64) * z[..., t]
    Yar = eta + np.sqrt(0.5) * z
    res = checks.reference(Yar, eta[None], np.full((1,) + eta.shape, 0.5), eta[..., None] + np.sqrt(0.5) * rs.normal(size=eta.shape + (n,)),
                           reps=n, which=("lag1",))
    assert res["overall"]["lag1"]["p_ge"] < 0.01
