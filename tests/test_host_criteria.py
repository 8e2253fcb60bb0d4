"""Host halves of the model-selection criteria (functionalmf_amd/criteria.py) and the DIC grid search
(genlasso._BayesianModel.select_hyperparams_DIC): no GPU."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import expit, logsumexp

from functionalmf_amd import criteria
from functionalmf_amd.genlasso import _BayesianModel


def _per_curve(S1, cnt, c0, c1, family, Mu, par=None):
    """The kernel's formula (csrc/btf_criteria.h) on the statistics, in numpy: (N,M)."""
    s1, n = S1.transpose(2, 0, 1), cnt.transpose(2, 0, 1)           # [M][T][N] -> (N,M,T)
    with np.errstate(divide="ignore", invalid="ignore"):
        if family == criteria.FAMILY_POISSON_LOG:
            a = s1 * Mu - n * np.exp(Mu)
        elif family == criteria.FAMILY_POISSON_IDENTITY:
            a = s1 * np.log(Mu) - n * Mu
        elif family == criteria.FAMILY_LOGIT:
            a = s1 * Mu - n * np.logaddexp(0, Mu)
        elif family == criteria.FAMILY_GAUSSIAN:
            a = s1 * Mu - 0.5 * n * Mu * Mu
        else:
            a = s1 * Mu - (s1 + n * par) * np.logaddexp(0, Mu)
    a = np.where(n > 0, a, 0.0).sum(axis=2)
    if family == criteria.FAMILY_GAUSSIAN:
        return np.where(c1 > 0, (a - 0.5 * c0) / par - 0.5 * c1 * np.log(2 * np.pi * par), 0.0)
    return a + c0


def _data(rs, kind, shape=(7, 5, 6, 3)):
    N, M, T, R = shape
    Mu = rs.normal(0, 0.7, size=(N, M, T))
    if kind == "poisson_identity":
        Mu = np.abs(Mu) + 0.1
    if kind == "gaussian":
        Y = Mu[..., None] + rs.normal(0, 0.5, size=shape)
    elif kind == "bernoulli":
        Y = (rs.uniform(size=shape) < expit(Mu)[..., None]).astype(float)
    else:
        Y = rs.poisson(2.0, size=shape).astype(float)
    Y[rs.uniform(size=shape) < 0.25] = np.nan
    Y[0, 0] = np.nan                                               # one curve without observations
    return Mu, Y


@pytest.mark.parametrize("kind,family,par", [("poisson_log", 0, None), ("poisson_identity", 1, None), ("bernoulli", 2, None),
                                             ("gaussian", 3, 0.4), ("negbin", 4, 2.5)])
def test_statistics_reproduce_scipy_per_curve(kind, family, par):
    rs = np.random.RandomState(family)
    Mu, Y = _data(rs, kind)
    S1, cnt, c0, c1, obs = criteria.statistics(family, Y, Y.shape[:3], par)
    assert S1.shape == (5, 6, 7) and S1.flags.c_contiguous and c0.shape == (7, 5)
    mu = Mu[..., None]
    ld = {0: lambda: stats.poisson.logpmf(Y, np.exp(mu)), 1: lambda: stats.poisson.logpmf(Y, mu),
          2: lambda: stats.bernoulli.logpmf(Y, expit(mu)), 3: lambda: stats.norm.logpdf(Y, mu, np.sqrt(par)),
          4: lambda: stats.nbinom.logpmf(Y, par, 1 - expit(mu))}[family]()
    want = np.where(np.isnan(Y), 0.0, ld).sum(axis=(2, 3))
    got = _per_curve(S1, cnt, c0, c1, family, Mu, par)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert not obs[0, 0] and obs.sum() == 34


def test_binomial_statistics_reproduce_scipy():
    rs = np.random.RandomState(7)
    Mu = rs.normal(size=(6, 4, 5))
    Nt = rs.randint(0, 9, size=Mu.shape).astype(float)
    Y = rs.binomial(Nt.astype(int), expit(Mu)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    Nt[rs.uniform(size=Y.shape) < 0.1] = np.nan
    S1, cnt, c0, c1, obs = criteria.statistics(criteria.FAMILY_LOGIT, (Y, Nt), Y.shape)
    miss = np.isnan(Y) | np.isnan(Nt)
    want = np.where(miss, 0.0, stats.binom.logpmf(Y, Nt, expit(Mu))).sum(axis=2)
    np.testing.assert_allclose(_per_curve(S1, cnt, c0, c1, 2, Mu), want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        criteria.statistics(criteria.FAMILY_GAUSSIAN, (Y, Nt), Y.shape)


def _accumulators(L):
    """What the kernel hands back for an (S,N,M) matrix: online log-sum-exp, Welford - in ascending sample order."""
    S = L.shape[0]
    mx = np.full(L.shape[1:], -np.inf)
    se, mean, m2 = np.zeros_like(mx), np.zeros_like(mx), np.zeros_like(mx)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            x = L[s]
            up = x > mx
            se = np.where(up, se * np.exp(mx - x) + 1.0, np.where(x == -np.inf, se, se + np.exp(x - mx)))
            mx = np.where(up, x, mx)
            d = x - mean
            mean = mean + d / (s + 1)
            m2 = m2 + d * (x - mean)
    return se, mx, mean, m2


@pytest.mark.parametrize("S", [1, 2, 9, 50])
def test_combine_reproduces_waic_and_dic(S):
    rs = np.random.RandomState(S)
    N, M = 6, 5
    L = rs.normal(-40, 5, size=(S, N, M))
    L[:, 1, 2] += 3000 * rs.uniform(size=S)              # a spread of thousands of nats
    obs = np.ones((N, M), dtype=bool)
    obs[0, :2] = False
    L[:, ~obs] = 0.0
    Lm = rs.normal(-38, 5, size=(N, M))
    se, mx, mean, m2 = _accumulators(L)
    out = criteria.combine(np.stack([se, mx, mean, m2, Lm]), np.where(obs[None], L, 0).sum(axis=(1, 2)), obs, loglik=L)
    want = criteria.from_loglik(L, obs, Lm)
    for k in ("waic", "elpd_waic", "p_waic", "lppd", "waic_se", "dic", "p_dic", "mean_deviance", "deviance_at_mean"):
        np.testing.assert_allclose(out[k], want[k], rtol=1e-10, atol=1e-10, err_msg=k)
    assert out["n_curves"] == N * M - 2 and out["nsamples"] == S and out["loglik"] is L
    lp = np.where(obs, logsumexp(L, axis=0) - np.log(S), 0.0)
    np.testing.assert_allclose(out["curves"]["lppd"], lp, rtol=1e-12)
    if S > 1:
        np.testing.assert_allclose(out["curves"]["p_waic"], np.where(obs, np.var(L, axis=0, ddof=1), 0), rtol=1e-9)
    else:
        assert np.all(out["curves"]["p_waic"] == 0)
    assert np.all(out["curves"]["lppd"][~obs] == 0) and np.all(out["curves"]["ll_at_mean"][~obs] == 0)
    np.testing.assert_allclose(out["dic"], 2 * out["mean_deviance"] - out["deviance_at_mean"], rtol=1e-12)


def test_combine_minus_infinity_follows_numpy():
    rs = np.random.RandomState(1)
    L = rs.normal(-10, 1, size=(5, 2, 3))
    L[2, 0, 1] = -np.inf
    L[:, 1, 2] = -np.inf
    obs = np.ones((2, 3), dtype=bool)
    se, mx, mean, m2 = _accumulators(L)
    out = criteria.combine(np.stack([se, mx, mean, m2, np.zeros((2, 3))]), L.sum(axis=(1, 2)), obs)
    with np.errstate(invalid="ignore"):
        want_p = np.var(L, axis=0, ddof=1)
    lp = logsumexp(L, axis=0) - np.log(5)
    np.testing.assert_allclose(out["curves"]["lppd"][np.isfinite(lp)], lp[np.isfinite(lp)], rtol=1e-12)
    assert out["curves"]["lppd"][1, 2] == -np.inf
    assert np.isnan(out["curves"]["p_waic"][0, 1]) and np.isnan(want_p[0, 1])
    assert np.isnan(out["curves"]["p_waic"][1, 2]) and np.isnan(out["waic"])


def _shape_groups():
    import test_gpu_criteria_shapes as shapes
    return shapes, list(shapes.GROUPS)


@pytest.mark.parametrize("group", _shape_groups()[1])
def test_shape_cases_of_the_gpu_suite_meet_their_conditions(group):
    """Every builder of tests/test_gpu_criteria_shapes.py, without a device: `build` asserts that the scipy reference is
    finite everywhere except where a poisson_identity design puts w . v = 0 under an observed cell, that those cells are
    the only zeros of the linear predictor, and that the seeds differ."""
    shapes = _shape_groups()[0]
    specs = shapes.GROUPS[group]
    assert len({shapes._seed(s) for s in specs}) == len(specs)
    for spec in specs:
        model, results, L, Lm, obs = shapes.build(spec, bind=False)
        assert model is None and results["W"].shape == (spec[6], spec[1], spec[5])
    if group == "infinities":
        kinds = {s[8]: shapes.build(s, bind=False)[2] for s in specs}
        assert (kinds["cells"] == -np.inf).sum() == 3 and np.isfinite(kinds["cells-unobserved"]).all()
        assert (kinds["sample"] == -np.inf).sum() == 65


class _Stub(_BayesianModel):
    """Scripted criteria: the DIC of each grid point is read off a table keyed by lam2."""

    def __init__(self, table):
        super().__init__()
        self.table, self.lam2, self.calls = table, None, []

    def _set_hyperparameters(self, hyperparams):
        self.lam2 = hyperparams["lam2"]

    def run_gibbs(self, data, **kwargs):
        self.calls.append((self.lam2, dict(kwargs)))
        return {"W": np.full((2, 1, 1), self.lam2)}

    def information_criteria(self, results=None, data=None, pointwise=False):
        return {"dic": self.table[round(float(results["W"][0, 0, 0]), 12)]}


def test_select_hyperparams_DIC_strips_grid_keywords_and_picks_the_argmin():
    grid = [3.0, 0.5, 0.01]
    stub = _Stub({3.0: 10.0, 0.5: -4.0, 0.01: 2.0})
    out = stub.select_hyperparams_DIC("data", verbose=False, lam2=grid, nburn=7, nsamples=2)
    assert [c[0] for c in stub.calls] == grid
    assert all(c[1] == {"verbose": False, "nburn": 7, "nsamples": 2} for c in stub.calls)
    np.testing.assert_array_equal(out["scores"], [10.0, -4.0, 2.0])
    assert out["best"] == {"lam2": 0.5} and stub.lam2 == 0.5
    assert out["fit"]["W"][0, 0, 0] == 0.5
    np.testing.assert_array_equal(out["options"]["lam2"], grid)


def test_default_lam2_grid():
    opts = {}
    _Stub({})._default_hyperparam_options(opts)
    np.testing.assert_allclose(opts["lam2"], np.exp(np.linspace(np.log(1e-6), np.log(1e3), 10))[::-1])
    opts = {}
    _Stub({})._default_hyperparam_options(opts, min_lam2=0.1, max_lam2=10.0, num_lam2=3, nburn=5)
    np.testing.assert_allclose(opts["lam2"], [10.0, 1.0, 0.1])
    table = {round(float(v), 12): -float(i) for i, v in enumerate(np.exp(np.linspace(np.log(1e-6), np.log(1e3), 10))[::-1])}
    stub = _Stub(table)
    out = stub.select_hyperparams_DIC("data", verbose=False, min_lam2=1e-6)
    assert len(stub.calls) == 10 and all("min_lam2" not in c[1] for c in stub.calls)
    assert out["best"]["lam2"] == pytest.approx(1e-6)
