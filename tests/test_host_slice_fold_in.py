"""Host halves of slice_fold_in_rows (functionalmf_amd/slice_fold_in.py): the numpy definition against direct formulas and
against a 2-D quadrature posterior, every refusal before the library is loaded, and the wiring of the new unit and symbols.
No GPU.  The problem builders and the quadrature are shared with tests/test_gpu_slice_fold_in.py."""
import functools
import os
import re
import types

import numpy as np
import pytest
from scipy.stats import gamma as gamma_dist
from scipy.stats import poisson

from functionalmf_amd import _native, utils
from functionalmf_amd import slice_fold_in as sf
from functionalmf_amd.factor import (ConstrainedNonconjugateBayesianTensorFiltering, NonconjugateBayesianTensorFiltering)
from functionalmf_amd.likelihoods import GammaGridLikelihood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = ["poisson_log", "poisson_identity", "bernoulli_logit", "gaussian", "negbin_logit", "gamma_grid"]

# Allowance on |mean - m| of the numpy chain against the quadrature posterior at QUAD_SWEEPS sweeps from the start of
# poisson2_problem: what the finite chain length leaves.  Seen with 65536 chains (numpy generator): |diff| = (0.00014,
# 0.00060) at 16 sweeps (standard errors there: 0.00074, 0.00175; at 8 sweeps the second coordinate is 0.034 off, at 32
# sweeps 0.0005 and 0.000004); the largest, doubled.
HOST_BIAS = 2 * 0.00060
QUAD_SWEEPS = 16


class _NoDevice:
    """Stands in for the native library and for a context: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def fit_constraints(T, at_most_one=False):
    """Positivity, (at most one,) monotone decreasing with slack 1e-2: the rows of doseresponse/fit.py:58-61."""
    C_zero = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(T - i - 2), [-1e-2]]) for i in range(T - 1)])
    C_one = np.concatenate([np.eye(T) * -1, np.full((T, 1), -1)], axis=1)
    return np.concatenate([C_zero, C_one, C_mono] if at_most_one else [C_zero, C_mono], axis=0)


def gamma_table(G, rs):
    lik = GammaGridLikelihood(np.linspace(0.6, 1.4, G), rs.gamma(2.0, 0.5, size=G), 0.03)
    return lik


def draw_rows(family, param, eta, nreps, rs):
    """Observations (R,M,T,nreps) of the family at the linear predictor eta (R,M,T)."""
    e = eta[..., None] * np.ones(nreps)
    if family in ("poisson", "poisson_log"):
        return rs.poisson(np.exp(e)).astype(float)
    if family == "poisson_identity":
        return rs.poisson(e).astype(float)
    if family == "bernoulli_logit":
        return (rs.uniform(size=e.shape) < 1 / (1 + np.exp(-e))).astype(float)
    if family == "gaussian":
        return e + np.sqrt(param) * rs.normal(size=e.shape)
    if family == "negbin_logit":
        return rs.negative_binomial(param, 1 - 1 / (1 + np.exp(-e))).astype(float)
    a, s, p = sf.check_param(family, param)
    g = rs.choice(a.size, size=eta.shape, p=p / p.sum())
    return rs.gamma(a[g][..., None], (s[g] * eta)[..., None], size=e.shape)


def halfplanes(family, stats, V, Constraints=None, U=None):
    """The truncation of a K = 2 row as half-planes (A (n,2), c (n,)): A w >= c.  The identity-link families keep
    w . v_jt >= 0 on every observed cell; then the curve constraints of every column and 0 <= w . u_f <= 1."""
    rows, rhs = [np.zeros((0, 2))], [np.zeros(0)]
    if sf.family_code(family) in (1, 5):
        obs = np.reshape(stats[1], -1) > 0
        rows.append(V.reshape(-1, 2)[obs])
        rhs.append(np.zeros(int(obs.sum())))
    if Constraints is not None:
        AV = np.einsum("ct,jtk->jck", Constraints[:, :-1], V).reshape(-1, 2)
        rows.append(AV)
        rhs.append(np.tile(Constraints[:, -1], V.shape[0]))
    if U is not None:
        rows += [U, -U]
        rhs += [np.zeros(len(U)), -np.ones(len(U))]
    return np.concatenate(rows), np.concatenate(rhs)


def quadrature_posterior(logdens, planes=None, half=6.0, centre=(0.0, 0.0), npts=257, inner=48, tol=1e-6, rounds=7):
    """Mean and covariance of the density exp(logdens(w0, w1)) (arrays in, array out) restricted to the half-planes
    A w >= c, around `centre`, refined (range and resolution) until both move by less than tol.  The truncation is the
    indicator of the half-planes, integrated exactly along w1: for every w0 of a trapezoid grid the feasible w1 form one
    interval (the set is convex), which a Gauss-Legendre rule covers (the integrand is smooth there: `inner` nodes, 16 more
    with every refinement) - a grid over the indicator itself converges with the first power of its step only."""
    A, c = planes if planes is not None else (np.zeros((0, 2)), np.zeros(0))

    def moments(half, npts, inner):
        w0 = centre[0] + np.linspace(-half, half, npts)
        lo = np.full(w0.shape, centre[1] - half)
        hi = np.full(w0.shape, centre[1] + half)
        with np.errstate(divide="ignore", invalid="ignore"):
            for (a0, a1), cc in zip(A, c):
                if a1 > 0:
                    lo = np.maximum(lo, (cc - a0 * w0) / a1)
                elif a1 < 0:
                    hi = np.minimum(hi, (cc - a0 * w0) / a1)
                else:
                    hi = np.where(a0 * w0 >= cc, hi, lo)
        ok = hi > lo
        x, wk = np.polynomial.legendre.leggauss(inner)
        w1 = lo[:, None] + (np.where(ok, hi - lo, 0.0))[:, None] * (x[None] + 1.0) / 2.0
        tw = np.ones(w0.shape)
        tw[0] = tw[-1] = 0.5
        wt = tw[:, None] * wk[None] * np.where(ok, hi - lo, 0.0)[:, None]
        W0 = np.broadcast_to(w0[:, None], w1.shape)
        ll = np.concatenate([logdens(W0[i:i + 256], w1[i:i + 256]) for i in range(0, len(w0), 256)])     # (bounded intermediates)
        ll = np.where(wt > 0, ll, -np.inf)
        p = np.exp(ll - ll.max()) * wt
        p /= p.sum()
        m = np.array([(p * W0).sum(), (p * w1).sum()])
        d0, d1 = W0 - m[0], w1 - m[1]
        C = np.array([[(p * d0 * d0).sum(), (p * d0 * d1).sum()], [(p * d0 * d1).sum(), (p * d1 * d1).sum()]])
        return m, C
    m, C = moments(half, npts, inner)
    for _ in range(rounds):
        half, npts, inner = half * 1.25, npts * 2 - 1, inner + 16
        m2, C2 = moments(half, npts, inner)
        moved = max(np.abs(m2 - m).max(), np.abs(C2 - C).max())
        m, C = m2, C2
        if moved < tol:
            return m, C
    raise AssertionError("quadrature did not converge: last move %g" % moved)


def grid_logdens(family, param, stats, V, sigma2, U=None, x_codes=None):
    """log of prior x likelihood (x feature term) of a K = 2 row, vectorised over arrays of (w0, w1) inside the truncation
    (halfplanes); outside it the value is not used."""
    S1, cnt, L = (None if a is None else np.reshape(a, -1) for a in stats)
    Vf = V.reshape(-1, 2)
    code = sf.family_code(family)
    obs = cnt > 0

    def logdens(w0, w1):
        out = -(w0 ** 2 + w1 ** 2) / (2 * sigma2)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if obs.any():
                e = w0[..., None] * Vf[obs, 0] + w1[..., None] * Vf[obs, 1]
                if code == 1:
                    out = out + (S1[obs] * np.log(np.where(e > 0, e, 1.0)) - cnt[obs] * e).sum(axis=-1)
                elif code == 2:
                    out = out + (S1[obs] * e - cnt[obs] * np.logaddexp(0.0, e)).sum(axis=-1)
                elif code == 5:
                    from scipy.special import gammaln, logsumexp
                    a, sc, p = param
                    e = np.where(e > 0, e, 1.0)
                    comp = np.log(p) + a * (L[obs] - cnt[obs] * np.log(e))[..., None] - (S1[obs] / e)[..., None] / sc \
                        - cnt[obs][:, None] * (a * np.log(sc) + gammaln(a))
                    out = out + logsumexp(comp, axis=-1).sum(axis=-1)
                else:
                    raise NotImplementedError(family)
            if U is not None:
                pf = w0[..., None] * U[:, 0] + w1[..., None] * U[:, 1]
                x = np.asarray(x_codes, dtype=float)
                out = out + (np.where(x == 1, np.log(np.clip(pf, 1e-300, None)), 0.0)
                             + np.where(x == 0, np.log(np.clip(1.0 - pf, 1e-300, None)), 0.0)).sum(axis=-1)
        return out
    return logdens


def moments_check(W, m, C, bias=0.0):
    """The 5-standard-error inequalities: |mean_k - m_k| <= 5 sqrt(C_kk / S) (+ bias, an allowance on the mean alone) and the
    covariance entries within 5 sqrt((C_ab^2 + C_aa C_bb) / S) (Wishart).  Returns the largest ratios (mean, covariance)
    in units of those 5-standard-error bounds' standard errors."""
    S = W.shape[0]
    d = np.abs(W.mean(axis=0) - m)
    se = np.sqrt(np.diag(C) / S)
    Chat = np.cov(W.T, ddof=1).reshape(C.shape)
    sec = np.sqrt((C ** 2 + np.outer(np.diag(C), np.diag(C))) / S)
    return float(np.max((d - bias) / se)), float(np.max(np.abs(Chat - C) / sec))


@functools.lru_cache(maxsize=None)
def poisson2_problem():
    """K = 2, Poisson identity link under positivity and monotone constraints, 40 observed cells (M = 4, T = 10): a curve
    factor that falls along the depth axis and one that rises, so that the monotone rows cut the posterior of w.  Returns a
    dict with the quadrature posterior (m, C) beside the inputs; nothing writes to it."""
    rs = np.random.RandomState(21)
    M, T, K = 4, 10, 2
    fall = np.linspace(1.0, 0.3, T)
    V = np.zeros((M, T, K))
    V[:, :, 0] = rs.uniform(2.0, 4.0, size=(M, 1)) * fall
    V[:, :, 1] = rs.uniform(0.5, 1.5, size=(M, 1)) * fall[::-1]
    sigma2 = 1.5
    w_true = np.array([1.0, 0.45])
    Cons = fit_constraints(T)
    assert sf.feasible(w_true, V, Cons)
    Y = rs.poisson(np.einsum("k,mtk->mt", w_true, V)).astype(float)[None]
    R, S1, cnt, L = sf.row_statistics(Y, "poisson_identity", M, T)
    stats = (S1[0], cnt[0], None)
    start = np.array([0.6, 0.1])
    assert sf.feasible(start, V, Cons)
    m, C = quadrature_posterior(grid_logdens("poisson_identity", None, stats, V, sigma2),
                                halfplanes("poisson_identity", stats, V, Cons), half=3.0, centre=tuple(w_true))
    out = dict(V=V, sigma2=sigma2, Cons=Cons, Y=Y, stats=stats, start=start, m=m, C=C)
    for a in (V, Cons, Y, start, m, C):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_loglik_against_direct_formulas(family):
    """1. loglik differences between two states against scipy's logpmf / logpdf sums (the state-independent terms cancel);
    the gamma grid against GammaGridLikelihood.logpdf itself.  Missing cells, missing replicates and an empty row."""
    rs = np.random.RandomState(FAMILY_NAMES.index(family))
    M, T, K, nreps = 3, 5, 3, 2
    V = rs.uniform(0.2, 1.0, size=(M, T, K))
    wa, wb = rs.uniform(0.2, 0.8, size=K), rs.uniform(0.2, 0.8, size=K)
    lik = gamma_table(6, rs)
    param = {"gaussian": 0.7, "negbin_logit": 3.5, "gamma_grid": lik}.get(family)
    eta = np.einsum("k,mtk->mt", wa, V)[None]
    Y = draw_rows(family, param, np.repeat(eta, 2, axis=0), nreps, rs)
    Y[0][rs.uniform(size=Y[0].shape) < 0.3] = np.nan           # missing replicates ...
    Y[0, 1, 2] = np.nan                                        # ... a missing cell ...
    Y[1] = np.nan                                              # ... and an empty row
    R, S1, cnt, L = sf.row_statistics(Y, family, M, T)
    assert R == 2 and cnt[1].sum() == 0 and cnt[0, 1, 2] == 0 and S1[0, 1, 2] == 0
    np.testing.assert_array_equal(cnt[0], (~np.isnan(Y[0])).sum(axis=-1))
    p = sf.check_param(family, param)

    def direct(w, r):
        e = np.einsum("k,mtk->mt", w, V)[..., None]
        y = Y[r]
        with np.errstate(invalid="ignore"):
            if family == "poisson_log":
                v = poisson.logpmf(y, np.exp(e))
            elif family == "poisson_identity":
                v = poisson.logpmf(y, e)
            elif family == "bernoulli_logit":
                v = y * e - np.logaddexp(0.0, e)
            elif family == "gaussian":
                v = -0.5 * (y - e) ** 2 / param
            elif family == "negbin_logit":
                from scipy.stats import nbinom
                v = nbinom.logpmf(y, param, 1 - 1 / (1 + np.exp(-e)))
            else:
                return float(lik.logpdf(y, e).sum())
        return float(np.nansum(v))
    for r in range(2):
        st = (S1[r], cnt[r], None if L is None else L[r])
        got = sf.loglik(family, p, st, V, wa) - sf.loglik(family, p, st, V, wb)
        want = direct(wa, r) - direct(wb, r)
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (family, r, got, want)
    if family == "gamma_grid":                                 # the complete value, and a scipy mixture for one cell
        st = (S1[0], cnt[0], L[0])
        assert abs(sf.loglik(family, p, st, V, wa) - direct(wa, 0)) <= 1e-10 * abs(direct(wa, 0))
        y = Y[0, 0, 0][~np.isnan(Y[0, 0, 0])]
        if y.size:
            e = float(np.dot(wa, V[0, 0]))
            mix = np.log(np.sum(p[2] * np.prod(gamma_dist.pdf(y[:, None], p[0][None], scale=p[1][None] * e), axis=0)))
            one = (np.where(np.arange(M * T) == 0, S1[0].reshape(-1), 0), np.where(np.arange(M * T) == 0, cnt[0].reshape(-1), 0),
                   np.where(np.arange(M * T) == 0, L[0].reshape(-1), 0))
            assert abs(sf.loglik(family, p, one, V, wa) - (mix + (M * T - 1) * np.log(p[2].sum()))) < 1e-10
    if family in ("poisson_identity", "gamma_grid"):           # eta <= 0 on an observed cell
        assert sf.loglik(family, p, (S1[0], cnt[0], None if L is None else L[0]), V, -wa) == -np.inf
    assert sf.loglik(family, p, (S1[1], cnt[1], None if L is None else L[1]), V, wa) == \
        (M * T * np.log(p[2].sum()) if family == "gamma_grid" else 0.0)


def test_feasible_and_feature_term():
    rs = np.random.RandomState(3)
    M, T, K = 2, 4, 2
    V = np.stack([np.linspace(1.0, 0.4, T)[None] * np.ones((M, 1)), np.linspace(0.2, 0.8, T)[None] * np.ones((M, 1))], axis=-1)
    Cons = fit_constraints(T)
    assert sf.feasible([1.0, 0.1], V, Cons) and not sf.feasible([0.1, 1.0], V, Cons) and not sf.feasible([-1.0, 0.0], V, Cons)
    assert not sf.feasible([np.nan, 0.0], V, Cons) and sf.feasible([5.0, -7.0], V)
    Rc = np.array([[1.0, 0.0, 0.5]])                            # w_0 >= 0.5
    assert sf.feasible([0.5, 0.0], V, None, Rc) and not sf.feasible([0.49, 0.0], V, None, Rc)
    U = np.array([[0.5, 0.5], [1.0, 0.0]])
    assert sf.feasible([0.5, 0.5], V, None, None, U) and not sf.feasible([1.5, 0.0], V, None, None, U)
    w = np.array([0.4, 0.2])
    got = sf.feature_term(w, U, [1, 0])
    assert abs(got - (np.log(0.3) + np.log(0.6))) < 1e-14
    assert sf.feature_term(w, U, [np.nan, 2]) == 0.0 and sf.feature_term(w, U, sf.feature_codes([[np.nan, 1]])[0]) == np.log(0.4)
    s = sf.slacks(w, V, Cons, Rc, U)
    assert s.size == M * Cons.shape[0] + 1 + 4


def test_chain_against_quadrature_posterior():
    """2. 1024 independent chains of the definition with numpy's generator against the 2-D quadrature posterior: mean and
    covariance within 5 standard errors (+ HOST_BIAS on the mean); an unconstrained empty row has the prior's moments."""
    c = poisson2_problem()
    rng = np.random.default_rng(7)
    n = 1024
    W = np.zeros((n, 2))
    unf = 0
    for i in range(n):
        o = sf.chain(c["start"], c["V"], c["sigma2"], "poisson_identity", None, c["stats"], Constraints=c["Cons"], rng=rng,
                     sweeps=QUAD_SWEEPS)
        assert not o["failed"] and sf.feasible(o["w"], c["V"], c["Cons"])
        W[i], unf = o["w"], unf + o["unfinished"]
    zm, zc = moments_check(W, c["m"], c["C"], bias=HOST_BIAS)
    print("host chain vs quadrature: mean %s (quadrature %s)  z_mean %.2f  z_cov %.2f  unfinished %d" % (W.mean(axis=0), c["m"], zm, zc, unf))
    assert zm < 5 and zc < 5
    # an empty row without constraints: the prior N(0, sigma2 I), whatever the family
    # (started from a draw of the prior: the chain leaves it invariant)
    W0 = np.array([sf.chain(np.sqrt(1.7) * rng.standard_normal(2), c["V"], 1.7, "gaussian", 0.5, None, rng=rng, sweeps=2)["w"]
                   for _ in range(n)])
    zm, zc = moments_check(W0, np.zeros(2), 1.7 * np.eye(2))
    assert zm < 5 and zc < 5


def test_chain_replays_its_draws_and_reports_margins():
    c = poisson2_problem()
    rs = np.random.RandomState(4)
    rec = sf.record_length(2, 12)
    d = np.concatenate([rs.normal(size=(5, 2)), rs.uniform(size=(5, rec - 2))], axis=1)
    a = sf.chain(c["start"], c["V"], c["sigma2"], "poisson_identity", None, c["stats"], Constraints=c["Cons"], draws=d, sweeps=5,
                 max_rounds=12)
    b = sf.chain(c["start"], c["V"], c["sigma2"], "poisson_identity", None, c["stats"], Constraints=c["Cons"], draws=d.copy(),
                 sweeps=5, max_rounds=12)
    assert np.array_equal(a["w"], b["w"]) and a["rounds"] == b["rounds"] and 0 < a["margin_ll"] < np.inf and 0 < a["margin_slack"] < np.inf
    bad = sf.chain([-1.0, 0.0], c["V"], c["sigma2"], "poisson_identity", None, c["stats"], Constraints=c["Cons"], draws=d, sweeps=5,
                   max_rounds=12)
    assert bad["failed"] and np.all(np.isnan(bad["w"])) and bad["rounds"] == 0
    one = sf.chain(c["start"], c["V"], c["sigma2"], "poisson_identity", None, c["stats"], Constraints=c["Cons"], draws=d[:, :4],
                   sweeps=5, max_rounds=1)
    assert one["unfinished"] + one["rounds"] >= 1 and one["unfinished"] <= 5


def _bare(cls, M=3, T=4, K=2, world=1, collected=0, family="poisson_identity", features=0):
    m = object.__new__(cls)
    m.nrows, m.ncols, m.ndepth, m.nembeds = 5, M, T, K
    m._plan = types.SimpleNamespace(world=world)
    m._exchange = types.SimpleNamespace(active=False)
    m._ctx = _NoDevice()
    m._collected = collected
    m._draws, m._device_seed = 0, 1
    m._callback = callable(family)
    m.loglikelihood = family
    m._link = -1 if m._callback else NonconjugateBayesianTensorFiltering.LINKS[family]
    m.likelihood_param = None
    if cls is ConstrainedNonconjugateBayesianTensorFiltering:
        m._cons = fit_constraints(T)
        m.Row_constraints = None
        m.nfeatures = features
        m._X_codes = np.zeros((5, features), dtype=np.uint8) if features else None
    return m


def test_model_refusals_raise_before_any_device_call(no_device):
    """3. Bad shapes, draws of the wrong record length, a callable likelihood, a sharded model, nothing collected, missing U
    with features - each before any device call, and without taking a seed."""
    Y = np.ones((2, 3, 4))
    res = {"W": np.ones((6, 5, 2)), "V": np.ones((6, 3, 4, 2)), "sigma2": np.ones((6, 1))}
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        g = _bare(cls)
        with pytest.raises(NotImplementedError):
            _bare(cls, world=2).slice_fold_in_rows(Y, results=res)
        with pytest.raises(NotImplementedError):
            _bare(cls, family=lambda W, V, d: 0.0).slice_fold_in_rows(Y, results=res)
        with pytest.raises(RuntimeError):
            g.slice_fold_in_rows(Y)                            # nothing collected, no results
        for bad_Y in (np.ones((2, 3, 5)), np.ones((3, 4)), np.ones((2, 4, 4, 1)), (Y, Y), np.full((2, 3, 4), np.inf), None):
            with pytest.raises(ValueError):
                g.slice_fold_in_rows(bad_Y, results=res)
        for key, val in (("V", np.ones((6, 3, 4, 3))), ("V", np.ones((3, 4, 2))), ("W", np.ones((6, 5, 3))), ("sigma2", np.ones(5)),
                         ("sigma2", np.array([1, 1, -1, 1, 1, 1.0])), ("sigma2", np.array([1, 1, np.inf, 1, 1, 1.0]))):
            with pytest.raises(ValueError):
                g.slice_fold_in_rows(Y, results=dict(res, **{key: val}))
        with pytest.raises(ValueError):
            g.slice_fold_in_rows(Y, results={"V": res["V"], "sigma2": res["sigma2"]})     # no W and no start
        with pytest.raises(ValueError):
            g.slice_fold_in_rows(Y, results=res, start=np.zeros(3))
        with pytest.raises(ValueError):
            g.slice_fold_in_rows(Y, results=res, start=np.full(2, np.nan))
        with pytest.raises(ValueError):                        # the record of 40 rounds is K + 41 long
            g.slice_fold_in_rows(Y, results=res, sweeps=3, draws=np.full((6, 2, 3, 2 + 40), 0.5))
        with pytest.raises(ValueError):
            g.slice_fold_in_rows(Y, results=res, sweeps=3, draws=np.full((6, 2, 3, 2 + 41), 1.5))     # uniforms outside (0, 1)
        for kw in (dict(sweeps=0), dict(max_rounds=0), dict(transform="log"), dict(q=(5, 101)), dict(sweeps=2.5)):
            with pytest.raises(ValueError):
                g.slice_fold_in_rows(Y, results=res, **kw)
        with pytest.raises(ValueError):
            g.slice_fold_in_rows(Y, results=res, row_features=np.zeros((2, 3)))           # a model without features
        assert g._draws == 0                                   # a refused call takes no seed
    f = _bare(ConstrainedNonconjugateBayesianTensorFiltering, features=3)
    X = np.array([[0, 1, np.nan], [1, 1, 0.0]])
    with pytest.raises(ValueError, match="U"):
        f.slice_fold_in_rows(Y, results=res, row_features=X)                              # features without results["U"]
    with pytest.raises(ValueError):
        f.slice_fold_in_rows(Y, results=dict(res, U=np.ones((6, 2, 2))), row_features=X)
    with pytest.raises(ValueError):
        f.slice_fold_in_rows(Y, results=dict(res, U=np.ones((6, 3, 2))), row_features=np.full((2, 3), 0.5))
    with pytest.raises(ValueError):
        f.slice_fold_in_rows(Y, results=dict(res, U=np.ones((6, 3, 2))), row_features=X[:1])     # one row of features, two of Y
    with pytest.raises(ValueError):
        f.slice_fold_in_rows(None, results=res)                                            # neither curves nor features
    gg = _bare(NonconjugateBayesianTensorFiltering, family="gamma_grid")
    gg._gg_table = sf.check_param("gamma_grid", gamma_table(4, np.random.RandomState(0)))
    with pytest.raises(ValueError, match="y > 0"):
        gg.slice_fold_in_rows(np.zeros((2, 3, 4)), results=res)
    big = {"W": np.ones((sf.MAX_SUMMARY_SAMPLES + 1, 1, 1)), "V": np.ones((sf.MAX_SUMMARY_SAMPLES + 1, 1, 2, 1)),
           "sigma2": np.ones(sf.MAX_SUMMARY_SAMPLES + 1)}
    with pytest.raises(ValueError):
        _bare(NonconjugateBayesianTensorFiltering, M=1, T=2, K=1).slice_fold_in_rows(np.ones((1, 1, 2)), results=big)
    assert f._draws == 0 and gg._draws == 0


def test_stateless_refusals_raise_before_any_device_call(no_device):
    V = np.ones((6, 3, 4, 2))
    W = np.ones((6, 5, 2))
    Y = np.ones((2, 3, 4))
    one = np.ones(6)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "binomial", sigma2=one, Ws=W)
    with pytest.raises(NotImplementedError):
        utils.slice_fold_in_rows(Y, V, lambda W, V, d: 0.0, sigma2=one, Ws=W)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V[0], "poisson", sigma2=one, Ws=W)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", Ws=W)                                   # no sigma2
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=-one, Ws=W)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one)                             # neither Ws nor start
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y[:, :2], V, "poisson", sigma2=one, Ws=W)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one, Ws=W, first_sample=-1)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one, Ws=W, first_sample=2 ** 31 // 2)
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "gaussian", sigma2=one, Ws=W)                      # no variance
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "gamma_grid", sigma2=one, Ws=W, likelihood_param=(np.ones(200), np.ones(200), 0.1))   # G > 128
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, np.ones((6, 3, 4, 11)), "poisson", sigma2=one, start=np.zeros(11))
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one, Ws=W, Constraints=np.ones((3, 4)))
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one, Ws=W, Row_constraints=np.ones((3, 2)))
    with pytest.raises(ValueError):
        utils.slice_fold_in_rows(Y, V, "poisson", sigma2=one, Ws=W, row_features=np.zeros((2, 3)))     # features without Us


def test_the_unit_and_the_symbols_are_wired():
    assert os.path.join(_native.CSRC, "btf_slice_fold.hip") in _native.SOURCES
    assert os.path.exists(os.path.join(_native.CSRC, "btf_slice_fold.h"))
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    analysis = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    for name in ("btf_slice_fold_rows", "btf_collect_slice_fold"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _native.SIGNATURES
        assert re.search(r"^int\s+%s\s*\(" % name, analysis, flags=re.M), name + " is defined beside the analysis entry points"
    assert len(_native.SIGNATURES["btf_fold_in_rows"][1]) == 24 and len(_native.SIGNATURES["btf_collect_fold_in"][1]) == 18
    assert sf.DEFAULT_SWEEPS in (4, 8, 16, 32, 64) and sf.DEFAULT_MAX_ROUNDS == 40


def test_fold_in_rows_still_refuses_these_models(no_device):
    Y = np.zeros((2, 3, 4))
    res = {"V": np.ones((6, 3, 4, 2)), "sigma2": np.ones((6, 1)), "nu2": np.ones((6, 1))}
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        with pytest.raises(NotImplementedError, match="slice_fold_in_rows"):
            _bare(cls).fold_in_rows(Y, results=res)
