"""Model-selection criteria on the GPU (csrc/btf_criteria.h via BayesianTensorFiltering.information_criteria /
logprob): the per-curve log-likelihood against scipy's elementwise densities, WAIC / DIC against numpy, consistency
with the existing likelihood code, determinism, an undisturbed chain, held-out scoring, behaviour and full size."""
import ctypes

import numpy as np
import pytest
from scipy import stats
from scipy.special import expit, logsumexp

from functionalmf_amd import criteria
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering,
                                     NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering)

pytestmark = pytest.mark.gpu

LINKS = ["poisson_log", "poisson_identity", "bernoulli_logit", "gaussian", "negbin_logit"]


def _logdens(kind, Y4, Mu, par=None, nu2=None, Ntr=None):
    """scipy's elementwise log densities, (S,N,M,T,R) with NaN cells 0, summed per curve -> (S,N,M)."""
    mu = Mu[..., None]
    if kind == "gauss":
        ld = stats.norm.logpdf(Y4[None], mu, np.sqrt(nu2)[:, None, None, None, None])
    elif kind == "binom":
        ld = stats.binom.logpmf(Y4[None], Ntr[None, ..., None], expit(mu))
    elif kind == "poisson_log":
        ld = stats.poisson.logpmf(Y4[None], np.exp(mu))
    elif kind == "poisson_identity":
        ld = stats.poisson.logpmf(Y4[None], mu)
    elif kind == "bernoulli_logit":
        ld = stats.bernoulli.logpmf(Y4[None], expit(mu))
    elif kind == "gaussian":
        ld = stats.norm.logpdf(Y4[None], mu, np.sqrt(par))
    else:
        ld = stats.nbinom.logpmf(Y4[None], par, 1.0 - expit(mu))
    return np.where(np.isnan(Y4)[None], 0.0, ld).sum(axis=(3, 4))


def _case(kind, N, M, T, R, K, S, seed, form="complete", bind=True, prepare=None):
    """(model, data, results, per-curve reference matrix L, plug-in reference, observed mask).

    bind=False builds the inputs and the references only (no model, no device: `model` is None).  prepare(Ws, Vs, Y4)
    edits the states and the observations in place before the references are formed from them."""
    rs = np.random.RandomState(seed)
    positive = kind == "poisson_identity"
    Ws = rs.uniform(0.2, 1.0, size=(S, N, K)) if positive else rs.normal(0, 0.6, size=(S, N, K))
    Vs = rs.uniform(0.2, 1.0, size=(S, M, T, K)) if positive else rs.normal(0, 0.6, size=(S, M, T, K)) / np.sqrt(K)
    Mu = np.einsum("snk,smtk->snmt", Ws, Vs)
    Mu0 = Mu[0]
    np.random.seed(seed)
    par, nu2, Ntr, extra = None, None, None, {}
    tf_order = min(2, T - 2)                               # (2, the default, at every T >= 4)
    make = None
    if kind == "gauss":
        Y4 = Mu0[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
        nu2 = rs.uniform(0.2, 0.4, size=S)
        make = lambda: GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=tf_order)
        extra["nu2"] = nu2[:, None]
    elif kind == "binom":
        Ntr = rs.randint(1, 9, size=(N, M, T)).astype(float)
        Y4 = rs.binomial(Ntr.astype(int), expit(Mu0)).astype(float)[..., None]
        make = lambda: BinomialBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=tf_order)
    else:
        lam = np.exp(Mu0) if kind == "poisson_log" else np.maximum(Mu0, 1e-3)
        if kind in ("poisson_log", "poisson_identity"):
            Y4 = rs.poisson(lam[..., None] * np.ones(R)).astype(float)
        elif kind == "bernoulli_logit":
            Y4 = (rs.uniform(size=(N, M, T, R)) < expit(Mu0)[..., None]).astype(float)
        elif kind == "gaussian":
            par = 0.3
            Y4 = Mu0[..., None] + rs.normal(0, np.sqrt(par), size=(N, M, T, R))
        else:
            par = 3.0
            Y4 = rs.negative_binomial(par, 1.0 - expit(Mu0)[..., None] * np.ones(R)).astype(float)
        make = lambda: NonconjugateBayesianTensorFiltering(N, M, T, loglikelihood=kind, nembeds=K, likelihood_param=par,
                                                           tf_order=tf_order)
    if form == "missing":
        Y4[rs.uniform(size=Y4.shape) < 0.3] = np.nan
    elif form == "curve":
        Y4[:3, :3] = np.nan
    if prepare is not None:
        prepare(Ws, Vs, Y4)
        Mu = np.einsum("snk,smtk->snmt", Ws, Vs)
    if kind == "binom":
        Y4[rs.uniform(size=Y4.shape) < 0.2] = np.nan
        Yb = Y4[..., 0].copy()
        Nb = np.where(np.isnan(Yb), np.nan, Ntr)
        data = (Yb, Nb)
    else:
        data = Y4[..., 0].copy() if form == "3d" else Y4
    L = _logdens(kind, Y4, Mu, par=par, nu2=nu2, Ntr=Ntr)
    Lm = _logdens(kind, Y4, Mu.mean(axis=0)[None], par=par, nu2=None if nu2 is None else np.array([nu2.mean()]), Ntr=Ntr)[0]
    obs = ~np.all(np.isnan(Y4), axis=(2, 3))
    model = None
    if bind:
        np.random.seed(seed)
        model = make()
        model.set_data(data)
    results = dict(W=Ws, V=Vs, **extra)
    return model, data, results, L, Lm, obs


CASES = [
    ("gauss", 20, 5, 7, 2, 3, 7, "complete"),
    ("gauss", 33, 4, 9, 3, 1, 1, "missing"),
    ("gauss", 70, 6, 11, 2, 10, 64, "curve"),
    ("gauss", 33, 1, 9, 1, 2, 257, "3d"),
    ("binom", 40, 5, 13, 1, 4, 7, "complete"),
] + [(k, 50, 4, 17, 2, 5 + i, (1, 7, 64, 257, 7)[i], "missing" if i % 2 else "complete") for i, k in enumerate(LINKS)]


@pytest.mark.parametrize("kind,N,M,T,R,K,S,form", CASES)
def test_pointwise_matches_scipy_and_keys_match_numpy(kind, N, M, T, R, K, S, form):
    model, data, results, L, Lm, obs = _case(kind, N, M, T, R, K, S, seed=N + S, form=form)
    ic = model.information_criteria(results, pointwise=True)
    got = ic["loglik"]
    assert got.shape == (S, N, M)
    ref = np.where(obs[None], L, 0.0)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10 * np.abs(ref).max())
    np.testing.assert_allclose(ic["curves"]["ll_at_mean"], np.where(obs, Lm, 0.0), rtol=1e-10, atol=1e-10 * np.abs(Lm).max())
    want = criteria.from_loglik(L, obs, Lm)
    for k in ("waic", "elpd_waic", "p_waic", "lppd", "waic_se", "dic", "p_dic", "mean_deviance", "deviance_at_mean"):
        np.testing.assert_allclose(ic[k], want[k], rtol=1e-10, atol=1e-9, err_msg=k)
    assert ic["n_curves"] == int(obs.sum()) and ic["nsamples"] == S
    np.testing.assert_allclose(ic["loglik_per_sample"], want["loglik_per_sample"], rtol=1e-10)
    np.testing.assert_allclose(ic["curves"]["lppd"], want["curves"]["lppd"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(ic["curves"]["p_waic"], want["curves"]["p_waic"], rtol=1e-9, atol=1e-10)


def test_logsumexp_over_a_wide_spread():
    """Per-sample curve log-likelihoods more than 1000 nats apart (the variance spans 1e-4..1): the online log-sum-exp
    neither overflows nor underflows."""
    model, data, results, L, Lm, obs = _case("gauss", 30, 4, 20, 2, 3, 40, seed=5)
    results["nu2"] = np.geomspace(1e-4, 1.0, 40)[:, None]
    Y4 = data
    Mu = np.einsum("snk,smtk->snmt", results["W"], results["V"])
    L = _logdens("gauss", Y4, Mu, nu2=results["nu2"][:, 0])
    assert np.ptp(L, axis=0).max() > 1000
    ic = model.information_criteria(results)
    np.testing.assert_allclose(ic["curves"]["lppd"], logsumexp(L, axis=0) - np.log(40), rtol=1e-10)
    assert np.all(np.isfinite(ic["curves"]["lppd"]))


def test_logprob_matches_sse_and_log_likelihood():
    rs = np.random.RandomState(3)
    N, M, T, K = 24, 6, 10, 3
    Y = rs.normal(size=(N, M, T, 2))
    Y[:2, :2] = np.nan
    np.random.seed(3)
    g = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, nu2_init=0.7)
    g.set_data(Y)
    g._push_state()
    sse, nobs = ctypes.c_double(), ctypes.c_double()
    g._ctx.call("btf_sse", ctypes.byref(sse), ctypes.byref(nobs))
    want = -0.5 * nobs.value * np.log(2 * np.pi * 0.7) - sse.value / (2 * 0.7)
    assert abs(g.logprob(Y) - want) <= 1e-10 * abs(want)
    assert abs(g.logprob(Y, W=g.W, V=g.V, nu2=0.7, Tau2=g.Tau2, lam2=1.0, sigma2=2.0) - want) <= 1e-10 * abs(want)
    assert g.logprob(Y, reduce="curve").shape == (N, M)
    Yc = rs.poisson(2.0, size=(N, M, T)).astype(float)
    for link in ("poisson_log", "bernoulli_logit", "gaussian"):
        Yl = (Yc > 1).astype(float) if link == "bernoulli_logit" else Yc
        np.random.seed(4)
        nc = NonconjugateBayesianTensorFiltering(N, M, T, loglikelihood=link, nembeds=K, rng="device",
                                                 likelihood_param=0.5 if link == "gaussian" else None)
        nc.run_gibbs(Yl, nburn=2, nsamples=1, verbose=False)
        want = nc.log_likelihood(Yl)
        got = nc.logprob(Yl)
        assert abs(got - want) <= 1e-10 * abs(want), (link, got, want)


def _gauss_data(N=30, M=6, T=12, K=3, seed=0, noise=0.3):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = np.cumsum(rs.normal(0, 0.3, size=(M, T, K)), axis=1)
    return np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, noise, size=(N, M, T, 2))


def test_device_collected_equals_uploaded_bit_for_bit():
    Y = _gauss_data()
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=5)
    res = m.run_gibbs(Y, nburn=10, nsamples=20, verbose=False)
    a = m.information_criteria(pointwise=True)
    b = m.information_criteria(res, pointwise=True)
    c = m.information_criteria(pointwise=True)
    for x in (b, c):
        for k in ("waic", "dic", "lppd", "p_waic", "waic_se", "deviance_at_mean"):
            assert a[k] == x[k] or (np.isnan(a[k]) and np.isnan(x[k])), k
        for k in a["curves"]:
            assert np.array_equal(a["curves"][k], x["curves"][k]), k
        assert np.array_equal(a["loglik"], x["loglik"]) and np.array_equal(a["loglik_per_sample"], x["loglik_per_sample"])


@pytest.mark.parametrize("rng", ["device", "host"])
def test_chain_is_undisturbed(rng):
    Y = _gauss_data(seed=1)
    Y[:3, :3] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng=rng, device_seed=7))
    a, b = models
    for m in models:
        np.random.seed(12)
        m.run_gibbs(Y, nburn=4, nsamples=3, verbose=False)
    np.random.seed(13)
    res = a.run_gibbs(Y, nburn=1, nsamples=3, verbose=False)
    np.random.seed(13)
    b.run_gibbs(Y, nburn=1, nsamples=3, verbose=False)
    a.information_criteria(res)
    if rng == "device":
        a.information_criteria()
    a.logprob(Y)
    a.logprob(Y, reduce="curve")
    for m in models:
        np.random.seed(14)
        m.run_gibbs(Y, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_heldout_curves():
    Y = _gauss_data(seed=2)
    train = Y.copy()
    train[:3, :3] = np.nan
    held = np.full_like(Y, np.nan)
    held[:3, :3] = Y[:3, :3]
    np.random.seed(2)
    m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=2)
    res = m.run_gibbs(train, nburn=20, nsamples=16, verbose=False)
    ic = m.information_criteria(res, data=held, pointwise=True)
    Mu = np.einsum("snk,smtk->snmt", res["W"], res["V"])
    L = _logdens("gauss", held, Mu, nu2=res["nu2"][:, 0])
    obs = np.zeros((30, 6), dtype=bool)
    obs[:3, :3] = True
    assert ic["n_curves"] == 9
    np.testing.assert_allclose(ic["loglik"], np.where(obs[None], L, 0.0), rtol=1e-10, atol=1e-9)
    want = logsumexp(L[:, :3, :3], axis=0) - np.log(16)
    np.testing.assert_allclose(ic["curves"]["lppd"][:3, :3], want, rtol=1e-10)
    assert np.all(ic["curves"]["lppd"][~obs] == 0) and np.all(ic["curves"]["p_waic"][~obs] == 0)
    np.testing.assert_allclose(ic["lppd"], want.sum(), rtol=1e-10)
    # the bound (training) data is scored again from its own slot
    assert m.information_criteria(res)["n_curves"] == 30 * 6 - 9


def test_criteria_pick_the_true_rank():
    """K = 3 data with noise sd 0.1 against unit-scale factors: a rank-1 fit leaves the two other components in the
    residual, which multiplies the noise variance by ~100 over 30*6*12*2 = 4320 observations - a deviance gap of
    thousands.  A margin of 500 deviance units leaves room for Monte-Carlo noise in both fits."""
    Y = _gauss_data(noise=0.1, seed=4)
    ics = {}
    for K in (1, 3):
        np.random.seed(5)
        m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=K, rng="device", device_seed=3)
        m.run_gibbs(Y, nburn=300, nsamples=100, verbose=False)
        ics[K] = m.information_criteria()
    assert ics[3]["waic"] < ics[1]["waic"] - 500
    assert ics[3]["dic"] < ics[1]["dic"] - 500
    np.random.seed(6)
    m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=4)
    out = m.select_hyperparams_DIC(Y, verbose=False, lam2=[1.0, 0.1, 0.01], nburn=20, nsamples=10)
    assert out["scores"].shape == (3,) and np.all(np.isfinite(out["scores"]))
    best = int(np.argmin(out["scores"]))
    assert out["best"]["lam2"] == out["options"]["lam2"][best]
    assert out["fit"]["W"].shape == (10, 30, 3)
    assert m.lam2 == out["best"]["lam2"]


def test_full_size_c3():
    N, M, T, R, K, S = 512, 256, 64, 4, 5, 64
    rs = np.random.RandomState(0)
    W0 = rs.normal(size=(N, K))
    V0 = 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W0, V0)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=1)
    res = m.run_gibbs(Y, nburn=20, nsamples=S, verbose=False)
    ic = m.information_criteria()
    L = np.zeros((S, N, M))
    for s in range(S):                                   # numpy, one sample at a time
        mu = np.einsum("nk,mtk->nmt", res["W"][s], res["V"][s])
        nu2 = res["nu2"][s, 0]
        sse = ((Y - mu[..., None]) ** 2).sum(axis=(2, 3))
        L[s] = -0.5 * T * R * np.log(2 * np.pi * nu2) - sse / (2 * nu2)
    np.testing.assert_allclose(ic["curves"]["lppd"], logsumexp(L, axis=0) - np.log(S), rtol=1e-10)
    np.testing.assert_allclose(ic["curves"]["p_waic"], np.var(L, axis=0, ddof=1), rtol=1e-7, atol=1e-9)


def test_refusals():
    Y = _gauss_data()
    np.random.seed(0)
    g = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device")
    with pytest.raises(RuntimeError, match="no samples collected"):
        g.information_criteria(data=Y)
    S = 4
    good = dict(W=np.zeros((S, 30, 3)), V=np.zeros((S, 6, 12, 3)), nu2=np.ones((S, 1)))
    for bad in (dict(good, W=np.zeros((S, 30, 2))), dict(good, V=np.zeros((S + 1, 6, 12, 3))), dict(good, nu2=np.ones((2, 1))),
                {"V": good["V"]}):
        with pytest.raises(ValueError):
            g.information_criteria(bad, data=Y)
    counts = np.random.RandomState(0).poisson(3.0, size=(30, 6, 12)).astype(float)
    nb = NegativeBinomialBayesianTensorFiltering(30, 6, 12, nembeds=3)
    with pytest.raises(NotImplementedError):
        nb.information_criteria(dict(W=good["W"], V=good["V"]), data=counts)
    with pytest.raises(NotImplementedError):
        nb.logprob(counts)
    cb = NonconjugateBayesianTensorFiltering(30, 6, 12, loglikelihood=lambda W, V, d: 0.0, nembeds=3)
    with pytest.raises(NotImplementedError):
        cb.information_criteria(dict(W=good["W"], V=good["V"]), data=counts)
    with pytest.raises(NotImplementedError):
        cb.logprob(counts)
