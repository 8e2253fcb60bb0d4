"""Posterior predictive on the GPU (csrc/btf_predict.h via BayesianTensorFiltering.posterior_predictive,
utils.posterior_predictive and predictive.batch): deterministic outputs against numpy, determinism and geometry
independence of the draws, error paths, and the distribution of the device samplers against scipy.

Statistical thresholds are derived, not tuned: a z-score of 5.5 (two-sided 4e-8) per moment check and a p-value floor of
1e-6 per goodness-of-fit check keep the false-failure rate of the file below 1e-4 at the few hundred checks it holds;
the seeds are fixed, so a run is repeatable."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import expit

from functionalmf_amd import _native, predictive, utils
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering,
                                     NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering)

pytestmark = pytest.mark.gpu

Z = 5.5
PFLOOR = 1e-6
NB = 200000
FAMS = ["poisson", "poisson_identity", "binomial", "gaussian", "negbin"]


def _states(rs, S, N, M, T, K, positive=False, scale=0.6):
    if positive:
        return rs.uniform(0.3, 1.2, size=(S, N, K)), rs.uniform(0.3, 1.2, size=(S, M, T, K))
    return rs.normal(0, scale, size=(S, N, K)), rs.normal(0, scale, size=(S, M, T, K))


def _eta(Ws, Vs):
    return np.einsum("znk,zmtk->znmt", Ws, Vs)


def _family_args(fam, rs, S, shape):
    """keyword arguments of utils.posterior_predictive and the aux (S,N,M,T)-broadcastable array of the mean function"""
    if fam == "gaussian":
        nu2 = rs.uniform(0.2, 0.6, size=S)
        return dict(nu2=nu2), nu2[:, None, None, None]
    if fam == "negbin":
        R = rs.uniform(0.5, 4.0, size=(S,) + (shape[0], 1, shape[2]))
        return dict(R=R), R
    if fam == "binomial":
        tr = rs.randint(0, 40, size=shape).astype(float)
        return dict(trials=tr), tr[None]
    return {}, None


# ---------------------------------------------------------------- 1. the deterministic mean, uploaded and collected
@pytest.fixture(scope="module")
def collected():
    N, M, T, K, S = 7, 5, 9, 3, 12
    rs = np.random.RandomState(0)
    Y = rs.normal(size=(N, M, T, 2))
    Y[:2, :2] = np.nan
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=5)
    res = model.run_gibbs(Y, nburn=3, nthin=1, nsamples=S, verbose=False)
    assert model._collected == S
    return model, Y, res


@pytest.mark.parametrize("fam", FAMS)
def test_mean_uploaded_and_collected(collected, fam):
    model, Y, res = collected
    S, shape, K = res["W"].shape[0], (model.nrows, model.ncols, model.ndepth), model.nembeds
    rs = np.random.RandomState(2)
    code = predictive.family_code(fam)
    kw = dict(param=0.7 if fam in ("gaussian", "negbin") else None,
              trials=rs.randint(1, 9, size=shape).astype(float) if fam == "binomial" else None)
    up = predictive.evaluate(model._ctx, shape, K, code, S, res["W"], res["V"], Y=Y, seed=11, cells=[0, 17], **kw)
    co = predictive.evaluate(model._ctx, shape, K, code, S, None, None, Y=Y, seed=11, cells=[0, 17], **kw)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(up[k], co[k], err_msg=k)                 # bit for bit, nan == nan
    aux = kw["trials"] if fam == "binomial" else kw["param"]
    with np.errstate(invalid="ignore"):
        ref = predictive.mean_function(code, _eta(res["W"], res["V"]), aux).mean(axis=0)
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(up["mean"]), ~ok)
    if fam == "poisson_identity":                # signed samples: a cell with w.v <= 0 in any sample has no mean (nan)
        assert not ok.all()
        if not ok.any():
            return
    err = np.abs(up["mean"] - ref)[ok].max()
    print("mean", fam, "max abs err", err, "max", np.abs(ref[ok]).max())
    assert err <= 1e-12 * np.abs(ref[ok]).max()


def test_model_method_collected_gaussian(collected):
    model, Y, res = collected
    a = model.posterior_predictive(seed=3, cells=[5])
    b = model.posterior_predictive(results=res, seed=3, cells=[5])
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    eta = _eta(res["W"], res["V"])
    assert np.abs(a["mean"] - eta.mean(0)).max() <= 1e-12 * np.abs(eta).max()
    # the draws of cell 5: eta_s + sqrt(nu2_s) z
    z = (a["draws"][0] - eta.reshape(len(eta), -1)[:, 5]) / np.sqrt(res["nu2"][:, 0])
    assert np.all(np.isfinite(z)) and np.abs(z).max() < 6
    assert a["nsamples"] == len(eta) and a["ndraws"] == len(eta) and abs(a["nominal"] - 0.95) < 1e-15
    d0 = model._draws
    model.posterior_predictive()                      # seed=None: the model's next device seed
    assert model._draws == d0 + 1


# ---------------------------------------------------------------- 2. + 3. reductions against numpy
def _patterns(Y, pattern, rs):
    Y = Y.copy()
    if pattern == "heldout":
        Y[:, :, -3:] = np.nan
    elif pattern == "replicates":
        Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    elif pattern == "empty_cell":
        Y[1, 2, 3] = np.nan
        Y[0, 0, 0, 0] = np.nan
    return Y


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("pattern", ["complete", "heldout", "replicates", "empty_cell"])
def test_reductions_against_numpy(fam, pattern):
    N, M, T, K, S, R, Rrep = 5, 4, 7, 3, 37, 3, 3
    shape = (N, M, T)
    rs = np.random.RandomState(FAMS.index(fam) * 10 + len(pattern))
    Ws, Vs = _states(rs, S, N, M, T, K, positive=fam == "poisson_identity")
    kw, aux = _family_args(fam, rs, S, shape)
    if fam == "binomial":
        kw["trials"][2, 1, 4] = np.nan                 # a missing trial count: nan in every draw-based output
    code = predictive.family_code(fam)
    eta = _eta(Ws, Vs)
    with np.errstate(invalid="ignore"):
        Mu = predictive.mean_function(code, eta, aux)              # (S,N,M,T)
    Y = Mu[0][..., None] + rs.normal(size=shape + (Rrep,))
    if fam != "gaussian":
        Y = np.round(np.abs(np.nan_to_num(Y)))
    Y = _patterns(Y, pattern, rs)
    q = (2.5, 30.0, 97.5)
    cells = np.arange(N * M * T, dtype=np.int32)[::-1]
    out = utils.posterior_predictive(Ws, Vs, fam, data=Y, q=q, draws_per_sample=R, seed=21, cells=cells, **kw)
    n = S * R
    d = out["draws"][np.argsort(cells)].reshape(shape + (n,))          # (N,M,T,n)
    assert d.shape[-1] == out["ndraws"] == n
    nanc = np.isnan(d).any(axis=-1)
    assert nanc.sum() == (1 if fam == "binomial" else 0)
    if fam != "gaussian":
        assert np.all((d == np.floor(d)) | np.isnan(d)) and np.nanmin(d) >= 0
    rel = lambda a, b: np.abs(a - b)[~np.isnan(b)].max() / max(np.abs(b[~np.isnan(b)]).max(), 1e-300)
    same_nan = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore"):
        ref_q = np.percentile(d, q, axis=-1)
        ref_m, ref_v = d.mean(-1), d.var(-1, ddof=1)
    for name, got, ref in (("quantiles", out["quantiles"], ref_q), ("y_mean", out["y_mean"], ref_m), ("y_var", out["y_var"], ref_v)):
        print(fam, pattern, name, rel(got, ref))
        assert same_nan(got, ref) and rel(got, ref) <= 1e-12, name
    obs = ~np.isnan(Y)
    nobs = obs.sum(-1).astype(float)
    np.testing.assert_array_equal(out["nobs"], nobs)
    with np.errstate(invalid="ignore", divide="ignore"):
        lt = np.where(obs, (d[..., None, :] < Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
        le = np.where(obs, (d[..., None, :] <= Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
    lt[nanc], le[nanc] = np.nan, np.nan
    ins = (obs & (Y >= ref_q[0][..., None]) & (Y <= ref_q[-1][..., None])).sum(-1).astype(float)
    ins[nanc] = np.nan
    assert same_nan(out["pit_lo"], lt) and same_nan(out["pit_hi"], le)
    assert rel(out["pit_lo"], lt) <= 1e-12 and rel(out["pit_hi"], le) <= 1e-12
    np.testing.assert_array_equal(out["inside"], ins)
    ok = ~nanc
    assert out["coverage"] == ins[ok].sum() / nobs[ok].sum()
    # politics/benchmark.py:158-164, per sample over the observed entries
    res = (Y[None] - Mu[..., None])[:, obs]                       # (S, n_obs)
    rmse, mae = np.sqrt((res ** 2).mean(axis=1)), np.abs(res).mean(axis=1)
    # (Binomial: a missing trial count under an observed y poisons E[y] of its cell, so every sample's score is nan)
    assert same_nan(out["rmse"], rmse) and same_nan(out["mae"], mae)
    if not np.isnan(rmse).any():
        print(fam, pattern, "rmse", rel(out["rmse"], rmse), "mae", rel(out["mae"], mae))
        assert rel(out["rmse"], rmse) <= 1e-10 and rel(out["mae"], mae) <= 1e-10


def test_binomial_rmse_without_missing_trials():
    N, M, T, K, S = 4, 3, 6, 2, 9
    rs = np.random.RandomState(8)
    Ws, Vs = _states(rs, S, N, M, T, K)
    tr = rs.randint(1, 30, size=(N, M, T)).astype(float)
    Yb = rs.binomial(tr.astype(int), 0.4).astype(float)
    Yb[0, 1] = np.nan
    out = utils.posterior_predictive(Ws, Vs, "binomial", data=(Yb, tr), seed=1)
    Mu = tr[None] * expit(_eta(Ws, Vs))
    res = (Yb[None] - Mu)[:, ~np.isnan(Yb)]
    assert np.abs(out["rmse"] - np.sqrt((res ** 2).mean(1))).max() <= 1e-10 * out["rmse"].max()
    assert np.abs(out["mae"] - np.abs(res).mean(1)).max() <= 1e-10 * out["mae"].max()


# ---------------------------------------------------------------- 4. determinism and geometry independence
@pytest.mark.parametrize("fam", FAMS)
def test_same_seed_same_bits_and_geometry_independence(fam):
    N, M, T, K, S, R = 6, 4, 5, 2, 50, 2
    rs = np.random.RandomState(30 + FAMS.index(fam))
    Ws, Vs = _states(rs, S, N + 9, M, T, K, positive=fam == "poisson_identity")
    kw, _ = _family_args(fam, rs, S, (N + 9, M, T))
    Y = np.round(np.abs(rs.normal(size=(N + 9, M, T, 2)) * 3))
    big = dict(kw)
    small = {k: (v[:, :N] if k == "R" else (v[:N] if k == "trials" else v)) for k, v in kw.items()}
    cells = [3, 40, 77, 119]                                       # flat (i,j,t) indices < N M T: unchanged when rows are appended
    a = utils.posterior_predictive(Ws[:, :N], Vs, fam, data=Y[:N], draws_per_sample=R, seed=99, cells=cells, **small)
    b = utils.posterior_predictive(Ws[:, :N], Vs, fam, data=Y[:N], draws_per_sample=R, seed=99, cells=cells, **small)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = utils.posterior_predictive(Ws[:, :N], Vs, fam, draws_per_sample=R, seed=99, cells=[77, 5, 3], **small)
    np.testing.assert_array_equal(c["draws"][0], a["draws"][2])
    np.testing.assert_array_equal(c["draws"][2], a["draws"][0])
    np.testing.assert_array_equal(c["quantiles"], a["quantiles"])
    g = utils.posterior_predictive(Ws, Vs, fam, draws_per_sample=R, seed=99, cells=cells, **big)     # N grows: another launch geometry
    np.testing.assert_array_equal(g["draws"], a["draws"])
    np.testing.assert_array_equal(g["quantiles"][:, :N], a["quantiles"])
    other = utils.posterior_predictive(Ws[:, :N], Vs, fam, draws_per_sample=R, seed=100, cells=cells, **small)
    assert not np.array_equal(other["draws"], a["draws"])


# ---------------------------------------------------------------- 5. error paths
def test_error_paths():
    N, M, T, K = 4, 3, 5, 2
    rs = np.random.RandomState(4)
    Y = rs.normal(size=(N, M, T))
    np.random.seed(0)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K)
    with pytest.raises(RuntimeError, match="no samples collected"):
        model.posterior_predictive()
    res = dict(W=rs.normal(size=(3, N, K)), V=rs.normal(size=(3, M, T, K)), nu2=np.ones((3, 1)))
    with pytest.raises(ValueError):
        model.posterior_predictive(results=dict(W=res["W"], V=res["V"][:, :, :4], nu2=res["nu2"]))
    with pytest.raises(ValueError):
        model.posterior_predictive(results=dict(W=res["W"], V=res["V"]))                  # no nu2
    with pytest.raises(ValueError):
        model.posterior_predictive(results=res, data=np.zeros((N, M, T + 1)))
    with pytest.raises(ValueError, match="16384"):
        model.posterior_predictive(results=res, draws_per_sample=6000)
    with pytest.raises(ValueError):
        model.posterior_predictive(results=res, cells=[N * M * T])
    out = model.posterior_predictive(results=res, data=Y, seed=1)
    assert np.isfinite(out["coverage"])
    # the C entry point refuses the same things on its own
    lib = _native.load()
    big = dict(W=np.zeros((16385, N, K)), V=np.zeros((16385, M, T, K)))
    m = np.zeros((N, M, T))
    rc = lib.btf_predict_eval(model._ctx.h, 0, 0.0, 16385, _native.dptr(big["W"]), _native.dptr(big["V"]), None, 0, None, None, 0, 1,
                              1, None, 0, None, 0, _native.dptr(m), *([None] * 10))
    assert rc == _native.BTF_EINVAL and b"16384" in lib.btf_last_error(model._ctx.h)
    rc = lib.btf_predict_eval(model._ctx.h, 3, 1.0, 2, None, None, None, 0, None, None, 0, 1, 1, None, 0, None, 0, _native.dptr(m),
                              *([None] * 10))
    assert rc == _native.BTF_ESTATE
    cb = NonconjugateBayesianTensorFiltering(N, M, T, loglikelihood=lambda data, mu: -0.5 * (data - mu) ** 2, nembeds=K)
    with pytest.raises(NotImplementedError, match="callable"):
        cb.posterior_predictive(results=res)


def test_gamma_grid_is_refused():
    import inspect
    N, M, T, K = 4, 3, 5, 2
    sig = inspect.signature(NonconjugateBayesianTensorFiltering.__init__)
    np.random.seed(0)
    model = NonconjugateBayesianTensorFiltering(N, M, T, loglikelihood="poisson_log", nembeds=K)
    model._link = 5                                    # the gamma_grid link id (LINKS["gamma_grid"])
    assert NonconjugateBayesianTensorFiltering.LINKS["gamma_grid"] == 5 and "loglikelihood" in sig.parameters
    with pytest.raises(NotImplementedError, match="gamma_grid"):
        model.posterior_predictive(results=dict(W=np.zeros((2, N, K)), V=np.zeros((2, M, T, K))))


def test_conjugate_count_models():
    """The Binomial model draws with the N of its (Y, N) pair; the Negative-Binomial model with results['R'] / its current R."""
    N, M, T, K, S = 5, 4, 6, 2, 20
    rs = np.random.RandomState(12)
    Ws, Vs = _states(rs, S, N, M, T, K)
    eta = _eta(Ws, Vs)
    tr = rs.randint(1, 20, size=(N, M, T)).astype(float)
    Yb = rs.binomial(tr.astype(int), expit(eta[0])).astype(float)
    np.random.seed(0)
    bm = BinomialBayesianTensorFiltering(N, M, T, nembeds=K)
    out = bm.posterior_predictive(results=dict(W=Ws, V=Vs), data=(Yb, tr), seed=2, cells=np.arange(N * M * T))
    assert np.abs(out["mean"] - (tr * expit(eta)).mean(0)).max() <= 1e-12 * tr.max()
    assert np.all(out["draws"] <= tr.reshape(-1, 1)) and np.all(out["draws"] >= 0)
    nb = NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, R_init=np.full((1, 1, 1), 2.5))
    Yn = rs.negative_binomial(2.5, 1 - expit(eta[0])).astype(float)
    R = rs.uniform(1, 3, size=(S, 1, 1, 1))
    out = nb.posterior_predictive(results=dict(W=Ws, V=Vs, R=R), data=Yn, seed=2)
    assert np.abs(out["mean"] - (R * np.exp(eta)).mean(0)).max() <= 1e-12 * (R * np.exp(eta)).max()
    out = nb.posterior_predictive(results=dict(W=Ws, V=Vs), data=Yn, seed=2)             # the current rate
    assert np.abs(out["mean"] - (2.5 * np.exp(eta)).mean(0)).max() <= 1e-12 * (2.5 * np.exp(eta)).max()
    assert np.isfinite(out["rmse"]).all() and 0 <= out["coverage"] <= 1


# ---------------------------------------------------------------- 6. the samplers against scipy
def _moment_checks(x, dist, label):
    n = x.size
    m, v, _, k = (float(a) for a in dist.stats(moments="mvsk"))
    mu4 = (k + 3.0) * v * v
    z1 = abs(x.mean() - m) / np.sqrt(v / n)
    print(label, "mean z %.2f" % z1)
    assert z1 <= Z, label
    # the variance of (x - m)^2 is mu4 - v^2; for a symmetric two-point law it is 0 and the sample variance is a function of the mean
    if mu4 - v * v > 1e-12 * v * v:
        z2 = abs(((x - m) ** 2).mean() - v) / np.sqrt((mu4 - v * v) / n)
        print(label, "var z %.2f" % z2)
        assert z2 <= Z, label


def _chi2_p(x, dist):
    n = x.size
    lo, hi = int(x.min()), int(x.max())
    ks = np.arange(lo, hi + 1)
    obs = np.bincount((x - lo).astype(np.int64), minlength=len(ks)).astype(float)
    exp = n * dist.pmf(ks)
    exp[0] += n * dist.cdf(lo - 1)
    exp[-1] += n * dist.sf(hi)
    O, E, o, e = [], [], 0.0, 0.0
    for a, b in zip(obs, exp):                   # merge bins to expected >= 5
        o, e = o + a, e + b
        if e >= 5:
            O.append(o), E.append(e)
            o = e = 0.0
    if E:
        O[-1] += o
        E[-1] += e
    if len(E) < 2:
        return 1.0
    O, E = np.array(O), np.array(E)
    return float(stats.chi2.sf(((O - E) ** 2 / E).sum(), len(E) - 1))


SW = predictive.POISSON_SWITCH
POISSON_GRID = [1e-3, 0.5, 3.0, SW - 1e-9, SW, SW + 1e-9, 30.0, 1e3, 1e6]


@pytest.mark.parametrize("lam", POISSON_GRID)
def test_poisson_sampler(lam):
    dist = stats.poisson(lam)
    for fam, eta in (("poisson_identity", lam), ("poisson", np.log(lam))):
        x = predictive.batch(fam, np.full(NB, eta), 0.0, seed=1000 + POISSON_GRID.index(lam))
        assert np.all(x == np.floor(x)) and x.min() >= 0
        _moment_checks(x, dist, "poisson %s %g" % (fam, lam))
        p = _chi2_p(x, dist)
        print("poisson", fam, lam, "chi2 p", p)
        assert p >= PFLOOR


def test_poisson_edges():
    x = predictive.batch("poisson", np.array([-np.inf, np.inf, np.nan, 800.0]), 0.0)
    assert x[0] == 0 and np.isnan(x[1:]).all()
    x = predictive.batch("poisson_identity", np.array([0.0, -1.0, np.nan, 2.0]), 0.0)
    assert np.isnan(x[:3]).all() and x[3] >= 0


# the issue's grid, and n = 19, 20, 21 at p = 1/2: n min(p, 1-p) crosses this sampler's switch (10) there
BINOMIAL_N = [1, 2, 4, 19, 20, 21, 31, 32, 33, 100, 10**4, 10**6]


@pytest.mark.parametrize("n", BINOMIAL_N)
@pytest.mark.parametrize("p", [1e-4, 0.03, 0.5, 0.97])
def test_binomial_sampler(n, p):
    dist = stats.binom(n, p)
    x = predictive.batch("binomial", np.full(NB, np.log(p / (1 - p))), float(n), seed=2000 + 7 * BINOMIAL_N.index(n))
    assert np.all(x == np.floor(x)) and x.min() >= 0 and x.max() <= n
    _moment_checks(x, dist, "binomial %d %g" % (n, p))
    pv = _chi2_p(x, dist)
    print("binomial", n, p, "chi2 p", pv)
    assert pv >= PFLOOR


def test_binomial_edges():
    x = predictive.batch("binomial", np.zeros(5), np.array([0.0, np.nan, -1.0, 2.5, 3.0]))
    assert x[0] == 0 and np.isnan(x[1:4]).all() and 0 <= x[4] <= 3


@pytest.mark.parametrize("r", [0.3, 1.0, 5.0, 50.0])
@pytest.mark.parametrize("p", [0.05, 0.5, 0.95])
def test_negative_binomial_sampler(r, p):
    dist = stats.nbinom(r, 1 - p)                    # mean r p / (1 - p)
    x = predictive.batch("negbin", np.full(NB, np.log(p / (1 - p))), r, seed=3000 + int(10 * r))
    assert np.all(x == np.floor(x)) and x.min() >= 0
    _moment_checks(x, dist, "negbin %g %g" % (r, p))
    pv = _chi2_p(x, dist)
    print("negbin", r, p, "chi2 p", pv)
    assert pv >= PFLOOR


def test_normal_sampler():
    x = predictive.batch("gaussian", np.full(NB, 1.5), 4.0, seed=4000)
    dist = stats.norm(1.5, 2.0)
    _moment_checks(x, dist, "normal")
    p = stats.kstest(x, dist.cdf).pvalue
    print("normal KS p", p)
    assert p >= PFLOOR
    assert np.array_equal(x, predictive.batch("gaussian", np.full(NB, 1.5), 4.0, seed=4000))


# ---------------------------------------------------------------- 7. end to end against the exact mixture CDF
MIX = dict(S=200, R=4, N=10, M=10, T=30, K=3)
PS = (2.5, 50.0, 97.5)


def _mixture_case(fam, seed):
    S, R, N, M, T, K = (MIX[k] for k in "SRNMTK")
    rs = np.random.RandomState(seed)
    Ws, Vs = _states(rs, S, N, M, T, K, scale=0.7)
    eta = _eta(Ws, Vs) + (1.0 if fam == "poisson" else 0.0)
    Vs = Vs.copy()
    kw, aux = _family_args(fam, rs, S, (N, M, T))
    if fam == "binomial":
        kw["trials"] = np.maximum(kw["trials"], 1.0)
        aux = kw["trials"][None]
    out = utils.posterior_predictive(Ws, Vs, fam, q=PS, draws_per_sample=R, seed=seed, **kw)
    return out, _eta(Ws, Vs), aux, S * R, N * M * T


def test_mixture_quantiles_gaussian():
    out, eta, aux, n, C = _mixture_case("gaussian", 41)
    assert C >= 3000
    sd = np.sqrt(aux)
    for k, pc in enumerate(PS):
        p = pc / 100.0
        F = stats.norm.cdf((out["quantiles"][k][None] - eta) / sd).mean(axis=0)
        dev, bound = abs(F.mean() - p), Z * np.sqrt(p * (1 - p) / (n * C)) + 1.0 / n
        print("gaussian mixture p=%g deviation %.2e bound %.2e" % (p, dev, bound))
        assert dev <= bound


@pytest.mark.parametrize("fam", ["poisson", "binomial"])
def test_mixture_quantiles_counts(fam):
    out, eta, aux, n, C = _mixture_case(fam, 43 if fam == "poisson" else 47)
    assert C >= 3000
    cdf = (lambda y: stats.poisson.cdf(y[None], np.exp(eta)).mean(axis=0)) if fam == "poisson" else \
        (lambda y: stats.binom.cdf(y[None], aux, expit(eta)).mean(axis=0))
    for k, pc in enumerate(PS):
        p = pc / 100.0
        z = 6.5 * np.sqrt(p * (1 - p) / n) + 1.0 / n
        qv = out["quantiles"][k]
        hi, lo = cdf(np.ceil(qv)), cdf(np.floor(qv) - 1)
        print(fam, "mixture p=%g smallest margins %.3g %.3g" % (p, (hi - (p - z)).min(), ((p + z) - lo).min()))
        assert np.all(hi >= p - z) and np.all(lo <= p + z)


# ---------------------------------------------------------------- 8. well-specified coverage
@pytest.mark.parametrize("fam", ["gaussian", "poisson", "binomial", "negbin"])
def test_well_specified_coverage(fam):
    S, R, N, M, T, K = 200, 4, 10, 10, 30, 3
    rs = np.random.RandomState(60 + FAMS.index(fam))
    W, V = rs.normal(0, 0.7, size=(N, K)), rs.normal(0, 0.7, size=(M, T, K))
    eta = np.einsum("nk,mtk->nmt", W, V)
    Ws, Vs = np.repeat(W[None], S, 0), np.repeat(V[None], S, 0)
    if fam == "gaussian":
        Y, kw = eta + rs.normal(0, np.sqrt(0.4), size=eta.shape), dict(param=0.4)
    elif fam == "poisson":
        Y, kw = rs.poisson(np.exp(eta)).astype(float), {}
    elif fam == "binomial":
        tr = rs.randint(1, 40, size=eta.shape)
        Y, kw = rs.binomial(tr, expit(eta)).astype(float), dict(trials=tr.astype(float))
    else:
        Y, kw = rs.negative_binomial(2.0, 1 - expit(eta)).astype(float), dict(param=2.0)
    out = utils.posterior_predictive(Ws, Vs, fam, data=Y, q=(2.5, 97.5), draws_per_sample=R, seed=70, **kw)
    C, n = N * M * T, S * R
    assert out["nobs"].sum() == C
    term = Z * np.sqrt(0.95 * 0.05 / C) + 2.0 / n
    print(fam, "coverage %.4f, 0.95 -/+ %.4f" % (out["coverage"], term))
    assert out["coverage"] >= 0.95 - term
    if fam == "gaussian":
        assert out["coverage"] <= 0.95 + term
    # PIT of a well-specified model is uniform: its mid-point has mean 1/2 (variance <= 1/12 per cell)
    mid = 0.5 * (out["pit_lo"] + out["pit_hi"])
    assert abs(mid.mean() - 0.5) <= Z * np.sqrt(1.0 / 12.0 / C) + 1.0 / n
