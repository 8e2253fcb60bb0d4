"""Posterior predictive of the gamma-grid likelihood on the GPU (csrc/btf_gg_predict.h via predictive.gamma_grid_batch,
utils.gamma_grid_predictive and the models' gamma_grid_predictive): the sampler against scipy, the reductions against
numpy from the returned draws, geometry independence, the model method, and the bands end to end.

Z, PFLOOR and NB are those of tests/test_gpu_predictive.py (a z-score of 5.5 per moment check, a p-value floor of 1e-6 per
goodness-of-fit check, 200000 draws), the deterministic tolerances too: 1e-12 relative for the reductions of the draws and
for `mean`, 1e-10 for rmse / mae.  Seeds are fixed.  Every statistical check goes through _batch / _predict, so that it can
be run with numpy's draws in their place: a check the host sampler could not pass would be mis-derived."""

import numpy as np
import pytest
from scipy import stats
from scipy.special import gammainc

from functionalmf_amd import _native, predictive, utils
from functionalmf_amd.likelihoods import GammaGridLikelihood

from test_gpu_predictive import NB, PFLOOR, Z, _eta, _moment_checks, _patterns, _states

pytestmark = pytest.mark.gpu


def _batch(eta, lik, seed):
    return predictive.gamma_grid_batch(eta, lik, seed=seed, components=True)


def _predict(Ws, Vs, lik, **kw):
    return utils.gamma_grid_predictive(Ws, Vs, lik, **kw)


def _rate_table(G=50):
    """The table of scripts/gamma_grid_predictive_rate.py: means 0.5 .. 1.5, a bump of weights around 1, variance 0.01."""
    grid = np.linspace(0.5, 1.5, G)
    return GammaGridLikelihood(grid, np.exp(-0.5 * ((grid - 1.0) / 0.25) ** 2), 0.01)


def _table(G, seed, zeros=0.0):
    """G components with shapes on both sides of 1, unnormalised weights, a share `zeros` of them exactly 0: the first,
    the last (a uniform above every cumulative weight has to fall back past it) and others at random."""
    rs = np.random.RandomState(seed)
    p = rs.gamma(2.0, 1.0, size=G)
    if zeros:
        p[[0, G - 1]] = 0.0
        p[1 + rs.permutation(G - 2)[:int(round(zeros * G)) - 2]] = 0.0
    return GammaGridLikelihood.from_table(rs.uniform(0.4, 20.0, size=G), rs.uniform(0.05, 0.5, size=G), p)


def _weights(lik):
    return lik.probs_grid / lik.probs_grid.sum()


# ---------------------------------------------------------------- 1. the sampler
SHAPES, ETAS = [0.3, 1.0, 5.0, 200.0], [0.05, 1.0, 30.0]


@pytest.mark.parametrize("a", SHAPES)
def test_one_component_is_a_gamma(a):
    s = 0.37
    lik = GammaGridLikelihood.from_table([a], [s], [2.5])
    for eta in ETAS:
        x, comp = _batch(np.full(NB, eta), lik, seed=5000 + 10 * SHAPES.index(a) + ETAS.index(eta))
        assert np.all(comp == 0) and np.all(x > 0) and np.all(np.isfinite(x))
        dist = stats.gamma(a, scale=s * eta)
        p = stats.kstest(x, dist.cdf).pvalue
        print("gamma a=%g eta=%g KS p %.3g" % (a, eta, p))
        assert p >= PFLOOR
        _moment_checks(x, dist, "gamma a=%g eta=%g" % (a, eta))


def _chi2_components(comp, w):
    """p-value of the component counts against n w_g, components merged in index order to expected >= 5"""
    n = comp.size
    obs, exp = np.bincount(comp, minlength=w.size).astype(float), n * w
    O, E, o, e = [], [], 0.0, 0.0
    for a, b in zip(obs, exp):
        o, e = o + a, e + b
        if e >= 5:
            O.append(o), E.append(e)
            o = e = 0.0
    O[-1] += o
    E[-1] += e
    O, E = np.array(O), np.array(E)
    assert len(E) >= 2 and O.sum() == n
    return float(stats.chi2.sf(((O - E) ** 2 / E).sum(), len(E) - 1))


@pytest.mark.parametrize("case", ["G3", "G128"])
def test_components_follow_the_weights(case):
    if case == "G3":
        lik = GammaGridLikelihood.from_table([2.0, 0.5, 9.0], [0.3, 0.2, 0.1], [0.2, 0.5, 0.3])
    else:
        lik = _table(128, 6, zeros=0.25)
        assert (lik.probs_grid == 0).sum() == 32 and lik.probs_grid[0] == 0 and lik.probs_grid[-1] == 0
    w = _weights(lik)
    eta = np.full(NB, 0.8)
    x, comp = _batch(eta, lik, seed=6000)
    assert comp.min() >= 0 and comp.max() < w.size
    counts = np.bincount(comp, minlength=w.size)
    assert np.all(counts[w == 0] == 0)                 # a zero-weight component is hit exactly 0 times
    p = _chi2_components(comp, w)
    print(case, "components chi2 p %.3g" % p)
    assert p >= PFLOOR
    # unnormalised weights: the same bits
    x7, comp7 = _batch(eta, GammaGridLikelihood.from_table(lik.shape_grid, lik.scale_grid, lik.probs_grid * 7.0), seed=6000)
    np.testing.assert_array_equal(comp7, comp)
    np.testing.assert_array_equal(x7, x)


def _mixture_cdf(lik, eta):
    w, a, s = _weights(lik), lik.shape_grid, lik.scale_grid
    keep = w > 0
    return lambda y: (w[keep] * gammainc(a[keep], np.asarray(y)[..., None] / (s[keep] * eta))).sum(axis=-1)


def test_mixture_of_the_rate_table():
    lik = _rate_table()
    assert lik.shape_grid.size == 50
    x, comp = _batch(np.full(NB, 0.6), lik, seed=6100)
    p = stats.kstest(x, _mixture_cdf(lik, 0.6)).pvalue
    print("mixture G=50 KS p %.3g" % p)
    assert p >= PFLOOR
    # and the mean: eta mbar, with the mixture's variance
    m = predictive.gamma_grid_mean(lik, 0.6)
    w, a, s = _weights(lik), lik.shape_grid, lik.scale_grid * 0.6
    var = (w * (a * s * s + (a * s) ** 2)).sum() - m * m
    z = abs(x.mean() - m) / np.sqrt(var / NB)
    print("mixture mean z %.2f" % z)
    assert z <= Z


def test_edges_and_determinism():
    lik = _table(7, 8)
    eta = np.array([0.0, -1.0, np.nan, 2.0, -0.0, np.inf])
    x, comp = _batch(eta, lik, seed=1)
    assert np.isnan(x[[0, 1, 2, 4]]).all() and np.all(comp[[0, 1, 2, 4]] == -1)
    assert x[3] > 0 and 0 <= comp[3] < 7 and x[5] == np.inf
    eta = np.random.RandomState(2).uniform(0.1, 3.0, size=5000)
    a, ca = _batch(eta, lik, seed=77)
    b, cb = _batch(eta, lik, seed=77)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ca, cb)
    c, _ = _batch(eta, lik, seed=78)
    assert not np.array_equal(a, c)
    # draw i is a function of (seed, table, eta[i], i): a prefix of the batch gives the same bits
    np.testing.assert_array_equal(_batch(eta[:1234], lik, seed=77)[0], a[:1234])
    np.testing.assert_array_equal(predictive.gamma_grid_batch(eta, lik, seed=77), a)          # without comp_out


# ---------------------------------------------------------------- 2. reductions against numpy from the returned draws
Q = (2.5, 30.0, 97.5)


def _check_reductions(N, M, T, K, S, R, Rrep, G, pattern, seed):
    shape = (N, M, T)
    rs = np.random.RandomState(seed)
    Ws, Vs = _states(rs, S, N, M, T, K, positive=True)
    lik = _table(G, seed + 1, zeros=0.25 if G >= 8 else 0.0)
    eta = _eta(Ws, Vs)
    Mu = predictive.gamma_grid_mean(lik, eta)                      # (S,N,M,T)
    Y = Mu[0][..., None] * rs.gamma(5.0, 0.2, size=shape + (Rrep,))
    Y = _patterns(Y, pattern, rs)
    cells = np.arange(N * M * T, dtype=np.int32)[::-1]
    out = _predict(Ws, Vs, lik, data=Y, q=Q, draws_per_sample=R, seed=21, cells=cells)
    n = S * R
    d = out["draws"][np.argsort(cells)].reshape(shape + (n,))
    assert d.shape[-1] == out["ndraws"] == n and out["nsamples"] == S
    assert np.all(np.isfinite(d)) and np.all(d > 0)
    rel = lambda a, b: np.abs(a - b)[~np.isnan(b)].max() / max(np.abs(b[~np.isnan(b)]).max(), 1e-300) if (~np.isnan(b)).any() else 0.0
    same_nan = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        ref_q = np.percentile(d, Q, axis=-1)
        ref_m = d.mean(-1)
        ref_v = d.var(-1, ddof=1) if n > 1 else np.full(shape, np.nan)
    for name, got, ref in (("quantiles", out["quantiles"], ref_q), ("y_mean", out["y_mean"], ref_m), ("y_var", out["y_var"], ref_v),
                           ("mean", out["mean"], Mu.mean(axis=0))):
        print(pattern, G, name, rel(got, ref))
        assert same_nan(got, ref) and rel(got, ref) <= 1e-12, name
    obs = ~np.isnan(Y)
    nobs = obs.sum(-1).astype(float)
    np.testing.assert_array_equal(out["nobs"], nobs)
    with np.errstate(invalid="ignore", divide="ignore"):
        lt = np.where(obs, (d[..., None, :] < Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
        le = np.where(obs, (d[..., None, :] <= Y[..., None]).mean(-1), 0.0).sum(-1) / nobs
    ins = (obs & (Y >= ref_q[0][..., None]) & (Y <= ref_q[-1][..., None])).sum(-1).astype(float)
    assert same_nan(out["pit_lo"], lt) and same_nan(out["pit_hi"], le)
    assert rel(out["pit_lo"], lt) <= 1e-12 and rel(out["pit_hi"], le) <= 1e-12
    np.testing.assert_array_equal(out["inside"], ins)
    assert out["coverage"] == ins.sum() / nobs.sum() and abs(out["nominal"] - 0.95) < 1e-15
    res = (Y[None] - Mu[..., None])[:, obs]
    rmse, mae = np.sqrt((res ** 2).mean(axis=1)), np.abs(res).mean(axis=1)
    print(pattern, G, "rmse", rel(out["rmse"], rmse), "mae", rel(out["mae"], mae))
    assert rel(out["rmse"], rmse) <= 1e-10 and rel(out["mae"], mae) <= 1e-10
    return out


PATTERNS = ["complete", "heldout", "replicates", "empty_cell"]


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 128])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_reductions_against_numpy(pattern, G):
    # n = 111 is no power of two; M T = 28 is no multiple of the 16 cells a workgroup takes at this n
    _check_reductions(5, 4, 7, 3, 37, 3, 3, G, pattern, seed=100 + 10 * PATTERNS.index(pattern) + G)


@pytest.mark.parametrize("name,dims", [
    ("one_draw", dict(N=5, M=4, T=7, K=3, S=1, R=1)),              # S R = 1: a row of two, no variance
    ("K1", dict(N=5, M=4, T=7, K=1, S=37, R=3)),
    ("K10", dict(N=5, M=4, T=7, K=10, S=37, R=3)),
    ("one_row_two_depths", dict(N=1, M=4, T=2, K=3, S=37, R=3)),
    ("cells_not_a_multiple", dict(N=3, M=7, T=5, K=2, S=300, R=1)),       # P = 512: 16 cells a workgroup, M T = 35
    ("one_cell_a_workgroup", dict(N=2, M=3, T=2, K=2, S=2100, R=2)),      # P = 8192: the row budget holds one cell
])
def test_reductions_at_other_geometries(name, dims):
    _check_reductions(Rrep=2, G=5, pattern="replicates", seed=300 + len(name), **dims)


def test_a_negative_row_poisons_what_poisson_identity_poisons():
    N, M, T, K, S, R = 5, 4, 7, 3, 37, 3
    rs = np.random.RandomState(9)
    Ws, Vs = _states(rs, S, N, M, T, K, positive=True)
    Ws[3, 2] = -Ws[3, 2]                               # sample 3, row 2: eta < 0
    lik = _table(6, 10)
    Y = np.ceil(rs.gamma(3.0, 1.0, size=(N, M, T, 2)))
    Y[0, 1] = np.nan
    cells = np.arange(N * M * T, dtype=np.int32)
    gg = _predict(Ws, Vs, lik, data=Y, q=Q, draws_per_sample=R, seed=4, cells=cells)
    po = utils.posterior_predictive(Ws, Vs, "poisson_identity", data=Y, q=Q, draws_per_sample=R, seed=4, cells=cells)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(np.isnan(gg[k]), np.isnan(po[k]), err_msg=k)
    assert np.isnan(gg["mean"][2]).all() and np.isfinite(np.delete(gg["mean"], 2, axis=0)).all()
    assert np.isnan(gg["rmse"][3]) and np.isfinite(np.delete(gg["rmse"], 3)).all()
    assert np.isnan(gg["draws"].reshape(N, M * T, S, R)[2, :, 3]).all()
    np.testing.assert_array_equal(gg["nobs"], po["nobs"])
    assert np.isfinite(gg["coverage"])                 # (the poisoned cells are left out of it)


# ---------------------------------------------------------------- 3. geometry independence
def test_same_seed_same_bits_and_geometry_independence():
    N, M, T, K, S, R = 6, 4, 5, 2, 50, 2
    rs = np.random.RandomState(36)
    Ws, Vs = _states(rs, S, N + 9, M, T, K, positive=True)
    lik = _table(20, 37, zeros=0.25)
    Y = rs.gamma(3.0, 0.4, size=(N + 9, M, T, 2))
    cells = [3, 40, 77, 119]                                       # flat (i,j,t) indices < N M T: unchanged when rows are appended
    kw = dict(draws_per_sample=R, seed=99)
    a = _predict(Ws[:, :N], Vs, lik, data=Y[:N], cells=cells, **kw)
    b = _predict(Ws[:, :N], Vs, lik, data=Y[:N], cells=cells, **kw)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = _predict(Ws[:, :N], Vs, lik, cells=[77, 5, 3], **kw)        # the order of cells is free, and so is what is listed
    np.testing.assert_array_equal(c["draws"][0], a["draws"][2])
    np.testing.assert_array_equal(c["draws"][2], a["draws"][0])
    np.testing.assert_array_equal(c["quantiles"], a["quantiles"])
    g = _predict(Ws, Vs, lik, cells=cells, **kw)                    # N grows: another launch geometry
    np.testing.assert_array_equal(g["draws"], a["draws"])
    np.testing.assert_array_equal(g["quantiles"][:, :N], a["quantiles"])
    np.testing.assert_array_equal(g["mean"][:N], a["mean"])
    other = _predict(Ws[:, :N], Vs, lik, cells=cells, draws_per_sample=R, seed=100)
    assert not np.array_equal(other["draws"], a["draws"])
    # a draw of the call is the batch's draw at the same global index, (cell S + s) R + r: the same component and gamma
    # variate, times an eta that the host's einsum rounds differently from the kernel's fma chain
    eta = _eta(Ws[:, :N], Vs).reshape(S, -1)
    idx = (np.asarray(cells)[:, None, None] * S + np.arange(S)[None, :, None]) * R + np.arange(R)[None, None, :]
    full = np.zeros(idx.max() + 1)
    full[idx.ravel()] = np.repeat(eta[:, cells].T, R, axis=1).ravel()
    full[full == 0] = 1.0
    np.testing.assert_allclose(predictive.gamma_grid_batch(full, lik, seed=99)[idx.ravel()], a["draws"].ravel(), rtol=1e-13)


# ---------------------------------------------------------------- 4. the model method
def test_model_method_collected_uploaded_and_stateless():
    from test_gpu_gg_criteria import _chain_problem, _constrained
    (N, M, T, K), W, V, Y, lik = _chain_problem(21)
    m = _constrained(N, M, T, K, lik, W, V, seed=3)
    res = m.run_gibbs(Y, nburn=5, nsamples=12, verbose=False)
    assert m._collected == 12
    cells = [0, 17, N * M * T - 1]
    a = m.gamma_grid_predictive(seed=3, cells=cells, draws_per_sample=2)
    b = m.gamma_grid_predictive(res, seed=3, cells=cells, draws_per_sample=2)
    u = utils.gamma_grid_predictive(res["W"], res["V"], lik, data=Y, seed=3, cells=cells, draws_per_sample=2)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)       # bit for bit, nan == nan
        np.testing.assert_array_equal(a[k], u[k], err_msg=k)
    assert a["coverage"] == b["coverage"] == u["coverage"] and a["nsamples"] == 12 and a["ndraws"] == 24
    assert np.isfinite(a["coverage"]) and np.all(np.isfinite(a["draws"])) and np.all(a["draws"] > 0)
    assert a["nobs"].sum() == (~np.isnan(Y)).sum()
    ref = predictive.gamma_grid_mean(lik, _eta(res["W"], res["V"])).mean(axis=0)
    assert np.abs(a["mean"] - ref).max() <= 1e-12 * np.abs(ref).max()
    # held-out data through data=
    Yh = np.full_like(Y, np.nan)
    Yh[::3, ::2] = Y[::3, ::2]
    h = m.gamma_grid_predictive(data=Yh, seed=3)
    np.testing.assert_array_equal(h["quantiles"], m.gamma_grid_predictive(seed=3)["quantiles"])
    assert h["nobs"].sum() == (~np.isnan(Yh)).sum() < a["nobs"].sum()
    d0 = m._draws
    m.gamma_grid_predictive()                          # seed=None: the model's next device seed
    assert m._draws == d0 + 1
    with pytest.raises(NotImplementedError, match="gamma_grid"):
        m.posterior_predictive(res)
    # after posterior_monotone(in_place=True): the projected states, where they lie
    m.posterior_monotone(in_place=True)
    projected = utils.posterior_monotone(res["W"], res["V"])["V"]
    assert not np.array_equal(projected, res["V"])
    p = m.gamma_grid_predictive(seed=3, cells=cells, draws_per_sample=2)
    pu = utils.gamma_grid_predictive(res["W"], projected, lik, data=Y, seed=3, cells=cells, draws_per_sample=2)
    for k in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(p[k], pu[k], err_msg=k)


def test_entry_point_refusals():
    N, M, T, K, S = 4, 3, 5, 2, 3
    rs = np.random.RandomState(4)
    Ws, Vs = _states(rs, S, N, M, T, K, positive=True)
    lib = _native.load()
    dp = _native.dptr
    m = np.zeros((N, M, T))
    bare = _native.Context(N, M, T, K, 0)
    try:
        # no table: BTF_ESTATE, nothing launched (the output stays as it was)
        m[:] = -7.0
        rc = lib.btf_predict_gg_eval(bare.h, S, dp(Ws), dp(Vs), None, 0, 1, 1, None, 0, None, 0, dp(m), *([None] * 10))
        assert rc == _native.BTF_ESTATE and b"btf_set_likelihood_table" in lib.btf_last_error(bare.h) and np.all(m == -7.0)
        a, s, p = (np.array(v) for v in ([2.0, 3.0], [0.1, 0.2], [1.0, 1.0]))
        bare.call("btf_set_likelihood_table", 5, dp(a), dp(s), dp(p), 2)
        rc = lib.btf_predict_gg_eval(bare.h, S, dp(Ws), dp(Vs), None, 0, 1, 1, None, 0, None, 0, dp(m), *([None] * 10))
        assert rc == _native.BTF_OK and np.all(m > 0)
        # the limits of btf_predict_eval, in its words
        big = dict(W=np.zeros((16385, N, K)), V=np.zeros((16385, M, T, K)))
        rc = lib.btf_predict_gg_eval(bare.h, 16385, dp(big["W"]), dp(big["V"]), None, 0, 1, 1, None, 0, None, 0, dp(m), *([None] * 10))
        assert rc == _native.BTF_EINVAL and b"exceeds 16384 (the draws of a cell are sorted in LDS)" in lib.btf_last_error(bare.h)
        rc = lib.btf_predict_gg_eval(bare.h, 2, None, None, None, 0, 1, 1, None, 0, None, 0, dp(m), *([None] * 10))
        assert rc == _native.BTF_ESTATE and b"collected" in lib.btf_last_error(bare.h)
        rc = lib.btf_predict_gg_eval(bare.h, S, dp(Ws), dp(Vs), None, 0, 1, 1, None, 0, None, 0, dp(m), None, None, None, dp(m), *([None] * 6))
        assert rc == _native.BTF_EINVAL and b"pass Y" in lib.btf_last_error(bare.h)
        bad = np.array([N * M * T], dtype=np.int32)
        rc = lib.btf_predict_gg_eval(bare.h, S, dp(Ws), dp(Vs), None, 0, 1, 1, None, 0, bad.ctypes.data_as(_native._c_ip), 1, dp(m),
                                     *([None] * 9), dp(np.zeros((1, S))))
        assert rc == _native.BTF_EINVAL and b"out of range" in lib.btf_last_error(bare.h)
        # the old entry keeps refusing the family
        rc = lib.btf_predict_eval(bare.h, 5, 0.0, S, dp(Ws), dp(Vs), None, 0, None, None, 0, 1, 1, None, 0, None, 0, dp(m), *([None] * 10))
        assert rc == _native.BTF_EINVAL
    finally:
        bare.close()
    out = np.zeros(3)
    for G, tab in ((0, (a, s, p)), (129, (np.ones(129),) * 3), (2, (a, s, np.zeros(2))), (2, (a, -s, p)), (2, (a, s, np.array([1.0, np.nan])))):
        rc = lib.btf_predict_gg_batch(0, 3, dp(np.ones(3)), G, *(dp(np.ascontiguousarray(v, dtype=float)) for v in tab), 1, dp(out), None)
        assert rc == _native.BTF_EINVAL, G


# ---------------------------------------------------------------- 5. end to end: the bands against the exact mixture CDF
MIX = dict(S=200, R=4, N=10, M=10, T=30, K=3)
PS = (2.5, 50.0, 97.5)


def test_mixture_quantiles():
    S, R, N, M, T, K = (MIX[k] for k in "SRNMTK")
    rs = np.random.RandomState(41)
    Ws, Vs = _states(rs, S, N, M, T, K, positive=True)
    lik = _table(12, 42)
    out = _predict(Ws, Vs, lik, q=PS, draws_per_sample=R, seed=41)
    eta, n, C = _eta(Ws, Vs), S * R, N * M * T
    assert C >= 3000
    w, a, s = _weights(lik), lik.shape_grid, lik.scale_grid
    for k, pc in enumerate(PS):
        p = pc / 100.0
        F = np.zeros(eta.shape)
        for g in range(w.size):                        # the exact CDF of the cell's mixture over samples and components
            F += w[g] * gammainc(a[g], out["quantiles"][k][None] / (s[g] * eta))
        F = F.mean(axis=0)
        dev, bound = abs(F.mean() - p), Z * np.sqrt(p * (1 - p) / (n * C)) + 1.0 / n
        print("gamma-grid mixture p=%g deviation %.2e bound %.2e" % (p, dev, bound))
        assert dev <= bound


def test_well_specified_coverage():
    S, R, N, M, T, K = (MIX[k] for k in "SRNMTK")
    rs = np.random.RandomState(65)
    W, V = rs.uniform(0.3, 1.2, size=(N, K)), rs.uniform(0.3, 1.2, size=(M, T, K))
    eta = np.einsum("nk,mtk->nmt", W, V)
    Ws, Vs = np.repeat(W[None], S, 0), np.repeat(V[None], S, 0)
    lik = _table(12, 66)
    Y = lik.sample(eta, size=eta.shape, rng=rs)        # numpy, from the same table at the fixed states
    out = _predict(Ws, Vs, lik, data=Y, q=(2.5, 97.5), draws_per_sample=R, seed=70)
    C, n = N * M * T, S * R
    assert out["nobs"].sum() == C
    term = Z * np.sqrt(0.95 * 0.05 / C) + 2.0 / n
    print("gamma-grid coverage %.4f, 0.95 -/+ %.4f" % (out["coverage"], term))
    assert abs(out["coverage"] - 0.95) <= term
    mid = 0.5 * (out["pit_lo"] + out["pit_hi"])
    bound = Z * np.sqrt(1.0 / 12.0 / C) + 1.0 / n
    print("gamma-grid PIT mean %.4f, 0.5 -/+ %.4f" % (mid.mean(), bound))
    assert abs(mid.mean() - 0.5) <= bound
