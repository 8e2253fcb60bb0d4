"""Binary row features in the constrained model on the GPU (csrc/btf_gass_features.h): the reference's own row and
feature updates (tests/golden/g16_row_features.npz), candidate log-likelihoods and valid grids against numpy, the
stationary distribution of the U step against quadrature, whole chains, and the unchanged path without features."""
import ctypes

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

GRID = 10000


def _cls():
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    return ConstrainedNonconjugateBayesianTensorFiltering


def _fixture_model(g, ep=False, **kw):
    N, M, T, R, K, tf = [int(x) for x in g["dims"]]
    F = int(g["nfeat"])
    model = _cls()(
        N, M, T, "poisson_identity", g["Cons"], ep_approx=(g["b_Mu_ep"], g["b_Sigma_ep"]) if ep else None,
        Row_constraints=g["Row_constraints"], gass_ngrid=int(g["ngrid"]), nembeds=K, tf_order=tf,
        sigma2_init=float(g["s0_sigma2"]), lam2_init=float(g["s0_lam2"]), W_init=g["s0_W"].copy(), V_init=g["s0_V"].copy(),
        Tau2_init=g["s0_Tau2"].copy(), sampler="banded", row_features=g["X"], feature_embeddings=g["U0"].copy(), **kw)
    base = {0: 2000, 1: 3000, 2: 4000}
    model.chain_rngs = lambda what: [np.random.RandomState(base[what] + c) for c in range((N, M, F)[what])]
    return model, (N, M, T, R, K, tf, F)


def _side(X, P):
    """The reference's term (fit.py:49): nansum over the last axis of x log p + (1 - x) log(1 - p)."""
    with np.errstate(all="ignore"):
        return np.nansum(X * np.log(P) + (1 - X) * np.log(1 - P), axis=-1)


def _begin(model, what, Y, z, u, pick=0, seed=1):
    """Everything the model pushes before an update, then btf_gass_begin / btf_gass_grid: (info, mask, slice, cur_ll)."""
    from functionalmf_amd import _native
    if what != 2:
        model._bind_data(Y)
    model._push_state()
    rc = model.Row_constraints
    model._ctx.call("btf_gass_set_constraints", _native.dptr(model._cons), int(model._cons.shape[0]), _native.dptr(rc),
                    0 if rc is None else int(rc.shape[0]))
    model._cons_set = True
    model._push_ep()
    model._push_features()
    nch = (model.nrows, model.ncols, model.nfeatures)[what]
    model._ctx.call("btf_gass_begin", what, model._link, _native.dptr(z), _native.dptr(u), seed, 1e-6, 0, pick)
    info = np.zeros((nch, 2), dtype=np.int32)
    mask = np.zeros((nch, GRID), dtype=np.uint8)
    hh, cur = np.empty(nch), np.empty(nch)
    model._ctx.call("btf_gass_grid", what, info.ctypes.data_as(_native._c_ip), mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                    _native.dptr(hh), _native.dptr(cur))
    return info, mask, hh, cur


def _eval(model, what, thetas, nth):
    from functionalmf_amd import _native
    ll = np.empty(thetas.shape)
    model._ctx.call("btf_gass_eval", what, _native.dptr(thetas), nth.ctypes.data_as(_native._c_ip), _native.dptr(ll))
    return ll


# ---- 1. the reference's own updates ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_row_updates_vs_reference_fixture(golden, case):
    g = golden("g16_row_features.npz")
    model, _ = _fixture_model(g, ep=case == "b")
    model._resample_W(g["Y"])
    assert relerr(model.W, g[case + "_W_after"]) < 1e-10
    assert model.gass_info["accepted"].max() > 0
    np.testing.assert_array_equal(model.U, g["U0"])


def test_feature_updates_vs_reference_fixture(golden):
    g = golden("g16_row_features.npz")
    model, _ = _fixture_model(g)
    model.gass_ngrid = 100                       # (fit.py:130 calls gass with its default)
    model._resample_U()
    assert relerr(model.U, g["c_U_after"]) < 1e-10
    gi = model.gass_info
    assert set(gi) == {"valid", "unrestricted", "candidates", "accepted"} and gi["accepted"].max() > 0
    assert np.any(model.U != g["U0"], axis=1).all()
    np.testing.assert_array_equal(model.W, g["s0_W"])


# ---- 2. log-likelihood values ---------------------------------------------------------------------------------------
COUNTS = (1, 64, 65, 128)


def _small_problem(N, K, F, seed, M=2, T=4, ep=False, **kw):
    rs = np.random.RandomState(seed)
    W = rs.uniform(0.2, 1.0, size=(N, K))
    r, c = np.triu_indices(K, 1)
    W[r[r < N], c[r < N]] = 0
    V = np.zeros((M, T, K))
    V[:, -1] = rs.gamma(2.0, 0.5, size=(M, K))
    for t in range(T - 2, -1, -1):
        V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.3, size=(M, K))
    Y = rs.poisson(np.repeat(np.einsum("nk,mtk->nmt", W, V)[..., None], 2, axis=-1)).astype(float)
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    U = rs.uniform(0.05, 1.0, (F, K)) / (1.25 * W.sum(axis=1).max())
    X = (rs.rand(N, F) < 0.4).astype(float)
    X[rs.rand(N, F) < 0.1] = np.nan
    epa = None
    if ep:
        Mu = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.1, size=(N, M, T))
        epa = (Mu, 0.5 * 10.0 ** rs.uniform(0, 1, size=(N, M, T)))
    sigma2 = 0.7
    model = _cls()(N, M, T, "poisson_identity", Cons, ep_approx=epa, nembeds=K, tf_order=0, sigma2_init=sigma2, lam2_init=0.3,
                   W_init=W, V_init=V, Tau2_init=np.ones((M, T)), sampler="banded", row_features=X, feature_embeddings=U, **kw)
    return model, W, V, Y, U, X, epa, sigma2, rs


def _thetas(rs, nch, width):
    nth = np.array([COUNTS[c % 4] for c in range(nch)], dtype=np.int32)
    th = np.zeros((nch, 128))
    for c in range(nch):
        th[c, :nth[c]] = rs.uniform(-width, width, size=nth[c])
    return th, nth


def _check_ll(dev, ref, nth):
    for c in range(len(nth)):
        assert np.all(np.isneginf(dev[c, nth[c]:])), c
        d, r = dev[c, :nth[c]], ref[c]
        inf = np.isneginf(r)
        assert np.array_equal(np.isneginf(d), inf), c
        err = np.abs(d[~inf] - r[~inf]) / np.maximum(1.0, np.abs(r[~inf]))
        assert err.size == 0 or err.max() <= 1e-9, (c, err.max())


@pytest.mark.parametrize("F,K,ep", [(1, 3, False), (63, 3, False), (65, 3, False), (1025, 3, False), (65, 10, False), (63, 3, True)])
def test_row_chain_loglikelihoods_vs_numpy(F, K, ep):
    from oracle import btf_oracle as orc
    from scipy.stats import norm
    N = 12 if K == 10 else 6
    model, W, V, Y, U, X, epa, sigma2, rs = _small_problem(N, K, F, 100 + F + K, ep=ep)
    z = rs.normal(size=K * (K + 1) // 2 + (N - K) * K)
    u = rs.uniform(0.1, 0.9, size=N)
    info, mask, hh, cur = _begin(model, 0, Y, z, u)
    th, nth = _thetas(rs, N, 0.4)
    dev = _eval(model, 0, th, nth)
    ref, off = [], 0
    for i in range(N):
        d = min(K, i + 1)
        Vi = V[:, :, :d]
        if ep:
            p = 1.0 / epa[1][i] ** 2
            Q = np.einsum("jt,jtk,jtl->kl", p, Vi, Vi) + np.eye(d) / sigma2
            mu = np.linalg.solve(Q, np.einsum("jt,jtk->k", p * epa[0][i], Vi))
            nu = np.linalg.solve(np.linalg.cholesky(Q).T, z[off:off + d])
        else:
            mu, nu = np.zeros(d), np.sqrt(sigma2) * z[off:off + d]
        off += d

        def ll(w):
            tau = np.einsum("jtk,k->jt", Vi, w)
            v = orc.poisson_curves_loglik(Y[i], tau, "identity")
            if ep:
                v -= norm.logpdf(tau, epa[0][i], epa[1][i]).sum()
            return v + _side(X[i], U[:, :d] @ w)
        cands = (W[i, :d] - mu)[None] * np.cos(th[i, :nth[i], None]) + nu[None] * np.sin(th[i, :nth[i], None]) + mu[None]
        ref.append(np.array([ll(w) for w in cands]))
        c0 = ll(W[i, :d])
        assert abs(cur[i] - c0) <= 1e-9 * max(1.0, abs(c0)), (i, cur[i], c0)
        assert abs(hh[i] - (c0 + np.log(u[i]))) <= 1e-9 * max(1.0, abs(c0)), i
    _check_ll(dev, ref, nth)


@pytest.mark.parametrize("N,K", [(2, 3), (65, 3), (1030, 3), (65, 10)])
def test_feature_chain_loglikelihoods_vs_numpy(N, K):
    F = 9
    model, W, V, Y, U, X, _, _, rs = _small_problem(N, K, F, 200 + N + K)
    z = rs.normal(size=(F, K)) * 0.3 / W.sum(axis=1).max()
    u = rs.uniform(0.1, 0.9, size=F)
    info, mask, hh, cur = _begin(model, 2, None, z, u)
    th, nth = _thetas(rs, F, np.pi)
    dev = _eval(model, 2, th, nth)
    ref = []
    for f in range(F):
        cands = U[f][None] * np.cos(th[f, :nth[f], None]) + z[f][None] * np.sin(th[f, :nth[f], None])
        ref.append(_side(X[None, :, f], cands @ W.T))
        c0 = float(_side(X[:, f], W @ U[f]))
        assert abs(cur[f] - c0) <= 1e-9 * max(1.0, abs(c0)), (f, cur[f], c0)
        assert abs(hh[f] - (c0 + np.log(u[f]))) <= 1e-9 * max(1.0, abs(c0)), f
    _check_ll(dev, ref, nth)


def test_a_pair_at_exactly_zero():
    """p = w_i . u_f exactly 0 for every candidate (the zeros of W's leading rows against zeros in u_f and its proposal):
    x = 1 makes every candidate -inf, x = 0 contributes nothing."""
    N, K, F = 6, 3, 4
    model, W, V, Y, U, X, _, sigma2, rs = _small_problem(N, K, F, 7)
    U[1, :2] = 0.0
    U[2, :2] = 0.0
    X[:, :] = (rs.rand(N, F) < 0.5).astype(float)
    X[0, 1], X[1, 1] = 1.0, 0.0              # rows: pair (0, 1) is log(0), pair (1, 1) is 0 * log(0)
    X[0, 2], X[1, 2] = 0.0, 0.0              # features: chain 1 holds the log(0), chain 2 only dropped pairs
    model = _cls()(N, 2, 4, "poisson_identity", model._cons, nembeds=K, tf_order=0, sigma2_init=sigma2, lam2_init=0.3, W_init=W,
                   V_init=V, Tau2_init=np.ones((2, 4)), sampler="banded", row_features=X, feature_embeddings=U)
    # rows
    z = rs.normal(size=K * (K + 1) // 2 + (N - K) * K)
    info, mask, hh, cur = _begin(model, 0, Y, z, np.full(N, 0.5))
    th, nth = _thetas(rs, N, 0.3)
    dev = _eval(model, 0, th, nth)
    assert np.isneginf(cur[0]) and np.all(np.isneginf(dev[0]))
    assert np.all(np.isfinite(cur[1:]))
    X2 = X.copy()
    X2[1, 1] = np.nan                         # the dropped pair equals a missing one
    m2 = _cls()(N, 2, 4, "poisson_identity", model._cons, nembeds=K, tf_order=0, sigma2_init=sigma2, lam2_init=0.3, W_init=W,
                V_init=V, Tau2_init=np.ones((2, 4)), sampler="banded", row_features=X2, feature_embeddings=U)
    _begin(m2, 0, Y, z, np.full(N, 0.5))
    np.testing.assert_array_equal(_eval(m2, 0, th, nth)[1], dev[1])
    # features
    zf = rs.normal(size=(F, K)) * 0.2
    zf[1, :2] = 0.0
    zf[2, :2] = 0.0
    info, mask, hh, cur = _begin(model, 2, None, zf, np.full(F, 0.5))
    thf, nthf = _thetas(rs, F, np.pi)
    dev = _eval(model, 2, thf, nthf)
    assert np.isneginf(cur[1]) and np.all(np.isneginf(dev[1]))
    assert np.isfinite(cur[2])
    cands = U[2][None] * np.cos(thf[2, :nthf[2], None]) + zf[2][None] * np.sin(thf[2, :nthf[2], None])
    _check_ll(dev[2:3], [_side(X[None, :, 2], cands @ W.T)], nthf[2:3])


# ---- 3. valid grids -------------------------------------------------------------------------------------------------
def _feature_constraints(W):
    N = W.shape[0]
    return np.concatenate([W, -W], axis=0), np.concatenate([np.zeros(N), -np.ones(N)])


def test_valid_grids_of_the_fixture_chains_equal_the_oracles(golden):
    from oracle import btf_oracle as orc
    g = golden("g16_row_features.npz")
    model, (N, M, T, R, K, tf, F) = _fixture_model(g)
    full = np.linspace(-np.pi, np.pi, GRID)
    W, U = g["s0_W"], g["U0"]
    # feature chains, from the fixture's own streams
    z, u = np.empty((F, K)), np.empty(F)
    for f, r in enumerate(model.chain_rngs(2)):
        u[f] = r.random_sample()
        z[f] = r.normal(size=K)
    info, mask, _, _ = _begin(model, 2, None, z, u)
    A, c = _feature_constraints(W)
    for f in range(F):
        grid, restricted = orc.gass_valid_grid(U[f], z[f], A, c)
        assert bool(info[f, 1]) == (not restricted)
        if restricted:
            assert info[f, 0] == len(grid) and np.array_equal(full[mask[f] != 0], grid), f
    # row chains: the 2F derived rows behind the user's
    zr, ur, rows = [], np.empty(N), []
    for i, r in enumerate(model.chain_rngs(0)):
        ur[i] = r.random_sample()
        rows.append(r.normal(size=min(K, i + 1)))
    zr = np.concatenate(rows)
    info, mask, _, _ = _begin(model, 0, g["Y"], zr, ur)
    Rall = np.concatenate([g["Row_constraints"], np.concatenate([U, np.zeros((F, 1))], axis=1),
                           np.concatenate([-U, -np.ones((F, 1))], axis=1)], axis=0)
    for i in range(N):
        d = min(K, i + 1)
        Ci = orc.constrained_w_constraints(g["s0_V"], g["Cons"], d, Rall)
        grid, restricted = orc.gass_valid_grid(W[i, :d], np.sqrt(float(g["s0_sigma2"])) * rows[i], Ci[:, :-1], Ci[:, -1])
        assert bool(info[i, 1]) == (not restricted)
        if restricted:
            assert info[i, 0] == len(grid) and np.array_equal(full[mask[i] != 0], grid), i


def test_valid_grids_of_300_rows_equal_the_oracles():
    from oracle import btf_oracle as orc
    N, K, F = 300, 3, 5
    model, W, V, Y, U, X, _, _, rs = _small_problem(N, K, F, 31)
    full = np.linspace(-np.pi, np.pi, GRID)
    z = rs.normal(size=(F, K))
    info, mask, _, _ = _begin(model, 2, None, z, np.full(F, 0.5))
    A, c = _feature_constraints(W)
    for f in range(F):
        grid, restricted = orc.gass_valid_grid(U[f], z[f], A, c)
        assert restricted and not info[f, 1]
        dev = full[mask[f] != 0]
        assert info[f, 0] == len(dev)
        # (an arc end within 1e-9 of a grid angle: one boundary angle may differ, as for the columns)
        assert abs(len(dev) - len(grid)) <= 2 and len(np.setxor1d(dev, grid)) <= 2, f


# ---- 4. stationary distribution of the U step -----------------------------------------------------------------------
def test_feature_chains_sample_the_truncated_posterior():
    """256 identical features, 40 device-mode U steps, the last 20 kept: the per-chain averages of u and u^2 against a
    1401 x 1401 quadrature of N(0, I) x Bernoulli on {0 <= W u <= 1}; |mean - quadrature| <= 5 sd / sqrt(256).  (The
    oracle's gass, 512 chains, same schedule: z = 0.29, 0.41, 0.86, 2.15.)"""
    K, N, F = 2, 12, 256
    W = np.random.RandomState(3).uniform(0.2, 1.0, (N, K))
    W[0, 1] = 0
    x = np.array([1, 0, 0, 1, np.nan, 0, 1, 0, 0, np.nan, 1, 0], dtype=float)
    # quadrature
    ax = np.linspace(-0.5, 3.0, 1401)
    g1, g2 = np.meshgrid(ax, ax, indexing="ij")
    P = g1[..., None] * W[:, 0] + g2[..., None] * W[:, 1]
    ok = np.all((P >= 0) & (P <= 1), axis=-1)
    with np.errstate(all="ignore"):
        ll = np.nansum(x * np.log(P) + (1 - x) * np.log(1 - P), axis=-1) - 0.5 * (g1 ** 2 + g2 ** 2)
    dens = np.where(ok, np.exp(ll), 0.0)
    dens /= dens.sum()
    quad = np.array([(dens * g1).sum(), (dens * g2).sum(), (dens * g1 ** 2).sum(), (dens * g2 ** 2).sum()])
    print("quadrature", quad)
    assert np.allclose(quad, [0.6511, 0.0327, 0.5081, 0.0588], atol=2e-4)
    M, T = 2, 3
    V = np.ones((M, T, K))
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    model = _cls()(N, M, T, "poisson_identity", Cons, nembeds=K, tf_order=0, W_true=W, V_true=V, rng="device", device_seed=11,
                   row_features=np.repeat(x[:, None], F, axis=1), feature_embeddings=np.full((F, K), 0.3))
    assert not model.sample_W and not model.sample_V
    acc = np.zeros((F, 4))
    for it in range(40):
        model._resample_U()
        if it >= 20:
            U = model.U
            acc += np.concatenate([U, U ** 2], axis=1) / 20.0
    zs = (acc.mean(axis=0) - quad) / (acc.std(axis=0, ddof=1) / np.sqrt(F))
    print("z", zs)
    assert np.all(np.abs(zs) <= 5.0), zs


# ---- 5. whole chains ------------------------------------------------------------------------------------------------
def _chain_problem(lik_name, **kw):
    N, M, T, R, K, F = 12, 6, 8, 2, 3, 5
    rs = np.random.RandomState(41)
    if lik_name == "gamma_grid":
        from test_gpu_gamma_grid import _problem, _fit_constraints
        W, V, Y, lik, _ = _problem(N, M, T, R, K, 7, 5)
        W[np.triu_indices(K, 1)] = 0
        Cons, par = _fit_constraints(T), lik
    else:
        W = rs.gamma(2.0, 0.5, size=(N, K)) + 0.1
        W[np.triu_indices(K, 1)] = 0
        V = np.zeros((M, T, K))
        V[:, -1] = rs.gamma(2.0, 0.5, size=(M, K))
        for t in range(T - 2, -1, -1):
            V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.3, size=(M, K)) * (rs.rand(M, 1) < 0.5)
        Y = rs.poisson(np.repeat(np.einsum("nk,mtk->nmt", W, V)[..., None], R, axis=-1)).astype(float)
        Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
        mono = np.array([np.concatenate([np.zeros(t), [1, -1], np.zeros(T - t - 2), [-1e-2]]) for t in range(T - 1)])
        Cons, par = np.concatenate([Cons, mono], axis=0), None
    U = rs.uniform(0.05, 1.0, (F, K)) / (1.25 * W.sum(axis=1).max())
    P = W @ U.T
    X = (rs.rand(N, F) < P / P.max() * 0.8 + 0.1).astype(float)
    X[3, 2] = np.nan
    Rc = np.array([[1.0, 0.0, 0.0, -1e-3]])

    def make(**kw2):
        np.random.seed(6)
        args = dict(likelihood_param=par, Row_constraints=Rc, gass_ngrid=32, nembeds=K, tf_order=1, W_init=W.copy(),
                    V_init=V.copy(), rng="device", device_seed=9, row_features=kw2.pop("X", X), feature_embeddings=U.copy())
        args.update(kw)
        args.update(kw2)
        return _cls()(N, M, T, lik_name, Cons, **args)
    return make, (W, V, Y, U, X, Cons, Rc)


def _feasible(model, Cons, Rc, it):
    W, V, U = model.W, model.V, model.U
    P = W @ U.T
    assert P.min() >= -1e-9 and P.max() <= 1 + 1e-9, (it, P.min(), P.max())
    tau = np.einsum("nk,mtk->nmt", W, V)
    assert (np.einsum("qt,nmt->nmq", Cons[:, :-1], tau) >= Cons[:, -1] - 1e-9).all(), it
    assert (W @ Rc[:, :-1].T >= Rc[:, -1] - 1e-9).all(), it


@pytest.mark.parametrize("lik_name", ["poisson_identity", "gamma_grid"])
def test_whole_chain_stays_feasible_collects_and_restores(lik_name):
    make, (W, V, Y, U, X, Cons, Rc) = _chain_problem(lik_name)
    model = make()
    for it in range(10):
        model.resample(Y)
        _feasible(model, Cons, Rc, it)
    st = model.checkpoint()
    assert st["U"].shape == U.shape
    fresh = make()
    fresh.restore(st)
    for it in range(5):
        model.resample(Y)
        fresh.resample(Y)
        for name in ("W", "V", "U"):
            np.testing.assert_array_equal(getattr(model, name), getattr(fresh, name), err_msg=name)
    for it in range(15, 30):
        model.resample(Y)
        _feasible(model, Cons, Rc, it)
    assert np.any(model.U != U) and np.any(model.W != W)
    res = model.run_gibbs(Y, nburn=1, nthin=1, nsamples=3, verbose=False)
    assert res["U"].shape == (3, U.shape[0], U.shape[1])
    np.testing.assert_array_equal(res["U"][-1], model.U)
    assert np.any(res["U"][0] != res["U"][-1])


def test_fixed_features_and_an_all_missing_column():
    from functionalmf_amd import _native
    make, (W, V, Y, U, X, Cons, Rc) = _chain_problem("poisson_identity")
    model = make(sample_features=False)
    assert model.sample_U is False
    for it in range(5):
        model.resample(Y)
    np.testing.assert_array_equal(model.U, U)
    assert np.any(model.W != W)
    _feasible(model, Cons, Rc, 5)
    # a feature nobody observed: its likelihood is constant, every candidate is on the slice
    X2 = X.copy()
    X2[:, 1] = np.nan
    model = make(X=X2)
    model._push_state()
    model._push_features()
    F, ngrid = X.shape[1], 32
    model._ctx.call("btf_gass_begin", 2, model._link, None, None, 77, 1e-6, 0, ngrid)
    info = np.zeros((F, 2), dtype=np.int32)
    model._ctx.call("btf_gass_grid", 2, info.ctypes.data_as(_native._c_ip), None, None, None)
    model._ctx.call("btf_gass_eval", 2, None, None, None)
    nacc = np.zeros(F, dtype=np.int32)
    model._ctx.call("btf_gass_select", 2, 77, nacc.ctypes.data_as(_native._c_ip))
    cand = np.where(info[:, 1] != 0, ngrid, np.minimum(info[:, 0], ngrid))
    assert cand[1] > 0 and nacc[1] == cand[1], (nacc, cand)
    assert np.all(nacc <= cand)
    host = make(X=X2, rng="host")
    host.chain_rngs = lambda what: [np.random.RandomState(50 + c) for c in range((12, 6, F)[what])]
    host._resample_U()
    gi = host.gass_info
    assert gi["candidates"][1] > 0 and gi["accepted"][1] == gi["candidates"][1]


# ---- 6. no features, no change --------------------------------------------------------------------------------------
def test_without_features_nothing_changes(golden):
    from functionalmf_amd import _native
    make, (W, V, Y, U, X, Cons, Rc) = _chain_problem("poisson_identity")
    N, M, T, K = 12, 6, 8, 3
    runs = []
    for explicit in (False, True):
        np.random.seed(6)
        kw = dict(row_features=None, feature_embeddings=None, sample_features=True) if explicit else {}
        model = _cls()(N, M, T, "poisson_identity", Cons, Row_constraints=Rc, gass_ngrid=32, nembeds=K, tf_order=1, W_init=W.copy(),
                       V_init=V.copy(), rng="device", device_seed=9, **kw)
        counts = []
        for it in range(4):
            before = {k: n for k, (_, n) in model._ctx.kernel_times().items()}
            model.resample(Y)
            after = {k: n for k, (_, n) in model._ctx.kernel_times().items()}
            counts.append({k: after[k] - before[k] for k in after})
        runs.append((model.W.copy(), model.V.copy(), counts))
        assert model.U is None and model.sample_U is False
        with pytest.raises(_native.BTFError) as e:
            model._ctx.call("btf_gass_begin", 2, model._link, None, None, 1, 1e-6, 0, 8)
        assert e.value.code == _native.BTF_ESTATE
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]
    # the launches of a sweep without features, as counted before this feature existed: per GASS step of the rows
    # (prior draw, likelihood of the state, slice, av, analysis, eval, select) and nothing of the feature kernels
    withf = make()
    before = {k: n for k, (_, n) in withf._ctx.kernel_times().items()}
    withf.resample(Y)
    after = {k: n for k, (_, n) in withf._ctx.kernel_times().items()}
    extra = (after["ess"] - before["ess"]) - runs[0][2][0]["ess"]
    assert extra == 4 + 5, extra     # rows: state term, its fix, derived rows, candidates' term; U step: analysis, state, slice, eval, select


def test_the_example_runs_from_the_nmf_start_to_a_chain_that_returns_U():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("doseresponse_row_features", os.path.join(ROOT, "examples", "doseresponse_row_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    results, (fit0, fit1) = mod.main(seed=3, nburn=10, nsamples=10, n=16, m=8, nfeatures=4, verbose=False)
    assert results["U"].shape == (10, 4, 3) and np.any(results["U"][0] != results["U"][-1])
    P = np.einsum("snk,sfk->snf", results["W"], results["U"])
    assert P.min() >= -1e-9 and P.max() <= 1 + 1e-9
    assert np.isfinite(fit0) and np.isfinite(fit1)
