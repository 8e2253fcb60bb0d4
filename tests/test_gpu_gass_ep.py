"""EP-centred GASS updates (ep_approx) on the GPU: the reference's own updates (tests/golden/g13_gass_ep.npz), the centre
at full size against numpy solves, the exact-Gaussian invariance, the limits, and device-mode chains."""
import ctypes

import numpy as np
import pytest
from scipy.special import gammaln

from conftest import relerr

pytestmark = pytest.mark.gpu


def _model(g, case, **kw):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    N, M, T, R, K, tf = [int(x) for x in g["dims"]]
    ep = None if case is None else (g[case + "_Mu_ep"], g[case + "_Sigma_ep"])
    model = ConstrainedNonconjugateBayesianTensorFiltering(
        N, M, T, "poisson_identity", g["Cons"], ep_approx=ep, Row_constraints=g["Row_constraints"], gass_ngrid=int(g["ngrid"]),
        nembeds=K, tf_order=tf, sigma2_init=float(g["s0_sigma2"]), lam2_init=float(g["s0_lam2"]), W_init=g["s0_W"].copy(),
        V_init=g["s0_V"].copy(), Tau2_init=g["s0_Tau2"].copy(), sampler="banded", **kw)
    model.chain_rngs = lambda what: [np.random.RandomState((2000 if what == 0 else 3000) + c) for c in range(N if what == 0 else M)]
    return model, (N, M, T, R, K, tf)


def _cur_ll(model, what, Y):
    """btf_gass_grid's cur_ll after a begin (it does not depend on the proposal or the slice uniform)."""
    from functionalmf_amd import _native
    model._bind_data(Y)
    model._push_state()
    rc = model.Row_constraints
    model._ctx.call("btf_gass_set_constraints", _native.dptr(model._cons), int(model._cons.shape[0]), _native.dptr(rc),
                    0 if rc is None else int(rc.shape[0]))
    model._cons_set = True
    model._push_ep()
    N, M, T, K = model.nrows, model.ncols, model.ndepth, model.nembeds
    nch = N if what == 0 else M
    z = np.zeros(K * (K + 1) // 2 + (N - K) * K) if what == 0 else np.zeros((M, K * T))
    u = np.full(nch, 0.5)
    model._ctx.call("btf_gass_begin", what, model._link, _native.dptr(z), _native.dptr(u), 1, 1e-6, 0, 0)
    info = np.zeros((nch, 2), dtype=np.int32)
    cur = np.empty(nch)
    model._ctx.call("btf_gass_grid", what, info.ctypes.data_as(_native._c_ip), None, None, _native.dptr(cur))
    return cur


@pytest.mark.parametrize("case", ["a", "b"])
def test_ep_updates_vs_reference_fixture(golden, case):
    g = golden("g13_gass_ep.npz")
    Y = g["Y"]
    model, (N, M, T, R, K, tf) = _model(g, case)
    model._resample_W(Y)
    assert relerr(model.W, g[case + "_W_after"]) < 1e-10
    acc_w = model.gass_info["accepted"].copy()
    model.W = g["s0_W"].copy()
    model._resample_V(Y)
    assert relerr(model.V, g[case + "_V_after"]) < 1e-7
    assert max(acc_w.max(), model.gass_info["accepted"].max()) > 0
    # corrected log-likelihood of the current state: the device leaves out - sum lgamma(y + 1) of the observed entries
    lg = np.where(np.isnan(Y), 0.0, gammaln(np.nan_to_num(Y) + 1.0))
    m2, _ = _model(g, case)
    cw = _cur_ll(m2, 0, Y) - lg.sum(axis=(1, 2, 3))
    assert np.max(np.abs(cw - g[case + "_cur_w"]) / np.abs(g[case + "_cur_w"])) < 1e-10
    cv = _cur_ll(m2, 1, Y) - lg.sum(axis=(0, 2, 3))
    assert np.max(np.abs(cv - g[case + "_cur_v"]) / np.abs(g[case + "_cur_v"])) < 1e-10


def test_limits_wide_ep_equals_plain_and_cleared_ep_is_the_plain_path(golden):
    g = golden("g13_gass_ep.npz")
    Y = g["Y"]
    plain, dims = _model(g, None)
    plain._resample_W(Y)
    plain._resample_V(Y)
    wide, _ = _model(g, "a")
    wide.Mu_ep, wide.Sigma_ep = g["a_Mu_ep"], np.full(g["a_Mu_ep"].shape, 1e8)
    wide._resample_W(Y)
    wide._resample_V(Y)
    assert relerr(wide.W, plain.W) < 1e-8
    assert relerr(wide.V, plain.V) < 1e-8
    cleared, _ = _model(g, "b")
    cleared._resample_W(Y)                  # one EP-centred update, then back to the start without EP
    cleared.W, cleared.V = g["s0_W"].copy(), g["s0_V"].copy()
    cleared.Mu_ep, cleared.Sigma_ep = None, None
    cleared._resample_W(Y)
    cleared._resample_V(Y)
    np.testing.assert_array_equal(cleared.W, plain.W)
    np.testing.assert_array_equal(cleared.V, plain.V)


def _poisson_problem(N, M, T, K, tf, seed):
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    W[np.triu_indices(K, 1)] = 0
    V = np.zeros((M, T, K))
    V[:, -1] = rs.gamma(2.0, 0.5, size=(M, K))
    for t in range(T - 2, -1, -1):
        V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.3, size=(M, K)) * (rs.rand(M, 1) < 0.5)
    rate = np.einsum("nk,mtk->nmt", W, V)
    Y = rs.poisson(np.repeat(rate[..., None], 2, axis=-1)).astype(float)
    Y[rs.rand(*Y.shape) < 0.05] = np.nan
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    mono = np.array([np.concatenate([np.zeros(t), [1, -1], np.zeros(T - t - 2), [-1e-2]]) for t in range(T - 1)])
    Cons = np.concatenate([Cons, mono], axis=0)
    Tau2 = rs.gamma(2.0, 0.5, size=(M, T + tf + 1 if tf >= 0 else T))
    return W, V, Y, Cons, Tau2, rs


def test_centre_at_full_size_matches_numpy_solves():
    """(512,256,64) K=5, z = 0, theta = pi/2 committed everywhere: W (then V) becomes the centre mu."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd import _native, utils
    N, M, T, K, tf = 512, 256, 64, 5, 1
    W, V, Y, Cons, _, rs = _poisson_problem(N, M, T, K, tf, 5)
    Delta = utils.bayes_grid_penalty(T, tf).toarray()
    Tau2 = rs.gamma(4.0, 0.5, size=(M, Delta.shape[0]))
    with np.errstate(all="ignore"):
        Mu_ep = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.1, size=(N, M, T))
    Sig = 0.5 * 10.0 ** rs.uniform(0, 1, size=(N, M, T))
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", Cons, ep_approx=(Mu_ep, Sig), nembeds=K,
                                                           tf_order=tf, sigma2_init=0.7, lam2_init=0.3, W_init=W, V_init=V,
                                                           Tau2_init=Tau2, sampler="banded")
    _cur_ll(model, 0, Y)
    p = 1.0 / Sig ** 2
    for what in (0, 1):
        nch = N if what == 0 else M
        if what == 1:
            _cur_ll(model, 1, Y)
        th = np.full(nch, np.pi / 2)
        keep = np.zeros(nch, dtype=np.int32)
        model._ctx.call("btf_gass_commit", what, _native.dptr(th), keep.ctypes.data_as(_native._c_ip))
        model._W_dev_new = model._V_dev_new = True
        if what == 0:
            Wg = model.W
            for i in list(range(32)) + list(range(N - 8, N)):
                d = min(K, i + 1)
                Vi = V[:, :, :d]
                Q = np.einsum("jt,jtk,jtl->kl", p[i], Vi, Vi) + np.eye(d) / 0.7
                mu = np.linalg.solve(Q, np.einsum("jt,jtk->k", p[i] * Mu_ep[i], Vi))
                assert np.max(np.abs(Wg[i, :d] - mu)) <= 1e-11 * np.max(np.abs(mu)), i
            model.W = W                      # the columns from the starting W
        else:
            Vg = model.V
            for j in range(0, M, M // 16):
                DLD = Delta.T @ np.diag(1.0 / (0.3 * Tau2[j])) @ Delta
                Q = np.kron(np.eye(K), DLD)
                X = np.kron(W, np.eye(T))
                pj = p[:, j].reshape(-1)
                Q = Q + X.T @ (pj[:, None] * X)
                mu = np.linalg.solve(Q, X.T @ (pj * Mu_ep[:, j].reshape(-1)))
                got = Vg[j].T.reshape(-1)
                tol = 50 * np.linalg.cond(Q) * np.finfo(float).eps
                assert np.max(np.abs(got - mu)) <= tol * np.max(np.abs(mu)), (j, np.max(np.abs(got - mu)) / np.max(np.abs(mu)), tol)


def _gaussian_problem(N, M, T, K, tf, s, seed, Cons=None, **kw):
    """Gaussian data (variance s2, 4 replicates, 5 % missing, no empty cell) and the constrained model with the "gaussian"
    device likelihood whose ep_approx is the exact per-cell fit: Mu_ep = the replicate mean, Sigma_ep = s / sqrt(n)."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    R = 4
    W, V, _, Cons0, _, rs = _poisson_problem(N, M, T, K, tf, seed)
    Cons = Cons0 if Cons is None else Cons
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, s, size=(N, M, T, R))
    Y[rs.rand(N, M, T, R) < 0.05] = np.nan
    Y[..., 0] = np.where(np.isnan(Y[..., 0]), 1.0, Y[..., 0])
    n = (~np.isnan(Y)).sum(axis=-1)
    Mu_ep = np.nanmean(Y, axis=-1)
    Sig = s / np.sqrt(n)
    from functionalmf_amd import utils
    Tau2 = rs.gamma(4.0, 0.5, size=(M, utils.bayes_grid_penalty(T, tf).shape[0]))
    np.random.seed(seed)
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "gaussian", Cons, ep_approx=(Mu_ep, Sig), nembeds=K, tf_order=tf,
                                                           likelihood_param=s * s, sigma2_init=0.8, lam2_init=0.3, W_init=W,
                                                           V_init=V, Tau2_init=Tau2, sampler="banded", **kw)
    return model, Y, W, V, Mu_ep, Sig, Tau2


def test_exact_gaussian_likelihood_makes_every_candidate_equal():
    """Gaussian likelihood with variance s2 and Mu_ep / Sigma_ep its exact per-cell fit: the corrected likelihood is
    constant in (W, V), so every candidate's ll equals cur_ll, and in a host-driven update (grid, eval, selection and
    commit) every candidate is above the slice of every chain whose log u < -1e-6."""
    from functionalmf_amd import _native
    N, M, T, K, tf, s = 24, 12, 10, 3, 1, 0.7
    model, Y = _gaussian_problem(N, M, T, K, tf, s, 9, gass_ngrid=64)[:2]
    for what in (0, 1):
        cur = _cur_ll(model, what, Y)
        nch = N if what == 0 else M
        ths = np.zeros((nch, 128))
        ths[:, :64] = np.linspace(-np.pi, np.pi, 64)
        nth = np.full(nch, 64, dtype=np.int32)
        ll = np.empty((nch, 128))
        model._ctx.call("btf_gass_eval", what, _native.dptr(ths), nth.ctypes.data_as(_native._c_ip), _native.dptr(ll))
        err = np.abs(ll[:, :64] - cur[:, None]) / np.abs(cur[:, None])
        assert err.max() < 1e-9, (what, err.max())
    model.chain_rngs = lambda what: [np.random.RandomState((40 if what == 0 else 50) + c) for c in range(N if what == 0 else M)]
    for what in (0, 1):
        nch = N if what == 0 else M
        logu = np.log([np.random.RandomState((40 if what == 0 else 50) + c).random_sample() for c in range(nch)])
        before = (model.W if what == 0 else model.V).copy()
        (model._resample_W if what == 0 else model._resample_V)(Y)
        gi = model.gass_info
        sel = logu < -1e-6
        assert sel.sum() >= nch // 2 and np.all(gi["candidates"][sel] > 0)
        np.testing.assert_array_equal(gi["accepted"][sel], gi["candidates"][sel])
        after = model.W if what == 0 else model.V
        moved = np.any((after != before).reshape(nch, -1), axis=1)
        assert np.all(moved[sel])


def _device_chain(seed, sweeps):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd import utils
    N, M, T, K, tf = 64, 32, 16, 3, 1
    W, V, Y, Cons, _, rs = _poisson_problem(N, M, T, K, tf, 11)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        Mu_ep, Sig = utils.ep_from_mf(Y, W, V, mode="multiplier", multiplier=3)
    np.random.seed(3)                        # (the starting hyper-parameters come from the legacy generator)
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", Cons, ep_approx=(Mu_ep, Sig), nembeds=K,
                                                           tf_order=tf, gass_ngrid=50, sigma2_init=1.0, lam2_init=0.3, W_init=W,
                                                           V_init=V, sampler="banded", rng="device", device_seed=seed)
    for _ in range(sweeps):
        model._resample_W(Y)
        model._resample_V(Y)
    return model, Cons


def test_device_mode_is_deterministic_and_stays_feasible():
    a, Cons = _device_chain(7, 3)
    b, _ = _device_chain(7, 3)
    np.testing.assert_array_equal(a.W, b.W)
    np.testing.assert_array_equal(a.V, b.V)
    m, _ = _device_chain(8, 50)
    tau = np.einsum("nk,mtk->nmt", m.W, m.V)
    lhs = np.einsum("ct,nmt->nmc", Cons[:, :-1], tau)
    assert np.all(lhs - Cons[:, -1] >= -1e-9), (lhs - Cons[:, -1]).min()
    W0, V0 = _poisson_problem(64, 32, 16, 3, 1, 11)[:2]
    assert np.all(np.any(m.W != W0, axis=1)) and np.all(np.any(m.V.reshape(32, -1) != V0.reshape(32, -1), axis=1))


def _batch_z(x, mean, var, nb=39):
    """z-scores of the chain's mean and of its mean squared deviation from `mean` against (mean, var), standard errors
    from nb batch means (x: [samples, ...])."""
    b = x[: (x.shape[0] // nb) * nb].reshape((nb, -1) + x.shape[1:])
    m = b.mean(axis=1)
    q = ((b - mean) ** 2).mean(axis=1)
    zm = (m.mean(axis=0) - mean) / (m.std(axis=0, ddof=1) / np.sqrt(nb))
    zv = (q.mean(axis=0) - var) / (q.std(axis=0, ddof=1) / np.sqrt(nb))
    return zm, zv


def test_device_mode_draws_the_exact_gaussian_conditionals():
    """rng="device", a constraint that never binds and the exact-Gaussian EP fit: every GASS update is then a draw-and-
    rotate on N(mu, Q^-1), the exact conditional.  4000 W updates against a fixed V (then 4000 V updates against a fixed
    W): per-entry mean and variance within z-score 5 of the numpy N(mu_i, Q_i^-1) (rows, truncated rows included) and
    N(mu_j, Q_j^-1) (columns, dense Q of the reference formula), standard errors by batch means."""
    from functionalmf_amd import utils
    N, M, T, K, tf, s = 12, 6, 8, 3, 1, 0.7
    Cons = np.concatenate([np.zeros((1, T)), [[-1e6]]], axis=1)
    Cons[0, 0] = 1.0
    model, Y, W, V, Mu_ep, Sig, Tau2 = _gaussian_problem(N, M, T, K, tf, s, 21, Cons=Cons, gass_ngrid=16, rng="device",
                                                         device_seed=5)
    p = 1.0 / Sig ** 2
    nkeep, burn = 3900, 100
    xs = []
    for it in range(burn + nkeep):
        model._resample_W(Y)
        if it >= burn:
            xs.append(model.W.copy())
    xs = np.array(xs)
    for i in range(N):
        d = min(K, i + 1)
        Q = np.einsum("jt,jtk,jtl->kl", p[i], V[:, :, :d], V[:, :, :d]) + np.eye(d) / 0.8
        mu = np.linalg.solve(Q, np.einsum("jt,jtk->k", p[i] * Mu_ep[i], V[:, :, :d]))
        zm, zv = _batch_z(xs[:, i, :d], mu, np.diag(np.linalg.inv(Q)))
        assert np.all(np.abs(zm) < 5) and np.all(np.abs(zv) < 5), (i, zm, zv)
        assert np.all(xs[:, i, d:] == 0)
    model.W = W
    xs = []
    for it in range(burn + nkeep):
        model._resample_V(Y)
        if it >= burn:
            xs.append(model.V.copy())
    xs = np.array(xs)
    Delta = utils.bayes_grid_penalty(T, tf).toarray()
    X = np.kron(W, np.eye(T))
    for j in range(M):
        Q = np.kron(np.eye(K), Delta.T @ np.diag(1.0 / (0.3 * Tau2[j])) @ Delta)
        pj = p[:, j].reshape(-1)
        Q = Q + X.T @ (pj[:, None] * X)
        mu = np.linalg.solve(Q, X.T @ (pj * Mu_ep[:, j].reshape(-1)))
        got = xs[:, j].transpose(0, 2, 1).reshape(nkeep, -1)          # k-major, as mu
        zm, zv = _batch_z(got, mu, np.diag(np.linalg.inv(Q)))
        assert np.all(np.abs(zm) < 5) and np.all(np.abs(zv) < 5), (j, np.abs(zm).max(), np.abs(zv).max())


def _envelope_size(T, K, tf):
    """Entries of the column system's envelope in the twisted order (btf_gass_set_ep's host computation, restated)."""
    S = tf + 1
    n, ts = T * K, (T - S) // 2
    nl, nsep = ts * K, T * K - S * K

    def pos(g):
        return g if g < nl else (nl + (n - 1 - g) if g >= nl + S * K else nsep + (g - nl))

    order = [r if r < nl else (n - 1 - (r - nl) if r < nsep else nl + (r - nsep)) for r in range(n)]
    tot = 0
    for r, g in enumerate(order):
        t, k = divmod(g, K)
        nb = [pos(t * K + l) for l in range(K)] + [pos((t + d) * K + k) for d in range(1, S + 1) if t + d < T] + \
             [pos((t - d) * K + k) for d in range(1, S + 1) if t - d >= 0]
        tot += r - min([r] + nb) + 1
    return tot


def test_column_centre_with_the_envelope_in_hbm():
    """K=10, T=64, tf_order=1: the envelope of the column systems does not fit on chip beside the vectors (env_g);
    the centre (z = 0, theta = pi/2 committed) still matches the dense numpy solve of every column."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd import _native, utils
    N, M, T, K, tf = 12, 6, 64, 10, 1
    n = T * K
    assert 8 * (_envelope_size(T, K, tf) + 6 * n + T * K * (K + 1) // 2) > 150 * 1024
    W, V, Y, _, _, rs = _poisson_problem(N, M, T, K, tf, 13)
    Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    Delta = utils.bayes_grid_penalty(T, tf).toarray()
    Tau2 = rs.gamma(4.0, 0.5, size=(M, Delta.shape[0]))
    Mu_ep = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.1, size=(N, M, T))
    Sig = 0.5 * 10.0 ** rs.uniform(0, 1, size=(N, M, T))
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", Cons, ep_approx=(Mu_ep, Sig), nembeds=K,
                                                           tf_order=tf, sigma2_init=0.7, lam2_init=0.3, W_init=W, V_init=V,
                                                           Tau2_init=Tau2, sampler="banded")
    _cur_ll(model, 1, Y)
    th = np.full(M, np.pi / 2)
    keep = np.zeros(M, dtype=np.int32)
    model._ctx.call("btf_gass_commit", 1, _native.dptr(th), keep.ctypes.data_as(_native._c_ip))
    model._V_dev_new = True
    Vg = model.V
    p = 1.0 / Sig ** 2
    X = np.kron(W, np.eye(T))
    for j in range(M):
        Q = np.kron(np.eye(K), Delta.T @ np.diag(1.0 / (0.3 * Tau2[j])) @ Delta)
        pj = p[:, j].reshape(-1)
        Q = Q + X.T @ (pj[:, None] * X)
        mu = np.linalg.solve(Q, X.T @ (pj * Mu_ep[:, j].reshape(-1)))
        got = Vg[j].T.reshape(-1)
        tol = 50 * np.linalg.cond(Q) * np.finfo(float).eps
        assert np.max(np.abs(got - mu)) <= tol * np.max(np.abs(mu)), (j, np.max(np.abs(got - mu)) / np.max(np.abs(mu)), tol)
