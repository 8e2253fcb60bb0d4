"""The gamma-grid likelihood (loglikelihood="gamma_grid") on the GPU: the reference's own constrained updates
(tests/golden/g14_gamma_grid.npz), the whole-state and candidate log-likelihoods against the host class, table
invariances, the edge cases, determinism and feasibility of device-driven chains."""
import types

import numpy as np
import pytest
from scipy.stats import gamma as gamma_dist

from conftest import relerr

pytestmark = pytest.mark.gpu


def _fit_constraints(T):
    """doseresponse/fit.py:58-61: positivity, at most one, monotone with slack 1e-2."""
    C_zero = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(T - i - 2), [-1e-2]]) for i in range(T - 1)])
    C_one = np.concatenate([np.eye(T) * -1, np.full((T, 1), -1)], axis=1)
    return np.concatenate([C_zero, C_one, C_mono], axis=0)


def _param(g):
    return (g["mean_grid"], g["mean_probs"], float(g["variance"]))


def _fixture_model(g, ep, **kw):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    N, M, T, R, K, tf = [int(x) for x in g["dims"]]
    model = ConstrainedNonconjugateBayesianTensorFiltering(
        N, M, T, "gamma_grid", g["Cons"], likelihood_param=_param(g), ep_approx=(g["Mu_ep"], g["Sigma_ep"]) if ep else None,
        gass_ngrid=int(g["ngrid"]), nembeds=K, tf_order=tf, sigma2_init=float(g["s0_sigma2"]), lam2_init=float(g["s0_lam2"]),
        W_init=g["s0_W"].copy(), V_init=g["s0_V"].copy(), Tau2_init=g["s0_Tau2"].copy(), sampler="banded", **kw)
    model.chain_rngs = lambda what: [np.random.RandomState((2000 if what == 0 else 3000) + c) for c in range(N if what == 0 else M)]
    return model


def _begin(model, what, Y, z=None):
    """btf_gass_begin with the given (or zero) normals and u = 0.5; returns cur_ll of every chain."""
    from functionalmf_amd import _native
    model._bind_data(Y)
    model._push_state()
    model._ctx.call("btf_gass_set_constraints", _native.dptr(model._cons), int(model._cons.shape[0]), None, 0)
    model._cons_set = True
    if hasattr(model, "_push_ep"):
        model._push_ep()
    N, M, T, K = model.nrows, model.ncols, model.ndepth, model.nembeds
    nch = N if what == 0 else M
    if z is None:
        z = np.zeros(K * (K + 1) // 2 + (N - K) * K) if what == 0 else np.zeros((M, K * T))
    u = np.full(nch, 0.5)
    model._ctx.call("btf_gass_begin", what, model._link, _native.dptr(z), _native.dptr(u), 1, 1e-6, 0, 0)
    info = np.zeros((nch, 2), dtype=np.int32)
    cur = np.empty(nch)
    model._ctx.call("btf_gass_grid", what, info.ctypes.data_as(_native._c_ip), None, None, _native.dptr(cur))
    return cur


@pytest.mark.parametrize("ep", [False, True])
def test_updates_vs_reference_fixture(golden, ep):
    g = golden("g14_gamma_grid.npz")
    Y, case = g["Y"], "ep" if ep else "plain"
    model = _fixture_model(g, ep)
    model._resample_W(Y)
    assert relerr(model.W, g[case + "_W_after"]) < 1e-10
    model.W = g["s0_W"].copy()
    model._resample_V(Y)
    assert relerr(model.V, g[case + "_V_after"]) < 1e-7
    m2 = _fixture_model(g, ep)
    cw = _begin(m2, 0, Y)
    assert np.max(np.abs(cw - g[case + "_cur_w"]) / np.abs(g[case + "_cur_w"])) < 1e-10
    cv = _begin(m2, 1, Y)
    assert np.max(np.abs(cv - g[case + "_cur_v"]) / np.abs(g[case + "_cur_v"])) < 1e-10


def _problem(N, M, T, R, K, G, seed, missing=0.05):
    from functionalmf_amd.likelihoods import GammaGridLikelihood
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    V = np.zeros((M, T, K))
    V[:, -1] = rs.gamma(2.0, 0.2, size=(M, K))
    for t in range(T - 2, -1, -1):
        V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.2, size=(M, K)) * (rs.rand(M, 1) < 0.5)
    W *= 0.95 / np.einsum("nk,mtk->nmt", W, V).max()
    lik = GammaGridLikelihood(np.linspace(0.6, 1.4, G), rs.gamma(2.0, 0.5, size=G), 0.03)
    eta = np.einsum("nk,mtk->nmt", W, V)
    comp = rs.choice(G, size=eta.shape, p=lik.probs_grid / lik.probs_grid.sum())
    Y = rs.gamma(lik.shape_grid[comp][..., None], (lik.scale_grid[comp] * eta)[..., None], size=eta.shape + (R,))
    Y[rs.rand(*Y.shape) < missing] = np.nan
    return W, V, Y, lik, rs


def _nonconj(N, M, T, K, lik, W, V, **kw):
    from functionalmf_amd.factor import NonconjugateBayesianTensorFiltering
    return NonconjugateBayesianTensorFiltering(N, M, T, "gamma_grid", likelihood_param=lik, nembeds=K, W_init=W, V_init=V, **kw)


def _host_ll(lik, Y, W, V):
    return float(lik.logpdf(Y, np.einsum("nk,mtk->nmt", W, V)[..., None]).sum())


def test_log_likelihood_full_size_vs_host_class():
    N, M, T, R, K = 256, 128, 16, 4, 5
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 20, 1)
    Y[3, 4, 5] = np.nan                                      # a cell without observations: log sum p
    model = _nonconj(N, M, T, K, lik, W, V)
    ll = model.log_likelihood(Y)
    ref = _host_ll(lik, Y, W, V)
    assert abs(ll - ref) <= 1e-10 * abs(ref), (ll, ref)
    assert model.logprob(Y) == ll
    assert abs(model.logprob(Y, W=W, V=V) - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("what", [0, 1])
def test_candidate_values_vs_numpy(what):
    """btf_gass_eval at random candidates (chains with 0, <= 64 and > 64 of them) against the host class; -inf beyond a
    chain's count.  Rows: the proposal is sqrt(sigma2) z on the free entries; columns: z = 0 (proposal 0)."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd import _native
    N, M, T, R, K, G = 24, 12, 9, 3, 3, 7
    W, V, Y, lik, rs = _problem(N, M, T, R, K, G, 2)
    W[np.triu_indices(K, 1)] = 0
    sigma2 = 0.7
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "gamma_grid", _fit_constraints(T), likelihood_param=lik,
                                                           nembeds=K, W_init=W, V_init=V, sigma2_init=sigma2, sampler="banded")
    nch = N if what == 0 else M
    if what == 0:
        z = rs.normal(size=K * (K + 1) // 2 + (N - K) * K)
        nu = np.zeros((N, K))
        off = 0
        for i in range(N):
            d = min(K, i + 1)
            nu[i, :d] = np.sqrt(sigma2) * z[off:off + d]
            off += d
    else:
        z = np.zeros((M, K * T))
    _begin(model, what, Y, z)
    nth = rs.randint(0, 129, size=nch).astype(np.int32)
    nth[:4] = [0, 1, 64, 128]
    thetas = rs.uniform(-np.pi, np.pi, size=(nch, 128))
    ll = np.empty((nch, 128))
    model._ctx.call("btf_gass_eval", what, _native.dptr(thetas), nth.ctypes.data_as(_native._c_ip), _native.dptr(ll))
    for c in range(nch):
        assert np.all(ll[c, nth[c]:] == -np.inf)
        for q in range(nth[c]):
            cs, sn = np.cos(thetas[c, q]), np.sin(thetas[c, q])
            if what == 0:
                x = W[c] * cs + nu[c] * sn
                ref = float(lik.logpdf(Y[c], np.einsum("k,mtk->mt", x, V)[..., None]).sum())
            else:
                ref = float(lik.logpdf(Y[:, c], (np.einsum("nk,tk->nt", W, V[c]) * cs)[..., None]).sum())
            if ref == -np.inf:
                assert ll[c, q] == -np.inf, (c, q)
            else:
                assert abs(ll[c, q] - ref) <= 1e-10 * max(1.0, abs(ref)), (c, q, ll[c, q], ref)


def test_split_component_equals_merged_table():
    N, M, T, R, K = 40, 20, 8, 3, 3
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 6, 3)
    a, s, p = lik.shape_grid, lik.scale_grid, lik.probs_grid
    split = types.SimpleNamespace(shape_grid=np.r_[a, a[2]], scale_grid=np.r_[s, s[2]], probs_grid=np.r_[p[:2], p[2] / 2, p[3:], p[2] / 2])
    l1 = _nonconj(N, M, T, K, lik, W, V).log_likelihood(Y)
    l2 = _nonconj(N, M, T, K, split, W, V).log_likelihood(Y)
    assert abs(l1 - l2) <= 1e-12 * abs(l1), (l1, l2)


def test_single_component_is_the_gamma_logpdf():
    N, M, T, R, K = 30, 16, 8, 4, 2
    W, V, Y, _, _ = _problem(N, M, T, R, K, 3, 4)
    one = types.SimpleNamespace(shape_grid=np.array([30.0]), scale_grid=np.array([1.0 / 30.0]), probs_grid=np.array([1.0]))
    ll = _nonconj(N, M, T, K, one, W, V).log_likelihood(Y)
    eta = np.einsum("nk,mtk->nmt", W, V)[..., None]
    ref = float(np.nansum(gamma_dist.logpdf(Y, 30.0, scale=eta / 30.0)))
    assert abs(ll - ref) <= 1e-10 * abs(ref), (ll, ref)


def test_nonpositive_predictor_gives_minus_inf_and_criteria_refuse():
    N, M, T, R, K = 10, 6, 5, 2, 2
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 4, 5)
    model = _nonconj(N, M, T, K, lik, W, V)
    assert np.isfinite(model.log_likelihood(Y))
    W2 = W.copy()
    W2[3] = -W2[3]
    model.W = W2
    assert model.log_likelihood(Y) == -np.inf
    Y2 = Y.copy()
    Y2[3] = np.nan                                        # the row is unobserved: finite again
    assert np.isfinite(model.log_likelihood(Y2))
    with pytest.raises(NotImplementedError, match="gamma_grid"):
        model.information_criteria(results={"W": W[None], "V": V[None]})


def test_unset_statistics_are_refused():
    """The ABI refuses family 5 without L (btf_set_data_logsum) - BTF_ESTATE, not a launch."""
    from functionalmf_amd import _native
    N, M, T, R, K = 8, 5, 4, 2, 2
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 3, 6)
    model = _nonconj(N, M, T, K, lik, W, V)
    rows, cols = model._plan.slabs(Y)
    model._ctx.call("btf_set_data_gaussian", _native.dptr(rows), _native.dptr(cols), R)
    model._push_state()
    model._ctx.call("btf_ess_begin", 0, None, 0, 1e-6, 0)
    import ctypes
    ll = ctypes.c_double()
    with pytest.raises(_native.BTFError) as e:
        model._ctx.call("btf_ess_eval", 0, 0.0, 1, 5, ctypes.byref(ll))
    assert e.value.code == _native.BTF_ESTATE
    with pytest.raises(_native.BTFError):
        model._ctx.call("btf_set_likelihood_param", 5, 1.0)


@pytest.mark.parametrize("ess", ["joint", "rows"])
def test_ess_device_chains_are_bit_identical(ess):
    N, M, T, R, K = 32, 16, 8, 3, 3
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 8, 7)
    out = []
    for _ in range(2):
        np.random.seed(3)                        # (the starting hyper-parameters come from the legacy generator)
        model = _nonconj(N, M, T, K, lik, W, V, rng="device", ess=ess, device_seed=11, tf_order=1)
        for _ in range(5):
            model.resample(Y)
        out.append((model.W.copy(), model.V.copy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert np.any(out[0][0] != W) and np.all(np.isfinite(out[0][0]))


@pytest.mark.parametrize("ep", [False, True])
def test_constrained_device_chains_bit_identical_and_feasible(ep):
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd import utils
    import contextlib
    import io
    N, M, T, R, K = 24, 12, 9, 6, 3
    W, V, Y, lik, _ = _problem(N, M, T, R, K, 20, 8)
    W[np.triu_indices(K, 1)] = 0
    Cons = _fit_constraints(T)
    epa = None
    if ep:
        with contextlib.redirect_stdout(io.StringIO()):
            epa = utils.ep_from_mf(Y, W, V, mode="multiplier", multiplier=3)
    runs = []
    for _ in range(2):
        np.random.seed(3)
        model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "gamma_grid", Cons, likelihood_param=lik, ep_approx=epa,
                                                               nembeds=K, tf_order=2, W_init=W, V_init=V, rng="device",
                                                               device_seed=5)
        for _ in range(50):
            model.resample(Y)
        runs.append((model.W.copy(), model.V.copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    tau = np.einsum("nk,mtk->nmt", runs[0][0], runs[0][1])
    lhs = np.einsum("qt,nmt->nmq", Cons[:, :-1], tau)
    assert np.all(lhs >= Cons[:, -1] - 1e-9), (lhs - Cons[:, -1]).min()
    assert np.any(runs[0][0] != W)
