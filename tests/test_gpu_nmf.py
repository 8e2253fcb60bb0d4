"""tensor_nmf / factor_pav on the GPU (csrc/btf_nmf.h): parity with the reference (fixtures of
tests/golden/make_golden_nmf.py), the batched NNLS against scipy at C3 size, the rmse history, bit-identity and a chain
started from the factorisation."""
import numpy as np
import pytest
from scipy.optimize import nnls

from functionalmf_amd import _native, nmf, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


def _run(g, case, **over):
    p = case + "_"
    kw = dict(max_steps=int(g[p + "max_steps"]), monotone=bool(g[p + "monotone"]), fit_W=bool(g[p + "fit_W"]),
              fit_V=bool(g[p + "fit_V"]), W=g[p + "W_in"] if p + "W_in" in g else None,
              V=g[p + "V_in"] if p + "V_in" in g else None, return_info=True)
    kw.update(over)
    np.random.seed(int(g[p + "seed"]))
    return utils.tensor_nmf(g[p + "Y"], int(g[p + "K"]), **kw)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _rmse(Y, W, V):
    Y4 = Y if Y.ndim == 4 else Y[..., None]
    return np.sqrt(np.nansum((Y4 - np.einsum("nk,mtk->nmt", W, V)[..., None]) ** 2))


def test_one_step_from_given_factors_matches_the_reference(golden):
    """One ALS step from given (W, V) with gaps: within 50 cond(G) eps of the reference, G the Grams of the solves."""
    g = golden("g12_nmf.npz")
    W, V, info = _run(g, "one_step")
    assert info["steps"] == 1
    Y, K = g["one_step_Y"], int(g["one_step_K"])
    Vin = g["one_step_V_in"]
    conds = [np.linalg.cond(np.einsum("mtk,mtl->kl", Vin, Vin)), np.linalg.cond(np.einsum("nk,nl->kl", W, W))]
    tol = 50 * max(conds) * EPS
    assert _rel(W, g["one_step_W"]) <= tol, (_rel(W, g["one_step_W"]), tol)
    assert _rel(V, g["one_step_V"]) <= tol, (_rel(V, g["one_step_V"]), tol)


@pytest.mark.parametrize("case", ["complete_r1", "complete_r3", "missing", "monotone", "monotone_miss", "fixW", "fixV",
                                  "givenW", "k1", "k10"])
def test_seeded_runs_match_the_reference(golden, case):
    """Seeded full runs: W / V to 1e-8, the same number of steps, the reference's per-step deltas, and (where stored)
    the factors after every step."""
    g = golden("g12_nmf.npz")
    p = case + "_"
    W, V, info = _run(g, case)
    assert info["steps"] == int(g[p + "steps"]), (info["steps"], int(g[p + "steps"]))
    assert _rel(W, g[p + "W"]) <= 1e-8, _rel(W, g[p + "W"])
    assert _rel(V, g[p + "V"]) <= 1e-8, _rel(V, g[p + "V"])
    r = info["rmse"]
    delta = (np.concatenate([[np.inf], r[:-1]]) - r) / r
    ref = g[p + "deltas"]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(delta), fin)
    assert np.allclose(delta[fin], ref[fin], rtol=1e-6, atol=1e-9)
    if p + "Ws" in g:
        for n in range(info["steps"]):
            Wn, Vn, inf_n = _run(g, case, max_steps=n + 1)
            assert inf_n["steps"] == n + 1
            assert _rel(Wn, g[p + "Ws"][n]) <= 1e-8 and _rel(Vn, g[p + "Vs"][n]) <= 1e-8, n
    if not bool(g[p + "fit_W"]):
        assert np.array_equal(W, g[p + "W_in"])
    if p + "W_in" in g:
        Win = g[p + "W_in"]
        K = Win.shape[1]
        for i in range(min(K - 1, Win.shape[0])):
            assert np.array_equal(W[i, i + 1:], Win[i, i + 1:]), i       # entries past d = i+1 are never fitted
    if bool(g[p + "monotone"]):
        Mu = np.einsum("nk,mtk->nmt", W, V)
        assert (np.diff(Mu, axis=2) <= 1e-12 * np.abs(Mu).max()).all()


def test_factor_pav_matches_the_reference(golden):
    g = golden("g12_nmf.npz")
    for c in g["pav_cases"]:
        W, V, P = g["pav%d_W" % c], g["pav%d_V" % c], g["pav%d_P" % c]
        got = utils.factor_pav(W, V)
        assert _rel(got, P) <= 1e-12, (c, _rel(got, P))
        assert np.array_equal(V, g["pav%d_V" % c])                                 # not in place
        Mu = W @ got.T
        assert (np.diff(Mu, axis=1) <= 1e-12 * np.abs(Mu).max()).all(), c
        Vc = V.copy()
        assert utils.factor_pav(W, Vc, in_place=True) is Vc and _rel(Vc, P) <= 1e-12
    got = utils.factor_pav(g["pavb_W"], g["pavb_V"])
    assert got.shape == g["pavb_V"].shape and _rel(got, g["pavb_P"]) <= 1e-12


def _c3(missing, seed=0, N=512, M=256, T=64, R=4, K=5):
    rs = np.random.RandomState(seed)
    Wt = rs.gamma(2.0, 0.5, size=(N, K))
    Vt = rs.gamma(2.0, 0.5, size=(M, T, K))
    Y = np.einsum("nk,mtk->nmt", Wt, Vt)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    if missing:
        Y[rs.uniform(size=(N, M, T)) < missing] = np.nan
        Y[rs.uniform(size=Y.shape) < missing] = np.nan
        Y[:3, :3] = np.nan
    return Y, rs


@pytest.mark.parametrize("missing", [0.0, 0.05])
def test_nnls_steps_match_scipy_at_c3(missing):
    """At C3 (512, 256, 64, 4) K=5: one W step (fit_V=False) and one V step (fit_W=False) equal per-row and per-(j,t)
    scipy.optimize.nnls on the reference's systems (truncated rows i < K included), compared after the 1e-3 clip."""
    Y, rs = _c3(missing)
    N, M, T, R = Y.shape
    K = 5
    W0 = rs.gamma(1.0, 1.0, size=(N, K))
    V0 = rs.gamma(1.0, 1.0, size=(M, T, K))
    W1, _, info = utils.tensor_nmf(Y, K, max_steps=1, W=W0, V=V0, fit_V=False, return_info=True)
    _, V1, _ = utils.tensor_nmf(Y, K, max_steps=1, W=W0, V=V0, fit_W=False, return_info=True)
    assert info["steps"] == 1
    Vmat = np.repeat(V0.reshape(-1, K), R, axis=0)
    rows = list(range(8)) + list(rs.choice(np.arange(8, N), 24, replace=False))
    for i in rows:
        y = Y[i].ravel()
        ok = ~np.isnan(y)
        d = min(K, i + 1)
        want = nnls(Vmat[ok][:, :d], y[ok])[0].clip(1e-3, np.inf) if ok.any() else np.full(d, 1e-3)
        assert np.allclose(W1[i, :d], want, rtol=1e-9, atol=1e-12), (i, W1[i, :d], want)
        assert np.array_equal(W1[i, d:], W0[i, d:])
    Wmat = np.repeat(W0, R, axis=0)
    for j, t in [(0, 0), (1, 2), (2, 63)] + [tuple(x) for x in zip(rs.randint(0, M, 40), rs.randint(0, T, 40))]:
        y = Y[:, j, t].ravel()
        ok = ~np.isnan(y)
        want = nnls(Wmat[ok], y[ok])[0].clip(1e-3, np.inf)
        assert np.allclose(V1[j, t], want, rtol=1e-9, atol=1e-12), (j, t, V1[j, t], want)


def test_rmse_history_equals_numpy_from_the_factors_of_each_step():
    Y, rs = _c3(0.05, seed=3, N=64, M=32, T=16, R=2, K=3)
    np.random.seed(5)
    _, _, info = utils.tensor_nmf(Y, 3, max_steps=6, tol=-1.0, return_info=True)
    assert info["steps"] == 6
    for n in range(1, 7):
        np.random.seed(5)
        Wn, Vn, inf_n = utils.tensor_nmf(Y, 3, max_steps=n, tol=-1.0, return_info=True)
        assert abs(inf_n["rmse"][-1] - _rmse(Y, Wn, Vn)) <= 1e-11 * _rmse(Y, Wn, Vn)
        assert np.array_equal(inf_n["rmse"], info["rmse"][:n])


@pytest.mark.parametrize("monotone", [False, True])
def test_two_identical_calls_give_identical_bits(monotone):
    Y, rs = _c3(0.05, seed=4, N=200, M=40, T=24, R=3, K=4)
    outs = []
    for _ in range(2):
        np.random.seed(9)
        outs.append(utils.tensor_nmf(Y, 4, max_steps=8, monotone=monotone, return_info=True))
    (W1, V1, i1), (W2, V2, i2) = outs
    assert np.array_equal(W1, W2) and np.array_equal(V1, V2) and np.array_equal(i1["rmse"], i2["rmse"])
    assert i1["steps"] == i2["steps"]


def test_verbose_prints_steps_and_deltas(capfd):
    Y, _ = _c3(0.0, seed=6, N=20, M=6, T=8, R=1, K=2)
    np.random.seed(1)
    _, _, info = utils.tensor_nmf(Y[..., 0], 2, max_steps=4, verbose=True, return_info=True)
    out = capfd.readouterr().out
    assert out.count("Step ") == info["steps"] and out.count("delta: ") == info["steps"]


def test_a_gaussian_chain_starts_from_the_factorisation():
    """model.W[:] = W0; model.V[:] = V0: the chain's state before the first sweep is exactly the factorisation."""
    N, M, T, K = 24, 10, 12, 3
    rs = np.random.RandomState(2)
    Y = np.einsum("nk,mtk->nmt", rs.gamma(2, 0.5, (N, K)), rs.gamma(2, 0.5, (M, T, K))) + rs.normal(0, 0.3, (N, M, T))
    np.random.seed(3)
    W0, V0 = utils.tensor_nmf(Y, K)
    np.random.seed(4)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2)
    model.W[:] = W0
    model.V[:] = V0
    model._push_state()                                  # what the first sweep does before it reads the state
    Wd, Vd = np.zeros((N, K)), np.zeros((M, T, K))
    model._ctx.call("btf_get_W", _native.dptr(Wd))
    model._ctx.call("btf_get_V", _native.dptr(Vd))
    assert np.array_equal(Wd, W0) and np.array_equal(Vd, V0)
    out = model.run_gibbs(Y, nburn=5, nthin=1, nsamples=5, print_freq=1000, verbose=False)
    assert np.isfinite(out["W"]).all() and np.isfinite(out["V"]).all()


def test_statistics_are_built_once_and_reused():
    Y, _ = _c3(0.05, seed=7, N=40, M=8, T=10, R=2, K=2)
    data = nmf.NMFData(Y, 2)
    try:
        np.random.seed(2)
        W0, V0 = np.random.gamma(1, 1, (40, 2)), np.random.gamma(1, 1, (8, 10, 2))
        a = data.run(W0, V0, max_steps=5, timing=True)
        b = data.run(W0, V0, max_steps=5)
    finally:
        data.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["device_ms"] > 0
