"""fold_in_cols, the host halves (functionalmf_amd/fold_in_cols.py): the numpy definition against the reference's own
dense construction, the unit-variate convention of `draws`, the argument checks and the registration.  No GPU."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from functionalmf_amd import _native, fold_in_cols as fc, utils


def column_problem(K, tf_order, N=11, T=7, nreps=3, seed=0):
    """W, one column with missing cells and partial replicates, nu2, lam2, tau2."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    Y = rs.normal(size=(N, T, nreps))
    Y[rs.uniform(size=(N, T)) < 0.3] = np.nan                         # missing cells
    Y[:, :, 0][rs.uniform(size=(N, T)) < 0.4] = np.nan                # partial replicates
    nD = fc.penalty(T, tf_order).shape[0]
    return W, Y, 0.7, 0.2, rs.uniform(0.2, 3.0, size=nD)


def reference_dense(Y, W, nu2, lam2, tau2, tf_order):
    """Q and mu of factor.py:380-408 for one column, k-major (index k T + t): X = kron(W, I_T) over the observed cells,
    Q = X' C X + kron(I_K, Delta' Lambda Delta), mu = X' C ybar."""
    N, K = W.shape
    T = Y.shape[1]
    cnt = (~np.isnan(Y)).sum(axis=-1)
    with np.errstate(invalid="ignore"):
        ybar = np.where(cnt > 0, np.nansum(Y, axis=-1) / np.maximum(cnt, 1), np.nan)
    yflat, cflat = ybar.reshape(-1), cnt.reshape(-1)
    missing = np.isnan(yflat)
    X = sp.kron(sp.csc_matrix(W), sp.eye(T, format="csc"), format="csc").tocsr()[~missing]
    Cw = sp.diags(cflat[~missing] / nu2, 0)
    Xt = X.T.dot(Cw).tocsc()
    Delta = utils.bayes_grid_penalty(T, tf_order)
    lam_Tau = sp.spdiags(1 / (lam2 * tau2), 0, len(tau2), len(tau2), format="csc")
    Q = Xt.dot(X) + sp.kron(sp.eye(K, format="csc"), Delta.T.tocsc().dot(lam_Tau).dot(Delta))
    return np.asarray(Q.todense()), np.asarray(Xt.dot(yflat[~missing])).reshape(-1)


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("tf_order", [0, 1, 2])
def test_conditional_against_the_reference_dense_form(K, tf_order):
    """1. Q and the mean against kron(I_K, Delta' Lambda Delta) + X' C X, permuted from k-major to depth-major: 1e-12."""
    W, Y, nu2, lam2, tau2 = column_problem(K, tf_order, seed=10 * K + tf_order)
    T = Y.shape[1]
    mean, Q = fc.conditional(Y, W, nu2, lam2, tau2, tf_order)
    Qr, mu = reference_dense(Y, W, nu2, lam2, tau2, tf_order)
    perm = np.array([k * T + t for t in range(T) for k in range(K)])        # depth-major position -> k-major index
    Qp, mp = Qr[np.ix_(perm, perm)], np.linalg.solve(Qr, mu)[perm]
    assert np.abs(Q - Qp).max() <= 1e-12 * np.abs(Qp).max()
    assert np.abs(mean - mp).max() <= 1e-12 * max(np.abs(mp).max(), 1.0)
    bw = fc.half_bandwidth(K, tf_order)
    i, j = np.nonzero(Q)
    assert np.abs(i - j).max() <= bw                                       # the band the kernel stores


def transcription(Y, W, nu2, lam2, tf_order, sweeps, rs, stability=1e-6):
    """The chain with the legacy calls in the reference's order: sample_horseshoe_plus (utils.py:115-120) and the clip of
    _init_Tau2, then per sweep the column's normals and the four rs.gamma(shape, scale) of factor.py:136-141."""
    K, T = W.shape[1], Y.shape[1]
    D = fc.penalty(T, tf_order)
    nD = D.shape[0]
    a = 1 / rs.gamma(0.5, 1, size=nD)
    b = 1 / rs.gamma(0.5, a)
    c = 1 / rs.gamma(0.5, b)
    tau2 = (1 / rs.gamma(0.5, c)).clip(0, 9)
    lo, hi = stability, 1 / stability
    for _ in range(sweeps):
        mean, Q = fc.conditional(Y, W, nu2, lam2, tau2, tf_order)
        z = rs.normal(size=T * K)
        v = mean + np.linalg.solve(np.linalg.cholesky(Q).T, z)
        deltas = D.dot(v.reshape(T, K))
        rate = (deltas ** 2).sum(axis=1) / (2 * lam2) + 1 / c.clip(lo, hi)
        tau2 = 1 / rs.gamma((K + 1) / 2, 1 / rate.clip(lo, hi))
        c = 1 / rs.gamma(1, 1 / (1 / tau2 + 1 / b).clip(lo, hi))
        b = 1 / rs.gamma(1, 1 / (1 / c + 1 / a).clip(lo, hi))
        a = 1 / rs.gamma(1, 1 / (1 / b + 1).clip(lo, hi))
    return v.reshape(T, K), mean.reshape(T, K), tau2


@pytest.mark.parametrize("K,tf_order,sweeps", [(1, 0, 1), (3, 2, 3), (4, 1, 2)])
def test_chain_on_unit_variates_equals_the_transcription(K, tf_order, sweeps):
    """2. `draws` from RandomState.standard_gamma / normal in the chain's order give the chain of the legacy gamma(shape,
    scale) calls: the unit-variate convention (1 / gamma(shape, 1 / x) = x / standard_gamma(shape))."""
    W, Y, nu2, lam2, _ = column_problem(K, tf_order, seed=3 + K)
    T = Y.shape[1]
    draws = fc.random_draws(np.random.RandomState(42), T, K, tf_order, sweeps)
    assert draws.shape == (fc.draws_length(T, K, tf_order, sweeps),)
    v, m, t2 = fc.chain(Y, W, nu2, lam2, tf_order, sweeps, draws)
    vr, mr, tr = transcription(Y, W, nu2, lam2, tf_order, sweeps, np.random.RandomState(42))
    np.testing.assert_allclose(v, vr, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(m, mr, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(t2, tr, rtol=1e-9)


def test_empty_column_is_the_prior():
    """3. An all-nan column: conditional mean 0, Q the prior's kron(P, I_K)."""
    W, Y, nu2, lam2, tau2 = column_problem(3, 2, seed=5)
    mean, Q = fc.conditional(np.full_like(Y, np.nan), W, nu2, lam2, tau2, 2)
    D = fc.penalty(Y.shape[1], 2)
    P = D.T.dot(np.diag(1 / (lam2 * tau2))).dot(D)
    assert np.all(mean == 0.0)
    np.testing.assert_allclose(Q, np.kron(P, np.eye(3)), rtol=1e-14, atol=0)


def test_refusals_before_any_device_call():
    """4. check_args / column_statistics raise ValueError."""
    N, T, K, tf = 6, 8, 3, 2
    Y = np.zeros((2, N, T))
    with pytest.raises(ValueError, match="must be"):
        fc.column_statistics(np.zeros((2, N + 1, T)), "gaussian", N, T)
    with pytest.raises(ValueError, match="must be"):
        fc.column_statistics(np.zeros((N, T)), "gaussian", N, T)
    bad = Y.copy()
    bad[0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="infinite"):
        fc.column_statistics(bad, "gaussian", N, T)
    with pytest.raises(ValueError, match="family"):
        fc.column_statistics(Y, "poisson", N, T)
    for k in (0, 11):
        with pytest.raises(ValueError, match="nembeds"):
            fc.check_args("gaussian", 4, 2, T, k, tf)
    for sw in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sweeps"):
            fc.check_args("gaussian", 4, 2, T, K, tf, sweeps=sw)
    L = fc.draws_length(T, K, tf, 2)
    good = fc.random_draws(np.random.RandomState(0), T, K, tf, 2, size=(4, 2))
    assert fc.check_args("gaussian", 4, 2, T, K, tf, draws=good, sweeps=2)[1].shape == (4, 2, L)
    with pytest.raises(ValueError, match="draws must be"):
        fc.check_args("gaussian", 4, 2, T, K, tf, draws=good[..., :-1], sweeps=2)
    with pytest.raises(ValueError, match="draws must be"):
        fc.check_args("gaussian", 4, 2, T, K, tf, draws=good, sweeps=3)
    neg = good.copy()
    neg[1, 1, 5] = -0.5                                                   # inside the start block
    with pytest.raises(ValueError, match="positive"):
        fc.check_args("gaussian", 4, 2, T, K, tf, draws=neg, sweeps=2)
    neg = good.copy()
    neg[0, 0, -1] = 0.0                                                   # the last gamma of the last sweep
    with pytest.raises(ValueError, match="positive"):
        fc.check_args("gaussian", 4, 2, T, K, tf, draws=neg, sweeps=2)
    ok = good.copy()
    nD = fc.penalty(T, tf).shape[0]
    ok[..., 4 * nD:4 * nD + T * K] = -np.abs(ok[..., 4 * nD:4 * nD + T * K])    # normals may be negative
    fc.check_args("gaussian", 4, 2, T, K, tf, draws=ok, sweeps=2)
    with pytest.raises(ValueError, match="Gaussian model only"):
        fc.check_args("binomial", 4, 2, T, K, tf, draws=good, sweeps=2)
    with pytest.raises(ValueError, match="up to 32"):
        fc.column_statistics((np.zeros((1, N, T)), np.full((1, N, T), 33.0)), "binomial", N, T)
    with pytest.raises(ValueError, match="up to 32"):
        fc.column_statistics(np.zeros((1, N, T)), "binomial", N, T, trials=40)
    with pytest.raises(ValueError, match=r"successes must lie"):
        fc.column_statistics((np.full((1, N, T), 3.0), np.full((1, N, T), 2.0)), "binomial", N, T)
    # the band beyond the LDS limit: the flu shape at K = 10; C3 and the dose-response shapes fit
    assert fc.lds_bytes(370, 10, 2) > fc.LDS_LIMIT
    with pytest.raises(ValueError, match="LDS"):
        fc.check_args("gaussian", 4, 1, 370, 10, 2)
    assert fc.lds_bytes(64, 5, 2) <= fc.LDS_LIMIT and fc.lds_bytes(9, 10, 2) <= fc.LDS_LIMIT
    with pytest.raises(ValueError, match="LDS"):
        utils.fold_in_cols(np.zeros((1, 5, 370)), np.zeros((2, 5, 10)), "gaussian", nu2=np.ones(2), lam2=np.ones(2))
    with pytest.raises(ValueError):
        utils.fold_in_cols(np.zeros((1, 5, 9)), np.zeros((2, 5, 3)), "gaussian", nu2=np.ones(2), lam2=np.array([1.0, -1.0]))


def test_binomial_statistics():
    Yb = np.array([[[1.0, np.nan], [0.0, 2.0]]])
    Nb = np.array([[[2.0, 3.0], [0.0, 5.0]]])
    C, n, y = fc.column_statistics((Yb, Nb), "binomial", 2, 2)
    assert C == 1 and np.array_equal(n[0], [[2.0, 0.0], [0.0, 5.0]]) and np.array_equal(y[0], [[1.0, 0.0], [0.0, 2.0]])


def test_stored_numpy_reference_is_the_chain():
    """The reference of the device-generator test (tests/golden/fold_in_cols_numpy_replicates.npz: moments of 4096 replicates
    of `chain` under numpy's generator at the default sweeps) was computed at the current DEFAULT_SWEEPS, and its first
    replicates come out of `chain` again."""
    import importlib.util
    from conftest import ROOT, load_golden
    spec = importlib.util.spec_from_file_location("gpu_fold_in_cols", os.path.join(ROOT, "tests", "test_gpu_fold_in_cols.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    g = load_golden("fold_in_cols_numpy_replicates.npz")
    assert int(g["sweeps"]) == fc.DEFAULT_SWEEPS and int(g["nsamples"]) == t.Z_SAMPLES and int(g["seed"]) == t.Z_SEEDS[0]
    W, Y, nu2, lam2 = t.z_problem()
    first = t.numpy_replicates(W, Y, nu2, lam2, 2, t.Z_SEEDS[0])
    np.testing.assert_allclose(first, g["first"][:2], rtol=1e-9, atol=1e-12)
    assert g["mean"].shape == first.shape[1:] and np.all(g["var"] > 0) and float(g["z_numpy_vs_numpy"]) <= 5


def test_registration():
    """5. The unit, its header and both signatures are registered; the header declares both entry points."""
    assert any(os.path.basename(src) == "btf_fold_in_cols.hip" for src, _ in _native.UNITS)
    assert any(os.path.basename(h) == "btf_fold_in_cols.h" for h in _native.HEADERS)
    assert len(_native.SIGNATURES["btf_fold_in_cols"][1]) == 27
    assert len(_native.SIGNATURES["btf_collect_fold_in_cols"][1]) == 20
    with open(os.path.join(_native.ROOT, "include", "btf.h")) as f:
        text = f.read()
    assert "int btf_fold_in_cols(" in text and "int btf_collect_fold_in_cols(" in text
    assert fc.DEFAULT_SWEEPS >= 1 and fc.DEFAULT_SWEEPS & (fc.DEFAULT_SWEEPS - 1) == 0
