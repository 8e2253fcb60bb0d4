"""Host halves of fold_in_depth (functionalmf_amd/fold_in_depth.py): no GPU needed.

The numpy definition against the Schur conditional of fold_in_cols.conditional on the extended grid, the new penalty rows,
the chain's consistency, and every refusal that has to happen before a device call.
"""
import importlib.util
import os
import types

import numpy as np
import pytest

from functionalmf_amd import _native, fold_in_cols as fc, fold_in_depth as fd, utils
from functionalmf_amd.factor import (GaussianBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)

SHAPES = ((2, 1), (3, 1), (4, 3), (9, 8))


def gpu_test_module():
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("gpu_fold_in_depth", os.path.join(ROOT, "tests", "test_gpu_fold_in_depth.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


@pytest.mark.parametrize("TH", SHAPES)
@pytest.mark.parametrize("tf_order", [0, 1, 2])
def test_conditional_is_the_schur_conditional_of_the_extended_grid(tf_order, TH):
    """1. `conditional` equals the conditional of the new depths given the kept ones under fold_in_cols.conditional on T + H
    points: the same Q_nn block, mean Q_nn^-1 (b_n - Q_no v_old).  Only the scales of the new rows enter."""
    T, H = TH
    rs = np.random.RandomState(100 * tf_order + 10 * T + H)
    N, K = 9, 3
    W = rs.normal(size=(N, K))
    Y = rs.normal(size=(N, T + H, 2))
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    V_old = rs.normal(size=(T, K))
    nu2, lam2 = 0.5, 0.2
    R, D_o, D_n = fd.new_rows(T, H, tf_order)
    tau2 = rs.gamma(1.0, size=fc.penalty(T + H, tf_order).shape[0]) + 0.1
    mean_f, Q_f = fc.conditional(Y, W, nu2, lam2, tau2, tf_order)
    n0 = T * K
    Q_nn, Q_no, b = Q_f[n0:, n0:], Q_f[n0:, :n0], Q_f.dot(mean_f)
    want = np.linalg.solve(Q_nn, b[n0:] - Q_no.dot(V_old.reshape(-1)))
    mean, Q = fd.conditional(Y[:, T:], W, V_old, nu2, lam2, tau2[R], tf_order)
    np.testing.assert_allclose(Q, Q_nn, rtol=0, atol=1e-10)
    np.testing.assert_allclose(mean, want, rtol=0, atol=1e-10)
    other = tau2.copy()
    other[np.setdiff1d(np.arange(tau2.size), R)] *= 7.0                  # the scales of rows on kept depths alone are not read
    Q_other = fc.conditional(Y, W, nu2, lam2, other, tf_order)[1]
    np.testing.assert_allclose(Q_other[n0:, n0:], Q, rtol=0, atol=1e-10)
    np.testing.assert_allclose(Q_other[n0:, :n0], Q_no, rtol=0, atol=1e-10)


@pytest.mark.parametrize("TH", SHAPES + ((12, 4), (370, 8)))
@pytest.mark.parametrize("tf_order", [0, 1, 2])
def test_new_rows(tf_order, TH):
    """2. nR = H, 2 H + 1, 3 H + 2 at tf_order 0, 1, 2 (T >= tf_order + 1); D_n has full column rank, D_o reaches back at
    most min(T, tf_order + 1) kept depths, and every new row fits a window of tf_order + 2 depths."""
    T, H = TH
    R, D_o, D_n = fd.new_rows(T, H, tf_order)
    assert D_o.shape == (R.size, T) and D_n.shape == (R.size, H)
    if T >= tf_order + 1:
        assert R.size == (tf_order + 1) * H + tf_order
    assert np.linalg.matrix_rank(D_n) == H
    back = fd.tail_depths(T, tf_order)
    assert not np.any(D_o[:, :T - back])
    D = fc.penalty(T + H, tf_order)[R]
    for row in D:
        nz = np.flatnonzero(row)
        assert nz.max() - nz.min() <= tf_order + 1
    assert fd.draws_length(T, H, 3, tf_order, 5) == 4 * R.size + 5 * (3 * H + 4 * R.size)
    assert fd.half_bandwidth(H, 3, tf_order) == min((tf_order + 1) * 3, 3 * H - 1)


def chain_problem(seed=3, N=11, T=7, H=3, K=2):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V_old = 0.4 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = rs.normal(size=(N, H))
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    return W, V_old, Y


@pytest.mark.parametrize("family", ["gaussian", "binomial"])
def test_chain_is_reproducible_and_nested(family):
    """3. `chain` returns the same values twice; on_sweep shows that the chain of r + 1 sweeps on the leading draws ends at
    the state after sweep r; on_system sees one symmetric positive definite precision per sweep."""
    W, V_old, Y = chain_problem()
    T, H, K, tf, sweeps = V_old.shape[0], Y.shape[1], W.shape[1], 2, 4
    data = Y if family == "gaussian" else (np.where(np.isnan(Y), np.nan, (Y > 0) * 2.0), np.full(Y.shape, 3.0))
    draws = fd.random_draws(np.random.RandomState(1), T, H, K, tf, sweeps)
    assert draws.shape == (fd.draws_length(T, H, K, tf, sweeps),)
    states, systems = [], []
    kw = dict(family=family, seed=9)
    a = fd.chain(data, W, V_old, 0.5, 0.1, tf, sweeps, draws, on_sweep=lambda r, v: states.append(v.copy()),
                 on_system=systems.append, **kw)
    b = fd.chain(data, W, V_old, 0.5, 0.1, tf, sweeps, draws, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert len(states) == sweeps and len(systems) == sweeps and np.array_equal(states[-1], a[0])
    nR = fd.new_rows(T, H, tf)[0].size
    assert a[0].shape == (H, K) and a[1].shape == (H, K) and a[2].shape == (nR,)
    for Q in systems:
        assert np.allclose(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    for r in range(sweeps):
        lead = draws[:fd.draws_length(T, H, K, tf, r + 1)]
        assert np.array_equal(fd.chain(data, W, V_old, 0.5, 0.1, tf, r + 1, lead, **kw)[0], states[r])
    with pytest.raises(ValueError, match="draws must hold"):
        fd.chain(data, W, V_old, 0.5, 0.1, tf, sweeps, draws[:-1], **kw)


def test_data_free_draw_is_the_prior_given_the_kept_curve():
    """With no data Q is the prior's precision of the new rows and the mean continues the kept curve: for tf_order 0 and one
    new depth the mean is the last kept depth itself."""
    W, V_old, Y = chain_problem()
    T, K = V_old.shape
    R, D_o, D_n = fd.new_rows(T, 1, 0)
    mean, Q = fd.conditional(np.full((W.shape[0], 1), np.nan), W, V_old, 0.5, 0.1, np.array([2.0]), 0)
    np.testing.assert_allclose(mean, V_old[-1], rtol=1e-13)
    np.testing.assert_allclose(Q, np.eye(K) / (0.1 * 2.0), rtol=1e-13)


def test_refusals_before_any_device_call():
    """4. check_args / slice_statistics / draws_length raise ValueError; lds_bytes restates the header's count."""
    N, M, T, H, K, tf = 6, 3, 8, 2, 3, 2
    Y = np.zeros((N, M, H))
    for bad in (np.zeros((N + 1, M, H)), np.zeros((N, M)), np.zeros((N, M + 1, H)), np.zeros((N, M, 0)), np.zeros((N, M, H, 2, 2))):
        with pytest.raises(ValueError, match="must be"):
            fd.slice_statistics(bad, "gaussian", N, M)
    inf = Y.copy()
    inf[0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="infinite"):
        fd.slice_statistics(inf, "gaussian", N, M)
    with pytest.raises(ValueError, match="infinite"):
        fd.slice_statistics((Y, np.full(Y.shape, np.inf)), "binomial", N, M)
    with pytest.raises(ValueError, match="family"):
        fd.slice_statistics(Y, "poisson", N, M)
    with pytest.raises(ValueError, match="not a pair"):
        fd.slice_statistics((Y, Y), "gaussian", N, M)
    for h in (None, 0, -1, 1.5):
        with pytest.raises(ValueError, match="horizon"):
            fd.slice_statistics(None, "gaussian", N, M, horizon=h)
    with pytest.raises(ValueError, match="horizon"):
        fd.slice_statistics(Y, "gaussian", N, M, horizon=H + 1)
    Hh, cnt, ysum = fd.slice_statistics(None, "gaussian", N, M, horizon=4)
    assert Hh == 4 and cnt.shape == (M, 4, N) and not cnt.any() and not ysum.any()
    Yr = np.arange(N * M * H * 2, dtype=float).reshape(N, M, H, 2)
    Yr[1, 2, 0, 1] = np.nan
    Hh, cnt, ysum = fd.slice_statistics(Yr, "gaussian", N, M)
    assert Hh == H and cnt.shape == (M, H, N) and cnt[2, 0, 1] == 1 and ysum[2, 0, 1] == Yr[1, 2, 0, 0] and cnt[0, 1, 3] == 2
    with pytest.raises(ValueError, match="up to 32"):
        fd.slice_statistics((Y, np.full(Y.shape, 33.0)), "binomial", N, M)
    with pytest.raises(ValueError, match="up to 32"):
        fd.slice_statistics(Y, "binomial", N, M, trials=40)
    with pytest.raises(ValueError, match="successes must lie"):
        fd.slice_statistics((np.full(Y.shape, 3.0), np.full(Y.shape, 2.0)), "binomial", N, M)
    Yb, Nb = np.array([[[1.0, np.nan]], [[0.0, 2.0]]]), np.array([[[2.0, 3.0]], [[0.0, 5.0]]])
    _, n, y = fd.slice_statistics((Yb, Nb), "binomial", 2, 1)
    assert np.array_equal(n[0], [[2.0, 0.0], [0.0, 5.0]]) and np.array_equal(y[0], [[1.0, 0.0], [0.0, 2.0]])
    # check_args
    for h, t in ((0, T), (-2, T), (H, 1)):
        with pytest.raises(ValueError, match="horizon >= 1"):
            fd.check_args("gaussian", 4, M, t, h, K, tf)
        with pytest.raises(ValueError):
            fd.draws_length(t, h, K, tf, 2)
    for k in (0, 11):
        with pytest.raises(ValueError, match="nembeds"):
            fd.check_args("gaussian", 4, M, T, H, k, tf)
    for sw in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sweeps"):
            fd.check_args("gaussian", 4, M, T, H, K, tf, sweeps=sw)
    assert fd.check_args("gaussian", 4, M, T, H, K, tf)[4] == fd.DEFAULT_SWEEPS
    with pytest.raises(ValueError, match="16384"):
        fd.check_args("gaussian", 16385, M, T, H, K, tf)
    fd.check_args("gaussian", 16385, M, T, H, K, tf, summary=False)
    with pytest.raises(ValueError, match="below 64"):
        fd.check_args("gaussian", 4, M, T, H, 8, 7)                       # (tf_order + 1) K = 64
    with pytest.raises(ValueError, match="first_sample"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, first_sample=-1)
    with pytest.raises(ValueError, match="first_sample"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, first_sample=2 ** 31)
    with pytest.raises(ValueError, match="within"):
        fd.check_args("gaussian", 4, M, fd.MAX_GRID, 1, K, tf)
    L = fd.draws_length(T, H, K, tf, 2)
    good = fd.random_draws(np.random.RandomState(0), T, H, K, tf, 2, size=(4, M))
    assert fd.check_args("gaussian", 4, M, T, H, K, tf, draws=good, sweeps=2)[1].shape == (4, M, L)
    with pytest.raises(ValueError, match="draws must be"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, draws=good[..., :-1], sweeps=2)
    with pytest.raises(ValueError, match="draws must be"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, draws=good, sweeps=3)
    nR = fd.new_rows(T, H, tf)[0].size
    neg = good.copy()
    neg[1, 1, 5] = -0.5                                                   # inside the start block
    with pytest.raises(ValueError, match="positive"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, draws=neg, sweeps=2)
    neg = good.copy()
    neg[0, 0, -1] = 0.0                                                   # the last gamma of the last sweep
    with pytest.raises(ValueError, match="positive"):
        fd.check_args("gaussian", 4, M, T, H, K, tf, draws=neg, sweeps=2)
    ok = good.copy()
    ok[..., 4 * nR:4 * nR + H * K] = -np.abs(ok[..., 4 * nR:4 * nR + H * K])    # normals may be negative
    fd.check_args("gaussian", 4, M, T, H, K, tf, draws=ok, sweeps=2)
    with pytest.raises(ValueError, match="Gaussian model only"):
        fd.check_args("binomial", 4, M, T, H, K, tf, draws=good, sweeps=2)
    # lds_bytes: the count of foldd_lds_bytes (csrc/btf_fold_in_depth.h), restated
    for (t, h, k, o) in ((2, 1, 1, 0), (2, 1, 10, 2), (9, 8, 5, 2), (370, 8, 10, 2), (64, 8, 5, 1), (9, 2, 5, 2)):
        n, bw, nr, tail = h * k, min((o + 1) * k, h * k - 1), fd.new_rows(t, h, o)[0].size, min(t, o + 1)
        want = 8 * (n * (bw + 1) + 4 * n + h * (k * (k + 1) // 2) + 5 * nr + nr * k + h * (o + 2) + tail * k) \
            + 8 * ((bw * (bw + 1) // 2 + 3) // 4)
        assert fd.lds_bytes(t, h, k, o) == want <= fd.LDS_LIMIT
    assert fd.LDS_LIMIT == 156 * 1024 and fd.lds_bytes(9, 8, 5, 2) == 8 * (40 * 16 + 160 + 120 + 130 + 130 + 32 + 15) + 8 * 30
    assert fd.lds_bytes(370, 370, 10, 2) > fd.LDS_LIMIT
    with pytest.raises(ValueError, match="LDS"):
        fd.check_args("gaussian", 4, 1, 370, 370, 10, 2)
    with pytest.raises(ValueError, match="LDS"):
        utils.fold_in_depth(None, np.zeros((2, 5, 10)), np.zeros((2, 1, 370, 10)), "gaussian", horizon=370, nu2=np.ones(2), lam2=np.ones(2))
    with pytest.raises(ValueError):
        utils.fold_in_depth(np.zeros((5, 1, 2)), np.zeros((2, 5, 3)), np.zeros((2, 1, 9, 3)), "gaussian", nu2=np.ones(2),
                            lam2=np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        utils.fold_in_depth(np.zeros((5, 1, 2)), np.zeros((2, 5, 3)), np.zeros((2, 1, 9, 4)), "gaussian", nu2=np.ones(2), lam2=np.ones(2))
    with pytest.raises(ValueError, match="finite"):
        utils.fold_in_depth(np.zeros((5, 1, 2)), np.zeros((2, 5, 3)), np.full((2, 1, 9, 3), np.nan), "gaussian", nu2=np.ones(2),
                            lam2=np.ones(2))


class _NoDevice:
    device = 0

    def call(self, *a):
        raise AssertionError("a device call was made")


def _bare(cls, world=1, collected=0):
    m = object.__new__(cls)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.tf_order, m.stability = 6, 3, 5, 2, 2, 1e-6
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    m._collected, m._draws, m._device_seed, m._callback = collected, 0, 1, False
    return m


def test_model_refusals_raise_before_any_device_call():
    """5. The unsupported models, a sharded model, nothing collected and bad arguments - each before any device call and
    without taking a seed."""
    Y = np.zeros((6, 3, 2))
    res = {"W": np.ones((4, 6, 2)), "V": np.ones((4, 3, 5, 2)), "nu2": np.ones((4, 1)), "lam2": np.ones((4, 1))}
    with pytest.raises(NotImplementedError, match="Negative-Binomial"):
        _bare(NegativeBinomialBayesianTensorFiltering).fold_in_depth(Y, results=res)
    with pytest.raises(NotImplementedError, match="slice-sampled"):
        _bare(NonconjugateBayesianTensorFiltering).fold_in_depth(Y, results=res)
    cb = _bare(NonconjugateBayesianTensorFiltering)
    cb._callback = True
    with pytest.raises(NotImplementedError, match="Python-callable"):
        cb.fold_in_depth(Y, results=res)
    with pytest.raises(NotImplementedError, match="unsharded"):
        _bare(GaussianBayesianTensorFiltering, world=2).fold_in_depth(Y, results=res)
    g = _bare(GaussianBayesianTensorFiltering)
    with pytest.raises(RuntimeError, match="no samples collected"):
        g.fold_in_depth(Y)
    for bad_Y, kw in ((np.zeros((6, 3)), {}), (np.zeros((5, 3, 2)), {}), (None, {}), (None, dict(horizon=0)), (Y, dict(horizon=3)),
                      (Y, dict(sweeps=0)), (Y, dict(q=(5, 120))), (Y, dict(transform="cube")), (Y, dict(draws=np.ones((4, 3, 7))))):
        with pytest.raises(ValueError):
            g.fold_in_depth(bad_Y, results=res, **kw)
    for key, val in (("V", np.ones((4, 3, 5, 3))), ("W", np.ones((4, 5, 2))), ("nu2", np.ones(3)), ("lam2", -np.ones(4))):
        with pytest.raises(ValueError):
            g.fold_in_depth(Y, results=dict(res, **{key: val}))
    assert g._draws == 0


def test_stored_numpy_references_are_the_chain():
    """The references of the device-generator tests (tests/golden/fold_in_depth_numpy_replicates.npz) were computed at the
    current DEFAULT_SWEEPS and their first replicates come out of `chain` again; two numpy seeds pass the
    Kolmogorov-Smirnov check of the data-free test against each other."""
    from conftest import load_golden
    t = gpu_test_module()
    g = load_golden("fold_in_depth_numpy_replicates.npz")
    assert int(g["sweeps"]) == fd.DEFAULT_SWEEPS and int(g["nsamples"]) == t.Z_SAMPLES and int(g["seed"]) == t.Z_SEEDS[0]
    W, V_old, Y, nu2, lam2 = t.z_problem()
    first = t.numpy_replicates(W, V_old, Y, nu2, lam2, 2, t.Z_SEEDS[0])
    np.testing.assert_allclose(first, g["first"][:2], rtol=1e-9, atol=1e-12)
    assert g["mean"].shape == first.shape[1:] and np.all(g["var"] > 0) and float(g["z_numpy_vs_numpy"]) <= 5
    assert g["forecast"].shape == (t.Z_SAMPLES, 4, 2)
    np.testing.assert_allclose(t.forecast_replicates(3, t.Z_SEEDS[0]), g["forecast"][:3], rtol=1e-9, atol=1e-12)
    other = t.forecast_replicates(t.Z_SAMPLES, t.Z_SEEDS[1])
    ks = t.ks_two_sample(other, g["forecast"])
    assert abs(ks - float(g["ks_numpy_vs_numpy"])) < 1e-9 and ks <= t.KS_LIMIT
    assert abs(t.KS_LIMIT - 0.0492) < 5e-5
    b = load_golden("fold_in_depth_binomial_oracle.npz")
    assert b["mean"].shape == t.binomial_problem()[2].shape and np.all(b["se"] > 0) and np.all((b["mean"] > 0) & (b["mean"] < 1))


def test_registration():
    """6. The unit, its header and both signatures are registered; the header declares both entry points."""
    assert any(os.path.basename(src) == "btf_fold_in_depth.hip" for src, _ in _native.UNITS)
    assert any(os.path.basename(h) == "btf_fold_in_depth.h" for h in _native.HEADERS)
    assert len(_native.SIGNATURES["btf_fold_in_depth"][1]) == 29
    assert len(_native.SIGNATURES["btf_collect_fold_in_depth"][1]) == 20
    with open(os.path.join(_native.ROOT, "include", "btf.h")) as f:
        text = f.read()
    assert "int btf_fold_in_depth(" in text and "int btf_collect_fold_in_depth(" in text
    assert fd.DEFAULT_SWEEPS >= 1 and fd.DEFAULT_SWEEPS & (fd.DEFAULT_SWEEPS - 1) == 0
