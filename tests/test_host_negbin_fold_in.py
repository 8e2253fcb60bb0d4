"""The host halves of negbin_fold_in_cols / negbin_fold_in_depth (functionalmf_amd/negbin_fold_in.py): no GPU."""
import os
import types

import numpy as np
import pytest

from functionalmf_amd import _native, fold_in_cols as fc, fold_in_depth as fd, negbin_fold_in as nf, utils
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

SWEEPS = 4


def column_problem(seed=0, N=9, T=7, K=3, tf=2):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    Y = rs.poisson(3.0, size=(N, T)).astype(float)
    Y[rs.uniform(size=(N, T)) < 0.25] = np.nan
    R = rs.randint(1, 6, size=(N, T)).astype(float)
    return W, Y, R, 0.2, tf, fc.random_draws(rs, T, K, tf, SWEEPS)


def slice_problem(seed=1, N=9, T=7, H=3, K=3, tf=2):
    rs = np.random.RandomState(seed)
    W, V_old = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = rs.poisson(3.0, size=(N, H)).astype(float)
    Y[rs.uniform(size=(N, H)) < 0.25] = np.nan
    R = rs.randint(1, 6, size=(N, H)).astype(float)
    return W, V_old, Y, R, 0.2, tf, fd.random_draws(rs, T, H, K, tf, SWEEPS)


def test_integer_rates_give_the_binomial_chain_on_the_pseudo_data():
    """With integer R and the same draws and the same seeded polya_gamma stream (fold_in_cols.chain and fold_in_depth.chain
    have no omega hook), chain_cols / chain_depth equal the Binomial chains on (Y, Y + R), bit for bit."""
    W, Y, R, lam2, tf, draws = column_problem()
    a = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, seed=5)
    b = fc.chain((Y, Y + R), W, None, lam2, tf, SWEEPS, draws, family="binomial", seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.all(np.isfinite(a[0]))
    W, V_old, Y, R, lam2, tf, draws = slice_problem()
    a = nf.chain_depth(Y, W, V_old, R, lam2, tf, SWEEPS, draws, seed=5)
    b = fd.chain((Y, Y + R), W, V_old, None, lam2, tf, SWEEPS, draws, family="binomial", seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.all(np.isfinite(a[0]))


def test_omega_replay_is_deterministic_and_read_where_observed():
    """draws and omega together make a chain a function of its inputs; omega is read at the observed cells alone; with the
    weights polya_gamma would have drawn the replay is the seeded chain."""
    W, Y, R, lam2, tf, draws = column_problem()
    N, T = Y.shape
    rs = np.random.RandomState(3)
    omega = rs.gamma(2.0, 0.5, size=(SWEEPS, N, T))
    a = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, omega=omega)
    other = omega.copy()
    other[:, np.isnan(Y)] = 77.0
    b = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, omega=other, seed=123)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    seen = []
    pg = fc.polya_gamma
    try:
        fc.polya_gamma = lambda rng, n, psi: seen.append(pg(rng, n, psi)) or seen[-1]
        c = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, seed=9)
    finally:
        fc.polya_gamma = pg
    d = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, omega=np.array(seen))
    assert all(np.array_equal(x, y) for x, y in zip(c, d))
    with pytest.raises(ValueError, match="omega"):
        nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, omega=omega[:-1])


def dense_rate(kind, R):
    """The (N,D) rate of a layout written out cell by cell, without numpy's broadcasting: "scalar" 2.5 everywhere, "row"
    R[i, 0], "depth" R[0, t], "cell" R[i, t]."""
    out = np.empty(R.shape)
    for i in range(R.shape[0]):
        for t in range(R.shape[1]):
            out[i, t] = {"scalar": 2.5, "row": R[i, 0], "depth": R[0, t], "cell": R[i, t]}[kind]
    return out


def test_every_rate_layout_is_the_chain_of_the_dense_rate():
    """A shared axis means the same rate at every cell along it: the chain of a compact rate equals the chain of the dense
    rate assembled cell by cell, and - integer rates - the Binomial chain on (Y, Y + dense) with the same seeded stream, so
    a rate read along the wrong axis cannot pass."""
    W, Y, R, lam2, tf, draws = column_problem()
    N, T = Y.shape
    omega = np.random.RandomState(4).gamma(2.0, 0.5, size=(SWEEPS, N, T))
    seen_v = []
    for kind, rate in (("scalar", 2.5), ("row", R[:, :1]), ("depth", R[:1]), ("cell", R)):
        full = dense_rate(kind, R)
        a = nf.chain_cols(Y, W, rate, lam2, tf, SWEEPS, draws, omega=omega)
        b = nf.chain_cols(Y, W, full, lam2, tf, SWEEPS, draws, omega=omega)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        if kind != "scalar":
            c = nf.chain_cols(Y, W, rate, lam2, tf, SWEEPS, draws, seed=5)
            e = fc.chain((Y, Y + full), W, None, lam2, tf, SWEEPS, draws, family="binomial", seed=5)
            assert all(np.array_equal(x, y) for x, y in zip(c, e))
        seen_v.append(a[0])
    assert all(not np.array_equal(seen_v[0], v) for v in seen_v[1:]) and not np.array_equal(seen_v[1], seen_v[2])   # the layouts differ
    W, V_old, Y, R, lam2, tf, draws = slice_problem()
    H = Y.shape[1]
    omega = omega[:, :, :H]
    for kind, rate in (("scalar", 2.5), ("row", R[:, :1]), ("depth", R[:1]), ("cell", R)):
        full = dense_rate(kind, R)
        a = nf.chain_depth(Y, W, V_old, rate, lam2, tf, SWEEPS, draws, omega=omega)
        b = nf.chain_depth(Y, W, V_old, full, lam2, tf, SWEEPS, draws, omega=omega)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        if kind != "scalar":
            c = nf.chain_depth(Y, W, V_old, rate, lam2, tf, SWEEPS, draws, seed=5)
            e = fd.chain((Y, Y + full), W, V_old, None, lam2, tf, SWEEPS, draws, family="binomial", seed=5)
            assert all(np.array_equal(x, y) for x, y in zip(c, e))
    # resolve_rate and rate_strides: the kernels' (sample, chain, row, depth) order and the strides of the compact array
    S, C = 3, 2
    rs = np.random.RandomState(5)
    for shape, strides in (((S,), (1, 0, 0, 0)), ((S, 1, N, 1), (N, 0, 1, 0)), ((S, 1, 1, T), (T, 0, 0, 1)), ((S, 1, N, T), (N * T, 0, T, 1)),
                           ((S, C, 1, 1), (C, 1, 0, 0)), ((S, C, N, T), (C * N * T, N * T, T, 1))):
        r = rs.uniform(1, 2, size=shape)
        arr, st = nf.rate_strides(nf.resolve_rate("cols", None, r, S, C, N, T))
        assert st == strides and arr.flags["C_CONTIGUOUS"]
        full = np.broadcast_to(r.reshape(shape + (1,) * (4 - len(shape))), (S, C, N, T))
        idx = np.add.outer(np.add.outer(np.add.outer(np.arange(S) * st[0], np.arange(C) * st[1]), np.arange(N) * st[2]), np.arange(T) * st[3])
        assert np.array_equal(arr.reshape(-1)[idx], full)
    Rfit = rs.uniform(1, 2, size=(S, N, 1, T))                            # the model's (rows, columns, depths) order
    arr = nf.resolve_rate("cols", Rfit, None, S, C, N, T)
    assert arr.shape == (S, 1, N, T) and np.array_equal(arr[:, 0], Rfit[:, :, 0])
    Rfit = rs.uniform(1, 2, size=(S, N, C, 1))
    arr = nf.resolve_rate("depth", Rfit, None, S, C, N, H)
    assert arr.shape == (S, C, N, 1) and np.array_equal(arr[:, :, :, 0], Rfit[:, :, :, 0].transpose(0, 2, 1))
    r = rs.uniform(1, 2, size=(S, N, 1, H))                               # rate= for depths: against (N,M,H)
    assert np.array_equal(nf.resolve_rate("depth", None, r, S, C, N, H), r.transpose(0, 2, 1, 3))


def test_replicates():
    """(C,N,T,2) with one replicate nan equals the single-replicate call; two observed replicates double c."""
    W, Y, R, lam2, tf, draws = column_problem()
    N, T = Y.shape
    omega = np.random.RandomState(4).gamma(2.0, 0.5, size=(SWEEPS, N, T))
    Y2 = np.stack([Y, np.full(Y.shape, np.nan)], axis=-1)
    a = nf.chain_cols(Y, W, R, lam2, tf, SWEEPS, draws, omega=omega)
    b = nf.chain_cols(Y2, W, R, lam2, tf, SWEEPS, draws, omega=omega)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c1, y1 = nf.cell_statistics(Y[None], (1, N, T))
    c2, y2 = nf.cell_statistics(Y2[None], (1, N, T))
    assert np.array_equal(c1, c2) and np.array_equal(y1, y2) and set(np.unique(c1)) == {0.0, 1.0}
    c3, y3 = nf.cell_statistics(np.stack([Y, Y], axis=-1)[None], (1, N, T))
    assert np.array_equal(c3, 2 * c1) and np.array_equal(y3, 2 * y1)
    b_pg, kappa = nf._pseudo(c3[0], y3[0], R)
    seen = c3[0] > 0
    assert np.array_equal(b_pg[seen], (y3[0] + 2 * R)[seen]) and np.array_equal(kappa[seen], ((y3[0] - 2 * R) / 2)[seen])
    assert np.all(b_pg[~seen] == 0) and np.all(kappa[~seen] == 0)


def test_argument_checks():
    S, C, N, T, K, tf = 3, 2, 6, 5, 2, 2
    rs = np.random.RandomState(0)
    Y = rs.poisson(3.0, size=(C, N, T)).astype(float)
    # counts
    for bad in (-Y - 1, Y + 0.5, np.where(Y > 2, np.inf, Y)):
        with pytest.raises(ValueError, match="non-negative integers"):
            nf.cell_statistics(bad, (C, N, T))
    for bad in (np.zeros((C, N)), np.zeros((C, N + 1, T)), np.zeros((C, N, T, 2, 2)), np.zeros((C, N, T, 0))):
        with pytest.raises(ValueError, match="must be"):
            nf.cell_statistics(bad, (C, N, T))
    # the rate
    with pytest.raises(ValueError, match="pass rate="):
        nf.resolve_rate("cols", np.ones((S, N, 4, T)), None, S, C, N, T)          # varies along the columns
    with pytest.raises(ValueError, match="pass rate="):
        nf.resolve_rate("depth", np.ones((S, N, C, T)), None, S, C, N, 3)         # varies along the depths
    with pytest.raises(ValueError, match="pass rate="):
        nf.resolve_rate("cols", None, None, S, C, N, T)
    for bad in (np.zeros(S), -np.ones(S), np.full(S, np.nan), np.full(S, np.inf)):
        with pytest.raises(ValueError, match="finite and positive"):
            nf.resolve_rate("cols", None, bad, S, C, N, T)
    for bad in (np.ones(S + 1), np.ones((S, C, N + 1, T)), np.ones((S, 2, 2)), 3.0):
        with pytest.raises(ValueError):
            nf.resolve_rate("cols", None, bad, S, C, N, T)
    assert nf.resolve_rate("depth", None, None, S, C, N, 3, needed=False).shape == (S, 1, 1, 1)
    # draws, omega, sizes
    draws = fc.random_draws(rs, T, K, tf, 2, size=(S, C))
    omega = np.ones((S, C, 2, N, T))
    with pytest.raises(ValueError, match="omega"):
        nf.check_args("cols", S, C, N, T, K, tf, draws=draws, sweeps=2)
    d, o, qs, tcode, sweeps = nf.check_args("cols", S, C, N, T, K, tf, draws=draws, omega=omega, sweeps=2)
    assert d.shape == draws.shape and o.shape == omega.shape and sweeps == 2
    assert nf.check_args("cols", S, C, N, T, K, tf)[4] == fc.DEFAULT_SWEEPS == nf.DEFAULT_SWEEPS["cols"]
    assert nf.check_args("depth", S, C, N, T, K, tf, horizon=3)[4] == fd.DEFAULT_SWEEPS == nf.DEFAULT_SWEEPS["depth"]
    for kw in (dict(omega=omega[:, :, :1], sweeps=2), dict(omega=-omega, sweeps=2), dict(omega=omega * np.nan, sweeps=2), dict(sweeps=0),
               dict(q=(5, 120)), dict(transform="cube"), dict(first_sample=-1)):
        with pytest.raises(ValueError):
            nf.check_args("cols", S, C, N, T, K, tf, **kw)
    with pytest.raises(ValueError):
        nf.check_args("rows", S, C, N, T, K, tf)
    with pytest.raises(ValueError, match="LDS"):
        nf.check_args("cols", S, C, 20000, T, K, tf)
    with pytest.raises(ValueError, match="horizon"):
        nf.slice_cells(None, N, C)
    with pytest.raises(ValueError, match="horizon"):
        nf.slice_cells(np.zeros((N, C, 3)), N, C, horizon=2)
    assert nf.slice_cells(None, N, C, horizon=4)[1].shape == (N, C, 4)
    # the stateless calls refuse before any device call
    Ws = np.ones((S, N, K))
    with pytest.raises(ValueError):
        utils.negbin_fold_in_cols(Y, Ws, None, lam2=np.ones(S))
    with pytest.raises(ValueError):
        utils.negbin_fold_in_cols(Y, Ws, np.ones(S), lam2=-np.ones(S))
    with pytest.raises(ValueError, match="1e\\+15|below"):
        utils.negbin_fold_in_cols(Y, Ws, np.full(S, 1e15), lam2=np.ones(S))
    with pytest.raises(ValueError):
        utils.negbin_fold_in_depth(np.zeros((N, C, 2)), Ws, np.ones((S, C, T, K)), None, lam2=np.ones(S))
    with pytest.raises(ValueError, match="finite"):
        utils.negbin_fold_in_depth(np.zeros((N, C, 2)), Ws, np.full((S, C, T, K), np.nan), np.ones(S), lam2=np.ones(S))


def test_lds_bytes_is_the_c_count():
    lib = _native.load()
    for (n, t, h, k, o) in ((5, 6, None, 3, 2), (130, 8, None, 10, 2), (64, 9, 3, 5, 1), (512, 64, 8, 5, 2), (50, 370, 8, 10, 2), (19, 228, 8, 5, 0)):
        want = (fc.lds_bytes(t, k, o) if h is None else fd.lds_bytes(t, h, k, o)) + 8 * n
        assert nf.lds_bytes(n, t, k, o, h) == want == lib.btf_negbin_fold_lds_bytes(n, t, h or 0, k, o)
    assert lib.btf_negbin_fold_lds_bytes(0, 6, 0, 3, 2) == -1 and lib.btf_negbin_fold_lds_bytes(5, 6, 0, 11, 2) == -1
    assert nf.LDS_LIMIT == 156 * 1024


class _NoDevice:
    device = 0

    def call(self, *a):
        raise AssertionError("a device call was made")


def _bare(world=1):
    m = object.__new__(NegativeBinomialBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.tf_order, m.stability = 6, 3, 5, 2, 2, 1e-6
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    m._collected, m._draws, m._device_seed, m._callback = 0, 0, 1, False
    return m


def test_the_model_routes_to_the_module_and_the_old_calls_still_raise(monkeypatch):
    S = 4
    res = {"W": np.ones((S, 6, 2)), "V": np.ones((S, 3, 5, 2)), "lam2": np.ones((S, 1)), "R": np.full((S, 6, 1, 1), 2.0)}
    m = _bare()
    for call, Y in ((m.fold_in_cols, np.zeros((1, 6, 5))), (m.fold_in_depth, np.zeros((6, 3, 2))), (m.slice_fold_in_depth, np.zeros((6, 3, 2))),
                    (m.fold_in_rows, np.zeros((1, 3, 5)))):
        with pytest.raises(NotImplementedError, match="Negative-Binomial"):
            call(Y, results=res)
    seen = []
    monkeypatch.setattr(nf, "evaluate", lambda *a, **kw: seen.append((a, kw)) or {"V": None})
    m.negbin_fold_in_cols(np.ones((2, 6, 5)), res, seed=3, sweeps=7)
    a, kw = seen[-1]
    assert a[:7] == ("cols", S, 2, 6, 5, 2, 2) and a[9].shape == (S, 1, 6, 1) and kw["seed"] == 3 and kw["sweeps"] == 7
    assert a[7].shape == (2, 6, 5) and np.all(a[7] == 1) and np.all(a[8] == 1)
    m.negbin_fold_in_depth(np.ones((6, 3, 2)), res, rate=np.full((S, 1, 3, 2), 4.0))
    a, kw = seen[-1]
    assert a[:7] == ("depth", S, 3, 6, 5, 2, 2) and a[9].shape == (S, 3, 1, 2) and np.all(a[9] == 4.0) and kw["horizon"] == 2
    m.negbin_fold_in_depth(None, dict(res, R=np.ones((S, 6, 3, 5))), horizon=3)          # the forecast reads no rate
    assert seen[-1][1]["horizon"] == 3 and not seen[-1][0][7].any()
    with pytest.raises(ValueError, match="pass rate="):
        m.negbin_fold_in_depth(np.ones((6, 3, 2)), dict(res, R=np.ones((S, 6, 3, 5))))
    with pytest.raises(ValueError, match="pass rate="):
        m.negbin_fold_in_cols(np.ones((2, 6, 5)), dict(res, R=np.ones((S, 1, 3, 1))))
    with pytest.raises(RuntimeError, match="keeps its samples on the host"):
        m.negbin_fold_in_cols(np.ones((2, 6, 5)), None)
    with pytest.raises(NotImplementedError, match="unsharded"):
        _bare(world=2).negbin_fold_in_cols(np.ones((2, 6, 5)), res)
    for bad in (np.ones((2, 5, 5)), np.ones((6, 5)), -np.ones((2, 6, 5))):
        with pytest.raises(ValueError):
            m.negbin_fold_in_cols(bad, res)
    with pytest.raises(ValueError):
        m.negbin_fold_in_cols(np.ones((2, 6, 5)), dict(res, lam2=-np.ones(S)))


def test_registration_and_the_stored_oracle():
    for unit, getter in (("btf_fold_in_cols.hip", "fold_cols_negbin_fn"), ("btf_fold_in_depth.hip", "fold_depth_negbin_fn")):
        with open(os.path.join(_native.CSRC, unit)) as f:                 # the family is instantiated in its siblings' units
            assert getter in f.read()
    assert len(_native.SIGNATURES["btf_negbin_fold_in_cols"][1]) == 30 and len(_native.SIGNATURES["btf_negbin_fold_in_depth"][1]) == 32
    with open(os.path.join(_native.ROOT, "include", "btf.h")) as f:
        text = f.read()
    for name in ("int btf_negbin_fold_in_cols(", "int btf_negbin_fold_in_depth(", "long long btf_negbin_fold_lds_bytes("):
        assert name in text
    assert set(fc.FAMILIES.values()) == {0, 1} and set(fd.FAMILIES.values()) == {0, 1}      # the Gibbs tables keep their two families
    from conftest import load_golden
    g = load_golden("negbin_fold_in_oracle.npz")
    b = np.where(np.isnan(g["Y"]), 0.0, g["Y"] + float(g["rate"]))
    assert float(g["rate"]) == 50.0 and (b >= 200).any() and ((b > 0) & (b < 200)).any() and np.nanmax(g["Y"]) >= 200
    assert g["mean"].shape == g["Y"].shape and np.all(g["se"] > 0) and np.all((g["mean"] > 0) & (g["mean"] < 1))
