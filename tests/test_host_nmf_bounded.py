"""Host halves of bounded_tensor_nmf (functionalmf_amd/nmf.py): the argument checks made before any device call, the
seeded starting point with its R draw, the self-consistency of the fixture of make_golden_nmf_bounded.py and the normal
equations the device projects on.  No GPU."""
import numpy as np
import pytest

from functionalmf_amd import _native, nmf, utils
from test_host_nmf import no_device  # noqa: F401  (the fixture: any call into the native library fails the test)

CASES = ["complete", "missing", "monotone", "k1", "k10", "fixW_neg", "features", "features_free", "features_mono"]


def test_bad_arguments_raise_before_any_device_call(no_device):  # noqa: F811
    Y = np.ones((4, 3, 5, 2))
    X = np.ones((4, 2))
    for kw in (dict(max_entry=0.0), dict(max_entry=-1.0), dict(max_entry=np.nan), dict(max_entry=np.inf),
               dict(R=np.ones((2, 2))), dict(row_features=np.ones((3, 2))), dict(row_features=np.ones(4)),
               dict(row_features=np.ones((4, 0))), dict(row_features=X, R=np.ones((3, 2))),
               dict(row_features=X, R=np.ones((2, 3))), dict(row_features=np.full((4, 2), np.inf)),
               dict(W=np.ones((4, 3))), dict(V=np.ones((3, 4, 2))), dict(max_steps=-1)):
        with pytest.raises(ValueError):
            utils.bounded_tensor_nmf(Y, 2, **kw)
    for bad in (np.nan, np.inf, -np.inf):                    # non-finite input (nan in Y or row_features is "missing")
        Wb, Vb, Rb = np.ones((4, 2)), np.ones((3, 5, 2)), np.ones((2, 2))
        Wb[0, 1] = bad
        Vb[0, 0, 1] = bad
        Rb[1, 1] = bad
        for kw, name in ((dict(W=Wb), "W"), (dict(V=Vb), "V"), (dict(row_features=X, R=Rb), "R")):
            with pytest.raises(ValueError, match=name + " must be finite"):
                utils.bounded_tensor_nmf(Y, 2, max_entry=0.999, **kw)
        if np.isinf(bad):
            Yb = Y.copy()
            Yb[3, 0, 0, 0] = bad
            with pytest.raises(ValueError, match="Y must be finite"):
                utils.bounded_tensor_nmf(Yb, 2, max_entry=0.999, row_features=X)
    for k in (0, 11, 2.5, True):
        with pytest.raises(ValueError):
            utils.bounded_tensor_nmf(Y, k, max_entry=0.999)
    with pytest.raises(ValueError):
        utils.bounded_tensor_nmf(np.ones((4, 3)), 2, max_entry=0.999)


def test_tensor_nmf_still_refuses_and_names_the_new_function(no_device):  # noqa: F811
    Y = np.ones((4, 3, 5, 2))
    with pytest.raises(NotImplementedError, match="bounded_tensor_nmf"):
        utils.tensor_nmf(Y, 2, max_entry=0.999)
    with pytest.raises(NotImplementedError, match="bounded_tensor_nmf"):
        utils.tensor_nmf(Y, 2, row_features=np.ones((4, 2)))


def test_entry_points_are_declared():
    for name in ("btf_nmf_set_bounds", "btf_nmf_set_row_features", "btf_nmf_run_bounded"):
        assert name in _native.SIGNATURES
    assert utils.bounded_tensor_nmf is nmf.bounded_tensor_nmf


def test_seeded_starting_point_draws_R_after_W_and_V(golden, monkeypatch):
    """np.random.seed(s) gives the reference's W0, V0 and then R0 (utils.py:283-295); given factors are passed on."""
    g = golden("g15_nmf_bounded.npz")
    seen = {}

    class _Started(Exception):
        pass

    def fake_run(self, W, V, **kw):
        seen.update(W=np.array(W), V=np.array(V), R=kw.get("R"), X=kw.get("row_features"), max_entry=kw.get("max_entry"))
        raise _Started

    monkeypatch.setattr(nmf.NMFData, "__init__", lambda self, Y, K, device=0: None)
    monkeypatch.setattr(nmf.NMFData, "run", fake_run)
    monkeypatch.setattr(nmf.NMFData, "close", lambda self: None)
    for case in CASES:
        p = case + "_"
        X = g[p + "X"] if p + "X" in g else None
        np.random.seed(int(g[p + "seed"]))
        with pytest.raises(_Started):
            utils.bounded_tensor_nmf(g[p + "Y"], int(g[p + "K"]), max_entry=0.999, row_features=X,
                                     W=g[p + "W_in"] if p + "W_in" in g else None)
        assert np.array_equal(seen["W"], g[p + "W0"]) and np.array_equal(seen["V"], g[p + "V0"]), case
        assert seen["max_entry"] == 0.999
        if X is None:
            assert seen["R"] is None and seen["X"] is None
        else:
            assert np.array_equal(seen["R"], g[p + "R0"]), case
            assert np.array_equal(seen["X"], X, equal_nan=True)


def test_fixture_is_self_consistent(golden):
    """tol_x is the largest distance between the reference's projected solutions and the tight ones, tol_gpu ten times
    it; projected systems are those with a positive overshoot; at most 5 % of a half-step's systems lie within tol_x of
    the bound; the tight solutions are feasible and no worse than the reference's."""
    g = golden("g15_nmf_bounded.npz")
    assert [str(c) for c in g["cases"]] == CASES
    tol_all, viol = 0.0, 0.0
    for case in CASES:
        p = case + "_"
        tol = 0.0
        kinds = ["rows", "cells"] + (["feats"] if p + "X" in g else [])
        for kind in kinds:
            over, rx, tx = g[p + "over_" + kind], g[p + "ref_x_" + kind], g[p + "tight_x_" + kind]
            proj = over > 0
            assert np.array_equal(~np.isnan(rx[..., 0]), proj) and np.array_equal(~np.isnan(tx[..., 0]), proj), (case, kind)
            if proj.any():
                tol = max(tol, float(np.nanmax(np.abs(rx - tx))))
                assert np.nanmin(tx) >= 1e-6 - 1e-12
            for n in range(over.shape[0]):
                v = over[n][~np.isnan(over[n])]
                if v.size:
                    assert np.mean(np.abs(v) < float(g[p + "tol_x"])) <= 0.05, (case, kind, n)
        assert tol == float(g[p + "tol_x"]) and float(g[p + "tol_gpu"]) == 10 * tol, case
        assert float(g[p + "excused_share"]) <= 0.05 and float(g[p + "cond"]) < 1e10
        k = min(int(g[p + "steps"]), int(g[p + "steps_exact"]))
        dd = np.abs(g[p + "deltas"][1:k] - g[p + "deltas_exact"][1:k])
        assert float(g[p + "delta_slack"]) == (dd.max() if dd.size else 0.0) and int(g[p + "steps_exact"]) == int(g[p + "steps"])
        tol_all = max(tol_all, tol)
        if case != "features_free":
            assert np.isfinite(float(g[p + "max_entry"])) and tol > 0
    assert float(g["tol_x"]) == tol_all and float(g["tol_gpu"]) == 10 * tol_all
    assert 0.0 <= float(g["ref_viol"]) < 1e-6
    assert int(g["fixW_neg_lower_active"]) > 0
    # rows with fewer unknowns than K are among the projected ones of the complete-data case
    assert (g["complete_over_rows"][:, :2] > 0).any()
    X = g["features_X"]
    assert np.isnan(X[:, 3]).all() and np.isnan(X[5]).all() and 0.1 < np.isnan(np.delete(np.delete(X, 3, 1), 5, 0)).mean() < 0.4


def test_normal_equation_objective_equals_the_references_up_to_a_constant():
    """1/2 |b - A x|^2 of a row's system (design rows v_jt repeated per observed replicate, plus the observed feature
    rows r_f) equals 1/2 x'G x - h'x + 1/2 b'b with G = sum C v v' + sum_f r_f r_f', h = sum S v + sum_f x_f r_f built
    from nmf_statistics: the device minimises the same function."""
    rs = np.random.RandomState(3)
    N, M, T, R, K, F = 5, 4, 3, 3, 3, 4
    Y = rs.uniform(size=(N, M, T, R))
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    Y[1, 2] = np.nan
    V = rs.gamma(1, 1, size=(M, T, K))
    Rf = rs.gamma(1, 1, size=(F, K))
    X = (rs.uniform(size=(N, F)) < 0.5).astype(float)
    X[rs.uniform(size=X.shape) < 0.3] = np.nan
    S, cnt, _ = nmf.nmf_statistics(Y)
    Vm = V.reshape(-1, K)
    for i in range(N):
        d = min(K, i + 1)
        y = Y[i].ravel()
        ok = ~np.isnan(y)
        fo = ~np.isnan(X[i])
        A = np.concatenate([np.repeat(Vm, R, axis=0)[ok], Rf[fo]])[:, :d]
        b = np.concatenate([y[ok], X[i, fo]])
        G = (Vm[:, :d] * cnt[i][:, None]).T @ Vm[:, :d] + Rf[fo, :d].T @ Rf[fo, :d]
        h = Vm[:, :d].T @ S[i] + Rf[fo, :d].T @ X[i, fo]
        for _ in range(3):
            x = rs.gamma(1, 1, size=d)
            ref = 0.5 * np.sum((b - A @ x) ** 2)
            got = 0.5 * x @ G @ x - h @ x + 0.5 * b @ b
            assert abs(got - ref) <= 1e-12 * max(1.0, ref)
