"""bounded_tensor_nmf on the GPU (nmf_project_kernel and the feature fit of csrc/btf_nmf.h) against the reference's
tensor_nmf(max_entry=..., row_features=...) as recorded by tests/golden/make_golden_nmf_bounded.py.

The reference projects with SLSQP at ftol 1e-8, which stops up to tol_x (recorded per case, 2e-10 .. 1e-2) short of the
QP's minimiser; the device solves the QP exactly.  So every comparison restarts from a recorded reference state and runs
one half-step (rows, or cells and features), where the systems are independent of each other and SLSQP's slack cannot
travel from one system to the next:
  * a projected system agrees with the reference to 10 tol_x (the fixture's tol_gpu: SLSQP's own stopping slack from
    another starting iterate) and with the fixture's tight solve of the same QP to 1e3 cond(A'A) eps (G and h are sums of
    a few hundred products taken in another order than numpy's, amplified by the conditioning of the system);
  * a system that is not projected agrees to test_gpu_nmf.py's rtol 1e-9;
  * with monotone=True the PAV projection pools the depths of a column: a column with a projected cell is compared at
    10 tol_x as a whole (a pool's value is a convex combination of its members, so the slack is not amplified).
"""
import numpy as np
import pytest

from functionalmf_amd import nmf, utils

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
XMIN = 1e-6
CASES = ["complete", "missing", "monotone", "k1", "k10", "fixW_neg", "features", "features_free", "features_mono"]


def _case(g, case):
    p = case + "_"
    me = float(g[p + "max_entry"])
    return dict(p=p, Y=g[p + "Y"], K=int(g[p + "K"]), max_entry=None if np.isnan(me) else me,
                X=g[p + "X"] if p + "X" in g else None, monotone=bool(g[p + "monotone"]), fit_W=bool(g[p + "fit_W"]),
                fit_V=bool(g[p + "fit_V"]), steps=int(g[p + "steps"]), tol_x=float(g[p + "tol_x"]),
                tol_gpu=float(g[p + "tol_gpu"]), tol_tight=1e3 * float(g[p + "cond"]) * EPS)


def _state(g, c, n):
    """The reference's factors after n steps (n = 0: the start)."""
    p = c["p"]
    if n == 0:
        return g[p + "W0"], g[p + "V0"], (g[p + "R0"] if c["X"] is not None else None)
    return g[p + "Ws"][n - 1], g[p + "Vs"][n - 1], (g[p + "Rs"][n - 1] if c["X"] is not None else None)


_halves = {}


def _half(g, case, n, which):
    """One half-step from the reference's state: which = "W": the rows from step n's start; "V": the cells and features
    from the reference's W of step n + 1 and the V, R of step n's start.  Computed once per (case, n, which)."""
    key = (case, n, which)
    if key not in _halves:
        c = _case(g, case)
        W, V, R = _state(g, c, n)
        if which == "V":
            W = _state(g, c, n + 1)[0]
        out = utils.bounded_tensor_nmf(c["Y"], c["K"], max_entry=c["max_entry"], row_features=c["X"], R=R, max_steps=1,
                                       monotone=c["monotone"], W=W, V=V, fit_W=which == "W", fit_V=which == "V",
                                       return_info=True)
        _halves[key] = out
    return _halves[key]


def _systems(g, case):
    """Every fitted system of every half-step: (n, kind, index, d, over, x_gpu, x_ref, x_tight, x_before, flag_gpu,
    constraint rows) with x_* the leading d entries."""
    c = _case(g, case)
    p = c["p"]
    K = c["K"]
    for n in range(c["steps"]):
        Wp, Vp, Rp = _state(g, c, n)
        Wn, Vn, Rn = _state(g, c, n + 1)
        if c["fit_W"]:
            out = _half(g, case, n, "W")
            info = out[-1]
            for i in range(Wp.shape[0]):
                d = min(K, i + 1)
                yield dict(n=n, kind="rows", idx=(i,), d=d, over=g[p + "over_rows"][n, i], x=out[0][i, :d], ref=Wn[i, :d],
                           tight=g[p + "tight_x_rows"][n, i, :d], rest=(out[0][i, d:], Wp[i, d:]),
                           flag=bool(info["projected_rows"][i]) if c["max_entry"] else False, Cq=Vp.reshape(-1, K)[:, :d])
        if c["fit_V"]:
            out = _half(g, case, n, "V")
            info = out[-1]
            for j in range(Vp.shape[0]):
                for t in range(Vp.shape[1]):
                    yield dict(n=n, kind="cells", idx=(j, t), d=K, over=g[p + "over_cells"][n, j, t], x=out[1][j, t],
                               ref=Vn[j, t], tight=g[p + "tight_x_cells"][n, j, t], rest=None,
                               flag=bool(info["projected_cells"][j, t]) if c["max_entry"] else False, Cq=Wn)
            if c["X"] is not None:
                for f in range(c["X"].shape[1]):
                    yield dict(n=n, kind="feats", idx=(f,), d=K, over=g[p + "over_feats"][n, f], x=out[2][f], ref=Rn[f],
                               tight=g[p + "tight_x_feats"][n, f], rest=(out[2][f], Rp[f]) if np.isnan(g[p + "over_feats"][n, f]) else None,
                               flag=bool(info["projected_features"][f]) if c["max_entry"] else False, Cq=Wn)


@pytest.mark.parametrize("case", CASES)
def test_half_steps_from_the_reference_states_match_the_reference(golden, case):
    """The module's contract for every system of every half-step; the largest distances are printed before they are
    asserted.  Measured on an MI355X: projected systems lie 2e-10 (k1) .. 1.0e-2 (k10) from the reference, which is
    the reference's own recorded tol_x in every case, and at most 7e-14 from the tight solutions; systems that are not
    projected agree to 4e-12 relative."""
    g = golden("g15_nmf_bounded.npz")
    c = _case(g, case)
    worst = {"projected_vs_ref": 0.0, "projected_vs_tight": 0.0, "plain_rel": 0.0}
    bad = []
    cols_projected = set()
    for s in _systems(g, case):
        ref_proj = s["over"] > 0
        if s["rest"] is not None:
            assert np.array_equal(*s["rest"]), (s["kind"], s["idx"])        # entries that are never fitted stay
        if np.isnan(s["over"]):
            continue                                                         # a feature nobody observed: checked above
        if s["kind"] == "cells" and (ref_proj or s["flag"]):
            cols_projected.add((s["n"], s["idx"][0]))
        if ref_proj != s["flag"]:
            continue                                                         # the flag test judges these
        if c["monotone"] and s["kind"] == "cells":
            continue                                                         # after PAV: by column, below
        if ref_proj:
            e_ref = float(np.max(np.abs(s["x"] - s["ref"])))
            e_tight = float(np.max(np.abs(s["x"] - s["tight"])) / max(1.0, np.max(np.abs(s["tight"]))))
            worst["projected_vs_ref"] = max(worst["projected_vs_ref"], e_ref)
            worst["projected_vs_tight"] = max(worst["projected_vs_tight"], e_tight)
            if e_ref > c["tol_gpu"] or e_tight > c["tol_tight"]:
                bad.append((s["n"], s["kind"], s["idx"], e_ref, e_tight))
        else:
            rel = float(np.max(np.abs(s["x"] - s["ref"]) / (1e-3 + np.abs(s["ref"]))))
            worst["plain_rel"] = max(worst["plain_rel"], rel)
            if not np.allclose(s["x"], s["ref"], rtol=1e-9, atol=1e-12):
                bad.append((s["n"], s["kind"], s["idx"], rel))
    if c["monotone"] and c["fit_V"]:
        for n in range(c["steps"]):
            Vg, Vr = _half(g, case, n, "V")[1], _state(g, c, n + 1)[1]
            for j in range(Vg.shape[0]):
                if (n, j) in cols_projected:
                    e = float(np.max(np.abs(Vg[j] - Vr[j])))
                    worst["projected_vs_ref"] = max(worst["projected_vs_ref"], e)
                    if e > c["tol_gpu"]:
                        bad.append((n, "column", j, e))
                elif not np.allclose(Vg[j], Vr[j], rtol=1e-9, atol=1e-12):
                    bad.append((n, "column", j, float(np.max(np.abs(Vg[j] - Vr[j])))))
    print(case, "tol_gpu %.3g tol_tight %.3g" % (c["tol_gpu"], c["tol_tight"]), worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("case", [c for c in CASES if c != "features_free"])
def test_the_same_systems_are_projected_as_in_the_reference(golden, case):
    """A flag may differ from the reference's only where its overshoot over max_entry is below tol_x, and for at most
    5 % of the systems of a half-step."""
    g = golden("g15_nmf_bounded.npz")
    c = _case(g, case)
    count, differ, nproj = {}, {}, 0
    for s in _systems(g, case):
        if np.isnan(s["over"]):
            assert not s["flag"]
            continue
        key = (s["n"], s["kind"])
        count[key] = count.get(key, 0) + 1
        nproj += s["flag"]
        if (s["over"] > 0) != s["flag"]:
            assert abs(s["over"]) < c["tol_x"], (s["n"], s["kind"], s["idx"], s["over"])
            differ[key] = differ.get(key, 0) + 1
    print(case, "projected", nproj, "flags that differ", differ)
    assert nproj > 0
    for key, k in differ.items():
        assert k <= 0.05 * count[key], (key, k, count[key])
    # the per-step count of the run equals the flags of its one step
    for n in range(c["steps"]):
        for which in ("W", "V"):
            if c["fit_" + which]:
                info = _half(g, case, n, which)[-1]
                flags = int(info["projected_rows"].sum() + info["projected_cells"].sum() + info["projected_features"].sum())
                assert int(info["projected"][0]) == flags


@pytest.mark.parametrize("case", [c for c in CASES if c != "features_free"])
def test_projected_systems_are_feasible(golden, case):
    """-v <= c_q . x <= max_entry + v with v = the reference's recorded violation + 1e-9, and x >= 1e-6 - 1e-12; after
    PAV every cell still respects the upper side."""
    g = golden("g15_nmf_bounded.npz")
    c = _case(g, case)
    v = float(g["ref_viol"]) + 1e-9
    worst = {"upper": -np.inf, "lower": -np.inf, "xmin": -np.inf}
    for s in _systems(g, case):
        if np.isnan(s["over"]):
            continue
        cx = s["Cq"] @ s["x"]
        if c["monotone"] and s["kind"] == "cells":
            assert cx.max() <= c["max_entry"] + v, (s["n"], s["idx"], cx.max())
            continue
        if s["flag"]:
            worst["upper"] = max(worst["upper"], float(cx.max() - c["max_entry"]))
            worst["lower"] = max(worst["lower"], float(-cx.min()))
            worst["xmin"] = max(worst["xmin"], float(XMIN - s["x"].min()))
            assert -v <= cx.min() and cx.max() <= c["max_entry"] + v, (s["n"], s["kind"], s["idx"], cx.min(), cx.max())
            assert s["x"].min() >= XMIN - 1e-12, (s["n"], s["kind"], s["idx"], s["x"].min())
        else:
            assert cx.max() <= c["max_entry"], (s["n"], s["kind"], s["idx"])
    print(case, "v %.3g" % v, worst)
    if case == "fixW_neg":
        assert int(g["fixW_neg_lower_active"]) > 0 and worst["lower"] > -1e-9      # a lower side binds


def _full(g, case, **over):
    c = _case(g, case)
    p = c["p"]
    kw = dict(max_entry=c["max_entry"], row_features=c["X"], max_steps=int(g[p + "max_steps"]), monotone=c["monotone"],
              W=g[p + "W_in"] if p + "W_in" in g else None, V=g[p + "V_in"] if p + "V_in" in g else None, fit_W=c["fit_W"],
              fit_V=c["fit_V"], return_info=True)
    kw.update(over)
    np.random.seed(int(g[p + "seed"]))
    return utils.bounded_tensor_nmf(c["Y"], c["K"], **kw)


@pytest.mark.parametrize("case", CASES)
def test_seeded_full_runs_take_the_references_steps(golden, case):
    """The seeded full run: the reference's number of steps and its per-step deltas at rtol 1e-4 plus twice delta_slack,
    the reference's own error in that quantity as the fixture measures it (its run repeated with every SLSQP result
    replaced by the exact minimiser: 1.6e-12 at K = 1 up to 8.9e-6 at K = 10).  A delta is a difference of two nearly
    equal rmse, so late deltas of 1e-4 .. 1e-5 carry SLSQP's slack at 1e-4 of their size and more: measured on the
    monotone case, 6.18172e-5 here against 6.18271e-5 in the reference and 6.18172e-5 with exact projections."""
    g = golden("g15_nmf_bounded.npz")
    p = case + "_"
    out = _full(g, case)
    info = out[-1]
    r = info["rmse"]
    delta = (np.concatenate([[np.inf], r[:-1]]) - r) / r
    ref = g[p + "deltas"]
    slack = float(g[p + "delta_slack"])
    print(case, "steps", info["steps"], int(g[p + "steps"]), "deltas", delta, "reference", ref, "with exact projections",
          g[p + "deltas_exact"], "delta_slack", slack)
    assert info["steps"] == int(g[p + "steps"])
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(delta), fin)
    assert np.allclose(delta[fin], ref[fin], rtol=1e-4, atol=1e-9 + 2 * slack)
    if case == "features_free":                              # nothing is projected: the factors are the reference's
        for got, key in zip(out[:3], ("W", "V", "R")):
            assert np.max(np.abs(got - g[p + key])) <= 1e-8 * np.max(np.abs(g[p + key])), key


def _c3(N, M, T, R, K, seed):
    rs = np.random.RandomState(seed)
    Y = np.einsum("nk,mtk->nmt", rs.dirichlet(0.5 * np.ones(K), size=N), rs.uniform(0.05, 1.0, size=(M, T, K)))[..., None]
    Y = Y + rs.normal(0, 0.08, size=(N, M, T, R))
    Y[rs.uniform(size=Y.shape) < 0.05] = np.nan
    return Y, rs


@pytest.mark.parametrize("monotone", [False, True])
def test_without_bounds_or_features_the_bits_are_tensor_nmfs(monotone):
    Y, _ = _c3(70, 12, 10, 2, 4, seed=1)
    for Yc in (Y, np.nan_to_num(Y, nan=0.5)):                # with gaps, and complete
        np.random.seed(4)
        W1, V1, i1 = utils.tensor_nmf(Yc, 4, max_steps=6, monotone=monotone, return_info=True)
        np.random.seed(4)
        W2, V2, i2 = utils.bounded_tensor_nmf(Yc, 4, max_steps=6, monotone=monotone, return_info=True)
        assert np.array_equal(W1, W2) and np.array_equal(V1, V2) and np.array_equal(i1["rmse"], i2["rmse"])
    # a handle that ran bounded goes back to the plain bits
    data = nmf.NMFData(Y, 4)
    try:
        rs = np.random.RandomState(0)
        W0, V0 = rs.gamma(1, 1, (70, 4)), rs.gamma(1, 1, (12, 10, 4))
        a = data.run(W0, V0, max_steps=3, monotone=monotone)
        data.run(W0, V0, max_steps=3, monotone=monotone, max_entry=0.999)
        b = data.run(W0, V0, max_steps=3, monotone=monotone)
    finally:
        data.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_identical_bounded_calls_give_identical_bits():
    Y, rs = _c3(130, 20, 12, 3, 4, seed=2)
    X = np.where(rs.uniform(size=(130, 6)) < 0.2, np.nan, (rs.uniform(size=(130, 6)) < 0.5).astype(float))
    outs = []
    for _ in range(2):
        np.random.seed(9)
        outs.append(utils.bounded_tensor_nmf(Y, 4, max_entry=0.999, row_features=X, max_steps=5, monotone=True, return_info=True))
    a, b = outs
    assert all(np.array_equal(a[q], b[q]) for q in range(3)) and np.array_equal(a[3]["rmse"], b[3]["rmse"])
    assert np.array_equal(a[3]["projected"], b[3]["projected"]) and a[3]["projected"].sum() > 0
    Mu = np.einsum("nk,mtk->nmt", a[0], a[1])
    assert Mu.max() <= 0.999 + 1e-9 and Mu.min() >= -1e-9


def test_the_R_draw_follows_W_and_V_in_the_legacy_stream(golden):
    g = golden("g15_nmf_bounded.npz")
    W, V, R, info = _full(g, "features", max_steps=0)
    assert info["steps"] == 0
    assert np.array_equal(W, g["features_W0"]) and np.array_equal(V, g["features_V0"]) and np.array_equal(R, g["features_R0"])
    R1 = np.full_like(R, 0.5)                                # a given R is used as it is
    assert np.array_equal(_full(g, "features", max_steps=0, R=R1)[2], R1)


def test_a_constrained_chain_accepts_the_bounded_start():
    """(16, 8, 9): a monotone start with max_entry=0.999 satisfies the [0,1] + monotone Constraints of the dose-response
    application, and a short constrained gamma-grid chain runs from it and stays inside them."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    from functionalmf_amd.likelihoods import GammaGridLikelihood
    N, M, T, R, K = 16, 8, 9, 4, 3
    rs = np.random.RandomState(5)
    Wt = rs.dirichlet(0.5 * np.ones(K), size=N)
    Vt = -np.sort(-rs.uniform(0.05, 1.0, size=(M, T, K)), axis=1)
    eta = np.einsum("nk,mtk->nmt", Wt, Vt)
    lik = GammaGridLikelihood(np.linspace(0.8, 1.2, 9), np.ones(9), 0.02)
    comp = rs.choice(9, size=eta.shape)
    Y = rs.gamma(lik.shape_grid[comp][..., None], (lik.scale_grid[comp] * eta)[..., None], size=eta.shape + (R,))
    Y[rs.rand(*Y.shape) < 0.05] = np.nan
    np.random.seed(6)
    W0, V0, info = utils.bounded_tensor_nmf(Y, K, max_entry=0.999, monotone=True, return_info=True)
    assert info["projected"].sum() > 0
    Cons = np.concatenate([np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1),
                           np.concatenate([-np.eye(T), np.full((T, 1), -1.0)], axis=1),
                           np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(T - i - 2), [-1e-2]]) for i in range(T - 1)])])

    def slack(W, V):
        return (np.einsum("qt,nmt->nmq", Cons[:, :-1], np.einsum("nk,mtk->nmt", W, V)) - Cons[:, -1]).min()

    assert slack(W0, V0) >= -1e-9, slack(W0, V0)
    np.random.seed(7)
    model = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "gamma_grid", Cons, likelihood_param=lik, nembeds=K,
                                                           tf_order=2, W_init=W0, V_init=V0, rng="device", device_seed=5)
    for _ in range(20):
        model.resample(Y)
    assert np.isfinite(model.W).all() and np.isfinite(model.V).all() and np.any(model.W != W0)
    assert slack(model.W, model.V) >= -1e-9
