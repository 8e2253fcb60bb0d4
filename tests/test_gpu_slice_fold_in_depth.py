"""slice_fold_in_depth on the GPU (csrc/btf_slice_fold_depth.h) against the numpy definition
(functionalmf_amd/slice_fold_in_depth.py), against the Gibbs chain of fold_in_depth and against 2-D quadrature posteriors.
The problem builders live in tests/test_host_slice_fold_in_depth.py."""
import numpy as np
import pytest

from functionalmf_amd import slice_fold_in_depth as sd
from functionalmf_amd import utils
from functionalmf_amd.factor import (ConstrainedNonconjugateBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)
from test_gpu_slice_fold_in import _gg_chain_problem, fitted_model
from test_host_slice_fold_in import draw_rows, fit_constraints, gamma_table
from test_host_slice_fold_in_depth import (MARGIN_MIN, QUAD_CASES, REPLAY_CASES, Z_SWEEPS, _depth_bare, capped_case, fixed_case,
                                           quadrature_case, reach_case, replay_case, replay_problem, safe, two_sample_z, z_problem)

pytestmark = pytest.mark.gpu

V_TOL = 1e-6                     # the project's tolerance for V: 1e-6 * max(1, |V|), conditioning-limited
Z_SAMPLES = 4096


def _call(c, **kw):
    args = dict(lam2=c["lam2"], likelihood_param=c["param"], Constraints=c["Cons"], tf_order=c["tf_order"], tau2=c["tau2"],
                sweeps=c["sweeps"], max_rounds=c["max_rounds"], summary=False)
    args.update(kw)
    return args


def _check_replay(c, label):
    want = c["want"]
    assert safe(want) and min(want["margin_ll"], want["margin_slack"]) > MARGIN_MIN
    out = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], c["family"], **_call(c, draws=c["draws"]))
    errV = float(np.max(np.abs(out["V"] - want["V"]) / np.maximum(1.0, np.abs(want["V"]))))
    errT = float(np.max(np.abs(out["Tau2"] - want["Tau2"]) / want["Tau2"]))
    print("%s: err V %.3e  Tau2 (rel) %.3e  rounds %d  unfinished %d  cond %.2e  margins %.2e %.2e"
          % (label, errV, errT, want["rounds"].sum(), want["unfinished"].sum(), want["cond"], want["margin_ll"], want["margin_slack"]))
    assert np.array_equal(out["rounds"], want["rounds"]) and np.array_equal(out["unfinished"], want["unfinished"])
    assert errV <= V_TOL and errT <= V_TOL
    assert np.array_equal(out["V_start"], np.repeat(c["Vs"][:, :, -1:], c["H"], axis=2))      # the last kept depth, bit for bit
    return out


def slacks_of(V_new, Ws, Vs, Cons):
    """The slack of every (sample, column, row, constraint that touches a new depth) of Cons (J, T + H + 1) on the stacked
    curves, in numpy: plain
    elementwise sums in ascending order (k, then depth), so that equal depths give equal bits and a tie stays a tie."""
    Vall = np.concatenate([Vs, V_new], axis=2)
    Cons = Cons[np.any(Cons[:, Vs.shape[2]:-1] != 0, axis=1)]
    used = np.flatnonzero(np.any(Cons[:, :-1] != 0, axis=0))
    out = np.zeros(Vall.shape[:2] + (Ws.shape[1], Cons.shape[0]))
    for t in used:
        eta = np.zeros(out.shape[:3])
        for k in range(Ws.shape[2]):
            eta += Ws[:, None, :, k] * Vall[:, :, None, t, k]
        out += eta[..., None] * Cons[:, t]
    return out - Cons[:, -1]


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("idx", range(len(REPLAY_CASES)))
def test_replay_equals_the_definition(idx):
    """1. Supplied draws: rounds and unfinished equal, V and Tau2 within 1e-6 of the definition, for every family, with and
    without constraints, K in {1, 3, 5, 8, 10}, tf_order in {0, 1, 2}, H in {1, 2, 5}, T in {2, 6}; four fitted columns
    (complete, half missing, a single observed cell, empty), S = 3, N = 70, 3 sweeps."""
    _check_replay(replay_case(idx), "%s K=%d tf=%d H=%d T=%d constrained=%s" % REPLAY_CASES[idx])


def test_replay_with_capped_sweeps():
    """1. max_rounds = 2: the definition has unfinished sweeps; they keep their state."""
    c = capped_case()
    assert c["want"]["unfinished"].sum() > 0
    _check_replay(c, "capped")


def test_replay_with_fixed_scales():
    """1. tau2= fixed: the scales come back as given."""
    c = fixed_case()
    out = _check_replay(c, "fixed")
    assert np.array_equal(out["Tau2"], np.broadcast_to(c["tau2"], out["Tau2"].shape))


def test_replay_with_a_constraint_reaching_every_kept_depth():
    """1. B = T: the kept tail in LDS is the whole kept curve."""
    _check_replay(reach_case(), "B = T")


def _same(a, b, keys=("V", "V_start", "Tau2", "rounds", "unfinished", "mean", "quantiles")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_same_bits():
    """2. Two calls with one seed; S split with first_sample; uploaded results against device-collected samples; the model
    method against utils; an integer seed leaves the draw counter untouched, seed=None moves it by one."""
    c = replay_case(5)
    family = c["family"]
    kw = dict(seed=5, sweeps=6)
    a = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], family, **_call(c, summary=True, **kw))
    b = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], family, **_call(c, summary=True, **kw))
    _same(a, b)
    assert np.all(np.isfinite(a["V"])) and a["mean"].shape == (70, 4, c["H"])
    assert not np.array_equal(a["V"], utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], family, **_call(c, seed=6, sweeps=6))["V"])
    lo = utils.slice_fold_in_depth(c["Y"], c["Ws"][:1], c["Vs"][:1], family, **_call(c, lam2=c["lam2"][:1], **kw))
    hi = utils.slice_fold_in_depth(c["Y"], c["Ws"][1:], c["Vs"][1:], family, **_call(c, lam2=c["lam2"][1:], first_sample=1, **kw))
    for k in ("V", "Tau2", "rounds", "unfinished"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k]), k
    m, res, _, lik = fitted_model()
    N, M, T, H = 20, m.ncols, m.ndepth, 2
    rs = np.random.RandomState(4)
    Y_new = draw_rows("gamma_grid", lik, 0.8 * np.einsum("snk,smk->nm", res["W"], res["V"][:, :, -1])[:, :, None]
                      / res["W"].shape[0] * np.ones(H), 2, rs)
    Y_new[rs.uniform(size=Y_new.shape) < 0.3] = np.nan
    Y_new[:, 2] = np.nan
    Cons = fit_constraints(T + H, True)
    draws0 = m._draws
    o1 = m.slice_fold_in_depth(Y_new, Constraints=Cons, seed=5, sweeps=8)                 # the device-collected samples, read where they lie
    o2 = m.slice_fold_in_depth(Y_new, Constraints=Cons, seed=5, sweeps=8)
    o3 = m.slice_fold_in_depth(Y_new, results=res, Constraints=Cons, seed=5, sweeps=8)    # the same samples, uploaded
    o4 = utils.slice_fold_in_depth(Y_new, res["W"], res["V"], "gamma_grid", lam2=res["lam2"], likelihood_param=lik, Constraints=Cons,
                                   tf_order=2, seed=5, sweeps=8, stability=float(m.stability))
    for o in (o2, o3, o4):
        _same(o1, o)
    assert m._draws == draws0
    assert np.all(np.isfinite(o1["V"])) and np.all(np.isfinite(o1["mean"])) and o1["mean"].shape == (N, M, H)
    assert np.array_equal(o1["V_start"], np.repeat(res["V"][:, :, -1:], H, axis=2))
    assert slacks_of(o1["V"], res["W"], res["V"], Cons).min() >= 0
    m.slice_fold_in_depth(Y_new, Constraints=Cons, sweeps=2)                                # seed=None takes the model's next device seed
    assert m._draws == draws0 + 1
    m._draws = draws0


@pytest.mark.parametrize("family", ["poisson_identity", "gamma_grid"])
def test_every_returned_draw_is_feasible(family):
    """3. Constrained, S = 64, the device generator, the default start (accepted everywhere): the slack of every constraint
    that touches a new depth is >= 0 for every one of the N rows, recomputed in numpy - fit_constraints and, beside them,
    a monotone row with bound 0 between every new depth and its predecessor, which the default start ties exactly."""
    T, H = 6, 3
    c = replay_problem(family, 3, 2, H, T, True, seed=77, S=64)
    tie = np.zeros((H, T + H + 1))
    for h in range(H):
        tie[h, T - 1 + h], tie[h, T + h] = 1.0, -1.0
    Cons = np.concatenate([c["Cons"], tie])
    out = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], family, **_call(c, Constraints=Cons, seed=9, sweeps=24))
    assert np.all(np.isfinite(out["V"]))                       # (no start was refused: the call returned)
    slack = slacks_of(out["V"], c["Ws"], c["Vs"], Cons)
    # (the tied start is a corner of the feasible set: a chain may find no feasible proposal at all and stay there - feasible too)
    print("%s: smallest slack %.3e, proposals per sweep %.2f, unfinished %d, chains that never moved %d"
          % (family, slack.min(), out["rounds"].mean() / 24.0, out["unfinished"].sum(), int((out["rounds"] == 0).sum())))
    assert slack.min() >= 0 and out["rounds"].sum() > 0


def test_device_generator_against_fold_in_depth():
    """4. Gaussian family, exact fit, 4096 copies of one kept state (H = 4, K = 3, half the rows observed), the device
    generator, the sweep count of the host study in both calls: the V means of slice_fold_in_depth against those of
    utils.fold_in_depth on the same inputs, largest two-sample |z| below 5; every sweep accepts its first proposal."""
    from functionalmf_amd import slice_fold_in_cols as sc
    W, V_old, Y, nu2, lam2 = z_problem()
    S = Z_SAMPLES
    Ws, Vs = np.repeat(W[None], S, axis=0), np.repeat(V_old[None, None], S, axis=0)
    Yn = np.ascontiguousarray(Y[:, None, :])
    fit = sc.gaussian_fit(np.swapaxes(Yn, 0, 1), "gaussian", nu2, multiplier=1)
    a = utils.slice_fold_in_depth(Yn, Ws, Vs, "gaussian", lam2=np.full(S, lam2), likelihood_param=nu2, fit=fit, seed=12345,
                                  sweeps=Z_SWEEPS, summary=False)
    b = utils.fold_in_depth(Yn, Ws, Vs, "gaussian", nu2=np.full(S, nu2), lam2=np.full(S, lam2), seed=54321, sweeps=Z_SWEEPS, summary=False)
    z = two_sample_z(a["V"][:, 0], b["V"][:, 0])
    print("largest |z| of slice_fold_in_depth against fold_in_depth at %d sweeps: %.2f (limit 5)" % (Z_SWEEPS, z))
    assert np.all(a["rounds"] == Z_SWEEPS) and a["unfinished"].sum() == 0
    assert z < 5


@pytest.mark.parametrize("H,K", [(2, 1), (1, 2)])
def test_device_generator_against_quadrature(H, K):
    """5. 4096 copies of one state, the device generator, constrained, tau2 fixed: mean and covariance of the new curve
    against the 2-D quadrature posterior of the host file, within 5 standard errors (the host file's bound)."""
    from test_host_slice_fold_in import moments_check
    from test_host_slice_fold_in_depth import QUAD_SWEEPS
    assert (H, K, True) in QUAD_CASES
    c = quadrature_case(H, K, True)
    S = Z_SAMPLES
    Ws, Vs = np.repeat(c["W"][None], S, axis=0), np.repeat(c["V_old"][None, None], S, axis=0)
    out = utils.slice_fold_in_depth(np.ascontiguousarray(c["Y"][:, None]), Ws, Vs, c["family"], lam2=np.full(S, c["lam2"]),
                                    Constraints=c["Cons"], tf_order=c["tf"], tau2=c["tau2"][None], seed=77, sweeps=QUAD_SWEEPS,
                                    summary=False)
    X = out["V"][:, 0].reshape(S, 2)
    assert np.all(np.isfinite(X)) and np.array_equal(out["Tau2"], np.broadcast_to(c["tau2"], out["Tau2"].shape))
    zm, zc = moments_check(X, c["m"], c["C"])
    print("H=%d K=%d: mean %s (quadrature %s)  z_mean %.2f  z_cov %.2f  unfinished %d" % (H, K, X.mean(axis=0), c["m"], zm, zc,
                                                                                        out["unfinished"].sum()))
    assert zm < 5 and zc < 5


def test_forecast_under_positivity():
    """6. Y_new=None, horizon=3 under positivity: all draws finite and feasible; rounds >= sweeps."""
    c = replay_problem("poisson_identity", 5, 2, 3, 6, False, seed=5, S=16)
    T, H = 6, 3
    Cons = np.concatenate([np.eye(T + H), np.zeros((T + H, 1))], axis=1)
    out = utils.slice_fold_in_depth(None, c["Ws"], c["Vs"], "poisson_identity", horizon=H, lam2=c["lam2"], Constraints=Cons, tf_order=2,
                                    seed=3, sweeps=16)
    assert out["V"].shape == (16, 4, H, 5) and np.all(np.isfinite(out["V"])) and np.all(np.isfinite(out["mean"]))
    assert np.all(out["rounds"] >= 16)
    assert np.all(np.einsum("snk,smhk->smnh", c["Ws"], out["V"]) >= 0)
    assert out["mean"].shape == (70, 4, H) and out["quantiles"].shape == (2, 70, 4, H)


def test_failures():
    """7. A callable likelihood, a sharded model and the Negative-Binomial model raise NotImplementedError; a constrained
    model without Constraints raises ValueError; LDS beyond the limit raises ValueError before any launch; an infeasible
    start= raises RuntimeError naming the smallest (sample, column), and the next call is served."""
    c = replay_case(3)
    good = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], c["family"], **_call(c, seed=5))
    bad = np.repeat(c["Vs"][:, :, -1:], c["H"], axis=2).copy()
    bad[2, 1] = -bad[2, 1]
    bad[2, 3] = -bad[2, 3]
    with pytest.raises(RuntimeError, match=r"sample 2, column 1"):
        utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], c["family"], **_call(c, start=bad, seed=5))
    again = utils.slice_fold_in_depth(c["Y"], c["Ws"], c["Vs"], c["family"], **_call(c, seed=5))
    _same(good, again, keys=("V", "Tau2", "rounds", "unfinished"))
    with pytest.raises(ValueError, match="LDS"):
        utils.slice_fold_in_depth(np.ones((5, 1, 400)), np.ones((2, 5, 10)), np.ones((2, 1, 40, 10)), "poisson", lam2=np.ones(2))
    Y = np.ones((5, 3, 2))
    res = {"W": np.ones((6, 5, 2)), "V": np.ones((6, 3, 4, 2)), "lam2": np.ones((6, 1))}
    none = np.zeros((0, 7))
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        with pytest.raises(NotImplementedError):
            _depth_bare(cls, world=2).slice_fold_in_depth(Y, results=res, Constraints=none)
        with pytest.raises(NotImplementedError):
            _depth_bare(cls, family=lambda W, V, d: 0.0).slice_fold_in_depth(Y, results=res, Constraints=none)
    with pytest.raises(NotImplementedError):
        NegativeBinomialBayesianTensorFiltering.slice_fold_in_depth(object(), Y)
    with pytest.raises(ValueError, match="extended grid"):
        _depth_bare(ConstrainedNonconjugateBayesianTensorFiltering).slice_fold_in_depth(Y, results=res)
    m = fitted_model()[0]
    with pytest.raises(ValueError, match="extended grid"):
        m.slice_fold_in_depth(None, horizon=2)


def dose_response_depth_inputs(S=4, N=1024, M=256, T=9, H=2, K=5, G=50, seed=2):
    """The dose-response shape: positive factors with falling curves below one, gamma-grid data at two more doses (a third
    of the rows observed), the 26 constraints of fit.py extended by the rows for the two doses."""
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    V = np.zeros((M, T + H, K))
    V[:, -1] = rs.gamma(2.0, 0.2, size=(M, K))
    for t in range(T + H - 2, -1, -1):
        V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.2, size=(M, K)) * (rs.rand(M, 1) < 0.5)
    W *= 0.6 / np.einsum("nk,mtk->nmt", W, V).max()
    lik = gamma_table(G, rs)
    Ws = W[None] * np.exp(0.05 * rs.normal(size=(S, N, K)))
    Vs = np.ascontiguousarray(V[None, :, :T] * (1.0 + 0.05 * rs.uniform(-1, 1, size=(S, 1, 1, 1))))
    Y_new = draw_rows("gamma_grid", lik, np.einsum("nk,mtk->nmt", W, V[:, T:]), 2, rs)
    Y_new[rs.permutation(N)[N // 3:]] = np.nan
    return Ws, Vs, np.full(S, 1.0), Y_new, lik, fit_constraints(T + H, True)


def test_one_call_at_the_dose_response_shape():
    """8. (1024,256,9), H = 2, K = 5, G = 50, the 26 constraints of fit.py extended by the rows for two more doses, S = 4,
    sweeps = 16: shapes, finiteness and the feasibility of every draw."""
    Ws, Vs, lam2, Y_new, lik, Cons = dose_response_depth_inputs()
    assert fit_constraints(9, True).shape == (26, 10) and Cons.shape == (32, 12)
    out = utils.slice_fold_in_depth(Y_new, Ws, Vs, "gamma_grid", lam2=lam2, likelihood_param=lik, Constraints=Cons, seed=3, sweeps=16)
    nR = 3 * 2 + 2                                            # tf_order 2: 3 H + 2 new penalty rows
    assert out["V"].shape == (4, 256, 2, 5) and out["Tau2"].shape == (4, 256, nR) and out["rounds"].shape == (4, 256)
    assert out["mean"].shape == (1024, 256, 2) and out["quantiles"].shape == (2, 1024, 256, 2)
    for k in ("V", "V_start", "Tau2", "mean", "quantiles"):
        assert np.all(np.isfinite(out[k])), k
    assert out["rounds"].min() >= 1
    slack = slacks_of(out["V"], Ws, Vs, Cons)
    print("dose-response shape: smallest slack %.3e, proposals per sweep %.2f, unfinished %d"
          % (slack.min(), out["rounds"].mean() / 16.0, out["unfinished"].sum()))
    assert slack.min() >= 0
