"""slice_fold_in_cols on the GPU (csrc/btf_slice_fold_cols.h): replay of supplied draws against the numpy definition
(functionalmf_amd/slice_fold_in_cols.py), bit-identities, feasibility of every draw, the device generator against the stored
moments of the exact Gibbs chain and against 2-D quadrature posteriors under constraints, the refusals, and one call at the
dose-response shape."""
import functools

import numpy as np
import pytest

from functionalmf_amd import fold_in_cols as fc
from functionalmf_amd import slice_fold_in as sf
from functionalmf_amd import slice_fold_in_cols as sc
from functionalmf_amd import utils
from functionalmf_amd.factor import (ConstrainedNonconjugateBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)
from test_gpu_fold_in_cols import z_problem
from test_gpu_slice_fold_in import _gg_chain_problem, dose_response_inputs, fitted_model
from test_host_slice_fold_in import draw_rows, fit_constraints, gamma_table, grid_logdens, halfplanes, quadrature_posterior
from test_host_slice_fold_in_cols import (MARGIN_MIN, REPLAY_CASES, _cols_bare, capped_case, fixed_case, replay_case, replay_problem,
                                          safe, z_against_gibbs, z_inputs)

pytestmark = pytest.mark.gpu

V_TOL = 1e-6                     # the project's tolerance for V: 1e-6 * max(1, |V|), conditioning-limited
Z_SAMPLES = 4096
# sweeps of the Gibbs-moments test (a test input; the default's value): with the default fit, twice too wide on purpose,
# the largest |z| at S = 16384 was 22.1 at 256 sweeps, 4.3 at 512 and 0.8 at 1024 ("Folding new columns into a
# slice-sampled fit")
GIBBS_Z_SWEEPS = 1024
# Margin of test 7: the largest ratio fold-in RMSE / in-chain RMSE over 5 data seeds plus 20 % of it
# (scripts/slice_fold_in_cols_rate.py --step margin).
FOLD_MARGIN = 1.2 * 4.226        # ratios seen: 4.226, 2.261, 0.421, 1.311, 1.109 (at 8192 sweeps the first is 1.107: DESIGN.md)


def close(a, b, tol=V_TOL):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= tol


def _call(c, **kw):
    args = dict(lam2=c["lam2"], likelihood_param=c["param"], Constraints=c["Cons"], tf_order=c["tf_order"], start=c["start"],
                tau2=c["tau2"], sweeps=c["sweeps"], max_rounds=c["max_rounds"], summary=False)
    args.update(kw)
    return args


def _check_replay(c, label):
    want = c["want"]
    assert safe(want) and min(want["margin_ll"], want["margin_slack"]) > MARGIN_MIN
    out = utils.slice_fold_in_cols(c["Y"], c["Ws"], c["family"], **_call(c, draws=c["draws"]))
    errV = float(np.max(np.abs(out["V"] - want["V"]) / np.maximum(1.0, np.abs(want["V"]))))
    errT = float(np.max(np.abs(out["Tau2"] - want["Tau2"]) / want["Tau2"]))
    print("%s: err V %.3e  Tau2 (rel) %.3e  rounds %d  unfinished %d  cond %.2e  margins %.2e %.2e"
          % (label, errV, errT, want["rounds"].sum(), want["unfinished"].sum(), want["cond"], want["margin_ll"], want["margin_slack"]))
    assert np.array_equal(out["rounds"], want["rounds"]) and np.array_equal(out["unfinished"], want["unfinished"])
    assert errV <= V_TOL and errT <= V_TOL
    assert np.array_equal(out["V_start"], np.broadcast_to(c["start"], out["V"].shape))
    return out


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("idx", range(len(REPLAY_CASES)))
def test_replay_equals_the_definition(idx):
    """1. Supplied draws: rounds and unfinished equal, V and Tau2 within 1e-6 of the definition, for every family, with and
    without constraints, K in {1, 3, 5, 8, 10}, tf_order in {0, 1, 2}, T in {6, 9}; four columns (complete, half missing, a
    single observed cell, empty), S = 3, N = 70, 3 sweeps."""
    _check_replay(replay_case(idx), "%s K=%d tf=%d T=%d constrained=%s" % REPLAY_CASES[idx])


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


def _same(a, b, keys=("V", "V_start", "Tau2", "rounds", "unfinished", "mean", "quantiles")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_same_bits():
    """2. Two calls with one seed; S split with first_sample; C = 1 against the same column inside C = 3; uploaded results
    against device-collected samples; the model method against utils; an integer seed leaves the draw counter untouched."""
    c = replay_case(5)
    family = c["family"]
    kw = dict(seed=5, sweeps=6)
    a = utils.slice_fold_in_cols(c["Y"], c["Ws"], family, **_call(c, summary=True, **kw))
    b = utils.slice_fold_in_cols(c["Y"], c["Ws"], family, **_call(c, summary=True, **kw))
    _same(a, b)
    assert np.all(np.isfinite(a["V"]))
    assert not np.array_equal(a["V"], utils.slice_fold_in_cols(c["Y"], c["Ws"], family, **_call(c, seed=6, sweeps=6))["V"])
    lo = utils.slice_fold_in_cols(c["Y"], c["Ws"][:1], family, **_call(c, lam2=c["lam2"][:1], **kw))
    hi = utils.slice_fold_in_cols(c["Y"], c["Ws"][1:], family, **_call(c, lam2=c["lam2"][1:], first_sample=1, **kw))
    for k in ("V", "Tau2", "rounds", "unfinished"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k]), k
    three = utils.slice_fold_in_cols(c["Y"][:3], c["Ws"], family, **_call(c, start=c["start"][:3], **kw))
    one = utils.slice_fold_in_cols(c["Y"][:1], c["Ws"], family, **_call(c, start=c["start"][:1], **kw))
    for k in ("V", "Tau2", "rounds", "unfinished"):
        assert np.array_equal(one[k][:, 0], three[k][:, 0]) and np.array_equal(three[k], a[k][:, :3]), k
    m, res, _, lik = fitted_model()
    _, _, Y, _ = _gg_chain_problem(9)
    Y_new = np.ascontiguousarray(Y[:20, :3].transpose(1, 0, 2, 3))
    Y_new[1, 6:] = np.nan
    Y_new[2] = np.nan
    draws0 = m._draws
    o1 = m.slice_fold_in_cols(Y_new, seed=5, sweeps=8)                  # the device-collected samples, read where they lie
    o2 = m.slice_fold_in_cols(Y_new, seed=5, sweeps=8)
    o3 = m.slice_fold_in_cols(Y_new, results=res, seed=5, sweeps=8)     # the same samples, uploaded
    o4 = utils.slice_fold_in_cols(Y_new, res["W"], "gamma_grid", lam2=res["lam2"], Vs=res["V"], likelihood_param=lik,
                                  Constraints=m._cons, tf_order=2, seed=5, sweeps=8, stability=float(m.stability))
    for o in (o2, o3, o4):
        _same(o1, o)
    assert m._draws == draws0
    assert np.all(np.isfinite(o1["V"])) and np.all(np.isfinite(o1["mean"])) and o1["mean"].shape == (20, 3, 9)
    np.testing.assert_allclose(o1["V_start"][:, 0], res["V"].mean(axis=1), rtol=0, atol=1e-14)
    for s in range(o1["V"].shape[0]):                                   # every draw feasible, the empty column included
        for j in range(3):
            assert np.all(sc.slacks(o1["V"][s, j], res["W"][s], m._cons) >= 0)
    m.slice_fold_in_cols(Y_new, sweeps=2)                               # seed=None takes the model's next device seed
    assert m._draws == draws0 + 1
    m._draws = draws0


@pytest.mark.parametrize("family", ["poisson_identity", "gamma_grid"])
def test_every_returned_draw_is_feasible(family):
    """3. Constrained, S = 64, C = 3, the device generator: the slack of every constraint of every one of the N rows is
    >= 0 for every (s, c), recomputed in numpy from out["V"] and Ws."""
    c = replay_problem(family, 3, 2, 9, True, seed=77, S=64)
    out = utils.slice_fold_in_cols(c["Y"][:3], c["Ws"], family, **_call(c, start=c["start"][:3], seed=9, sweeps=24))
    assert np.all(np.isfinite(out["V"])) and out["rounds"].min() >= 1
    eta = np.einsum("snk,sctk->scnt", c["Ws"], out["V"])
    slack = np.einsum("scnt,qt->scnq", eta, c["Cons"][:, :-1]) - c["Cons"][:, -1]
    print("%s: smallest slack %.3e, proposals per sweep %.2f, unfinished %d" % (family, slack.min(), out["rounds"].mean() / 24.0,
                                                                               out["unfinished"].sum()))
    assert slack.min() >= 0


def test_device_generator_against_the_gibbs_moments():
    """4. S = 4096 copies of z_problem, Gaussian family, no constraints, the default fit, the device generator: the
    per-coordinate mean of V against the stored moments of the exact Gibbs chain, largest |z| below 5 with the standard
    error from both variances.  First, on the CPU: the definition at these inputs leaves no sweep unfinished."""
    W, Y, nu2, lam2 = z_problem()
    Wn, l2, _, stats, a, b = z_inputs(2)
    rng = np.random.default_rng(5)
    for _ in range(4):
        o = sc.chain(np.zeros((Y.shape[1], W.shape[1])), Wn, l2, 2, "gaussian", nu2, stats, a, b, rng=rng, sweeps=64, track_cond=False)
        assert o["unfinished"] == 0 and not o["failed"]
    S = Z_SAMPLES
    out = utils.slice_fold_in_cols(Y[None], np.repeat(W[None], S, axis=0), "gaussian", lam2=np.full(S, lam2), likelihood_param=nu2,
                                   start=np.zeros((Y.shape[1], W.shape[1])), seed=12345, sweeps=GIBBS_Z_SWEEPS, summary=False)
    assert out["unfinished"].sum() == 0
    z = z_against_gibbs(out["V"][:, 0])
    print("largest |z| of the device chain against the Gibbs moments at %d sweeps: %.2f (limit 5); proposals per sweep %.2f"
          % (GIBBS_Z_SWEEPS, z, out["rounds"].mean() / GIBBS_Z_SWEEPS))
    assert z < 5


@functools.lru_cache(maxsize=None)
def quadrature_case(family):
    """K = 1, T = 2, tf_order 0, N = 5 positive scalar rows, positivity plus a falling curve, tau2 fixed: the curve
    v = (v_0, v_1) has a 2-D posterior.  With the roles swapped - v as the "row", V[i,t,:] = w_i e_t as the "curves" - the
    log-likelihood and the half-planes are those of the row problem (grid_logdens with a flat prior, halfplanes); the prior
    - v' P v / 2, P = Delta' diag(1 / (lam2 tau2)) Delta, is added here."""
    rs = np.random.RandomState({"poisson_identity": 1, "gamma_grid": 2, "bernoulli_logit": 3}[family])
    w = np.array([0.6, 0.8, 1.0, 1.2, 1.4])
    lik = gamma_table(8, rs)
    v_true, half, nreps = {"poisson_identity": ((3.0, 1.5), 2.0, 2), "gamma_grid": ((0.8, 0.4), 0.5, 1),
                           "bernoulli_logit": ((1.0, 0.3), 2.5, 3)}[family]
    param = lik if family == "gamma_grid" else None
    Y = draw_rows(family, param, np.outer(w, v_true)[None], nreps, rs)              # (1,N,T,nreps)
    Y[0, 3, 1] = np.nan
    Cons = fit_constraints(2)
    lam2, tau2 = 1.0, np.ones((1, fc.penalty(2, 0).shape[0]))
    D = fc.penalty(2, 0)
    P = D.T.dot(D / (lam2 * tau2[0])[:, None])
    _, S1, cnt, L = sc.column_statistics(Y, family, 5, 2)
    stats = (S1[0], cnt[0], None if L is None else L[0])
    Vrole = np.zeros((5, 2, 2))
    Vrole[:, 0, 0] = Vrole[:, 1, 1] = w
    lik_dens = grid_logdens(family, sf.check_param(family, param), stats, Vrole, np.inf)

    def logdens(v0, v1):
        return lik_dens(v0, v1) - 0.5 * (P[0, 0] * v0 * v0 + 2 * P[0, 1] * v0 * v1 + P[1, 1] * v1 * v1)
    m, C = quadrature_posterior(logdens, halfplanes(family, stats, Vrole, Cons), half=half, centre=v_true)
    return dict(Y=Y, w=w, param=param, Cons=Cons, lam2=lam2, tau2=tau2, start=np.array([[0.9 * v_true[0]], [0.9 * v_true[1]]]), m=m, C=C)


@pytest.mark.parametrize("family", ["poisson_identity", "gamma_grid", "bernoulli_logit"])
def test_device_generator_against_quadrature(family):
    """5. S = 4096 copies of one state, the device generator, the default sweeps and fit: the mean of v against a 2-D grid
    quadrature of the truncated posterior, largest |z| below 5 with se = sample sd / sqrt(S)."""
    S = Z_SAMPLES
    c = quadrature_case(family)
    out = utils.slice_fold_in_cols(c["Y"], np.broadcast_to(c["w"][None, :, None], (S, 5, 1)), family, lam2=np.full(S, c["lam2"]),
                                   likelihood_param=c["param"], Constraints=c["Cons"], tf_order=0, start=c["start"], tau2=c["tau2"],
                                   seed=77, summary=False)
    v = out["V"][:, 0, :, 0]
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and np.all(v[:, 0] - v[:, 1] >= -1e-2 / 1.4 - 1e-12)
    z = np.abs(v.mean(axis=0) - c["m"]) / (v.std(axis=0, ddof=1) / np.sqrt(S))
    print("%s: quadrature mean %s sd %s; sample mean %s sd %s; z %s; proposals per sweep %.2f; unfinished %d"
          % (family, c["m"], np.sqrt(np.diag(c["C"])), v.mean(axis=0), v.std(axis=0, ddof=1), z, out["rounds"].mean() / sc.DEFAULT_SWEEPS,
             out["unfinished"].sum()))
    assert np.array_equal(out["Tau2"], np.broadcast_to(c["tau2"], out["Tau2"].shape))
    assert z.max() < 5


def test_failures():
    """6. An infeasible start is refused by name (sample, column), and the next call is served; a band beyond the LDS limit,
    a callable likelihood, a sharded model and the Negative-Binomial model are refused before any device call."""
    c = replay_case(3)
    good = utils.slice_fold_in_cols(c["Y"], c["Ws"], c["family"], **_call(c, seed=5))
    bad = np.broadcast_to(c["start"], (3,) + c["start"].shape).copy()
    bad[2, 1] = -bad[2, 1]
    bad[2, 3] = -bad[2, 3]
    with pytest.raises(RuntimeError, match=r"sample 2, column 1"):
        utils.slice_fold_in_cols(c["Y"], c["Ws"], c["family"], **_call(c, start=bad, seed=5))
    again = utils.slice_fold_in_cols(c["Y"], c["Ws"], c["family"], **_call(c, seed=5))
    _same(good, again, keys=("V", "Tau2", "rounds", "unfinished"))
    # without constraints w.v <= 0 on an observed cell is a likelihood of minus infinity: the same refusal
    u = replay_case(2)
    bad = np.broadcast_to(u["start"], (3,) + u["start"].shape).copy()
    bad[1, 0] = -bad[1, 0]
    with pytest.raises(RuntimeError, match=r"sample 1, column 0"):
        utils.slice_fold_in_cols(u["Y"], u["Ws"], u["family"], **_call(u, start=bad))
    with pytest.raises(ValueError, match="LDS"):
        utils.slice_fold_in_cols(np.ones((1, 5, 370)), np.ones((2, 5, 10)), "poisson", lam2=np.ones(2), start=np.zeros((370, 10)))
    Y = np.ones((2, 5, 4))
    res = {"W": np.ones((6, 5, 2)), "V": np.ones((6, 3, 4, 2)), "lam2": np.ones((6, 1))}
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        with pytest.raises(NotImplementedError):
            _cols_bare(cls, world=2).slice_fold_in_cols(Y, results=res)
        with pytest.raises(NotImplementedError):
            _cols_bare(cls, family=lambda W, V, d: 0.0).slice_fold_in_cols(Y, results=res)
    assert not hasattr(NegativeBinomialBayesianTensorFiltering, "slice_fold_in_cols")


def fold_vs_chain(seed, nburn=150, nsamples=100, **fold_kw):
    """(fold-in RMSE, in-chain RMSE, RMSE of the mean curve of the fitted columns) on the unobserved 70 % of the rows of the
    twelfth column of a constrained gamma-grid problem (24 x 12 x 9, K = 3)."""
    W, V, Y, lik = _gg_chain_problem(seed)
    N, M, T, K = W.shape[0], V.shape[0], V.shape[1], V.shape[2]
    truth = np.einsum("nk,tk->nt", W, V[M - 1])
    obs_rows = np.random.RandomState(seed + 100).permutation(N)[:(3 * N) // 10]
    hid = np.setdiff1d(np.arange(N), obs_rows)
    Y_new = np.full((1, N, T, Y.shape[3]), np.nan)
    Y_new[0, obs_rows] = Y[obs_rows, M - 1]
    Cons = fit_constraints(T, True)

    def model(m):
        # (the twelfth column starts where the fold-in starts: at the mean of the other eleven, never at its truth)
        V0 = np.concatenate([V[:M - 1], V[:M - 1].mean(axis=0, keepdims=True)])[:m]
        np.random.seed(seed)
        return ConstrainedNonconjugateBayesianTensorFiltering(N, m, T, "gamma_grid", Cons, likelihood_param=lik, nembeds=K, tf_order=2,
                                                              W_init=W.copy(), V_init=V0, rng="device", device_seed=seed + 1)
    fit = model(M - 1)
    res = fit.run_gibbs(np.ascontiguousarray(Y[:, :M - 1]), nburn=nburn, nsamples=nsamples, verbose=False)
    out = fit.slice_fold_in_cols(Y_new, results=res, seed=17, **fold_kw)
    mean_curve = utils.posterior_summary(res["W"], res["V"])[0].mean(axis=1)
    Y_all = Y.copy()
    Y_all[:, M - 1] = Y_new[0]
    full = model(M)
    res_full = full.run_gibbs(Y_all, nburn=nburn, nsamples=nsamples, verbose=False)
    mean_chain = utils.posterior_summary(res_full["W"], res_full["V"])[0][:, M - 1]
    rmse = lambda a: float(np.sqrt(np.mean((a - truth[hid]) ** 2)))
    return rmse(out["mean"][hid, 0]), rmse(mean_chain[hid]), rmse(mean_curve[hid])


def test_it_does_the_job():
    """7. A constrained gamma-grid problem (24 x 12 x 9, K = 3); the chain runs on 11 columns, the twelfth is folded in from
    30 % of its rows.  RMSE of `mean` on the other rows against the noiseless truth: below that of predicting the mean curve
    of the fitted columns, and below FOLD_MARGIN times that of the chain that had the column in the tensor with the same
    cells observed."""
    fold, chain, base = fold_vs_chain(0)
    print("RMSE on the unobserved rows: fold-in %.4f, in-chain %.4f (ratio %.3f, margin %.3f), the mean curve of the fitted columns %.4f"
          % (fold, chain, fold / chain, FOLD_MARGIN, base))
    assert fold < base
    assert fold < FOLD_MARGIN * chain


def test_one_call_at_the_dose_response_shape():
    """8. 1024 x 9, K = 5, G = 50, 26 constraints, S = 8, C = 2 (30 rows observed), 16 sweeps: finite output, every draw
    feasible, and the summary is utils.posterior_summary on (Ws, out["V"])."""
    Ws, Vs, _, _, lik, Cons = dose_response_inputs(S=8, R=2)
    assert Cons.shape == (26, 10) and Ws.shape == (8, 1024, 5)
    rs = np.random.RandomState(4)
    Y_new = draw_rows("gamma_grid", lik, np.einsum("nk,ctk->cnt", Ws[0], Vs[0, :2]), 3, rs)
    hide = np.setdiff1d(np.arange(1024), rs.choice(1024, size=30, replace=False))
    Y_new[:, hide] = np.nan
    out = utils.slice_fold_in_cols(Y_new, Ws, "gamma_grid", lam2=np.full(8, 0.1), Vs=Vs, likelihood_param=lik, Constraints=Cons,
                                   seed=3, sweeps=16, q=(5, 50, 95))
    for k in ("V", "V_start", "Tau2", "mean", "quantiles"):
        assert np.all(np.isfinite(out[k])), k
    assert out["V"].shape == (8, 2, 9, 5) and out["mean"].shape == (1024, 2, 9) and out["rounds"].min() >= 1
    mean, quant = utils.posterior_summary(Ws, out["V"], q=(5, 50, 95))
    assert np.array_equal(mean, out["mean"]) and np.array_equal(quant, out["quantiles"])
    for s in range(8):
        for j in range(2):
            assert np.all(sc.slacks(out["V"][s, j], Ws[s], Cons) >= 0), (s, j)
    print("dose-response shape: proposals per sweep %.2f, unfinished sweeps %d of %d" % (out["rounds"].mean() / 16.0, out["unfinished"].sum(), 8 * 2 * 16))
