"""Host halves of slice_fold_in_depth (functionalmf_amd/slice_fold_in_depth.py): the numpy definition against the Gibbs chain
of fold_in_depth (exact fit, and a fit of doubled variance), against 2-D quadrature posteriors, the reduced constraints and
the exact tie of the default start, every refusal before the library is loaded, the wiring of the new unit and symbols, and
the safety of the replay inputs.  No GPU.  The problem builders are shared with tests/test_gpu_slice_fold_in_depth.py."""
import functools
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, utils
from functionalmf_amd import fold_in_depth as fd
from functionalmf_amd import slice_fold_in as sf
from functionalmf_amd import slice_fold_in_cols as sc
from functionalmf_amd import slice_fold_in_depth as sd
from functionalmf_amd.factor import (ConstrainedNonconjugateBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)
from test_host_slice_fold_in import _bare, draw_rows, fit_constraints, gamma_table, moments_check, no_device, quadrature_posterior  # noqa: F401
from test_host_slice_fold_in_cols import COND_MAX, MARGIN_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The sweeps of the replicates below: a test input from the study behind DEFAULT_SWEEPS (scripts/slice_fold_in_depth_rate.py
# --step sweeps; DESIGN.md, "Folding new depth slices into a slice-sampled fit"): 1024, the default's value.  The level / curve
# pair mixes slowly from the flat start, so the count matters: on z_problem with the fit of doubled variance the largest |z| of
# 300 replicates against the Gibbs replicates below was 9.0 at 64 sweeps, 6.7 at 128, 4.2 at 256, 3.1 at 512, 2.3 at 1024.
Z_SWEEPS = 1024
# The long run of the Gibbs replicates (fold_in_depth.chain draws the curve exactly given the levels: its own study finds the
# noise floor at 64 to 128 sweeps, DESIGN.md, "Folding new depth slices in"; eight times that)
GIBBS_LONG = 1024
# Sweeps of the 2-D quadrature chains: tau2 is fixed there, so the target is log-concave and the ellipse is centred on its
# Gaussian fit; the chain forgets its start within a few sweeps and no allowance for the chain's length is taken (bias 0,
# stricter than the HOST_BIAS convention of test_host_slice_fold_in.py allows).
QUAD_SWEEPS = 64
QUAD_CHAINS = 1024

# family, K, tf_order, H, T, constrained: every family with and without constraints, K in {1, 3, 5, 8, 10}, tf_order in
# {0, 1, 2}, H in {1, 2, 5}, T in {2, 6} (T = 2: the kept tail is shorter than tf_order + 1)
REPLAY_CASES = [
    ("poisson_log", 1, 0, 1, 6, False), ("poisson_log", 5, 2, 5, 2, True),
    ("poisson_identity", 3, 1, 2, 6, False), ("poisson_identity", 10, 2, 1, 6, True),
    ("bernoulli_logit", 5, 0, 5, 2, False), ("bernoulli_logit", 8, 1, 2, 6, True),
    ("gaussian", 8, 2, 2, 2, False), ("gaussian", 1, 1, 5, 6, True),
    ("negbin_logit", 10, 0, 2, 6, False), ("negbin_logit", 3, 2, 1, 2, True),
    ("gamma_grid", 3, 1, 5, 6, False), ("gamma_grid", 5, 2, 2, 6, True),
]


def replay_problem(family, K, tf_order, H, T, constrained, seed, S=3, N=70, sweeps=3, max_rounds=40, fixed=False, reach_all=False,
                   M=4):
    """S states on N = 70 rows (one full pass of 64 lanes and a tail) and four fitted columns whose new slices are complete,
    half missing, a single observed cell, empty.  Every row of W is positive and every factor of the kept curves falls
    along the depth axis, so the curves are positive and falling: feasible under fit_constraints(T + H), and so is the
    default start.  reach_all: one more constraint that reaches every kept depth (the mean of the whole extended curve
    stays positive): B = T."""
    rs = np.random.RandomState(seed)
    falls = np.stack([np.linspace(1.0, 0.3 + 0.05 * k, T + H) for k in range(K)], axis=-1)          # (T+H,K)
    scale = 3.0 if family == "poisson_identity" else 1.0
    Ws = rs.uniform(0.5, 1.5, size=(S, N, K)) / K
    v_true = scale * rs.uniform(0.5, 1.5, size=(M, 1, K)) * falls[None]                             # (M,T+H,K)
    Vs = np.ascontiguousarray(v_true[None, :, :T] * (1.0 + 0.03 * rs.uniform(-1, 1, size=(S, M, 1, 1))))
    lam2 = np.resize([0.05, 0.1, 0.2], S)
    lik = gamma_table(6, rs)
    param = {"gaussian": 0.3, "negbin_logit": 4.0, "gamma_grid": lik}.get(family)
    Y = draw_rows(family, param, np.einsum("nk,mtk->nmt", Ws[0], v_true[:, T:]), 2, rs)            # (N,M,H,2)
    Y[:, 1][rs.uniform(size=Y[:, 1].shape) < 0.5] = np.nan
    if M > 2:
        one = Y[5, 2, H // 2, 0]
        Y[:, 2] = np.nan
        Y[5, 2, H // 2, 0] = one
        Y[:, 3:] = np.nan
    Cons = fit_constraints(T + H) if constrained else None
    if reach_all:
        Cons = np.concatenate([Cons, np.concatenate([np.full(T + H, 1.0 / (T + H)), [0.0]])[None]], axis=0)
    nR = fd.new_rows(T, H, tf_order)[0].size
    tau2 = rs.uniform(0.5, 2.0, size=(M, nR)) if fixed else None
    draws = sd.random_draws(rs, T, H, K, tf_order, sweeps, max_rounds, size=(S, M))
    return dict(family=family, K=K, tf_order=tf_order, T=T, H=H, Ws=Ws, Vs=Vs, lam2=lam2, Y=Y, Cons=Cons, tau2=tau2, draws=draws,
                param=param, sweeps=sweeps, max_rounds=max_rounds)


def definition(c, nu_scale=1.0):
    """The numpy definition on the inputs of replay_problem, with the default fit and the default start."""
    S, N = c["Ws"].shape[:2]
    M = c["Vs"].shape[1]
    p = sf.check_param(c["family"], c["param"])
    H, S1, cnt, L = sd.slice_statistics(c["Y"], c["family"], N, M)
    a, b = sc.fit_weights(sd.default_fit(c["Y"], c["family"], p, N, M), M, N, H)
    tau2 = None if c["tau2"] is None else np.broadcast_to(c["tau2"], (S,) + c["tau2"].shape)
    return sd.chains(c["Vs"], c["Ws"], c["lam2"], c["tf_order"], c["family"], p, (S1, cnt, L), a, b, c["Cons"], tau2=tau2,
                     draws=c["draws"], sweeps=c["sweeps"], max_rounds=c["max_rounds"], nu_scale=nu_scale)


def safe(want):
    return want["cond"] <= COND_MAX and min(want["margin_ll"], want["margin_slack"]) > MARGIN_MIN and np.all(np.isfinite(want["V"]))


def replay_inputs(family, K, tf_order, H, T, constrained, need_unfinished=False, **kw):
    """The inputs of a replay case, chosen by the definition alone: the first seed of a fixed sequence whose chains keep
    cond(Q) <= COND_MAX and both decision margins above MARGIN_MIN (and, need_unfinished, leave a sweep at the cap)."""
    base = 1000 * K + 100 * tf_order + 10 * T + H + (5 if constrained else 0)
    for k in range(200):
        c = replay_problem(family, K, tf_order, H, T, constrained, base + 7919 * k, **kw)
        want = definition(c)
        if safe(want) and (not need_unfinished or want["unfinished"].sum() > 0):
            c["want"] = want
            return c
    raise AssertionError("no seed with cond(Q) <= %g and margins above %g" % (COND_MAX, MARGIN_MIN))


@functools.lru_cache(maxsize=None)
def replay_case(idx):
    c = replay_inputs(*REPLAY_CASES[idx])
    for a in (c["Ws"], c["Vs"], c["Y"], c["draws"], c["want"]["V"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def capped_case():
    """max_rounds = 2: the definition has unfinished sweeps."""
    return replay_inputs("poisson_identity", 3, 1, 2, 6, True, need_unfinished=True, max_rounds=2)


@functools.lru_cache(maxsize=None)
def fixed_case():
    """tau2= fixed."""
    return replay_inputs("gamma_grid", 3, 2, 2, 6, True, fixed=True)


@functools.lru_cache(maxsize=None)
def reach_case():
    """A constraint that reaches every kept depth: B = T."""
    c = replay_inputs("poisson_identity", 3, 2, 2, 6, True, reach_all=True)
    assert sd.reduce_constraints(c["Cons"], 6, 2)[3] == 6
    return c


# ---- the Gaussian problem of the Gibbs comparisons -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def z_problem(N=40, T=8, H=4, K=3, seed=4):
    """One kept state of the Gaussian family, half the rows observed at the new depths: (W, V_old, Y (N,H), nu2, lam2)."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    v = 0.3 * np.cumsum(rs.normal(size=(T + H, K)), axis=0)
    Y = W.dot(v[T:].T) + rs.normal(0, 0.5, size=(N, H))
    Y[rs.permutation(N)[N // 2:]] = np.nan
    for a in (W, v, Y):
        a.setflags(write=False)
    return W, v[:T], Y, 0.25, 0.1


def z_inputs(multiplier):
    """z_problem as a slice_fold_in_depth problem of the Gaussian family: (stats, weights, sums) of the one column."""
    W, V_old, Y, nu2, lam2 = z_problem()
    N, H = Y.shape
    _, S1, cnt, L = sf.row_statistics(Y[None], "gaussian", N, H)
    a, b = sc.fit_weights(sc.gaussian_fit(Y[None], "gaussian", nu2, multiplier=multiplier), 1, N, H)
    return (S1[0], cnt[0], None), a[0], b[0]


def two_sample_z(A, B):
    """Largest two-sample |z| of the per-coordinate means of A and B (replicates along axis 0)."""
    se = np.sqrt(A.var(axis=0, ddof=1) / A.shape[0] + B.var(axis=0, ddof=1) / B.shape[0])
    return float(np.max(np.abs(A.mean(axis=0) - B.mean(axis=0)) / se))


def gibbs_replicates(R, seed, sweeps):
    """R replicates of fold_in_depth.chain on z_problem under numpy's generator: V (R,H,K)."""
    W, V_old, Y, nu2, lam2 = z_problem()
    rng = np.random.default_rng(seed)
    T, (H, K) = V_old.shape[0], (Y.shape[1], W.shape[1])
    return np.array([fd.chain(Y, W, V_old, nu2, lam2, 2, sweeps, fd.random_draws(rng, T, H, K, 2, sweeps))[0] for _ in range(R)])


# ---- the 2-D quadrature problems ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quadrature_case(H, K, constrained, family="poisson_identity"):
    """H K = 2 new coordinates, tau2 fixed, tf_order 1, N = 6 positive rows, T = 3 kept depths of a falling positive curve;
    constrained: fit_constraints(T + H) (positivity and falling with slack 1e-2, one row couples the last kept depth).  The
    posterior of x = vec(v) is N(prior | off, D_n, tau2) x likelihood on the half-planes: quadrature_posterior gives (m, C)."""
    assert H * K == 2
    rs = np.random.RandomState(10 * H + K + (100 if constrained else 0))
    N, T, tf = 6, 3, 1
    W = rs.uniform(0.4, 1.2, size=(N, K))
    V_old = np.linspace(3.0, 2.0, T)[:, None] * rs.uniform(0.8, 1.2, size=(1, K))
    v_true = np.linspace(1.8, 1.5, H)[:, None] * (V_old[-1] / 2.0)[None]
    Y = draw_rows(family, None, W.dot(v_true.T)[None], 2, rs)[0]                                     # (N,H,2)
    Y[4] = np.nan
    lam2 = 0.5
    _, D_o, D_n = fd.new_rows(T, H, tf)
    tau2 = np.linspace(0.8, 1.6, D_n.shape[0])
    off = D_o.dot(V_old)
    _, S1, cnt, _ = sf.row_statistics(Y[None], family, N, H)
    S1, cnt = S1[0], cnt[0]
    Cons = fit_constraints(T + H) if constrained else None
    red = sd.reduce_constraints(Cons, T, H)

    def curve(x0, x1):                       # v[h][k] as arrays of the grid's shape
        return [[x0], [x1]] if K == 1 else [[x0, x1]]

    def logdens(x0, x1):
        v = curve(x0, x1)
        out = np.zeros(np.shape(x0))
        for r in range(D_n.shape[0]):
            for k in range(K):
                dv = off[r, k] + sum(D_n[r, h] * v[h][k] for h in range(H))
                out = out - 0.5 * dv * dv / (lam2 * tau2[r])
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(N):
                for h in range(H):
                    if cnt[i, h] > 0:
                        e = sum(W[i, k] * v[h][k] for k in range(K))
                        out = out + S1[i, h] * np.log(np.where(e > 0, e, 1.0)) - cnt[i, h] * e
        return out
    # half-planes a . x >= c: w_i . v_h >= 0 on every observed cell (the identity link), then the reduced constraints
    rows, rhs = [], []

    def plane(i, coef_h, bound):             # sum_h coef_h (w_i . v_h) >= bound as a . x >= bound
        a = np.zeros(2)
        for h in range(H):
            for k in range(K):
                a[h * K + k] += coef_h[h] * W[i, k]
        rows.append(a)
        rhs.append(bound)
    for i in range(N):
        for h in range(H):
            if cnt[i, h] > 0:
                plane(i, np.eye(H)[h], 0.0)
    A_o, A_n, cc, B = red
    eta_old = W.dot(V_old[T - B:].T) if B else np.zeros((N, 0))
    for i in range(N):
        for q in range(cc.size):
            plane(i, A_n[q], cc[q] - float(A_o[q].dot(eta_old[i])))
    # The quadrature integrates a half-plane exactly along its second coordinate only; positivity and the row that couples the
    # last kept depth bound ONE coordinate of x.  So it runs in rotated coordinates u = R x, where no plane is parallel to
    # an axis, and the moments are turned back: m_x = R' m_u, C_x = R' C_u R.
    cs, sn = np.cos(0.5), np.sin(0.5)
    R = np.array([[cs, sn], [-sn, cs]])
    m, C = quadrature_posterior(lambda u0, u1: logdens(cs * u0 - sn * u1, sn * u0 + cs * u1), (np.array(rows).dot(R.T), np.array(rhs)),
                                half=2.5, centre=tuple(R.dot(v_true.reshape(-1))))
    m, C = R.T.dot(m), R.T.dot(C).dot(R)
    a, b = sc.fit_weights(sc.gaussian_fit(Y[None], family, None), 1, N, H)
    out = dict(W=W, V_old=V_old, Y=Y, lam2=lam2, tau2=tau2, Cons=Cons, red=red, stats=(S1, cnt, None), a=a[0], b=b[0], m=m, C=C, tf=tf,
               H=H, K=K, family=family)
    for arr in (W, V_old, Y, tau2, m, C):
        arr.setflags(write=False)
    return out


QUAD_CASES = [(2, 1, False), (2, 1, True), (1, 2, False), (1, 2, True)]


# ------------------------------------------------------------------------------------------------------------------ tests
def test_exact_fit_walks_the_gibbs_chain_of_fold_in_depth():
    """Gaussian family, exact fit (multiplier 1), u_a = 1 / 4 (phi = pi / 2: the accepted proposal is m + nu): on the record
    of fold_in_depth.chain (same normals and gammas) the chain walks that chain's path, v and tau2 within 1e-12, and every
    sweep accepts its first proposal."""
    W, V_old, Y, nu2, lam2 = z_problem()
    stats, a, b = z_inputs(1.0)
    T, H, K, sweeps = V_old.shape[0], Y.shape[1], W.shape[1], 5
    nR, n = fd.new_rows(T, H, 2)[0].size, H * K
    d = sd.random_draws(np.random.RandomState(3), T, H, K, 2, sweeps).copy()
    body = d[4 * nR:].reshape(sweeps, -1)
    body[:, n + 1] = 0.25
    gibbs = np.concatenate([d[:4 * nR]] + [np.concatenate([body[r, :n], body[r, n + 1 + sd.DEFAULT_MAX_ROUNDS:]]) for r in range(sweeps)])
    v, _, tau2 = fd.chain(Y, W, V_old, nu2, lam2, 2, sweeps, gibbs)
    o = sd.chain(V_old, W, lam2, 2, "gaussian", nu2, stats, a, b, draws=d, sweeps=sweeps)
    assert o["rounds"] == sweeps and o["unfinished"] == 0 and not o["failed"]
    ev = float(np.max(np.abs(o["v"] - v) / np.maximum(1.0, np.abs(v))))
    et = float(np.max(np.abs(o["tau2"] - tau2) / np.maximum(1.0, np.abs(tau2))))
    print("exact fit against the Gibbs chain: err v %.2e  tau2 %.2e" % (ev, et))
    assert ev <= 1e-12 and et <= 1e-12


def test_reduce_constraints():
    T, H, K, N = 6, 3, 2, 7
    rs = np.random.RandomState(0)
    Cons = fit_constraints(T + H)
    A_o, A_n, c, B = sd.reduce_constraints(Cons, T, H)
    touches = np.any(Cons[:, T:T + H] != 0, axis=1)
    assert B == 1 and A_o.shape == (touches.sum(), 1) and A_n.shape == (touches.sum(), H)       # the monotone row (T - 1, T)
    assert touches.sum() == H + H                                                                # H positivity rows, H monotone rows
    assert np.array_equal(np.concatenate([A_o, A_n, c[:, None]], axis=1), Cons[touches][:, T - 1:])
    W, V_old, v = rs.normal(size=(N, K)), rs.normal(size=(T, K)), rs.normal(size=(H, K))
    got = sd.reduced_slacks(v, W, V_old, (A_o, A_n, c, B)).reshape(N, -1)
    want = sc.slacks(np.concatenate([V_old, v]), W, Cons).reshape(N, -1)[:, touches]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    full = np.concatenate([Cons, np.concatenate([np.ones(T + H), [0.5]])[None]])
    assert sd.reduce_constraints(full, T, H)[3] == T                                             # a row reaching every kept depth
    got = sd.reduced_slacks(v, W, V_old, sd.reduce_constraints(full, T, H)).reshape(N, -1)
    want = sc.slacks(np.concatenate([V_old, v]), W, full).reshape(N, -1)[:, np.append(touches, True)]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    none = sd.reduce_constraints(None, T, H)
    assert none[3] == 0 and none[2].size == 0 and sd.reduce_constraints(np.zeros((0, T + H + 1)), T, H)[2].size == 0
    assert sd.reduce_constraints(Cons[:T - 1], T, H)[2].size == 0                                # rows on kept depths alone drop out
    with pytest.raises(ValueError, match="extended grid"):
        sd.reduce_constraints(fit_constraints(T), T, H)                                          # the model's own (J, T + 1) rows


def test_default_start_is_feasible_and_ties_exactly():
    """Carrying the last kept depth forward is feasible under fit_constraints whenever the kept curve is, and a (+1, -1) row
    with bound 0 evaluates to exactly 0 there and passes."""
    c = replay_problem("poisson_identity", 5, 2, 3, 6, True, seed=1)
    T, H = 6, 3
    tie = np.zeros((H, T + H + 1))
    for h in range(H):
        tie[h, T - 1 + h], tie[h, T + h] = 1.0, -1.0                                            # v_{T-1+h} - v_{T+h} >= 0
    Cons = np.concatenate([c["Cons"], tie])
    red = sd.reduce_constraints(Cons, T, H)
    for s in range(3):
        for j in range(4):
            V_old = c["Vs"][s, j]
            assert np.all(sc.slacks(V_old, c["Ws"][s], fit_constraints(T)) >= 0)                 # the kept curve is feasible
            start = np.tile(V_old[T - 1], (H, 1))
            sl = sd.reduced_slacks(start, c["Ws"][s], V_old, red).reshape(70, -1)
            assert np.all(sl >= 0)
            assert np.all(sl[:, -H:] == 0.0)                                                     # the ties: exactly 0
            o = sd.chain(V_old, c["Ws"][s], 0.1, 2, "poisson_identity", None, None, Constraints=red, horizon=H,
                         rng=np.random.default_rng(s), sweeps=2, track_cond=False)
            assert not o["failed"] and np.all(sd.reduced_slacks(o["v"], c["Ws"][s], V_old, red) >= 0)


@pytest.mark.parametrize("H,K,constrained", QUAD_CASES)
def test_chain_against_quadrature_posterior(H, K, constrained):
    """1024 replicates of `chain` (numpy's generator, tau2 fixed, the default start and fit) against the 2-D quadrature
    posterior: mean and covariance within 5 standard errors."""
    c = quadrature_case(H, K, constrained)
    rng = np.random.default_rng(7)
    X, unf = np.zeros((QUAD_CHAINS, 2)), 0
    for i in range(QUAD_CHAINS):
        o = sd.chain(c["V_old"], c["W"], c["lam2"], c["tf"], c["family"], None, c["stats"], c["a"], c["b"], c["red"], tau2=c["tau2"],
                     rng=rng, sweeps=QUAD_SWEEPS, track_cond=False)
        assert not o["failed"] and np.array_equal(o["tau2"], c["tau2"])
        X[i], unf = o["v"].reshape(-1), unf + o["unfinished"]
    zm, zc = moments_check(X, c["m"], c["C"])
    print("H=%d K=%d constrained=%s: mean %s (quadrature %s)  z_mean %.2f  z_cov %.2f  unfinished %d"
          % (H, K, constrained, X.mean(axis=0), c["m"], zm, zc, unf))
    assert zm < 5 and zc < 5


def test_doubled_variance_fit_against_the_gibbs_chain():
    """Gaussian family with a fit of doubled variance (multiplier sqrt 2): 300 replicates at Z_SWEEPS sweeps against 300
    long-run replicates (GIBBS_LONG sweeps) of fold_in_depth.chain on the same inputs, largest two-sample |z| below 5."""
    W, V_old, Y, nu2, lam2 = z_problem()
    stats, a, b = z_inputs(np.sqrt(2.0))
    rng = np.random.default_rng(11)
    V, rounds, unf = [], 0, 0
    for _ in range(300):
        o = sd.chain(V_old, W, lam2, 2, "gaussian", nu2, stats, a, b, rng=rng, sweeps=Z_SWEEPS, track_cond=False)
        V.append(o["v"])
        rounds, unf = rounds + o["rounds"], unf + o["unfinished"]
    z = two_sample_z(np.array(V), gibbs_replicates(300, 12, GIBBS_LONG))
    print("doubled variance: largest |z| %.2f, proposals per sweep %.2f, unfinished %d" % (z, rounds / (300.0 * Z_SWEEPS), unf))
    assert unf == 0 and z < 5


def test_layout_and_lds_count():
    assert Z_SWEEPS == sd.DEFAULT_SWEEPS
    T, H, K, tf = 9, 2, 5, 2
    nR = fd.new_rows(T, H, tf)[0].size
    n, bw = H * K, fd.half_bandwidth(H, K, tf)
    assert sd.sweep_length(T, H, K, tf, 40) == n + 41 + 4 * nR
    assert sd.record_length(T, H, K, tf, 3, 40) == 4 * nR + 3 * (n + 41 + 4 * nR)
    assert sd.random_draws(np.random.RandomState(0), T, H, K, tf, 3, 40, size=(2, 3)).shape == (2, 3, sd.record_length(T, H, K, tf, 3))
    for B in (0, 1, 3, 4, 9):
        Lt = max(min(T, tf + 1), B)
        assert sd.tail_depths(T, tf, B) == Lt
        assert sd.lds_bytes(T, H, K, tf, B) == 8 * (n * (bw + 1) + 6 * n + H * 15 + 5 * nR + nR * K + H * 4 + Lt * K) \
            + 8 * ((bw * (bw + 1) // 2 + 3) // 4) + 8192
    assert sd.lds_bytes(T, H, K, tf, 1) == fd.lds_bytes(T, H, K, tf) + 8 * 2 * n + sc.STATIC_LDS
    assert sd.lds_bytes(T, H, K, tf, 1) < sd.LDS_LIMIT and sd.lds_bytes(40, 400, 10, 2) > sd.LDS_LIMIT
    assert sd.DEFAULT_SWEEPS & (sd.DEFAULT_SWEEPS - 1) == 0 and sd.DEFAULT_MAX_ROUNDS == 40


def test_check_args_refusals():
    S, M, N, T, H, K, tf = 3, 2, 5, 4, 2, 2, 2
    nR = fd.new_rows(T, H, tf)[0].size
    L = sd.record_length(T, H, K, tf, 3)
    ok = lambda **kw: sd.check_args("poisson_identity", None, S, M, N, T, H, K, tf, **kw)
    ok()
    assert ok(start=np.ones((H, K)))[2].shape == (S, M, H, K) and ok(start=np.ones((M, H, K)))[2].shape == (S, M, H, K)
    assert ok(tau2=np.ones((M, nR)))[3].shape == (S, M, nR)
    good = np.full((S, M, L), 0.5)
    assert ok(sweeps=3, draws=good)[4].shape == (S, M, L)
    gam = good.copy()
    gam[0, 0, 0] = -1.0
    for kw in (dict(start=np.zeros(3)), dict(start=np.zeros((H + 1, K))), dict(start=np.full((H, K), np.nan)),
               dict(tau2=np.ones((M, nR + 1))), dict(tau2=np.ones((S, nR))), dict(tau2=-np.ones((M, nR))),
               dict(sweeps=3, draws=np.full((S, M, L - 1), 0.5)), dict(sweeps=3, draws=np.full((S, M, L), 1.5)),
               dict(sweeps=3, draws=np.full((S, M, L), -0.5)), dict(sweeps=3, draws=gam), dict(sweeps=0), dict(sweeps=2.5),
               dict(max_rounds=0), dict(transform="log"), dict(q=(5, 101)), dict(first_sample=-1), dict(first_sample=2 ** 30),
               dict(horizon=H + 1), dict(B=T + 1)):
        with pytest.raises(ValueError):
            ok(**kw)
    with pytest.raises(ValueError, match="LDS"):
        sd.check_args("poisson_identity", None, S, M, N, 40, 400, 10, 2)
    with pytest.raises(ValueError, match="LDS"):                       # the kept tail alone: a constraint that reaches 4000 depths
        sd.check_args("poisson_identity", None, S, M, N, 4000, 8, 10, 2, B=4000)
    sd.check_args("poisson_identity", None, S, M, N, 4000, 8, 10, 2, B=1)
    with pytest.raises(ValueError, match="below 64"):
        sd.check_args("poisson_identity", None, S, M, N, T, H, 10, 6)
    with pytest.raises(ValueError):
        sd.check_args("binomial", None, S, M, N, T, H, K, tf)
    with pytest.raises(NotImplementedError):
        sd.check_args(lambda W, V, d: 0.0, None, S, M, N, T, H, K, tf)
    with pytest.raises(ValueError, match="horizon"):
        sd.slice_statistics(np.ones((N, M, H)), "poisson", N, M, horizon=H + 1)
    with pytest.raises(ValueError, match="horizon"):
        sd.slice_statistics(None, "poisson", N, M)
    assert sd.slice_statistics(None, "gamma_grid", N, M, horizon=3)[3].shape == (M, N, 3)
    for bad in (np.ones((N, M)), np.ones((N + 1, M, H)), (np.ones((N, M, H)),) * 2, np.full((N, M, H), np.inf)):
        with pytest.raises(ValueError):
            sd.slice_statistics(bad, "poisson", N, M)


def _depth_bare(cls, **kw):
    m = _bare(cls, **kw)
    m.tf_order, m.stability = 2, 1e-6
    return m


def test_model_and_stateless_refusals_raise_before_any_device_call(no_device):
    """A callable likelihood, a sharded model, the Negative-Binomial model, a constrained model without Constraints (or with
    its own (J, T + 1) rows), bad shapes, an LDS refusal - each before any device call, and without taking a seed."""
    N, M, T, K, H = 5, 3, 4, 2, 2
    Y = np.ones((N, M, H))
    res = {"W": np.ones((6, N, K)), "V": np.ones((6, M, T, K)), "lam2": np.ones((6, 1))}
    none = np.zeros((0, T + H + 1))
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        g = _depth_bare(cls)
        with pytest.raises(NotImplementedError):
            _depth_bare(cls, world=2).slice_fold_in_depth(Y, results=res, Constraints=none)
        with pytest.raises(NotImplementedError):
            _depth_bare(cls, family=lambda W, V, d: 0.0).slice_fold_in_depth(Y, results=res, Constraints=none)
        with pytest.raises(RuntimeError):
            g.slice_fold_in_depth(Y, Constraints=none)         # nothing collected, no results
        for bad_Y in (np.ones((N, M + 1, H)), np.ones((N, M)), (Y, Y), np.full((N, M, H), np.inf)):
            with pytest.raises(ValueError):
                g.slice_fold_in_depth(bad_Y, results=res, Constraints=none)
        for kw in (dict(horizon=3), dict(start=np.zeros(3)), dict(tau2=np.ones((M, 1))), dict(sweeps=0), dict(q=(5, 101)),
                   dict(Constraints=fit_constraints(T)), dict(fit=(np.ones((M, N, H)),))):
            with pytest.raises(ValueError):
                g.slice_fold_in_depth(Y, results=res, **dict(dict(Constraints=none), **kw))
        with pytest.raises(ValueError):
            g.slice_fold_in_depth(None, results=res, Constraints=none)                      # no data and no horizon
        assert g._draws == 0                                   # a refused call takes no seed
    with pytest.raises(ValueError, match="extended grid"):
        _depth_bare(ConstrainedNonconjugateBayesianTensorFiltering).slice_fold_in_depth(Y, results=res)
    with pytest.raises(NotImplementedError):
        NegativeBinomialBayesianTensorFiltering.slice_fold_in_depth(object(), Y)
    with pytest.raises(NotImplementedError, match="slice_fold_in_depth"):
        _depth_bare(NonconjugateBayesianTensorFiltering).fold_in_depth(Y, results=res)
    big = _depth_bare(NonconjugateBayesianTensorFiltering, M=1, T=40, K=10)
    with pytest.raises(ValueError, match="LDS"):
        big.slice_fold_in_depth(np.ones((N, 1, 400)), results={"W": np.ones((2, N, 10)), "V": np.ones((2, 1, 40, 10)), "lam2": np.ones(2)})
    W, V, one = res["W"], res["V"], np.ones(6)
    with pytest.raises(ValueError):
        utils.slice_fold_in_depth(Y, W, V, "binomial", lam2=one)
    with pytest.raises(NotImplementedError):
        utils.slice_fold_in_depth(Y, W, V, lambda W, V, d: 0.0, lam2=one)
    for kw in (dict(), dict(lam2=-one), dict(lam2=one, first_sample=-1), dict(lam2=one, stability=0.0), dict(lam2=one, horizon=3),
               dict(lam2=one, Constraints=fit_constraints(T)), dict(lam2=one, tf_order=-1)):
        with pytest.raises(ValueError):
            utils.slice_fold_in_depth(Y, W, V, "poisson", **kw)
    with pytest.raises(ValueError):
        utils.slice_fold_in_depth(Y, W, V, "gaussian", lam2=one)                          # no variance
    with pytest.raises(ValueError, match="LDS"):
        utils.slice_fold_in_depth(np.ones((N, 1, 400)), np.ones((2, N, 10)), np.ones((2, 1, 40, 10)), "poisson", lam2=np.ones(2))
    with pytest.raises(ValueError, match="below 64"):
        utils.slice_fold_in_depth(np.ones((N, 1, 2)), np.ones((2, N, 10)), np.ones((2, 1, 4, 10)), "poisson", lam2=np.ones(2), tf_order=6)


def test_chain_refuses_a_bad_start():
    c = replay_case(3)
    p = sf.check_param(c["family"], c["param"])
    bad = sd.chain(c["Vs"][0, 0], c["Ws"][0], 0.1, c["tf_order"], c["family"], p, None, Constraints=c["Cons"],
                   start=-np.ones((c["H"], c["K"])), draws=c["draws"][0, 0], sweeps=c["sweeps"])
    assert bad["failed"] and np.all(np.isnan(bad["v"])) and np.all(np.isnan(bad["tau2"])) and bad["rounds"] == 0


@pytest.mark.parametrize("which", list(range(len(REPLAY_CASES))) + ["capped", "fixed", "reach"])
def test_replay_inputs_are_safe(which):
    """The inputs of every replay case are chosen by the definition alone (cond(Q) <= COND_MAX, margins above MARGIN_MIN),
    and with such margins scaling every nu by 1 + 1e-6 changes no rounds / unfinished count."""
    c = {"capped": capped_case, "fixed": fixed_case, "reach": reach_case}[which]() if isinstance(which, str) else replay_case(which)
    want = c["want"]
    assert safe(want), (want["cond"], want["margin_ll"], want["margin_slack"])
    assert want["rounds"].sum() > 0 and not want["failed"].any()
    if which == "capped":
        assert want["unfinished"].sum() > 0
    if which == "fixed":
        assert np.array_equal(want["Tau2"], np.broadcast_to(c["tau2"], want["Tau2"].shape))
    moved = definition(c, nu_scale=1.0 + 1e-6)
    assert np.array_equal(moved["rounds"], want["rounds"]) and np.array_equal(moved["unfinished"], want["unfinished"])
    assert np.max(np.abs(moved["V"] - want["V"]) / np.maximum(1.0, np.abs(want["V"]))) < 1e-4


def test_the_unit_and_the_symbols_are_wired():
    assert os.path.join(_native.CSRC, "btf_slice_fold_depth.hip") in _native.SOURCES
    assert os.path.exists(os.path.join(_native.CSRC, "btf_slice_fold_depth.h"))
    assert len(_native.UNITS) + _native.INST_PARTS == 32
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    analysis = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    for name in ("btf_slice_fold_depth", "btf_collect_slice_fold_depth"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _native.SIGNATURES
        assert re.search(r"^int\s+%s\s*\(" % name, analysis, flags=re.M), name + " is defined beside the analysis entry points"
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_native.SIGNATURES[name][1]), name
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load()
        assert hasattr(lib, "btf_slice_fold_depth") and hasattr(lib, "btf_collect_slice_fold_depth")
