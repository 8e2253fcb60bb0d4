"""negbin_fold_in_cols / negbin_fold_in_depth on the GPU (csrc/btf_fold_chain.h: negbin_draw_depth, negbin_accumulate).

Yardsticks: the numpy definitions functionalmf_amd.negbin_fold_in.chain_cols / chain_depth on the same variates AND the
same Polya-Gamma weights (the tolerance of test_replay_equals_numpy_chain of the sibling kernels: 1e-6 * max(1, |V|) with
cond(Q) < 1e9 asserted on the numpy side), the Gaussian fold-ins where there is no data, the Binomial fold-ins on (Y, Y + R)
where the counts are small, and a long numpy run of chain_cols where they are large.
"""
import numpy as np
import pytest
from conftest import load_golden

from functionalmf_amd import _native, fold_in_cols as fc, fold_in_depth as fd, negbin_fold_in as nf, utils
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

pytestmark = pytest.mark.gpu

V_TOL = 1e-6
COND_MAX = 1e9
S_REPLAY, C_REPLAY, SWEEPS_REPLAY = 3, 2, 3

# ---- measured constants ("Folding new columns and depth slices into a Negative-Binomial fit"; scripts/negbin_fold_in_rate.py --step bias
# writes profiles/r28_negbin_fold_in_rate.jsonl).  Each: the largest |difference| of the means of ilogit(W v) at S = 16384,
# doubled.
NB_VS_BINOMIAL_BIAS_COLS = 2 * 0.00037     # sweeps = 512: largest |NB - Binomial| = 0.00037 at S = 16384 (5 se of the difference there: 0.00217)
NB_VS_BINOMIAL_BIAS_DEPTH = 2 * 0.00048    # sweeps = 128: largest |NB - Binomial| = 0.00048 at S = 16384 (5 se of the difference there: 0.00509)
LARGE_COUNT_BIAS = 2 * 0.00183             # sweeps = 512: largest |fold-in - oracle| = 0.00183 at S = 16384 (oracle: 60000 sweeps, batch-means se <= 0.00051)
S_STAT = 4096

LAYOUTS = ("scalar", "row", "chain_or_depth", "row_depth")


def close(a, b, tol=V_TOL):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= tol


def rate_of(rs, layout, axis, S, C, N, D):
    """A rate (S,) + a shape that broadcasts against the new tensor - (C,N,T) for columns, (N,M,H) for depths - varying
    along: nothing; the rows; the depths (columns) / the fitted columns (depths); rows and depths."""
    lead = {"scalar": (1, 1, 1), "row": (1, N, 1), "chain_or_depth": (1, 1, D) if axis == "cols" else (C, 1, 1),
            "row_depth": (1, N, D)}[layout]                               # in (chain, row, depth) order
    r = rs.uniform(0.5, 6.0, size=(S,) + lead)
    return r if axis == "cols" else r.transpose(0, 2, 1, 3)


def dense(rate, axis, S, C, N, D):
    """The same rate broadcast to (S, chain, row, depth)."""
    r = rate if axis == "cols" else rate.transpose(0, 2, 1, 3)
    return np.broadcast_to(r, (S, C, N, D))


def cols_problem(K, tf, N, T, layout, seed, nreps=1, holes=False):
    rs = np.random.RandomState(seed)
    S, C, sw = S_REPLAY, C_REPLAY, SWEEPS_REPLAY
    Ws = rs.normal(size=(S, N, K))
    lam2 = rs.uniform(0.05, 0.3, size=S)
    Y = rs.poisson(4.0, size=(C, N, T, nreps)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    if holes:
        Y[:, N // 2] = np.nan                                             # a wholly missing row
        Y[:, :, T // 2] = np.nan                                          # a wholly missing depth
    rate = rate_of(rs, layout, "cols", S, C, N, T)
    draws = fc.random_draws(rs, T, K, tf, sw, size=(S, C))
    omega = rs.gamma(2.0, 0.4, size=(S, C, sw, N, T))
    return Ws, lam2, Y if nreps > 1 else Y[..., 0], rate, draws, omega


def cols_numpy(K, tf, N, T, layout, nreps=1, holes=False):
    """A case whose numpy chains keep cond(Q) under COND_MAX (the first of a fixed sequence of seeds), and their results."""
    base = 100000 * K + 10000 * tf + 10 * N + T + (500 if holes else 0)
    for k in range(50):
        Ws, lam2, Y, rate, draws, omega = p = cols_problem(K, tf, N, T, layout, base + 7919 * k, nreps, holes)
        S, C = draws.shape[:2]
        r = dense(rate, "cols", S, C, N, T)
        conds, out = [], []
        for s in range(S):
            for c in range(C):
                out.append(nf.chain_cols(Y[c], Ws[s], r[s, c], lam2[s], tf, SWEEPS_REPLAY, draws[s, c], omega=omega[s, c],
                                         on_system=lambda Q: conds.append(np.linalg.cond(Q))))
        if max(conds) < COND_MAX:
            V, Vm, T2 = (np.array([o[i] for o in out]).reshape((S, C) + out[0][i].shape) for i in range(3))
            return p, V, Vm, T2, max(conds)
    raise AssertionError("no seed with cond(Q) < %g" % COND_MAX)


def depth_problem(K, tf, N, T, H, layout, seed, nreps=1, holes=False):
    rs = np.random.RandomState(seed)
    S, M, sw = S_REPLAY, C_REPLAY, SWEEPS_REPLAY
    Ws = rs.normal(size=(S, N, K))
    Vs = 0.3 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2)
    lam2 = rs.uniform(0.05, 0.3, size=S)
    Y = rs.poisson(4.0, size=(N, M, H, nreps)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    if holes:
        Y[N // 2] = np.nan
        Y[:, :, H // 2] = np.nan
    rate = rate_of(rs, layout, "depth", S, M, N, H)
    draws = fd.random_draws(rs, T, H, K, tf, sw, size=(S, M))
    omega = rs.gamma(2.0, 0.4, size=(S, M, sw, N, H))
    return Ws, Vs, lam2, Y if nreps > 1 else Y[..., 0], rate, draws, omega


def depth_numpy(K, tf, N, T, H, layout, nreps=1, holes=False):
    base = 100000 * K + 10000 * tf + 10 * N + 3 * T + H + (500 if holes else 0)
    for k in range(50):
        Ws, Vs, lam2, Y, rate, draws, omega = p = depth_problem(K, tf, N, T, H, layout, base + 7919 * k, nreps, holes)
        S, M = draws.shape[:2]
        r = dense(rate, "depth", S, M, N, H)
        conds, out = [], []
        for s in range(S):
            for j in range(M):
                out.append(nf.chain_depth(Y[:, j], Ws[s], Vs[s, j], r[s, j], lam2[s], tf, SWEEPS_REPLAY, draws[s, j], omega=omega[s, j],
                                          on_system=lambda Q: conds.append(np.linalg.cond(Q))))
        if max(conds) < COND_MAX:
            V, Vm, T2 = (np.array([o[i] for o in out]).reshape((S, M) + out[0][i].shape) for i in range(3))
            return p, V, Vm, T2, max(conds)
    raise AssertionError("no seed with cond(Q) < %g" % COND_MAX)


def check_replay(out, V, Vm, T2, cond, label):
    print("%s  max cond(Q) %.2e  max|V| %.2f  err V %.2e  V_mean %.2e  Tau2 (rel) %.2e"
          % (label, cond, np.abs(V).max(), np.abs(out["V"] - V).max(), np.abs(out["V_mean"] - Vm).max(),
             np.max(np.abs(out["Tau2"] - T2) / T2)))
    assert cond < COND_MAX
    assert close(out["V_mean"], Vm)
    assert close(out["V"], V)
    assert float(np.max(np.abs(out["Tau2"] - T2) / T2)) <= V_TOL


def nb_model(N, M, T, K, tf, rdims):
    np.random.seed(0)
    return NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=tf, rdims=rdims)


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("Tsel", [0, 1])
@pytest.mark.parametrize("N", [5, 64, 65, 130])
@pytest.mark.parametrize("tf_order", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 3, 5, 10])
def test_replay_cols(K, tf_order, N, Tsel):
    """1. With draws= and omega= the kernel equals chain_cols: S = 3, C = 2, sweeps = 3, T in {tf + 2, 6}, N at the 64-row
    block edge and in a third block, 20 % of the cells missing; the rate layout changes from case to case."""
    T = (tf_order + 2, 6)[Tsel]
    layout = LAYOUTS[(K + tf_order + N + Tsel) % 4]
    (Ws, lam2, Y, rate, draws, omega), V, Vm, T2, cond = cols_numpy(K, tf_order, N, T, layout)
    out = utils.negbin_fold_in_cols(Y, Ws, rate, lam2=lam2, tf_order=tf_order, draws=draws, omega=omega, sweeps=SWEEPS_REPLAY,
                                    summary=False)
    check_replay(out, V, Vm, T2, cond, "cols K=%d tf=%d N=%d T=%d rate=%s" % (K, tf_order, N, T, layout))


@pytest.mark.parametrize("Hsel", [0, 1, 2])
@pytest.mark.parametrize("N", [5, 64, 65, 130])
@pytest.mark.parametrize("tf_order", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 3, 5, 10])
def test_replay_depth(K, tf_order, N, Hsel):
    """1. The same for chain_depth: M = 2 fitted columns of T = 6 kept depths, H in {1, tf + 1, tf + 3}."""
    H = (1, tf_order + 1, tf_order + 3)[Hsel]
    layout = LAYOUTS[(K + tf_order + N + Hsel) % 4]
    (Ws, Vs, lam2, Y, rate, draws, omega), V, Vm, T2, cond = depth_numpy(K, tf_order, N, 6, H, layout)
    out = utils.negbin_fold_in_depth(Y, Ws, Vs, rate, lam2=lam2, tf_order=tf_order, draws=draws, omega=omega, sweeps=SWEEPS_REPLAY,
                                     summary=False)
    check_replay(out, V, Vm, T2, cond, "depth K=%d tf=%d N=%d H=%d rate=%s" % (K, tf_order, N, H, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_replay_through_the_model_and_with_holes(layout):
    """1. A wholly missing row, a wholly missing depth and two replicates; and every rate layout through results["R"] of the
    model (where the layout does not vary along the folded axis) against rate=: the same bits."""
    K, tf, N, T, H = 3, 2, 65, 6, 3
    (Ws, lam2, Y, rate, draws, omega), V, Vm, T2, cond = cols_numpy(K, tf, N, T, layout, nreps=2, holes=True)
    kw = dict(draws=draws, omega=omega, sweeps=SWEEPS_REPLAY, summary=False)
    out = utils.negbin_fold_in_cols(Y, Ws, rate, lam2=lam2, tf_order=tf, **kw)
    check_replay(out, V, Vm, T2, cond, "cols with holes, rate=%s" % layout)
    hole = np.isnan(Y).all(axis=(1, 3))                                   # (C,T): depths nobody observed
    assert hole.any() and np.isnan(Y[:, N // 2]).all()
    # through the model: R over (N,M,T) with the column axis shared
    S, C = draws.shape[:2]
    R = rate.transpose(0, 2, 1, 3)                                        # (S,1,N|1,T|1) -> (S,N|1,1,T|1)
    rdims = tuple(a for a, e in enumerate(R.shape[1:]) if e == 1)
    m = nb_model(N, 4, T, K, tf, rdims)
    res = {"W": Ws, "V": np.zeros((S, 4, T, K)), "lam2": lam2, "R": R}
    via_R = m.negbin_fold_in_cols(Y, res, **kw)
    via_rate = m.negbin_fold_in_cols(Y, dict(res, R=np.ones((S, N, 4, T))), rate=rate, **kw)
    for k in ("V", "V_mean", "Tau2"):
        assert np.array_equal(via_R[k], out[k]) and np.array_equal(via_rate[k], out[k]), k
    # depths
    (Ws, Vs, lam2, Y, rate, draws, omega), V, Vm, T2, cond = depth_numpy(K, tf, N, T, H, layout, nreps=2, holes=True)
    kw = dict(draws=draws, omega=omega, sweeps=SWEEPS_REPLAY, summary=False)
    out = utils.negbin_fold_in_depth(Y, Ws, Vs, rate, lam2=lam2, tf_order=tf, **kw)
    check_replay(out, V, Vm, T2, cond, "depth with holes, rate=%s" % layout)
    M = Vs.shape[1]
    m = nb_model(N, M, T, K, tf, tuple(a for a, e in enumerate(rate.shape[1:]) if e == 1) if rate.shape[3] == 1 else (2,))
    res = {"W": Ws, "V": Vs, "lam2": lam2, "R": rate}
    if rate.shape[3] == 1:                                                # the fitted layout may not vary along the depths
        via_R = m.negbin_fold_in_depth(Y, res, **kw)
        assert all(np.array_equal(via_R[k], out[k]) for k in ("V", "V_mean", "Tau2"))
    else:
        with pytest.raises(ValueError, match="pass rate="):
            m.negbin_fold_in_depth(Y, dict(res, R=np.ones((S, N, 1, T))), **kw)
    via_rate = m.negbin_fold_in_depth(Y, dict(res, R=np.ones((S, 1, 1, T))), rate=rate, **kw)
    assert all(np.array_equal(via_rate[k], out[k]) for k in ("V", "V_mean", "Tau2"))


def test_same_bits():
    """2. first_sample splits, the first column folded alone, a scalar rate as (S,) against the same value as a dense
    (S,N,1,T) array of the model's layout, and the same seed twice: np.array_equal.  (A chain's stream holds the column's
    index in the call, as in fold_in_cols: a column folded alone has the bits of column 0 of a larger call, so "one column at
    a time" is held for the column that keeps its index - the limit of the sibling's test.)"""
    rs = np.random.RandomState(3)
    S, C, N, T, K, tf, sw = 6, 3, 70, 7, 3, 2, 5
    Ws, lam2 = rs.normal(size=(S, N, K)), np.full(S, 0.1)
    Y = rs.poisson(5.0, size=(C, N, T)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    r = rs.uniform(1.0, 80.0, size=S)                                     # (cells on both sides of the normal range's edge)
    Y[0, :10] = 150.0
    keys = ("V", "V_mean", "Tau2", "mean", "quantiles")
    kw = dict(lam2=lam2, tf_order=tf, seed=11, sweeps=sw)
    a = utils.negbin_fold_in_cols(Y, Ws, r, **kw)
    b = utils.negbin_fold_in_cols(Y, Ws, r, **kw)
    assert all(np.array_equal(a[k], b[k]) for k in keys) and np.all(np.isfinite(a["V"]))
    assert not np.array_equal(a["V"], utils.negbin_fold_in_cols(Y, Ws, r, **dict(kw, seed=12))["V"])
    lo = utils.negbin_fold_in_cols(Y, Ws[:2], r[:2], **dict(kw, lam2=lam2[:2]))
    hi = utils.negbin_fold_in_cols(Y, Ws[2:], r[2:], first_sample=2, **dict(kw, lam2=lam2[2:]))
    for k in keys[:3]:
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k]), k
    one = utils.negbin_fold_in_cols(Y[:1], Ws, r, **kw)
    assert all(np.array_equal(one[k][:, 0], a[k][:, 0]) for k in keys[:3])
    m = nb_model(N, 2, T, K, tf, (1,))
    res = {"W": Ws, "V": np.zeros((S, 2, T, K)), "lam2": lam2, "R": np.broadcast_to(r[:, None, None, None], (S, N, 1, T)).copy()}
    d = m.negbin_fold_in_cols(Y, res, seed=11, sweeps=sw)
    assert all(np.array_equal(d[k], a[k]) for k in keys)
    # depths
    M, H = 3, 4
    Vs = 0.3 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2)
    Yd = rs.poisson(5.0, size=(N, M, H)).astype(float)
    Yd[rs.uniform(size=Yd.shape) < 0.3] = np.nan
    a = utils.negbin_fold_in_depth(Yd, Ws, Vs, r, **kw)
    b = utils.negbin_fold_in_depth(Yd, Ws, Vs, np.broadcast_to(r[:, None, None, None], (S, N, M, 1)).copy(), **kw)
    assert all(np.array_equal(a[k], b[k]) for k in keys) and np.all(np.isfinite(a["V"]))
    lo = utils.negbin_fold_in_depth(Yd, Ws[:4], Vs[:4], r[:4], **dict(kw, lam2=lam2[:4]))
    hi = utils.negbin_fold_in_depth(Yd, Ws[4:], Vs[4:], r[4:], first_sample=4, **dict(kw, lam2=lam2[4:]))
    for k in keys[:3]:
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k]), k


def test_no_data_is_the_gaussian_chain():
    """3. Without data no Polya-Gamma draw is made and the other generator keys are the Gaussian family's: the forecast
    (Y_new=None, horizon=H) equals fold_in_depth's with the same seed, W, V, lam2 and sweeps, bit for bit, and wholly
    unobserved columns equal fold_in_cols' (the Gaussian call takes them: their chain is the prior's)."""
    rs = np.random.RandomState(9)
    S, N, M, T, K, tf, H = 5, 66, 3, 8, 3, 2, 4
    Ws, Vs, lam2 = rs.normal(size=(S, N, K)), 0.3 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2), rs.uniform(0.05, 0.3, size=S)
    nb = utils.negbin_fold_in_depth(None, Ws, Vs, None, horizon=H, lam2=lam2, tf_order=tf, seed=4, sweeps=6, summary=False)
    ga = utils.fold_in_depth(None, Ws, Vs, "gaussian", horizon=H, nu2=np.ones(S), lam2=lam2, tf_order=tf, seed=4, sweeps=6, summary=False)
    assert np.array_equal(nb["V"], ga["V"]) and np.array_equal(nb["Tau2"], ga["Tau2"])
    Y = np.full((2, N, T), np.nan)
    nb = utils.negbin_fold_in_cols(Y, Ws, np.full(S, 3.0), lam2=lam2, tf_order=tf, seed=4, sweeps=6, summary=False)
    ga = utils.fold_in_cols(Y, Ws, "gaussian", nu2=np.ones(S), lam2=lam2, tf_order=tf, seed=4, sweeps=6, summary=False)
    assert np.array_equal(nb["V"], ga["V"]) and np.array_equal(nb["Tau2"], ga["Tau2"])


def small_count_problem(seed=17):
    """N = 12, T = 6, K = 2, integer R with every y + R <= 32."""
    rs = np.random.RandomState(seed)
    N, T, K = 12, 6, 2
    W = rs.normal(size=(N, K))
    v = 0.5 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    R = rs.randint(2, 9, size=(N, 1)).astype(float)
    Y = np.minimum(rs.negative_binomial(R.astype(int) * np.ones((N, T), dtype=int), 1.0 - utils.ilogit(W.dot(v.T))), 24).astype(float)
    Y[rs.uniform(size=(N, T)) < 0.15] = np.nan
    assert np.nanmax(Y + R) <= 32
    return W, v, Y, R, 0.1


def nb_vs_binomial(axis, S):
    """(|difference| of the means of ilogit(W v), 5 standard errors of the difference) between the NB fold-in and the
    Binomial fold-in on (Y, Y + R), per cell, at the default sweeps from the same start."""
    W, v, Y, R, lam2 = small_count_problem()
    N, T = Y.shape
    Ws, l2 = np.repeat(W[None], S, axis=0), np.full(S, lam2)
    if axis == "cols":
        nb = utils.negbin_fold_in_cols(Y[None], Ws, np.broadcast_to(R[None, None], (S, 1, N, 1)), lam2=l2, seed=21, summary=False)
        bi = utils.fold_in_cols((Y[None], (Y + R)[None]), Ws, "binomial", lam2=l2, seed=22, summary=False)
        pa, pb = (utils.ilogit(np.einsum("nk,stk->snt", W, o["V"][:, 0])) for o in (nb, bi))
    else:
        H = 3
        Vs = np.repeat(v[None, None, :T - H], S, axis=0)
        Yd = Y[:, None, T - H:]
        nb = utils.negbin_fold_in_depth(Yd, Ws, Vs, np.broadcast_to(R[None, :, None], (S, N, 1, 1)), lam2=l2, seed=21, summary=False)
        bi = utils.fold_in_depth((Yd, Yd + R[:, None]), Ws, Vs, "binomial", lam2=l2, seed=22, summary=False)
        pa, pb = (utils.ilogit(np.einsum("nk,stk->snt", W, o["V"][:, 0])) for o in (nb, bi))
    d = np.abs(pa.mean(axis=0) - pb.mean(axis=0))
    return d, 5 * np.sqrt(pa.var(axis=0, ddof=1) / S + pb.var(axis=0, ddof=1) / S)


@pytest.mark.parametrize("axis", ["cols", "depth"])
def test_against_the_binomial_fold_in(axis):
    """4. At the same sweeps and start the NB call and the Binomial fold-in on (Y, Y + R) target the same finite-sweep
    distribution: the means of ilogit(W v) over S = 4096 samples differ by at most 5 standard errors of the difference plus
    the series-bias allowance (measured once at S = 16384, doubled: NB_VS_BINOMIAL_BIAS_*)."""
    d, se5 = nb_vs_binomial(axis, S_STAT)
    bias = NB_VS_BINOMIAL_BIAS_COLS if axis == "cols" else NB_VS_BINOMIAL_BIAS_DEPTH
    print("%s: largest |NB - Binomial| %.5f (5 se there %.5f, bias allowance %.5f)" % (axis, d.max(), se5.reshape(-1)[np.argmax(d)], bias))
    assert np.all(d <= se5 + bias)


def large_count_problem():
    g = load_golden("negbin_fold_in_oracle.npz")
    return g["W"], g["Y"], float(g["rate"]), float(g["lam2"]), g["mean"], g["se"]


def large_count_bias(S):
    W, Y, rate, lam2, m, se = large_count_problem()
    b = np.where(np.isnan(Y), 0.0, Y + rate)
    assert (b >= 200).any() and ((b > 0) & (b < 200)).any()                # cells on both sides of PG_NORMAL_B
    out = utils.negbin_fold_in_cols(Y[None], np.repeat(W[None], S, axis=0), np.full(S, rate), lam2=np.full(S, lam2), seed=5,
                                    summary=False)
    p = utils.ilogit(np.einsum("nk,stk->snt", W, out["V"][:, 0]))
    return np.abs(p.mean(axis=0) - m), 5 * np.sqrt(p.var(axis=0, ddof=1) / S + se ** 2), float(se.max())


def test_large_counts_against_a_long_numpy_chain():
    """5. R = 50 and counts into the hundreds (cells on both sides of PG_NORMAL_B = 200): the mean of ilogit(W v) at the
    default sweeps over S = 4096 copies of one state against a long numpy run of chain_cols (scripts/negbin_fold_in_rate.py
    --step oracle; tests/golden/negbin_fold_in_oracle.npz).  Allowance: the measured bias doubled plus 5 standard errors."""
    d, se5, se = large_count_bias(S_STAT)
    print("large counts: largest |fold-in - oracle| %.5f (5 se there %.5f; bias allowance %.5f, oracle se <= %.5f)"
          % (d.max(), se5.reshape(-1)[np.argmax(d)], LARGE_COUNT_BIAS, se))
    assert np.all(d <= se5 + LARGE_COUNT_BIAS)


def c_cols(Ws, lam2, Y, rate, seed=3, sweeps=4, first_sample=0):
    """btf_negbin_fold_in_cols called directly (no summary): (rc, message, fail index, V, V_mean, Tau2)."""
    lib, d = _native.load(), _native.dptr
    S, N, K = Ws.shape
    C, T = Y.shape[0], Y.shape[2]
    cnt, ys = nf.cell_statistics(Y, (C, N, T))
    r, rs = nf.rate_strides(nf.resolve_rate("cols", None, rate, S, C, N, T))
    nD = fc.penalty(T, 2).shape[0]
    V, Vm, T2 = np.zeros((S, C, T, K)), np.zeros((S, C, T, K)), np.zeros((S, C, nD))
    rc = lib.btf_negbin_fold_in_cols(0, S, C, N, T, K, 2, d(np.ascontiguousarray(Ws)), d(lam2), d(cnt), d(ys), d(r), *rs, None, None, seed,
                                     sweeps, first_sample, 1e-6, d(V), d(Vm), d(T2), 0, None, 0, None, None)
    return rc, lib.btf_last_error(None).decode(), lib.btf_fail_index(None), V, Vm, T2


def c_depth(Ws, Vs, lam2, Y, rate, seed=3, sweeps=4, first_sample=0, T_arg=None, draws=None):
    """btf_negbin_fold_in_depth called directly (no summary): (rc, message, fail index, V, V_mean, Tau2)."""
    lib, d = _native.load(), _native.dptr
    S, N, K = Ws.shape
    M, T = Vs.shape[1:3]
    H, cnt, ys = nf.slice_cells(Y, N, M)
    r, rs = nf.rate_strides(nf.resolve_rate("depth", None, rate, S, M, N, H))
    cnt, ys = np.ascontiguousarray(cnt.transpose(1, 2, 0)), np.ascontiguousarray(ys.transpose(1, 2, 0))
    nR = fd.new_rows(T, H, 2)[0].size
    Vt = np.ascontiguousarray(Vs[:, :, T - fd.tail_depths(T, 2):])
    V, Vm, T2 = np.zeros((S, M, H, K)), np.zeros((S, M, H, K)), np.zeros((S, M, nR))
    rc = lib.btf_negbin_fold_in_depth(0, S, N, M, T if T_arg is None else T_arg, H, K, 2, d(np.ascontiguousarray(Ws)), d(Vt), d(lam2), d(cnt),
                                      d(ys), d(r), *rs, None, d(draws), seed, sweeps, first_sample, 1e-6, d(V), d(Vm), d(T2), 0, None, 0,
                                      None, None)
    return rc, lib.btf_last_error(None).decode(), lib.btf_fail_index(None), V, Vm, T2


def check_failed_sample(clean, failed, s_bad, index, nchains):
    """The call with a non-finite W in sample s_bad: BTF_ESTATE, the smallest failing chain, nan for every chain of that
    sample (W is shared by its chains) and the clean call's bits everywhere else."""
    rc, msg, idx, V, Vm, T2 = failed
    assert clean[0] == _native.BTF_OK and clean[2] == -1
    assert rc == _native.BTF_ESTATE and idx == index and ("index %d " % index) in msg and "nan" in msg
    assert index == (index // nchains) * nchains                          # column 0 of the failing sample: the smallest
    for got, want in zip((V, Vm, T2), clean[3:]):
        assert np.all(np.isnan(got[s_bad])) and np.all(np.isfinite(want))
        keep = np.arange(got.shape[0]) != s_bad
        assert np.array_equal(got[keep], want[keep])


def test_failures():
    """6. BTF_EINVAL for every refusal of the C entry points (reached past the Python checks), and a non-finite W: nan
    outputs for the failing sample's chains, the clean call's bits for the others, BTF_ESTATE, and btf_fail_index at the
    smallest failing chain - through the C entry points, which hand the outputs back beside the code."""
    lib = _native.load()
    d = _native.dptr
    S, C, N, T, K, tf, sw = 2, 2, 6, 5, 2, 1, 2
    nD = fc.penalty(T, tf).shape[0]
    Ws, lam2 = np.ones((S, N, K)), np.ones(S)
    cnt, ys, rate = np.ones((C, N, T)), np.full((C, N, T), 3.0), np.full(S, 2.0)
    V, Vm, T2 = np.zeros((S, C, T, K)), np.zeros((S, C, T, K)), np.zeros((S, C, nD))

    def call(cnt=cnt, ys=ys, rate=rate, rs=(1, 0, 0, 0), omega=None, draws=None, sweeps=sw, lam2=lam2, N=N):
        rc = lib.btf_negbin_fold_in_cols(0, S, C, N, T, K, tf, d(Ws), d(lam2), d(cnt), d(ys), d(rate), *rs, d(omega), d(draws), 1, sweeps, 0,
                                         1e-6, d(V), d(Vm), d(T2), 0, None, 0, None, None)
        return rc, lib.btf_last_error(None).decode()

    assert call()[0] == _native.BTF_OK
    for kw, text in ((dict(ys=np.full((C, N, T), -1.0)), "finite and non-negative"),
                     (dict(cnt=np.full((C, N, T), np.inf)), "finite and non-negative"),
                     (dict(rate=np.array([2.0, 0.0])), "rate must be finite and positive"),
                     (dict(rate=np.array([2.0, np.nan])), "rate must be finite and positive"),
                     (dict(rs=(1, 3, 0, 0)), "rate strides"),
                     (dict(ys=np.full((C, N, T), 9e14), rate=np.array([2.0, 1e14])), "below 1e15"),
                     (dict(draws=np.ones((S, C, fc.draws_length(T, K, tf, sw)))), "needs omega"),
                     (dict(omega=np.full((S, C, sw, T, N), -1.0)), "omega must be finite"),
                     (dict(sweeps=0), "sweeps"),
                     (dict(lam2=np.array([1.0, -1.0])), "lam2"),
                     (dict(N=20000), "bytes of LDS")):
        big = kw.get("N", N) != N
        rc, msg = call(**dict(kw, cnt=np.ones((C, 20000, T)), ys=np.ones((C, 20000, T))) if big else kw)
        assert rc == _native.BTF_EINVAL and text in msg, (kw.keys(), msg)
    assert str(nf.lds_bytes(20000, T, K, tf)) in call(N=20000, cnt=np.ones((C, 20000, T)), ys=np.ones((C, 20000, T)))[1]
    with pytest.raises(ValueError, match="LDS"):
        utils.negbin_fold_in_cols(np.zeros((1, 20000, T)), np.ones((S, 20000, K)), rate, lam2=lam2, tf_order=tf)
    # the depth entry point's own refusals
    (Ws, Vs, lam2, Y, rate, _, _), _, _, _, _ = depth_numpy(3, 2, 65, 6, 3, "row")
    assert c_depth(Ws, Vs, lam2, Y, rate)[0] == _native.BTF_OK
    nanV = Vs.copy()
    nanV[1, 0, -1, 0] = np.nan
    for kw, text in ((dict(Vs=nanV), "kept curves must be finite"), (dict(T_arg=8190), "ndepth + horizon must stay within 8192"),
                     (dict(draws=np.ones((3, 2, fd.draws_length(6, 3, 3, 2, 4)))), "needs omega"),
                     (dict(sweeps=0), "sweeps"), (dict(lam2=-lam2), "lam2")):
        args = dict(Ws=Ws, Vs=Vs, lam2=lam2, Y=Y, rate=rate)
        args.update(kw)
        rc, msg = c_depth(**args)[:2]
        assert rc == _native.BTF_EINVAL and text in msg and "negbin_fold_in_depth" in msg, (list(kw), msg)
    bigW, bigY = np.ones((3, 20000, 3)), np.zeros((20000, 2, 3))
    rc, msg = c_depth(bigW, Vs, lam2, bigY, np.full(3, 2.0))[:2]
    assert rc == _native.BTF_EINVAL and "bytes of LDS" in msg and "negbin_fold_in_depth" in msg
    # a non-finite W, columns: sample 1 of 3, two new columns
    (Ws, lam2, Y, rate, _, _), _, _, _, _ = cols_numpy(3, 2, 65, 6, "row")
    clean = c_cols(Ws, lam2, Y, rate)
    bad = Ws.copy()
    bad[1, 7, 0] = np.nan
    check_failed_sample(clean, c_cols(bad, lam2, Y, rate), 1, 1 * 2 + 0, 2)
    check_failed_sample(c_cols(Ws, lam2, Y, rate, first_sample=10), c_cols(bad, lam2, Y, rate, first_sample=10), 1, (10 + 1) * 2 + 0, 2)
    with pytest.raises(_native.BTFError, match=r"index %d " % (1 * 2 + 0)) as e:      # the Python call raises what the code stands for
        utils.negbin_fold_in_cols(Y, bad, rate, lam2=lam2, seed=3, sweeps=4, summary=False)
    assert e.value.code == _native.BTF_ESTATE
    # depths: an infinite W in sample 2 of 3, two fitted columns
    (Ws, Vs, lam2, Y, rate, _, _), _, _, _, _ = depth_numpy(3, 2, 65, 6, 3, "row")
    clean = c_depth(Ws, Vs, lam2, Y, rate)
    bad = Ws.copy()
    bad[2, 0, 1] = np.inf
    check_failed_sample(clean, c_depth(bad, Vs, lam2, Y, rate), 2, 2 * 2 + 0, 2)
    with pytest.raises(_native.BTFError, match=r"index %d " % (2 * 2 + 0)) as e:
        utils.negbin_fold_in_depth(Y, bad, Vs, rate, lam2=lam2, seed=3, sweeps=4, summary=False)
    assert e.value.code == _native.BTF_ESTATE


def test_composition_with_summary_and_predictive():
    """7. The summary is the summary kernel's on (W, V_new); the returned draws go into posterior_summary and into
    posterior_predictive with the Negative-Binomial family."""
    rs = np.random.RandomState(2)
    S, N, M, T, K, H = 40, 20, 3, 8, 3, 3
    Ws, Vs = rs.normal(size=(S, N, K)), 0.3 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2)
    lam2, r = np.full(S, 0.1), rs.uniform(2.0, 5.0, size=S)
    Yd = rs.poisson(4.0, size=(N, M, H)).astype(float)
    q = (5, 50, 95)
    out = utils.negbin_fold_in_depth(Yd, Ws, Vs, r, lam2=lam2, seed=9, sweeps=16, q=q, transform="ilogit")
    mean, quant = utils.posterior_summary(Ws, out["V"], q=q, transform="ilogit")
    np.testing.assert_allclose(mean, out["mean"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(quant, out["quantiles"], rtol=0, atol=1e-12)
    assert np.all((out["mean"] > 0) & (out["mean"] < 1)) and out["nsamples"] == S
    V_all = np.concatenate([Vs, out["V"]], axis=2)
    pp = utils.posterior_predictive(Ws, V_all, "negative_binomial", R=r, seed=1)
    assert pp["mean"].shape == (N, M, T + H) and np.all(np.isfinite(pp["mean"]))
    Yc = rs.poisson(4.0, size=(2, N, T)).astype(float)
    oc = utils.negbin_fold_in_cols(Yc, Ws, r, lam2=lam2, seed=9, sweeps=16, q=q)
    mean, quant = utils.posterior_summary(Ws, oc["V"], q=q)
    assert np.array_equal(mean, oc["mean"]) and np.array_equal(quant, oc["quantiles"])
