"""fold_in_cols on the GPU (csrc/btf_fold_in_cols.h): the curves of columns the chain never saw, per kept sample.

Yardsticks: the numpy definition functionalmf_amd.fold_in_cols.chain on the same variates, draw for draw (the project's V
tolerance, 1e-6 * max(1, |V|): README "1e-6 (V, conditioning-limited)", with the numpy side asserting cond(Q) < 1e9 for every
system of the case), the project's own reference-pinned V step, numpy's generator (two-sample z), the stationary law of a
one-column Binomial model, and the chain that includes the column.
"""
import numpy as np
import pytest
from conftest import load_golden

from functionalmf_amd import fold_in_cols as fc, utils
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering,
                                     NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering)

pytestmark = pytest.mark.gpu

V_TOL = 1e-6
COND_MAX = 1e9

# ---- measured constants ("Folding new columns in"; scripts/fold_in_cols_rate.py writes
# profiles/r23_fold_in_cols_rate.jsonl)
Z_SAMPLES = 4096
Z_SEEDS = (7, 8)                  # numpy's generator: the reference set and the one it is checked against
# Binomial bias allowance: the largest |mean ilogit(W v) - oracle| at the default sweeps with S = 16384, doubled
# (scripts/fold_in_cols_rate.py --step binomial).
BINOMIAL_BIAS = 2 * 0.00711       # sweeps = 512: largest |diff| = 0.00711 at S = 16384 (oracle: 6000 sweeps, batch-means se <= 0.00073)
# Margin of test 7: the largest ratio fold-in RMSE / in-chain RMSE over 5 data seeds plus 20 % of it
# (scripts/fold_in_cols_rate.py --step margin).
FOLD_MARGIN = 1.2 * 2.025        # ratios seen: 0.288, 0.870, 0.934, 0.776, 2.025


# ---------------------------------------------------------------------------------------------------------------- helpers
def replay_problem(K, tf_order, T, seed, S=3, N=70, nreps=2):
    """W (S,N,K) ~ N(0,1), nu2 = 0.5, lam2 = 0.1, and six new columns on N = 70 rows (more than one pass of 64 lanes):
    complete, 30 % missing, 90 % missing, empty, a single observed cell, partial replicates."""
    rs = np.random.RandomState(seed)
    Ws = rs.normal(size=(S, N, K))
    nu2, lam2 = np.full(S, 0.5), np.full(S, 0.1)
    vt = 0.3 * np.cumsum(rs.normal(size=(6, T, K)), axis=1)
    Y = np.einsum("nk,ctk->cnt", Ws[0], vt)[..., None] + rs.normal(0, 0.7, size=(6, N, T, nreps))
    Y[1][rs.uniform(size=(N, T)) < 0.30] = np.nan
    Y[2][rs.uniform(size=(N, T)) < 0.90] = np.nan
    Y[3] = np.nan
    one = Y[4, 5, T // 2, 0]
    Y[4] = np.nan
    Y[4, 5, T // 2, 0] = one
    Y[5, :, :, 0][rs.uniform(size=(N, T)) < 0.5] = np.nan
    return Ws, nu2, lam2, Y


def numpy_chains(Y, Ws, nu2, lam2, tf_order, sweeps, draws):
    """`chain` for every (sample, column); returns V, V_mean, Tau2 and the largest cond(Q) over all systems."""
    S, C, K, T = Ws.shape[0], Y.shape[0], Ws.shape[2], Y.shape[2]
    nD = fc.penalty(T, tf_order).shape[0]
    V, Vm, T2 = np.zeros((S, C, T, K)), np.zeros((S, C, T, K)), np.zeros((S, C, nD))
    conds = []
    for s in range(S):
        for c in range(C):
            V[s, c], Vm[s, c], T2[s, c] = fc.chain(Y[c], Ws[s], nu2[s], lam2[s], tf_order, sweeps, draws[s, c],
                                                   on_system=lambda Q: conds.append(np.linalg.cond(Q)))
    return V, Vm, T2, max(conds)


def replay_seed(K, tf_order, T, sweeps):
    """The seed of a replay case: the first of a fixed sequence for which numpy alone keeps cond(Q) under COND_MAX."""
    base = 1000 * K + 100 * tf_order + 10 * T + sweeps
    for k in range(50):
        Ws, nu2, lam2, Y = replay_problem(K, tf_order, T, base + 7919 * k)
        draws = fc.random_draws(np.random.RandomState(base + 7919 * k + 1), T, K, tf_order, sweeps, size=(Ws.shape[0], Y.shape[0]))
        out = numpy_chains(Y, Ws, nu2, lam2, tf_order, sweeps, draws)
        if out[3] < COND_MAX:
            return (Ws, nu2, lam2, Y, draws) + out
    raise AssertionError("no seed with cond(Q) < %g" % COND_MAX)


def close(a, b, tol=V_TOL):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= tol


def z_problem(seed=41):
    """One kept state and one well-observed column: N = 12, T = 6, K = 2."""
    rs = np.random.RandomState(seed)
    N, T, K = 12, 6, 2
    W = rs.normal(size=(N, K))
    v = 0.4 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = W.dot(v.T) + rs.normal(0, 0.5, size=(N, T))
    Y[rs.uniform(size=(N, T)) < 0.1] = np.nan
    return W, Y, 0.25, 0.1


def two_sample_z(a, b):
    """Largest two-sample z of the per-coordinate means of a and b (replicates along axis 0)."""
    se = np.sqrt(a.var(axis=0, ddof=1) / a.shape[0] + b.var(axis=0, ddof=1) / b.shape[0])
    return float(np.max(np.abs(a.mean(axis=0) - b.mean(axis=0)) / se))


def numpy_replicates(W, Y, nu2, lam2, S, seed, sweeps=None):
    """S replicates of `chain` under numpy's generator, the draws of replicate after replicate from default_rng(seed)."""
    sweeps = fc.DEFAULT_SWEEPS if sweeps is None else sweeps
    T, K = Y.shape[1], W.shape[1]
    rng = np.random.default_rng(seed)
    return np.array([fc.chain(Y, W, nu2, lam2, 2, sweeps, fc.random_draws(rng, T, K, 2, sweeps))[0] for _ in range(S)])


def numpy_reference():
    """Per-coordinate mean and variance of V over Z_SAMPLES replicates of `chain` at the default sweeps under numpy's
    generator, computed once (scripts/fold_in_cols_rate.py --step golden; about a minute of numpy) and kept in
    tests/golden/fold_in_cols_numpy_replicates.npz; tests/test_host_fold_in_cols.py recomputes its first replicates."""
    g = load_golden("fold_in_cols_numpy_replicates.npz")
    assert int(g["sweeps"]) == fc.DEFAULT_SWEEPS and int(g["nsamples"]) == Z_SAMPLES
    return g


def device_generator_z(S=Z_SAMPLES):
    """(largest |z| device against numpy, largest |z| numpy against numpy with another seed) of the per-coordinate means
    of V."""
    W, Y, nu2, lam2 = z_problem()
    g = numpy_reference()
    out = utils.fold_in_cols(Y[None], np.repeat(W[None], S, axis=0), "gaussian", nu2=np.full(S, nu2), lam2=np.full(S, lam2),
                             seed=12345, summary=False)
    v = out["V"][:, 0]
    se = np.sqrt(v.var(axis=0, ddof=1) / S + g["var"] / S)
    return float(np.max(np.abs(v.mean(axis=0) - g["mean"]) / se)), float(g["z_numpy_vs_numpy"])


def binomial_problem(seed=5):
    rs = np.random.RandomState(seed)
    N, T, K = 30, 8, 2
    W = rs.normal(size=(N, K))
    v = 0.6 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Ntr = rs.randint(1, 9, size=(N, T)).astype(float)
    Y = rs.binomial(Ntr.astype(int), utils.ilogit(W.dot(v.T))).astype(float)
    Y[rs.uniform(size=(N, T)) < 0.2] = np.nan
    return W, Y, Ntr, 0.1


_ORACLE = {}


def binomial_oracle(nburn=500, nsamples=6000, batches=20):
    """Mean of ilogit(W v) over a long run of the one-column Binomial model's own chain with W_true, lam2_true and the same
    data (W and lam2 fixed, Tau2 and V sampled), and its Monte-Carlo standard error by batch means.  Computed once."""
    if "m" not in _ORACLE:
        W, Y, Ntr, lam2 = binomial_problem()
        N, T = Y.shape
        np.random.seed(1)
        model = BinomialBayesianTensorFiltering(N, 1, T, nembeds=W.shape[1], W_true=W, lam2_true=lam2, sigma2_true=1.0, rng="device",
                                                device_seed=9)
        res = model.run_gibbs((Y[:, None, :], Ntr[:, None, :]), nburn=nburn, nsamples=nsamples, verbose=False)
        p = utils.ilogit(np.einsum("nk,stk->snt", W, res["V"][:, 0]))
        bm = p.reshape(batches, nsamples // batches, N, T).mean(axis=1)
        _ORACLE["m"], _ORACLE["se"] = p.mean(axis=0), bm.std(axis=0, ddof=1) / np.sqrt(batches)
    return _ORACLE["m"], _ORACLE["se"]


def binomial_bias(S, sweeps=None):
    """(largest |fold-in mean - oracle mean| of ilogit(W v), the oracle's largest standard error)."""
    W, Y, Ntr, lam2 = binomial_problem()
    m, se = binomial_oracle()
    out = utils.fold_in_cols((Y[None], Ntr[None]), np.repeat(W[None], S, axis=0), "binomial", lam2=np.full(S, lam2), seed=31,
                             sweeps=sweeps, transform="ilogit", q=None)
    return float(np.abs(out["mean"][:, 0] - m).max()), float(se.max())


def simulate(seed, N=200, M=12, T=30, K=3):
    rs = np.random.RandomState(seed)
    Wt = rs.normal(size=(N, K))
    Vt = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    truth = np.einsum("nk,mtk->nmt", Wt, Vt)
    Y = truth + rs.normal(0, 0.5, size=truth.shape)
    return Y, truth


def fold_vs_chain(seed, nburn=300, nsamples=200):
    """(fold-in RMSE, in-chain RMSE, predict-zero RMSE) on the unobserved 70 % of the rows of the last column."""
    Y, truth = simulate(seed)
    N, M, T = Y.shape
    obs_rows = np.random.RandomState(seed + 100).permutation(N)[:(3 * N) // 10]
    hid = np.setdiff1d(np.arange(N), obs_rows)
    Y_new = np.full((1, N, T), np.nan)
    Y_new[0, obs_rows] = Y[obs_rows, M - 1]
    np.random.seed(seed)
    fit = GaussianBayesianTensorFiltering(N, M - 1, T, nembeds=3, rng="device", device_seed=seed + 1)
    fit.run_gibbs(np.ascontiguousarray(Y[:, :M - 1]), nburn=nburn, nsamples=nsamples, verbose=False)
    out = fit.fold_in_cols(Y_new, seed=17)
    Y_all = Y.copy()
    Y_all[:, M - 1] = Y_new[0]
    np.random.seed(seed)
    full = GaussianBayesianTensorFiltering(N, M, T, nembeds=3, rng="device", device_seed=seed + 1)
    full.run_gibbs(Y_all, nburn=nburn, nsamples=nsamples, verbose=False)
    mean_chain = full.posterior_summary()[0][:, M - 1]
    t = truth[hid, M - 1]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    return rmse(out["mean"][hid, 0]), rmse(mean_chain[hid]), rmse(np.zeros_like(t))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("T", [3, 9, 16])
@pytest.mark.parametrize("tf_order", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 3, 5, 8, 10])
def test_replay_equals_numpy_chain(K, tf_order, T, sweeps):
    """1. With supplied draws V, V_mean and Tau2 equal `chain`: six columns (complete, 30 % and 90 % missing, empty, a single
    cell, partial replicates), S = 3, N = 70."""
    Ws, nu2, lam2, Y, draws, V, Vm, T2, cond = replay_seed(K, tf_order, T, sweeps)
    out = utils.fold_in_cols(Y, Ws, "gaussian", nu2=nu2, lam2=lam2, tf_order=tf_order, draws=draws, sweeps=sweeps, summary=False)
    print("K=%d tf=%d T=%d sweeps=%d  max cond(Q) %.2e  max|V| %.2f  err V %.2e  V_mean %.2e  Tau2 (rel) %.2e"
          % (K, tf_order, T, sweeps, cond, np.abs(V).max(), np.abs(out["V"] - V).max(), np.abs(out["V_mean"] - Vm).max(),
             np.max(np.abs(out["Tau2"] - T2) / T2)))
    assert cond < COND_MAX
    assert close(out["V_mean"], Vm)
    assert close(out["V"], V)
    assert float(np.max(np.abs(out["Tau2"] - T2) / T2)) <= V_TOL
    assert np.all(out["V_mean"][:, 3] == 0.0)                         # the empty column: the prior's mean


def test_tied_to_the_reference_pinned_v_step():
    """2. Column j of _resample_V with zero normals is the conditional mean whatever the elimination order; fold_in_cols of
    that column with the model's Tau2[j] in the start block of draws (g0[0..2] = 1, g0[3] = 1 / (c tau2)) returns it."""
    rs = np.random.RandomState(2)
    N, M, T, K = 14, 5, 9, 3
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(N, K)), 0.4 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)) \
        + rs.normal(0, 0.5, size=(N, M, T))
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    np.random.seed(3)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_init=0.8, lam2_init=0.1, nu2_init=0.6,
                                        W_init=rs.normal(size=(N, K)), rng="host", sampler="banded", compat="exact")
    kept = {"W": m.W.copy()[None], "nu2": np.array([[float(m.nu2)]]), "lam2": np.array([[float(m.lam2)]])}
    Tau2 = m.Tau2.copy()
    m._v_normals = lambda: np.zeros((M, K * T))
    m._resample_V(Y)
    V_new = m.V.copy()
    assert np.abs(V_new).max() < 10
    nD = Tau2.shape[1]
    for j in (0, 2, M - 1):
        draws = np.ones((1, 1, fc.draws_length(T, K, 2, 1)))
        draws[0, 0, 3 * nD:4 * nD] = 1.0 / Tau2[j]                    # a = b = c = 1
        out = m.fold_in_cols(np.ascontiguousarray(Y[:, j])[None], results=kept, draws=draws, sweeps=1, summary=False)
        err = np.abs(out["V_mean"][0, 0] - V_new[j]).max()
        print("column %d  |fold-in mean - V step| %.3e" % (j, err))
        assert close(out["V_mean"][0, 0], V_new[j])


def test_same_bits():
    """3. Two calls with one seed; uploaded results against the device-collected samples; S split in two calls; C = 1 against
    the same column inside C = 3; and a chain continued after the call equal to one that never made it."""
    rs = np.random.RandomState(8)
    N, M, T, K = 30, 6, 12, 3
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)) \
        + rs.normal(0, 0.5, size=(N, M, T))
    Y_new = np.ascontiguousarray(Y[:, :3].transpose(1, 0, 2))
    Y_new[1, 10:] = np.nan
    Y_new[2] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=7))
    a, b = models
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        a.fold_in_cols(Y_new)
    for m in models:
        res = m.run_gibbs(Y, nburn=10, nsamples=20, verbose=False)
    keys = ("V", "V_mean", "Tau2", "mean", "quantiles")
    o1 = a.fold_in_cols(Y_new, seed=5)
    o2 = a.fold_in_cols(Y_new, seed=5)
    o3 = a.fold_in_cols(Y_new, results=res, seed=5)
    o4 = utils.fold_in_cols(Y_new, res["W"], "gaussian", nu2=res["nu2"], lam2=res["lam2"], seed=5)
    for o in (o2, o3, o4):
        for k in keys:
            assert np.array_equal(o1[k], o[k]), k
    assert np.all(np.isfinite(o1["V"])) and o1["mean"].shape == (N, 3, T) and o1["quantiles"].shape == (2, N, 3, T)
    assert not np.array_equal(o1["V"], a.fold_in_cols(Y_new, seed=6)["V"])
    kw = dict(seed=5, summary=False)
    lo = utils.fold_in_cols(Y_new, res["W"][:8], "gaussian", nu2=res["nu2"][:8], lam2=res["lam2"][:8], **kw)
    hi = utils.fold_in_cols(Y_new, res["W"][8:], "gaussian", nu2=res["nu2"][8:], lam2=res["lam2"][8:], first_sample=8, **kw)
    for k in keys[:3]:
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), o1[k]), k
    hi2 = a.fold_in_cols(Y_new, results={k: v[8:] for k, v in res.items()}, first_sample=8, **kw)
    assert np.array_equal(hi2["V"], o1["V"][8:])
    one = utils.fold_in_cols(Y_new[:1], res["W"], "gaussian", nu2=res["nu2"], lam2=res["lam2"], **kw)
    for k in keys[:3]:
        assert np.array_equal(one[k][:, 0], o1[k][:, 0]), k             # column 0 alone: the same chain
    for m in models:
        m.run_gibbs(Y, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_composition_with_summary_predictive_and_functionals():
    """4. results["W"] with out["V"] goes straight into the other posterior tools; the summary is the summary kernel's."""
    Ws, _, _, Y = replay_problem(3, 2, 9, seed=21, S=40)
    nu2, lam2 = np.full(40, 0.5), np.full(40, 0.1)
    q = (5, 50, 95)
    out = utils.fold_in_cols(Y, Ws, "gaussian", nu2=nu2, lam2=lam2, seed=9, q=q)
    mean, quant = utils.posterior_summary(Ws, out["V"], q=q)
    assert np.array_equal(mean, out["mean"]) and np.array_equal(quant, out["quantiles"])
    sq = utils.fold_in_cols(Y, Ws, "gaussian", nu2=nu2, lam2=lam2, seed=9, q=q, transform="square")
    assert np.array_equal(utils.posterior_summary(Ws, out["V"], q=q, transform="square")[0], sq["mean"])
    data = np.ascontiguousarray(Y.transpose(1, 0, 2, 3))
    pp = utils.posterior_predictive(Ws, out["V"], "gaussian", data=data, nu2=nu2, seed=1)
    assert pp["mean"].shape == data.shape[:3] and np.all(np.isfinite(pp["mean"]))
    np.testing.assert_allclose(pp["mean"], out["mean"], rtol=0, atol=1e-12)
    pf = utils.posterior_functionals(Ws, out["V"], which=("auc", "max"))
    assert pf["auc"]["mean"].shape == (Ws.shape[1], Y.shape[0]) and np.all(np.isfinite(pf["auc"]["mean"]))
    assert out["nsamples"] == 40


def test_device_generator_against_numpy():
    """5. S = 4096 copies of one state, a well-observed column, the default sweeps: the per-coordinate mean of V against
    4096 replicates of `chain` under numpy's generator (stored moments: numpy_reference), two-sample z, seeds fixed.  Largest
    |z| seen: 1.01 (device against numpy; numpy against numpy with another seed: 1.09); bound 5."""
    z, zref = device_generator_z()
    print("largest two-sample |z|: device against numpy %.2f, numpy against numpy %.2f (limit 5)" % (z, zref))
    assert zref <= 5
    assert z <= 5


def test_binomial_against_the_one_column_model():
    """6. Mean of ilogit(W v): the fold-in at the default sweeps over S = 4096 copies of (W_true, lam2_true) against a long
    run of the one-column Binomial model's own chain with the same W, lam2 and data.  Allowance: the measured bias
    BINOMIAL_BIAS plus 5 standard errors of the difference (fold-in: binomial variance of a mean of S values in [0, 1] is
    at most 1 / (4 S); oracle: batch means)."""
    S = 4096
    W, Y, Ntr, lam2 = binomial_problem()
    m, se = binomial_oracle()
    Ws, l2 = np.repeat(W[None], S, axis=0), np.full(S, lam2)
    out = utils.fold_in_cols((Y[None], Ntr[None]), Ws, "binomial", lam2=l2, seed=31, transform="ilogit", q=None)
    assert "V_mean" not in out and np.all(np.isfinite(out["V"]))
    p = utils.ilogit(np.einsum("nk,stk->snt", W, out["V"][:, 0]))
    np.testing.assert_allclose(p.mean(axis=0), out["mean"][:, 0], rtol=0, atol=1e-12)
    d = np.abs(p.mean(axis=0) - m)
    allow = BINOMIAL_BIAS + 5 * np.sqrt(p.var(axis=0, ddof=1) / S + se ** 2)
    print("binomial: largest |fold-in - oracle| %.5f (allowance there %.5f; bias allowance %.5f, oracle se <= %.5f)"
          % (d.max(), allow.reshape(-1)[np.argmax(d)], BINOMIAL_BIAS, se.max()))
    assert np.all(d <= allow)
    again = utils.fold_in_cols((Y[None], Ntr[None]), Ws[100:200], "binomial", lam2=l2[100:200], seed=31, summary=False, first_sample=100)
    assert np.array_equal(again["V"], out["V"][100:200])
    with pytest.raises(ValueError, match="Gaussian model only"):
        utils.fold_in_cols((Y[None], Ntr[None]), Ws[:2], "binomial", lam2=l2[:2], draws=np.ones((2, 1, 5)))


def test_it_does_the_job():
    """7. (200,12,30) Gaussian data from a K = 3 model; the chain runs on 11 columns (device-collected), the twelfth is folded
    in from 30 % of its rows.  RMSE of `mean` on the other rows against the noiseless truth: below FOLD_MARGIN times that of
    the chain that had the column in the tensor with the same cells observed, and below predicting 0."""
    fold, chain, zero = fold_vs_chain(0)
    print("RMSE on the unobserved rows: fold-in %.4f, in-chain %.4f (ratio %.3f, margin %.3f), predicting zero %.4f"
          % (fold, chain, fold / chain, FOLD_MARGIN, zero))
    assert fold < zero
    assert fold <= FOLD_MARGIN * chain


def test_failures():
    """8. A band beyond the LDS limit is refused before any device call; so are the models without a conjugate column
    conditional."""
    with pytest.raises(ValueError, match="LDS"):
        utils.fold_in_cols(np.zeros((1, 5, 370)), np.zeros((2, 5, 10)), "gaussian", nu2=np.ones(2), lam2=np.ones(2))
    Y = np.zeros((1, 6, 5))
    res = {"W": np.ones((4, 6, 2)), "nu2": np.ones((4, 1)), "lam2": np.ones((4, 1))}
    np.random.seed(0)
    nb = NegativeBinomialBayesianTensorFiltering(6, 3, 5, nembeds=2)
    with pytest.raises(NotImplementedError, match="Negative-Binomial"):
        nb.fold_in_cols(Y, results=res)
    sl = NonconjugateBayesianTensorFiltering(6, 3, 5, loglikelihood="poisson_log", nembeds=2)
    with pytest.raises(NotImplementedError, match="slice-sampled"):
        sl.fold_in_cols(Y, results=res)
