"""fold_in_depth on the GPU (csrc/btf_fold_in_depth.h): the curves of the fitted columns at depths the chain never saw.

Yardsticks: the numpy definition functionalmf_amd.fold_in_depth.chain on the same variates, draw for draw (the project's V
tolerance, 1e-6 * max(1, |V|), with the numpy side asserting cond(Q) < 1e9 for every system of the case), numpy's generator
(two-sample Kolmogorov-Smirnov on the exact data-free draw; two-sample z with data), a long numpy chain of the Binomial
definition, and the forecast on the same kept samples.
"""
import types

import numpy as np
import pytest
from conftest import load_golden

from functionalmf_amd import fold_in_depth as fd, utils
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering,
                                     NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering)

pytestmark = pytest.mark.gpu

V_TOL = 1e-6
COND_MAX = 1e9
REPLAY_SHAPES = ((2, 1), (3, 1), (4, 3), (9, 8))          # (T, H): H = 1, H <= tf_order + 1, T < tf_order + 1, the flu horizon

# ---- measured constants ("Folding new depth slices in"; scripts/fold_in_depth_rate.py writes
# profiles/r26_fold_in_depth_rate.jsonl)
Z_SAMPLES = 4096
Z_SEEDS = (7, 8)                  # numpy's generator: the reference set and the one it is checked against
KS_LIMIT = 2.225 * np.sqrt(2.0 / Z_SAMPLES)       # 0.0492: alpha = 1e-4 per coordinate, two samples of 4096
# Binomial bias allowance: the largest |mean ilogit(W v) - oracle| at the default sweeps with S = 16384, doubled
# (scripts/fold_in_depth_rate.py --step binomial).
BINOMIAL_BIAS = 2 * 0.01597       # sweeps = 128: largest |diff| = 0.01597 at S = 16384 (oracle: 64 runs of `chain`, 2048 sweeps each, se <= 0.00848)


# ---------------------------------------------------------------------------------------------------------------- helpers
def replay_problem(K, tf_order, T, H, seed, S=3, N=70, M=5, nreps=2):
    """Ws (S,N,K) ~ N(0,1), Vs (S,M,T,K) random walks, nu2 = 0.5, lam2 = 0.1, and new slices of five columns on N = 70 rows
    (more than one pass of 64 lanes): complete, 30 % missing, 90 % missing, empty, a single observed cell."""
    rs = np.random.RandomState(seed)
    Ws = rs.normal(size=(S, N, K))
    walk = 0.3 * np.cumsum(rs.normal(size=(S, M, T + H, K)), axis=2)
    Vs = np.ascontiguousarray(walk[:, :, :T])
    nu2, lam2 = np.full(S, 0.5), np.full(S, 0.1)
    Y = np.einsum("nk,mtk->nmt", Ws[0], walk[0, :, T:])[..., None] + rs.normal(0, 0.7, size=(N, M, H, nreps))
    Y[:, 1][rs.uniform(size=(N, H)) < 0.30] = np.nan
    Y[:, 2][rs.uniform(size=(N, H)) < 0.90] = np.nan
    Y[:, 3] = np.nan
    one = Y[5, 4, H // 2, 0]
    Y[:, 4] = np.nan
    Y[5, 4, H // 2, 0] = one
    return Ws, Vs, nu2, lam2, Y


def numpy_chains(Y, Ws, Vs, nu2, lam2, tf_order, sweeps, draws):
    """`chain` for every (sample, column); returns V, V_mean, Tau2 and the largest cond(Q) over all systems."""
    S, M, T, K = Vs.shape
    H = Y.shape[2]
    nR = fd.new_rows(T, H, tf_order)[0].size
    V, Vm, T2 = np.zeros((S, M, H, K)), np.zeros((S, M, H, K)), np.zeros((S, M, nR))
    conds = []
    for s in range(S):
        for j in range(M):
            V[s, j], Vm[s, j], T2[s, j] = fd.chain(Y[:, j], Ws[s], Vs[s, j], nu2[s], lam2[s], tf_order, sweeps, draws[s, j],
                                                   on_system=lambda Q: conds.append(np.linalg.cond(Q)))
    return V, Vm, T2, max(conds)


def replay_seed(K, tf_order, T, H, sweeps):
    """The seed of a replay case: the first of a fixed sequence for which numpy alone keeps cond(Q) under COND_MAX."""
    base = 10000 * K + 1000 * tf_order + 100 * T + 10 * H + sweeps
    for k in range(50):
        Ws, Vs, nu2, lam2, Y = replay_problem(K, tf_order, T, H, base + 7919 * k)
        draws = fd.random_draws(np.random.RandomState(base + 7919 * k + 1), T, H, K, tf_order, sweeps, size=Vs.shape[:2])
        out = numpy_chains(Y, Ws, Vs, nu2, lam2, tf_order, sweeps, draws)
        if out[3] < COND_MAX:
            return (Ws, Vs, nu2, lam2, Y, draws, k) + out
    raise AssertionError("no seed with cond(Q) < %g" % COND_MAX)


def close(a, b, tol=V_TOL):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= tol


def ks_two_sample(a, b):
    """Largest two-sample Kolmogorov-Smirnov statistic over the coordinates of a and b (replicates along axis 0)."""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    worst = 0.0
    for c in range(a.shape[1]):
        x, y = np.sort(a[:, c]), np.sort(b[:, c])
        grid = np.concatenate([x, y])
        d = np.abs(np.searchsorted(x, grid, side="right") / x.size - np.searchsorted(y, grid, side="right") / y.size).max()
        worst = max(worst, float(d))
    return worst


def forecast_problem(seed=43):
    """One kept state for the data-free draw: N = 5, T = 6, H = 4, K = 2, tf_order 2."""
    rs = np.random.RandomState(seed)
    return rs.normal(size=(5, 2)), 0.4 * np.cumsum(rs.normal(size=(6, 2)), axis=0), 4, 0.25, 0.1


def forecast_replicates(S, seed):
    """S exact data-free draws (sweeps=1) of `chain` under numpy's generator."""
    W, V_old, H, nu2, lam2 = forecast_problem()
    rng = np.random.default_rng(seed)
    Y = np.full((W.shape[0], H), np.nan)
    return np.array([fd.chain(Y, W, V_old, nu2, lam2, 2, 1, fd.random_draws(rng, V_old.shape[0], H, W.shape[1], 2, 1))[0]
                     for _ in range(S)])


def z_problem(seed=41):
    """One kept state and well-observed new slices of one column: N = 12, T = 6, H = 4, K = 2."""
    rs = np.random.RandomState(seed)
    N, T, H, K = 12, 6, 4, 2
    W = rs.normal(size=(N, K))
    v = 0.4 * np.cumsum(rs.normal(size=(T + H, K)), axis=0)
    Y = W.dot(v[T:].T) + rs.normal(0, 0.5, size=(N, H))
    Y[rs.uniform(size=(N, H)) < 0.1] = np.nan
    return W, v[:T], Y, 0.25, 0.1


def two_sample_z(a, b):
    """Largest two-sample z of the per-coordinate means of a and b (replicates along axis 0)."""
    se = np.sqrt(a.var(axis=0, ddof=1) / a.shape[0] + b.var(axis=0, ddof=1) / b.shape[0])
    return float(np.max(np.abs(a.mean(axis=0) - b.mean(axis=0)) / se))


def numpy_replicates(W, V_old, Y, nu2, lam2, S, seed, sweeps=None):
    """S replicates of `chain` under numpy's generator, the draws of replicate after replicate from default_rng(seed)."""
    sweeps = fd.DEFAULT_SWEEPS if sweeps is None else sweeps
    T, H, K = V_old.shape[0], Y.shape[1], W.shape[1]
    rng = np.random.default_rng(seed)
    return np.array([fd.chain(Y, W, V_old, nu2, lam2, 2, sweeps, fd.random_draws(rng, T, H, K, 2, sweeps))[0] for _ in range(S)])


def numpy_reference():
    """The stored numpy side of tests 3 and 4 (scripts/fold_in_depth_rate.py --step golden; under a minute of numpy):
    the 4096 exact data-free replicates themselves, and the per-coordinate mean and variance of V over 4096 replicates of
    `chain` at the default sweeps on z_problem; tests/test_host_fold_in_depth.py recomputes their first replicates."""
    g = load_golden("fold_in_depth_numpy_replicates.npz")
    assert int(g["sweeps"]) == fd.DEFAULT_SWEEPS and int(g["nsamples"]) == Z_SAMPLES
    return g


def device_forecast(S=Z_SAMPLES):
    W, V_old, H, nu2, lam2 = forecast_problem()
    out = utils.fold_in_depth(None, np.repeat(W[None], S, axis=0), np.repeat(V_old[None, None], S, axis=0), "gaussian", horizon=H,
                              nu2=np.full(S, nu2), lam2=np.full(S, lam2), seed=2468, sweeps=1, summary=False)
    return out["V"][:, 0]


def device_generator_z(S=Z_SAMPLES):
    """(largest |z| device against numpy, largest |z| numpy against numpy with another seed) of the per-coordinate means
    of V."""
    W, V_old, Y, nu2, lam2 = z_problem()
    g = numpy_reference()
    out = utils.fold_in_depth(Y[:, None], np.repeat(W[None], S, axis=0), np.repeat(V_old[None, None], S, axis=0), "gaussian",
                              nu2=np.full(S, nu2), lam2=np.full(S, lam2), seed=12345, summary=False)
    v = out["V"][:, 0]
    se = np.sqrt(v.var(axis=0, ddof=1) / S + g["var"] / S)
    return float(np.max(np.abs(v.mean(axis=0) - g["mean"]) / se)), float(g["z_numpy_vs_numpy"])


def binomial_problem(seed=5):
    rs = np.random.RandomState(seed)
    N, T, H, K = 30, 8, 4, 2
    W = rs.normal(size=(N, K))
    v = 0.6 * np.cumsum(rs.normal(size=(T + H, K)), axis=0)
    Ntr = rs.randint(1, 9, size=(N, H)).astype(float)
    Y = rs.binomial(Ntr.astype(int), utils.ilogit(W.dot(v[T:].T))).astype(float)
    Y[rs.uniform(size=(N, H)) < 0.2] = np.nan
    return W, v[:T], Y, Ntr, 0.1


def binomial_oracle_chain(nchains=64, nburn=1024, nsamples=1024, seed=1):
    """Mean of ilogit(W v) over long runs of `chain` (the definition) on binomial_problem - 16 times the default sweeps, the
    second half kept - and its Monte-Carlo standard error from the spread BETWEEN the independent runs.  One run is not
    enough: a single run of 42000 sweeps sat 0.23 away from the replicates of 128 and of 1024 sweeps alike (the horseshoe+
    levels keep a chain near a collapsed state for tens of thousands of sweeps), with a batch-means error of 0.0003 that
    knew nothing of it.  scripts/fold_in_depth_rate.py --step golden stores the result (two minutes of numpy)."""
    W, V_old, Y, Ntr, lam2 = binomial_problem()
    T, H, K = V_old.shape[0], Y.shape[1], W.shape[1]
    total = nburn + nsamples
    rng = np.random.default_rng(seed)
    means = np.zeros((nchains,) + Y.shape)
    for c in range(nchains):
        def on_sweep(r, v, c=c):
            if r >= nburn:
                means[c] += utils.ilogit(W.dot(v.T)) / nsamples
        fd.chain((Y, Ntr), W, V_old, None, lam2, 2, total, fd.random_draws(rng, T, H, K, 2, total), family="binomial",
                 on_sweep=on_sweep, seed=seed + 1 + c)
    return means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(nchains)


def binomial_oracle():
    g = load_golden("fold_in_depth_binomial_oracle.npz")
    return g["mean"], g["se"]


def binomial_fold(S, sweeps=None, **kw):
    W, V_old, Y, Ntr, lam2 = binomial_problem()
    return utils.fold_in_depth((Y[:, None], Ntr[:, None]), np.repeat(W[None], S, axis=0), np.repeat(V_old[None, None], S, axis=0),
                               "binomial", lam2=np.full(S, lam2), seed=31, sweeps=sweeps, transform="ilogit", q=None, **kw)


def binomial_bias(S, sweeps=None):
    """(largest |fold-in mean - oracle mean| of ilogit(W v), the oracle's largest standard error)."""
    m, se = binomial_oracle()
    return float(np.abs(binomial_fold(S, sweeps)["mean"][:, 0] - m).max()), float(se.max())


def job_problem(seed, S=48, N=24, M=4, T=12, H=4, K=2, noise=0.5, kept_sd=0.05):
    """The recipe of the issue: smooth curves on T + H depths, the kept samples equal to the truth plus N(0, 0.05^2), new
    slices observed at half the rows with noise sd 0.5.  Returns Ws, Vs, nu2, lam2, Y_new, the noiseless truth (N,M,H) and
    the hidden rows."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = 0.1 * np.cumsum(np.cumsum(rs.normal(size=(M, T + H, K)), axis=1), axis=1)      # smooth: an integrated random walk
    truth = np.einsum("nk,mtk->nmt", W, V[:, T:])
    Y = truth + rs.normal(0, noise, size=truth.shape)
    hid = np.sort(rs.permutation(N)[:N // 2])
    Y[hid] = np.nan
    Ws = W[None] + rs.normal(0, kept_sd, size=(S, N, K))
    Vs = V[None, :, :T] + rs.normal(0, kept_sd, size=(S, M, T, K))
    return Ws, Vs, np.full(S, noise ** 2), np.full(S, 0.1), Y, truth, hid


def job_rmse(mean_data, mean_forecast, truth, hid):
    rmse = lambda a: float(np.sqrt(np.mean((a[hid] - truth[hid]) ** 2)))
    return rmse(mean_data), rmse(mean_forecast)


def does_the_job(seed):
    """(RMSE with data, RMSE of the forecast) of `mean` at the hidden rows, on the device."""
    Ws, Vs, nu2, lam2, Y, truth, hid = job_problem(seed)
    with_data = utils.fold_in_depth(Y, Ws, Vs, "gaussian", nu2=nu2, lam2=lam2, seed=17, q=None)
    forecast = utils.fold_in_depth(None, Ws, Vs, "gaussian", horizon=Y.shape[2], nu2=nu2, lam2=lam2, seed=17, q=None)
    return job_rmse(with_data["mean"], forecast["mean"], truth, hid)


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("TH", REPLAY_SHAPES)
@pytest.mark.parametrize("tf_order", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 3, 5, 8, 10])
def test_replay_equals_numpy_chain(K, tf_order, TH, sweeps):
    """1. With supplied draws V, V_mean and Tau2 equal `chain`: five column slices (complete, 30 % and 90 % missing, empty, a
    single cell), S = 3, N = 70."""
    T, H = TH
    Ws, Vs, nu2, lam2, Y, draws, tries, V, Vm, T2, cond = replay_seed(K, tf_order, T, H, sweeps)
    out = utils.fold_in_depth(Y, Ws, Vs, "gaussian", nu2=nu2, lam2=lam2, tf_order=tf_order, draws=draws, sweeps=sweeps, summary=False)
    print("K=%d tf=%d T=%d H=%d sweeps=%d  seed retries %d  max cond(Q) %.2e  max|V| %.2f  err V %.2e  V_mean %.2e  Tau2 (rel) %.2e"
          % (K, tf_order, T, H, sweeps, tries, cond, np.abs(V).max(), np.abs(out["V"] - V).max(), np.abs(out["V_mean"] - Vm).max(),
             np.max(np.abs(out["Tau2"] - T2) / T2)))
    assert cond < COND_MAX
    assert out["V"].shape == (3, 5, H, K) and out["Tau2"].shape == T2.shape
    assert close(out["V_mean"], Vm)
    assert close(out["V"], V)
    assert float(np.max(np.abs(out["Tau2"] - T2) / T2)) <= V_TOL


def test_same_bits():
    """2. Two calls with one seed; uploaded results against the device-collected samples; S split by first_sample; the
    forecast likewise; and a chain continued after the call equal to one that never made it."""
    rs = np.random.RandomState(8)
    N, M, T, K, H = 30, 6, 12, 3, 3
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T + H, K)), axis=1)) \
        + rs.normal(0, 0.5, size=(N, M, T + H))
    Y_fit, Y_new = np.ascontiguousarray(Y[:, :, :T]), np.ascontiguousarray(Y[:, :, T:])
    Y_new[10:, 1] = np.nan
    Y_new[:, 2] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=7))
    a, b = models
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        a.fold_in_depth(Y_new)
    for m in models:
        res = m.run_gibbs(Y_fit, nburn=10, nsamples=20, verbose=False)
    keys = ("V", "V_mean", "Tau2", "mean", "quantiles")
    o1 = a.fold_in_depth(Y_new, seed=5)
    o2 = a.fold_in_depth(Y_new, seed=5)
    o3 = a.fold_in_depth(Y_new, results=res, seed=5)
    o4 = utils.fold_in_depth(Y_new, res["W"], res["V"], "gaussian", nu2=res["nu2"], lam2=res["lam2"], seed=5)
    for o in (o2, o3, o4):
        for k in keys:
            assert np.array_equal(o1[k], o[k]), k
    assert np.all(np.isfinite(o1["V"])) and o1["V"].shape == (20, M, H, K)
    assert o1["mean"].shape == (N, M, H) and o1["quantiles"].shape == (2, N, M, H)
    assert not np.array_equal(o1["V"], a.fold_in_depth(Y_new, seed=6)["V"])
    kw = dict(seed=5, summary=False)
    lo = utils.fold_in_depth(Y_new, res["W"][:8], res["V"][:8], "gaussian", nu2=res["nu2"][:8], lam2=res["lam2"][:8], **kw)
    hi = utils.fold_in_depth(Y_new, res["W"][8:], res["V"][8:], "gaussian", nu2=res["nu2"][8:], lam2=res["lam2"][8:], first_sample=8, **kw)
    for k in keys[:3]:
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), o1[k]), k
    hi2 = a.fold_in_depth(Y_new, results={k: v[8:] for k, v in res.items()}, first_sample=8, **kw)
    assert np.array_equal(hi2["V"], o1["V"][8:])
    f1 = a.fold_in_depth(None, horizon=H, seed=5)
    f2 = a.fold_in_depth(np.full((N, M, H), np.nan), results=res, seed=5)
    for k in keys:
        assert np.array_equal(f1[k], f2[k]), k
    assert np.array_equal(f1["V"][:, 2], o1["V"][:, 2])                # the empty column slice: the forecast's chain
    drawn = a._draws
    a.fold_in_depth(Y_new, seed=5)
    assert a._draws == drawn                                           # an integer seed leaves the model's counter alone
    a.fold_in_depth(Y_new)
    b._next_seed()                                                     # seed=None moved it on by one
    for m in models:
        m.run_gibbs(Y_fit, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_device_generator_data_free():
    """3. S = 4096 copies of one kept state, no data, sweeps=1 (exact): every coordinate of V against 4096 numpy replicates
    of `chain` (stored), two-sample Kolmogorov-Smirnov, limit 2.225 sqrt(2 / 4096) = 0.0492 (alpha = 1e-4 per coordinate).
    Means are not compared: the forecast is heavy-tailed."""
    g = numpy_reference()
    v = device_forecast()
    d = ks_two_sample(v, g["forecast"])
    print("largest two-sample KS statistic over %d coordinates: device against numpy %.4f, numpy against numpy %.4f (limit %.4f)"
          % (v[0].size, d, float(g["ks_numpy_vs_numpy"]), KS_LIMIT))
    assert float(g["ks_numpy_vs_numpy"]) <= KS_LIMIT
    assert d <= KS_LIMIT


def test_device_generator_with_data():
    """4. S = 4096 copies of one state, well-observed new slices, the default sweeps: the per-coordinate mean of V against
    4096 replicates of `chain` under numpy's generator (stored moments), two-sample z, seeds fixed; bound 5 as in the
    fold_in_cols test."""
    z, zref = device_generator_z()
    print("largest two-sample |z|: device against numpy %.2f, numpy against numpy %.2f (limit 5)" % (z, zref))
    assert zref <= 5
    assert z <= 5


def test_binomial_against_a_long_numpy_chain():
    """5. Mean of ilogit(W v): the fold-in at the default sweeps over S = 4096 copies of one kept state against one long run
    of the numpy definition (stored).  Allowance: the measured bias BINOMIAL_BIAS plus 5 standard errors of the difference
    (fold-in: sample variance over S; oracle: batch means)."""
    S = 4096
    W, V_old, Y, Ntr, lam2 = binomial_problem()
    m, se = binomial_oracle()
    out = binomial_fold(S)
    assert "V_mean" not in out and np.all(np.isfinite(out["V"]))
    p = utils.ilogit(np.einsum("nk,stk->snt", W, out["V"][:, 0]))
    np.testing.assert_allclose(p.mean(axis=0), out["mean"][:, 0], rtol=0, atol=1e-12)
    d = np.abs(p.mean(axis=0) - m)
    allow = BINOMIAL_BIAS + 5 * np.sqrt(p.var(axis=0, ddof=1) / S + se ** 2)
    print("binomial: largest |fold-in - oracle| %.5f (allowance there %.5f; bias allowance %.5f, oracle se <= %.5f)"
          % (d.max(), allow.reshape(-1)[np.argmax(d)], BINOMIAL_BIAS, se.max()))
    assert np.all(d <= allow)
    Ws, Vs, l2 = np.repeat(W[None], 100, axis=0), np.repeat(V_old[None, None], 100, axis=0), np.full(100, lam2)
    again = utils.fold_in_depth((Y[:, None], Ntr[:, None]), Ws, Vs, "binomial", lam2=l2, seed=31, summary=False, first_sample=100)
    assert np.array_equal(again["V"], out["V"][100:200])
    with pytest.raises(ValueError, match="Gaussian model only"):
        utils.fold_in_depth((Y[:, None], Ntr[:, None]), Ws[:2], Vs[:2], "binomial", lam2=l2[:2], draws=np.ones((2, 1, 5)))


def test_it_does_the_job():
    """6. N = 24, M = 4, T = 12, H = 4, K = 2, tf_order 2, S = 48 kept samples equal to the truth plus N(0, 0.05^2), the new
    slices observed at half the rows (noise sd 0.5): at the hidden rows the RMSE of `mean` with data is below half that of
    the forecast call.  Ratios of the numpy definition over data seeds 0..4 (scripts/fold_in_depth_rate.py --step job):
    0.089, 0.168, 0.098, 0.240, 0.208 (the issue's prototype: 0.12-0.28)."""
    data, forecast = does_the_job(0)
    print("RMSE at the hidden rows: with data %.4f, forecast %.4f (ratio %.3f, limit 0.5)" % (data, forecast, data / forecast))
    assert data < 0.5 * forecast


def test_a_failed_factorisation_names_the_smallest_chain():
    """A kept sample whose W is not finite has no positive pivot: BTF_ESTATE naming the smallest failing (first_sample + s) M +
    column; the other samples' chains are what they are without it."""
    from functionalmf_amd import _native
    Ws, Vs, nu2, lam2, Y = replay_problem(3, 2, 9, 4, seed=33)
    good = utils.fold_in_depth(Y, Ws, Vs, "gaussian", nu2=nu2, lam2=lam2, seed=3, summary=False)
    assert np.all(np.isfinite(good["V"]))
    bad = Ws.copy()
    bad[1, 7, 0] = np.nan
    with pytest.raises(_native.BTFError, match=r"index %d " % (1 * 5 + 0)) as e:
        utils.fold_in_depth(Y, bad, Vs, "gaussian", nu2=nu2, lam2=lam2, seed=3, summary=False)
    assert e.value.code == _native.BTF_ESTATE and _native.load().btf_fail_index(None) == 5
    with pytest.raises(_native.BTFError, match=r"index %d " % ((10 + 1) * 5 + 0)):
        utils.fold_in_depth(Y, bad, Vs, "gaussian", nu2=nu2, lam2=lam2, seed=3, summary=False, first_sample=10)


def test_composition_and_refusals():
    """7. The summary is the summary kernel's on (W, V_new); the concatenated posterior goes into the other posterior tools;
    the unsupported models, a sharded model and bad arguments raise."""
    Ws, Vs, nu2, lam2, Y = replay_problem(3, 2, 9, 4, seed=21, S=40)
    nu2, lam2 = np.full(40, 0.5), np.full(40, 0.1)
    q = (5, 50, 95)
    out = utils.fold_in_depth(Y, Ws, Vs, "gaussian", nu2=nu2, lam2=lam2, seed=9, q=q)
    mean, quant = utils.posterior_summary(Ws, out["V"], q=q)
    np.testing.assert_allclose(mean, out["mean"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(quant, out["quantiles"], rtol=0, atol=1e-12)
    V_all = np.concatenate([Vs, out["V"]], axis=2)
    assert V_all.shape == (40, 5, 13, 3)
    full = utils.posterior_summary(Ws, V_all, q=q)[0]
    np.testing.assert_allclose(full[:, :, 9:], out["mean"], rtol=0, atol=1e-12)
    pf = utils.posterior_functionals(Ws, V_all, which=("auc", "max"))
    assert pf["auc"]["mean"].shape == (Ws.shape[1], 5) and np.all(np.isfinite(pf["auc"]["mean"]))
    data = np.full((Ws.shape[1], 5, 13, 2), np.nan)
    data[:, :, 9:] = Y
    pp = utils.posterior_predictive(Ws, V_all, "gaussian", data=data, nu2=nu2, seed=1)
    np.testing.assert_allclose(pp["mean"][:, :, 9:], out["mean"], rtol=0, atol=1e-12)
    assert out["nsamples"] == 40
    # refusals
    kw = dict(nu2=nu2, lam2=lam2)
    with pytest.raises(ValueError, match="LDS"):
        utils.fold_in_depth(None, Ws, Vs, "gaussian", horizon=370, **kw)
    for bad in (dict(horizon=0), dict(horizon=None), dict(horizon=2.5)):
        with pytest.raises(ValueError):
            utils.fold_in_depth(None, Ws, Vs, "gaussian", **kw, **bad)
    with pytest.raises(ValueError):
        utils.fold_in_depth(Y[:, :4], Ws, Vs, "gaussian", **kw)
    with pytest.raises(ValueError):
        utils.fold_in_depth(Y, Ws, Vs, "gaussian", nu2=nu2[:3], lam2=lam2)
    with pytest.raises(ValueError):
        utils.fold_in_depth(Y, Ws, Vs, "gaussian", sweeps=0, **kw)
    Yn = np.zeros((6, 3, 2))
    res = {"W": np.ones((4, 6, 2)), "V": np.ones((4, 3, 5, 2)), "nu2": np.ones((4, 1)), "lam2": np.ones((4, 1))}
    np.random.seed(0)
    nb = NegativeBinomialBayesianTensorFiltering(6, 3, 5, nembeds=2)
    with pytest.raises(NotImplementedError, match="Negative-Binomial"):
        nb.fold_in_depth(Yn, results=res)
    sl = NonconjugateBayesianTensorFiltering(6, 3, 5, loglikelihood="poisson_log", nembeds=2)
    with pytest.raises(NotImplementedError, match="slice-sampled"):
        sl.fold_in_depth(Yn, results=res)
    cb = NonconjugateBayesianTensorFiltering(6, 3, 5, loglikelihood=lambda W, V, d: 0.0, nembeds=2)
    with pytest.raises(NotImplementedError, match="Python-callable"):
        cb.fold_in_depth(Yn, results=res)
    g = GaussianBayesianTensorFiltering(6, 3, 5, nembeds=2)
    g._plan = types.SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="unsharded"):
        g.fold_in_depth(Yn, results=res)
    bn = BinomialBayesianTensorFiltering(6, 3, 5, nembeds=2)
    with pytest.raises(ValueError):
        bn.fold_in_depth((Yn, np.full(Yn.shape, 33.0)), results=res)
