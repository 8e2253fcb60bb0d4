"""fold_in_rows on the GPU (csrc/btf_fold_in.h): the embedding of rows the chain never saw, per kept sample.

Yardsticks: the numpy definition functionalmf_amd.fold_in.conditional (Gaussian, 1e-10 absolute with |w| = O(1): the
project's tolerance for W against the reference, tests/test_gpu_parity.py), the project's own reference-pinned W step,
a 2-D quadrature of the logistic posterior (Binomial; no Polya-Gamma code involved), and the chain that includes the rows.
"""
import numpy as np
import pytest

from functionalmf_amd import fold_in, utils
from functionalmf_amd.factor import BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering

pytestmark = pytest.mark.gpu

W_TOL = 1e-10
COND_MAX = 1e4

# ---- measured constants ("Folding new rows in"; scripts/fold_in_rate.py writes profiles/r13_fold_in_rate.jsonl)
# Binomial bias allowance: the largest |mean - m| against the quadrature posterior at the default inner_sweeps with
# S = 65536, doubled (scripts/fold_in_rate.py --sweeps).
BINOMIAL_BIAS = 2 * 0.000263      # inner_sweeps = 4: |diff| = (0.000099, 0.000263) at S = 65536
# Margin of test 7: the largest ratio fold-in RMSE / in-chain RMSE over 5 data seeds plus 20 % of it
# (scripts/fold_in_rate.py --margin).
FOLD_MARGIN = 1.2 * 1.164        # ratios seen: 1.164, 0.999, 1.015, 0.966, 1.004


# ---------------------------------------------------------------------------------------------------------------- helpers
def gaussian_problem(K, S=3, M=4, T=9, nreps=2, seed=0):
    """Vs, nu2, sigma2 and six new rows: complete, 5 % missing, 90 % missing, empty, partial replicates, complete again.
    Scaled so that |w| is O(1) and cond(Q) stays small: V entries O(1), few hundred cells."""
    rs = np.random.RandomState(seed)
    Vs = rs.normal(size=(S, M, T, K))
    nu2 = rs.uniform(0.5, 1.5, size=S)
    sigma2 = rs.uniform(0.5, 2.0, size=S)
    wt = rs.normal(size=(6, K))
    Y = np.einsum("rk,mtk->rmt", wt, Vs[0])[..., None] + rs.normal(0, 0.7, size=(6, M, T, nreps))
    Y[1][rs.uniform(size=(M, T)) < 0.05] = np.nan
    Y[2][rs.uniform(size=(M, T)) < 0.90] = np.nan
    Y[3] = np.nan
    Y[4, :, :, 0][rs.uniform(size=(M, T)) < 0.5] = np.nan     # replicates with partial NaNs
    return Vs, nu2, sigma2, Y


def numpy_fold_in(Y, Vs, nu2, sigma2, z=None):
    S, R, K = Vs.shape[0], Y.shape[0], Vs.shape[-1]
    Wm, W, cond = np.zeros((S, R, K)), np.zeros((S, R, K)), np.zeros((S, R))
    for s in range(S):
        for r in range(R):
            m, Q = fold_in.conditional(Y[r], Vs[s], nu2[s], sigma2[s])
            Wm[s, r], cond[s, r] = m, np.linalg.cond(Q)
            W[s, r] = fold_in.draw(m, Q, z[s, r]) if z is not None else m
    return W, Wm, cond


def moments_check(W, m, C, bias=0.0):
    """The 5-standard-error inequalities: |mean_k - m_k| <= 5 sqrt(C_kk / S) (+ bias, an allowance on the mean alone) and the
    covariance entries within 5 sqrt((C_ab^2 + C_aa C_bb) / S) (Wishart).  Returns the largest ratios (mean, covariance)."""
    S = W.shape[0]
    d = np.abs(W.mean(axis=0) - m)
    se = np.sqrt(np.diag(C) / S)
    Chat = np.cov(W.T, ddof=1).reshape(C.shape)
    sec = np.sqrt((C ** 2 + np.outer(np.diag(C), np.diag(C))) / S)
    zm, zc = float(np.max((d - bias) / se)), float(np.max(np.abs(Chat - C) / sec))
    return zm, zc


def binomial_problem(seed=3):
    """K = 2, one (V, sigma2) state, one new row with about 40 observed cells of 1 to 8 trials (M = 4, T = 12, 48 cells)."""
    rs = np.random.RandomState(seed)
    M, T, K = 4, 12, 2
    V = 0.8 * rs.normal(size=(M, T, K))
    sigma2 = 1.5
    w_true = np.array([0.9, -0.6])
    N = rs.randint(1, 9, size=(1, M, T)).astype(float)
    p = 1 / (1 + np.exp(-np.einsum("k,mtk->mt", w_true, V)))
    Y = rs.binomial(N.astype(int), p[None]).astype(float)
    miss = rs.uniform(size=(1, M, T)) < 0.17
    Y[miss] = np.nan
    return V, sigma2, Y, N


def quadrature_posterior(V, sigma2, Y, N):
    """Mean and covariance of p(w | y) proportional to prod ilogit(w.v)^y (1 - ilogit(w.v))^(n-y) N(w; 0, sigma2 I) on a 2-D
    grid, refined (range and resolution) until both move by less than 1e-6."""
    obs = ~np.isnan(Y[0])
    v, y, n = V[obs], Y[0][obs], N[0][obs]

    def moments(half, npts):
        g = np.linspace(-half, half, npts)
        w0, w1 = np.meshgrid(g, g, indexing="ij")
        eta = w0[..., None] * v[:, 0] + w1[..., None] * v[:, 1]
        ll = (y * eta - n * np.logaddexp(0.0, eta)).sum(axis=-1) - (w0 ** 2 + w1 ** 2) / (2 * sigma2)
        p = np.exp(ll - ll.max())
        p /= p.sum()
        m = np.array([(p * w0).sum(), (p * w1).sum()])
        d0, d1 = w0 - m[0], w1 - m[1]
        C = np.array([[(p * d0 * d0).sum(), (p * d0 * d1).sum()], [(p * d0 * d1).sum(), (p * d1 * d1).sum()]])
        return m, C
    half, npts = 6.0, 201
    m, C = moments(half, npts)
    for _ in range(6):
        half, npts = half * 1.25, npts * 2 - 1
        m2, C2 = moments(half, npts)
        moved = max(np.abs(m2 - m).max(), np.abs(C2 - C).max())
        m, C = m2, C2
        if moved < 1e-6:
            return m, C
    raise AssertionError("quadrature did not converge: last move %g" % moved)


def simulate(seed, N=200, M=12, T=30, K=3):
    rs = np.random.RandomState(seed)
    Wt = rs.normal(size=(N, K))
    Vt = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    truth = np.einsum("nk,mtk->nmt", Wt, Vt)
    Y = truth + rs.normal(0, 0.5, size=truth.shape)
    return Y, truth


def fold_vs_chain(seed, nburn=300, nsamples=200):
    """(fold-in RMSE, in-chain RMSE, predict-zero RMSE) on the 8 unobserved columns of the last 10 rows."""
    Y, truth = simulate(seed)
    N, M, T = Y.shape
    new, obs_cols = slice(N - 10, N), np.arange(0, M, 3)            # columns 0, 3, 6, 9 observed
    hid = np.setdiff1d(np.arange(M), obs_cols)
    Y_new = Y[new].copy()
    Y_new[:, hid] = np.nan
    np.random.seed(seed)
    fit = GaussianBayesianTensorFiltering(N - 10, M, T, nembeds=3, rng="device", device_seed=seed + 1)
    fit.run_gibbs(Y[:N - 10], nburn=nburn, nsamples=nsamples, verbose=False)
    out = fit.fold_in_rows(Y_new, seed=17)
    Y_all = Y.copy()
    Y_all[new] = Y_new
    np.random.seed(seed)
    full = GaussianBayesianTensorFiltering(N, M, T, nembeds=3, rng="device", device_seed=seed + 1)
    full.run_gibbs(Y_all, nburn=nburn, nsamples=nsamples, verbose=False)
    mean_chain = full.posterior_summary()[0][new]
    t = truth[new][:, hid]
    rmse = lambda a: float(np.sqrt(np.mean((a - t) ** 2)))
    return rmse(out["mean"][:, hid]), rmse(mean_chain[:, hid]), rmse(np.zeros_like(t))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("K", [1, 3, 5, 8, 10])
def test_gaussian_supplied_z_equals_numpy(K):
    """1. W and W_mean against the numpy definition: complete rows, 5 % and 90 % missing, an empty row, partial replicates."""
    Vs, nu2, sigma2, Y = gaussian_problem(K, seed=K)
    z = np.random.RandomState(100 + K).normal(size=(Vs.shape[0], Y.shape[0], K))
    out = utils.fold_in_rows(Y, Vs, "gaussian", nu2=nu2, sigma2=sigma2, z=z, summary=False)
    W, Wm, cond = numpy_fold_in(Y, Vs, nu2, sigma2, z)
    print("K=%d  max|W - numpy| %.3e  max|W_mean - numpy| %.3e  max cond(Q) %.1f  max|w| %.2f"
          % (K, np.abs(out["W"] - W).max(), np.abs(out["W_mean"] - Wm).max(), cond.max(), np.abs(W).max()))
    assert cond.max() < COND_MAX
    assert np.abs(out["W_mean"] - Wm).max() < W_TOL
    assert np.abs(out["W"] - W).max() < W_TOL
    assert np.all(out["W_mean"][:, 3] == 0.0)                  # the empty row: the prior's mean ...
    np.testing.assert_allclose(out["W"][:, 3], z[:, 3] * np.sqrt(sigma2)[:, None], rtol=0, atol=W_TOL)     # ... and its draw


def test_gaussian_one_column_flu_shape():
    """1, ncols = 1: the flu shape in small, (R, 1, T) without replicates."""
    rs = np.random.RandomState(5)
    S, T, K = 4, 37, 3
    Vs = rs.normal(size=(S, 1, T, K))
    nu2, sigma2 = rs.uniform(0.5, 1.5, size=S), rs.uniform(0.5, 2.0, size=S)
    Y = rs.normal(size=(70, 1, T))                             # more than one block of 64 rows
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    z = rs.normal(size=(S, 70, K))
    out = utils.fold_in_rows(Y, Vs, "gaussian", nu2=nu2, sigma2=sigma2, z=z, summary=False)
    W, Wm, cond = numpy_fold_in(Y[..., None], Vs, nu2, sigma2, z)
    assert cond.max() < COND_MAX
    assert np.abs(out["W_mean"] - Wm).max() < W_TOL and np.abs(out["W"] - W).max() < W_TOL


def test_tied_to_the_reference_pinned_w_step():
    """2. fold_in_rows of row i of the fitted tensor, with the kept state and row i's normals, is row i of _resample_W."""
    rs = np.random.RandomState(2)
    N, M, T, K = 12, 5, 8, 3
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(N, K)), rs.normal(size=(M, T, K))) + rs.normal(0, 0.5, size=(N, M, T))
    np.random.seed(3)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_init=0.8, lam2_init=0.1, nu2_init=0.6,
                                        V_init=rs.normal(size=(M, T, K)), rng="host", compat="exact")
    kept = {"V": m.V.copy()[None], "nu2": np.array([[float(m.nu2)]]), "sigma2": np.array([[float(m.sigma2)]])}
    np.random.seed(4)
    m._resample_W(Y)
    np.random.seed(4)
    zs = m._w_normals()
    W_new = m.W.copy()
    assert np.abs(W_new).max() < 10
    for i in (K, K + 1, 7, N - 1):
        off = K * (K + 1) // 2 + (i - K) * K
        out = m.fold_in_rows(Y[i:i + 1], results=kept, z=zs[off:off + K].reshape(1, 1, K), summary=False)
        err = np.abs(out["W"][0, 0] - W_new[i]).max()
        print("row %d  |fold-in - W step| %.3e" % (i, err))
        assert err < W_TOL


def test_same_bits():
    """3. Two calls with one seed; uploaded results against the device-collected samples; S split in two calls; and a chain
    continued after the call equal to one that never made it."""
    rs = np.random.RandomState(8)
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(30, 3)), 0.3 * np.cumsum(rs.normal(size=(6, 12, 3)), axis=1)) \
        + rs.normal(0, 0.5, size=(30, 6, 12))
    Y_new = Y[:5].copy()
    Y_new[1, 2:] = np.nan
    Y_new[2] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=7))
    a, b = models
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        a.fold_in_rows(Y_new)
    for m in models:
        res = m.run_gibbs(Y, nburn=10, nsamples=20, verbose=False)
    o1 = a.fold_in_rows(Y_new, seed=5)
    o2 = a.fold_in_rows(Y_new, seed=5)
    o3 = a.fold_in_rows(Y_new, results=res, seed=5)
    o4 = utils.fold_in_rows(Y_new, res["V"], "gaussian", nu2=res["nu2"], sigma2=res["sigma2"], seed=5)
    for o in (o2, o3, o4):
        for k in ("W", "W_mean", "mean", "quantiles"):
            assert np.array_equal(o1[k], o[k]), k
    assert not np.array_equal(o1["W"], a.fold_in_rows(Y_new, seed=6)["W"])
    lo = utils.fold_in_rows(Y_new, res["V"][:8], "gaussian", nu2=res["nu2"][:8], sigma2=res["sigma2"][:8], seed=5, summary=False)
    hi = utils.fold_in_rows(Y_new, res["V"][8:], "gaussian", nu2=res["nu2"][8:], sigma2=res["sigma2"][8:], seed=5, summary=False,
                            first_sample=8)
    assert np.array_equal(np.concatenate([lo["W"], hi["W"]]), o1["W"])
    assert np.array_equal(np.concatenate([lo["W_mean"], hi["W_mean"]]), o1["W_mean"])
    one = utils.fold_in_rows(Y_new[1:2], res["V"], "gaussian", nu2=res["nu2"], sigma2=res["sigma2"], seed=5, summary=False)
    assert np.array_equal(one["W_mean"][:, 0], o1["W_mean"][:, 1])       # a row's sums do not depend on its neighbours
    for m in models:
        m.run_gibbs(Y, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_composition_with_summary_predictive_and_functionals():
    """4. out["W"] with results["V"] goes straight into the other posterior tools; the summary is the summary kernel's."""
    Vs, nu2, sigma2, Y = gaussian_problem(3, S=40, seed=21)
    q = (5, 50, 95)
    out = utils.fold_in_rows(Y, Vs, "gaussian", nu2=nu2, sigma2=sigma2, seed=9, q=q)
    mean, quant = utils.posterior_summary(out["W"], Vs, q=q)
    assert np.array_equal(mean, out["mean"]) and np.array_equal(quant, out["quantiles"])
    sq = utils.fold_in_rows(Y, Vs, "gaussian", nu2=nu2, sigma2=sigma2, seed=9, q=q, transform="square")
    assert np.array_equal(utils.posterior_summary(out["W"], Vs, q=q, transform="square")[0], sq["mean"])
    pp = utils.posterior_predictive(out["W"], Vs, "gaussian", data=Y, nu2=nu2, seed=1)
    assert pp["mean"].shape == Y.shape[:3] and np.all(np.isfinite(pp["mean"]))
    np.testing.assert_allclose(pp["mean"], out["mean"], rtol=0, atol=1e-12)
    pf = utils.posterior_functionals(out["W"], Vs, which=("auc", "max"))
    assert pf["auc"]["mean"].shape == (Y.shape[0], Vs.shape[1]) and np.all(np.isfinite(pf["auc"]["mean"]))
    assert out["nsamples"] == 40


def test_device_generator_moments():
    """5. One target repeated S = 4096 times: sample mean and covariance of W against (Q^-1 b, Q^-1), 5 standard errors."""
    S, K = 4096, 4
    Vs1, nu2, sigma2, Y = gaussian_problem(K, S=1, seed=31)
    Y = Y[1:2]
    m, Q = fold_in.conditional(Y[0], Vs1[0], nu2[0], sigma2[0])
    C = np.linalg.inv(Q)
    # the statistic itself: numpy's generator passes the same inequalities on these inputs
    ref = np.array([fold_in.draw(m, Q, zz) for zz in np.random.RandomState(0).normal(size=(S, K))])
    zm, zc = moments_check(ref, m, C)
    assert zm <= 5 and zc <= 5, (zm, zc)
    out = utils.fold_in_rows(Y, np.repeat(Vs1, S, axis=0), "gaussian", nu2=np.repeat(nu2, S), sigma2=np.repeat(sigma2, S), seed=12345,
                             summary=False)
    assert np.abs(out["W_mean"] - m).max() < W_TOL
    zm, zc = moments_check(out["W"][:, 0], m, C)
    print("device generator: largest standardised deviation of the mean %.2f, of the covariance %.2f (limit 5)" % (zm, zc))
    assert zm <= 5 and zc <= 5


def test_binomial_against_quadrature():
    """6. K = 2, one state repeated S = 4096 times, one row of ~40 observed cells of 1..8 trials: mean and covariance of the
    draws against the quadrature posterior, 5 standard errors plus the measured bias allowance BINOMIAL_BIAS.
    Determinism as in 3; a Bernoulli tensor; a row with no observations (prior moments)."""
    S = 4096
    V, sigma2, Y, N = binomial_problem()
    assert 35 <= int((~np.isnan(Y)).sum()) <= 45
    m, C = quadrature_posterior(V, sigma2, Y, N)
    Vs, s2 = np.repeat(V[None], S, axis=0), np.full(S, sigma2)
    out = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, seed=77, summary=False)
    assert "W_mean" not in out and np.all(np.isfinite(out["W"]))
    zm, zc = moments_check(out["W"][:, 0], m, C, bias=BINOMIAL_BIAS)
    print("binomial: posterior mean %s; sample mean %s; |diff| %s; standardised (after the allowance %.4f): mean %.2f cov %.2f"
          % (m, out["W"][:, 0].mean(axis=0), np.abs(out["W"][:, 0].mean(axis=0) - m), BINOMIAL_BIAS, zm, zc))
    assert zm <= 5 and zc <= 5
    # same bits: two calls, a slice of the samples, the model's entry point with uploaded results
    again = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, seed=77, summary=False)
    assert np.array_equal(out["W"], again["W"])
    part = utils.fold_in_rows((Y, N), Vs[100:200], "binomial", sigma2=s2[100:200], seed=77, summary=False, first_sample=100)
    assert np.array_equal(part["W"], out["W"][100:200])
    np.random.seed(0)
    model = BinomialBayesianTensorFiltering(6, V.shape[0], V.shape[1], nembeds=2)
    res = {"V": Vs[:64], "sigma2": s2[:64]}
    o = model.fold_in_rows((Y, N), results=res, seed=77, transform="ilogit")
    assert np.array_equal(o["W"], out["W"][:64])
    assert np.array_equal(utils.posterior_summary(o["W"], res["V"], transform="ilogit")[0], o["mean"])
    with pytest.raises(RuntimeError):
        model.fold_in_rows((Y, N))
    # a Bernoulli tensor (trials = 1) next to an empty row: the empty row has the prior's moments
    Yb = np.stack([(Y[0] > 0).astype(float), np.full(Y[0].shape, np.nan)])
    ob = utils.fold_in_rows(Yb, Vs, "binomial", sigma2=s2, seed=78, summary=False)
    mb, Cb = quadrature_posterior(V, sigma2, Yb[:1], np.ones_like(Yb[:1]))
    zm, zc = moments_check(ob["W"][:, 0], mb, Cb, bias=BINOMIAL_BIAS)
    assert zm <= 5 and zc <= 5, (zm, zc)
    zm, zc = moments_check(ob["W"][:, 1], np.zeros(2), sigma2 * np.eye(2))
    assert zm <= 5 and zc <= 5, (zm, zc)


def test_it_does_the_job():
    """7. (200,12,30) Gaussian data from a K = 3 model; the chain runs on the first 190 rows (device-collected), the last 10
    are folded in from 4 of their 12 columns.  RMSE of `mean` on the 8 unobserved columns against the noiseless truth:
    below FOLD_MARGIN times that of the chain that includes the rows with the same columns held out, and below predicting 0."""
    fold, chain, zero = fold_vs_chain(0)
    print("RMSE on the unobserved columns: fold-in %.4f, in-chain %.4f (ratio %.3f, margin %.3f), prior mean %.4f"
          % (fold, chain, fold / chain, FOLD_MARGIN, zero))
    assert fold < zero
    assert fold < FOLD_MARGIN * chain


def test_full_size_c3():
    """8. C3 shape (512,256,64) K = 5, S = 200 device-collected, R = 64 new rows with half of the columns observed."""
    N, M, T, K, S, R = 512, 256, 64, 5, 200, 64
    rs = np.random.RandomState(1)
    Wt = rs.normal(size=(N + R, K))
    Vt = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", Wt, Vt) + rs.normal(0, 0.5, size=(N + R, M, T))
    Y_new = Y[N:].copy()
    Y_new[:, 1::2] = np.nan
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_init=1.0, lam2_init=0.1, nu2_init=1.0, rng="device",
                                            device_seed=3)
    res = model.run_gibbs(Y[:N], nburn=20, nsamples=S, verbose=False)
    out = model.fold_in_rows(Y_new, seed=4)
    for k in ("W", "W_mean", "mean", "quantiles"):
        assert np.all(np.isfinite(out[k])), k
    assert out["mean"].shape == (R, M, T) and out["quantiles"].shape == (2, R, M, T)
    scale = np.abs(out["W_mean"]).max()
    checks = []
    for s, r in ((0, 0), (57, 31), (S - 1, R - 1)):
        m, Q = fold_in.conditional(Y_new[r], res["V"][s], float(res["nu2"][s, 0]), float(res["sigma2"][s, 0]))
        checks.append((np.abs(out["W_mean"][s, r] - m).max(), np.linalg.cond(Q)))
        print("(s,r)=(%d,%d): |W_mean - numpy| %.3e  cond(Q) %.1f  max|w| %.2f" % (s, r, checks[-1][0], checks[-1][1], scale))
    assert scale < 10                                          # |w| is O(1): the absolute tolerance means what it says
    for err, cond in checks:
        assert cond < COND_MAX
        assert err < W_TOL


def _arrays(out, prefix=""):
    """Every array of a returned value (a tuple or a dict, nested) as (path, array) pairs."""
    if isinstance(out, dict):
        return [p for k in sorted(out) for p in _arrays(out[k], "%s%s." % (prefix, k))]
    if isinstance(out, (tuple, list)):
        return [p for i, v in enumerate(out) for p in _arrays(v, "%s%d." % (prefix, i))]
    return [(prefix, out)] if isinstance(out, np.ndarray) else []


def test_collected_and_uploaded_samples_agree_in_every_analysis_call():
    """9. Every analysis method resolves its samples in one place (PosteriorAnalysis._samples): each of them, called on the
    device-collected samples and on the same run's result dict uploaded, returns the same bits in every array."""
    N, M, T, K = 5, 3, 6, 2
    rs = np.random.RandomState(4)
    Y = np.einsum("nk,mtk->nmt", rs.normal(size=(N, K)), 0.4 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)) \
        + rs.normal(0, 0.5, size=(N, M, T))
    Y_new = Y[:2].copy()
    Y_new[1, 1:] = np.nan
    np.random.seed(3)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=2)
    res = model.run_gibbs(Y, nburn=2, nsamples=8, verbose=False)
    calls = {
        "posterior_summary": lambda r: model.posterior_summary() if r is None else utils.posterior_summary(r["W"], r["V"]),
        "information_criteria": lambda r: model.information_criteria(r, pointwise=True),
        "loo": lambda r: model.loo(r, mean=True, log_weights=True),
        "posterior_predictive": lambda r: model.posterior_predictive(r, seed=1),
        "posterior_functionals": lambda r: model.posterior_functionals(r, which=("auc", "max", "crossing"), level=0.0, pointwise=True),
        "fold_in_rows": lambda r: model.fold_in_rows(Y_new, results=r, seed=1),
    }
    collected = {name: call(None) for name, call in calls.items()}
    for name, call in calls.items():
        a, b = _arrays(collected[name]), _arrays(call(res))
        assert len(a) >= 2 and [p for p, _ in a] == [p for p, _ in b], name
        for (path, x), (_, y) in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (name, path)
