"""The host halves of negbin_fold_in_rows (functionalmf_amd/negbin_fold_in.py: chain_rows and its helpers): no GPU."""
import math
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, fold_in, fold_in_cols as fc, negbin_fold_in as nf, utils
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

SWEEPS = 3


def row_problem(seed=0, M=3, T=4, K=3, nreps=1):
    rs = np.random.RandomState(seed)
    V = 0.6 * rs.normal(size=(M, T, K))
    Y = rs.poisson(4.0, size=(M, T, nreps)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.25] = np.nan
    return V, (Y if nreps > 1 else Y[..., 0]), rs.uniform(0.5, 6.0, size=(M, T)), 1.3


def test_fixed_rate_with_omega_is_the_hand_written_draw():
    """chain_rows with a fixed rate and given omega: every sweep is Q = sum omega v v' + I / sigma2, b = sum kappa v and the
    Cholesky draw, written out cell by cell here; omega is read at the observed cells alone."""
    V, Y, rate, sigma2 = row_problem(nreps=2)
    M, T, K = V.shape
    rs = np.random.RandomState(1)
    draws = nf.random_draws_rows(rs, K, SWEEPS)
    assert draws.shape == (nf.draws_length_rows(K, SWEEPS),) == (SWEEPS * K,)
    omega = rs.gamma(2.0, 0.4, size=(SWEEPS, M, T))
    states, systems = [], []
    w, mean, r, acc = nf.chain_rows(Y, V, sigma2, rate, SWEEPS, draws, omega=omega, on_system=systems.append,
                                    on_sweep=lambda sw, w, r: states.append(w.copy()))
    assert r is rate and acc is None and len(states) == len(systems) == SWEEPS
    for sw in range(SWEEPS):
        Q, b = np.eye(K) / sigma2, np.zeros(K)
        for j in range(M):
            for t in range(T):
                obs = Y[j, t][~np.isnan(Y[j, t])]
                if obs.size:
                    Q += omega[sw, j, t] * np.outer(V[j, t], V[j, t])
                    b += 0.5 * (obs.sum() - obs.size * rate[j, t]) * V[j, t]
        L = np.linalg.cholesky(Q)
        want = np.linalg.solve(Q, b) + np.linalg.solve(L.T, draws[sw * K:(sw + 1) * K])
        np.testing.assert_allclose(systems[sw], Q, rtol=1e-13, atol=0)
        np.testing.assert_allclose(states[sw], want, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(w, states[-1], rtol=0, atol=0)
    other = omega.copy()
    other[:, np.isnan(Y).all(axis=2)] = 77.0
    assert np.isnan(Y).all(axis=2).any()
    assert np.array_equal(nf.chain_rows(Y, V, sigma2, rate, SWEEPS, draws, omega=other, seed=4)[0], w)
    # a scalar and a dense rate are the same chain; the seeded stand-in sampler is reproducible
    a = nf.chain_rows(Y, V, sigma2, 2.5, SWEEPS, draws, seed=7)
    b = nf.chain_rows(Y, V, sigma2, np.full((M, T), 2.5), SWEEPS, draws, seed=7)
    assert np.array_equal(a[0], b[0]) and np.all(np.isfinite(a[0])) and not np.array_equal(a[0], w)
    for bad in (dict(draws=draws[:-1]), dict(omega=omega[:-1]), dict(sweeps=0)):
        kw = dict(dict(sweeps=SWEEPS, draws=draws, omega=omega), **bad)
        with pytest.raises(ValueError):
            nf.chain_rows(Y, V, sigma2, rate, kw["sweeps"], kw["draws"], omega=kw["omega"])


def test_integer_rates_give_the_binomial_pseudo_data():
    """With rate = r integer and Y + r <= 32 the cells are the Binomial chain's (n, y - n / 2) of fold_in.row_statistics on
    (Y, Y + r), and the seeded chains draw the same weights: PG(n, psi) from the same generator."""
    rs = np.random.RandomState(2)
    M, T, K, r = 3, 4, 2, 3.0
    Y = rs.randint(0, 29, size=(1, M, T)).astype(float)
    Y[0, 1, 2] = np.nan
    assert np.nanmax(Y) + r <= fold_in.MAX_TRIALS
    cnt, ysum = nf.cell_statistics(Y, (1, M, T))
    b, kappa = nf._pseudo(cnt, ysum, r)
    _, n, y = fold_in.row_statistics((Y, Y + r), "binomial", M, T)
    assert np.array_equal(b, n) and np.array_equal(kappa, np.where(n > 0, y - n / 2, 0.0)) and (n == 0).sum() == 1
    V = 0.6 * rs.normal(size=(M, T, K))
    draws = nf.random_draws_rows(rs, K, SWEEPS)
    seen = []
    pg = fc.polya_gamma
    try:
        fc.polya_gamma = lambda rng, n, psi: seen.append((n.copy(), psi.copy())) or pg(rng, n, psi)
        nf.chain_rows(Y[0], V, 1.5, r, SWEEPS, draws, seed=3)
    finally:
        fc.polya_gamma = pg
    assert len(seen) == SWEEPS and all(np.array_equal(nn, n[0]) for nn, _ in seen) and not seen[0][1].any() and seen[1][1].any()


def test_histogram_form_of_the_likelihood_ratio():
    """The histogram form of ll equals the per-observation sum with math.lgamma to 1e-12 relative, at counts on both sides
    of 32 / 33 and 1024 and at rates below 1, above 33 and far above.  Relative to ll itself: the per-observation sum is
    taken with math.fsum, and rate_loglik_ratio pairs lgamma(y + cand) with lgamma(y + r) before anything is added."""
    counts = np.array([0, 31, 32, 33, 1023, 1024, 5000], dtype=float)
    rs = np.random.RandomState(3)
    Y = rs.choice(counts, size=(1, 4, 6, 3))
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    Y[0, 0, 0] = counts[:3]
    Y[0, 0, 1] = counts[3:6]
    Y[0, 0, 2, 0] = counts[6]
    yv, h = nf.row_histograms(Y)
    assert yv.shape == h.shape == (1, counts.size) and np.array_equal(yv[0], counts) and h.sum() == (~np.isnan(Y)).sum()
    obs = Y[~np.isnan(Y)]
    L = -17.25
    for r in (0.3, 1.5, 33.0, 400.0):
        for cand in (r * 1.1, r * 0.8, r + 1e-3):
            terms = [t for y in obs for t in (math.lgamma(y + cand), -math.lgamma(cand), -math.lgamma(y + r), math.lgamma(r))]
            want = math.fsum(terms) + (cand - r) * L
            got = nf.rate_loglik_ratio(yv[0], h[0], cand, r, L)
            assert abs(got - want) <= 1e-12 * abs(want), (r, cand, got, want)
    # padding and several rows: the widest row sets the width, h = 0 beyond a row's own counts
    yv, h = nf.row_histograms(np.array([[[1.0, 1.0, 4.0]], [[np.nan, np.nan, np.nan]], [[2.0, 0.0, 9.0]]]))
    assert np.array_equal(yv, [[1, 4, 0], [0, 0, 0], [0, 2, 9]]) and np.array_equal(h, [[2, 1, 0], [0, 0, 0], [1, 1, 1]])
    assert nf.rate_loglik_ratio(yv[1], h[1], 3.0, 2.0, 0.0) == 0.0
    for bad in (np.array([[-1.0]]), np.array([[0.5]]), np.array([[np.inf]])):
        with pytest.raises(ValueError, match="non-negative integers"):
            nf.row_histograms(bad)


def reference_step(data, W_row, V, R, n, u, rpropstdev, rstdev):
    """One step of the reference's _resample_R for a single row with one rate (rdims = (1, 2)), restated: data (M,T,nreps)."""
    psi = np.clip(np.einsum("k,mtk->mt", W_row, V), -10, 10)
    P = (1.0 / (1.0 + np.exp(-psi)))[..., None]
    logR = math.log(R)
    cand_log = logR + rpropstdev * n
    cand = math.exp(cand_log)
    logpdf = lambda x: -0.5 * (x / rstdev) ** 2 - math.log(rstdev) - 0.5 * math.log(2 * math.pi)
    accept_prior = logpdf(cand_log) - logpdf(logR)
    lg = np.vectorize(lambda x: math.lgamma(x) if x == x else np.nan)
    ll = lg(data + cand) - math.lgamma(cand) - lg(data + R) + math.lgamma(R) + (cand - R) * np.log(1 - P)
    prob = math.exp(min(max(accept_prior + np.nansum(ll), -10), 1))
    return (cand_log if (u <= prob and cand > 1) else logR), prob, cand


def test_metropolis_step_is_the_references():
    rs = np.random.RandomState(4)
    V, Y, _, _ = row_problem(seed=5, nreps=3)
    M, T, K = V.shape
    cnt, _ = nf.cell_statistics(Y, (M, T))
    yv, h = nf.row_histograms(Y[None])
    accepted = 0
    for trial in range(60):
        w = rs.normal(size=K) * (1 + 8 * (trial % 3 == 0))                # some psi beyond the clip
        R = float(rs.uniform(0.4, 5.0))
        n, u = float(rs.normal()), float(rs.uniform())
        rprop = (0.1, 0.5)[trial % 2]
        L = nf.failure_log_sum(cnt, V.reshape(-1, K).dot(w).reshape(M, T))
        logr, acc, prob, cand = nf.metropolis_step(math.log(R), n, u, yv[0], h[0], L, rprop, 1.5)
        want_logr, want_prob, want_cand = reference_step(Y, w, V, R, n, u, rprop, 1.5)
        assert abs(prob - want_prob) <= 1e-9 * want_prob and abs(cand - want_cand) <= 1e-14 * want_cand
        if abs(u - want_prob) > 1e-6:
            assert logr == pytest.approx(want_logr, rel=1e-14, abs=1e-15)
        accepted += acc
    assert 0 < accepted < 60
    # the floor: a candidate at or below 1 is refused whatever its probability
    logr, acc, prob, cand = nf.metropolis_step(math.log(1.05), -3.0, 1e-9, yv[0], h[0], L, 0.1, 1.0)
    assert cand < 1 and not acc and logr == math.log(1.05)


def test_sampled_chain_layout_and_hooks():
    """draws: per sweep nmetropolis normals, nmetropolis uniforms, K normals; the rate step runs before the weights; the
    chain is the composition of metropolis_step and the fixed-rate sweep; on_accept sees every decision."""
    V, Y, _, sigma2 = row_problem(seed=6, nreps=2)
    M, T, K = V.shape
    nm = 5
    rs = np.random.RandomState(7)
    draws = nf.random_draws_rows(rs, K, SWEEPS, nm)
    assert draws.shape == (nf.draws_length_rows(K, SWEEPS, nm),) == (SWEEPS * (2 * nm + K),)
    d = draws.reshape(SWEEPS, 2 * nm + K)
    assert np.all((d[:, nm:2 * nm] > 0) & (d[:, nm:2 * nm] < 1)) and np.abs(d[:, :nm]).max() > 1 and np.abs(d[:, 2 * nm:]).max() > 1
    assert nf.random_draws_rows(rs, K, SWEEPS, nm, size=(2, 3)).shape == (2, 3, SWEEPS * (2 * nm + K))
    omega = rs.gamma(2.0, 0.4, size=(SWEEPS, M, T))
    decisions, rates = [], []
    w, mean, r, share = nf.chain_rows(Y, V, sigma2, None, SWEEPS, draws, omega=omega, rate_init=2.5, nmetropolis=nm, rpropstdev=0.4,
                                      on_accept=lambda *a: decisions.append(a), on_sweep=lambda sw, w, r: rates.append(r))
    assert len(decisions) == SWEEPS * nm and [a[:2] for a in decisions] == [(s, k) for s in range(SWEEPS) for k in range(nm)]
    assert all(a[3] == d[a[0], nm + a[1]] for a in decisions) and r == rates[-1]
    # by hand
    cnt, _ = nf.cell_statistics(Y, (M, T))
    yv, h = nf.row_histograms(Y[None])
    logr, nacc = math.log(2.5), 0
    L = nf.failure_log_sum(cnt, np.zeros((M, T)))                          # the chain starts from w = 0
    assert L == pytest.approx(-math.log(2.0) * cnt.sum(), rel=1e-14)
    for k in range(nm):
        logr, acc, _, _ = nf.metropolis_step(logr, d[0, k], d[0, nm + k], yv[0], h[0], L, 0.4, 1)
        nacc += acc
    first = nf.chain_rows(Y, V, sigma2, math.exp(logr), 1, d[0, 2 * nm:], omega=omega[:1])[0]
    assert rates[0] == math.exp(logr)
    one = nf.chain_rows(Y, V, sigma2, None, 1, d[0], omega=omega[:1], rate_init=2.5, nmetropolis=nm, rpropstdev=0.4)
    assert np.array_equal(one[0], first) and one[2] == rates[0] and one[3] == nacc / nm
    assert share == sum(1 for a in decisions if a[3] <= a[2] and a[4] > 1) / (SWEEPS * nm) and 0 < share < 1
    for kw in (dict(rate_init=None), dict(rate_init=-1.0), dict(rate_init=np.nan), dict(nmetropolis=0)):
        with pytest.raises(ValueError):
            nf.chain_rows(Y, V, sigma2, None, SWEEPS, draws, omega=omega, **dict(dict(rate_init=2.5, nmetropolis=nm), **kw))


def test_where_the_rate_comes_from():
    """The rate-source table, case by case."""
    S, R, N, M, T = 3, 2, 6, 4, 5
    rs = np.random.RandomState(8)
    u = lambda *shape: rs.uniform(1, 3, size=shape)
    # rate= given: fixed, as given
    for shape in ((S,), (S, 1, 1, 1), (S, R, 1, 1), (S, 1, M, 1), (S, 1, 1, T), (S, 1, M, T), (S, R, M, T)):
        r = u(*shape)
        mode, arr = nf.resolve_row_rate(u(S, N, 1, 1), r, None, S, R, M, T)
        assert mode == "fixed" and arr.ndim == 4 and arr.flags["C_CONTIGUOUS"] and np.array_equal(arr.reshape(r.shape), r)
        assert np.array_equal(np.broadcast_to(arr, (S, R, M, T)), np.broadcast_to(r.reshape(arr.shape), (S, R, M, T)))
    arr, st = nf.rate_strides(nf.resolve_row_rate(None, u(S, R, 1, T), None, S, R, M, T)[1])
    assert st == (R * T, T, 0, 1)                                          # the kernel's (sample, row, column, depth)
    # the fitted layout does not vary along rows: fixed, the kept sample's
    for tail in ((1, 1, 1), (1, M, 1), (1, 1, T), (1, M, T)):
        Rfit = u(S, *tail)
        mode, arr = nf.resolve_row_rate(Rfit, None, None, S, R, M, T)
        assert mode == "fixed" and np.array_equal(arr, Rfit)
        assert nf.resolve_row_rate(Rfit, None, False, S, R, M, T)[0] == "fixed"
        assert nf.resolve_row_rate(Rfit, None, True, S, R, M, T) == ("sampled", None)
    assert nf.resolve_row_rate(u(S), None, None, S, R, M, T)[1].shape == (S, 1, 1, 1)
    # one rate per row: sampled
    Rfit = u(S, N, 1, 1)
    assert nf.resolve_row_rate(Rfit, None, None, S, R, M, T) == ("sampled", None)
    assert nf.resolve_row_rate(Rfit, None, True, S, R, M, T) == ("sampled", None)
    with pytest.raises(ValueError, match="sample_rate=False"):
        nf.resolve_row_rate(Rfit, None, False, S, R, M, T)
    # any other layout that varies along rows
    for tail in ((N, M, 1), (N, 1, T), (N, M, T)):
        for flag in (None, False):
            with pytest.raises(ValueError, match="pass rate="):
                nf.resolve_row_rate(u(S, *tail), None, flag, S, R, M, T)
        assert nf.resolve_row_rate(u(S, *tail), None, True, S, R, M, T) == ("sampled", None)
    with pytest.raises(ValueError, match="pass rate="):
        nf.resolve_row_rate(None, None, None, S, R, M, T)
    with pytest.raises(ValueError, match="one of them"):
        nf.resolve_row_rate(Rfit, u(S), True, S, R, M, T)
    # rate_init: (S,) or (S,R); default the geometric mean of the kept sample's rates
    np.testing.assert_allclose(nf.resolve_rate_init(None, Rfit, S, R), np.repeat(np.exp(np.log(Rfit).mean(axis=(1, 2, 3)))[:, None], R, axis=1), rtol=1e-15)
    assert np.array_equal(nf.resolve_rate_init(np.arange(1.0, S + 1), None, S, R), np.repeat(np.arange(1.0, S + 1)[:, None], R, axis=1))
    r0 = u(S, R)
    assert np.array_equal(nf.resolve_rate_init(r0, None, S, R), r0)


def test_argument_checks():
    """Every ValueError, before any device call."""
    S, R, N, M, T, K = 3, 2, 6, 4, 5, 2
    rs = np.random.RandomState(9)
    Vs, sigma2 = rs.normal(size=(S, M, T, K)), np.ones(S)
    Y = rs.poisson(3.0, size=(R, M, T)).astype(float)
    Rrow = np.full((S, N, 1, 1), 2.0)
    good = dict(R=Rrow)
    # shapes
    for bad in (np.zeros((R, M)), np.zeros((R, M + 1, T)), np.zeros((R, M, T, 2, 2)), np.zeros((R, M, T, 0)), np.zeros((0, M, T))):
        with pytest.raises(ValueError, match="must be"):
            utils.negbin_fold_in_rows(bad, Vs, sigma2, **good)
    with pytest.raises(ValueError, match="Vs must be"):
        utils.negbin_fold_in_rows(Y, Vs[0], sigma2, **good)
    for bad in (np.ones(S + 1), None):
        with pytest.raises(ValueError, match="sigma2"):
            utils.negbin_fold_in_rows(Y, Vs, bad, **good)
    with pytest.raises(ValueError, match="sigma2 must be positive"):
        utils.negbin_fold_in_rows(Y, Vs, -sigma2, **good)
    # counts
    for bad in (-Y - 1, Y + 0.5, np.where(Y > 2, np.inf, Y)):
        with pytest.raises(ValueError, match="non-negative integers"):
            utils.negbin_fold_in_rows(bad, Vs, sigma2, **good)
    # rates and rate_init
    for bad in (np.zeros(S), -np.ones(S), np.full(S, np.nan), np.full(S, np.inf)):
        with pytest.raises(ValueError, match="finite and positive"):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, rate=bad)
        with pytest.raises(ValueError, match="finite and positive"):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, rate_init=bad, **good)
        with pytest.raises(ValueError, match="finite and positive"):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, R=bad)
    for bad in (np.ones(S + 1), np.ones((S, R + 1, 1, 1)), np.ones((S, 2, 2)), 3.0):
        with pytest.raises(ValueError):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, rate=bad)
    for bad in (np.ones(S + 1), np.ones((S, R + 1)), np.ones((S, R, 1))):
        with pytest.raises(ValueError, match="rate_init must be"):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, rate_init=bad, **good)
    with pytest.raises(ValueError, match="rate_init"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, sample_rate=True)        # nothing to start from
    with pytest.raises(ValueError, match="pass rate="):
        utils.negbin_fold_in_rows(Y, Vs, sigma2)
    with pytest.raises(ValueError, match="pass rate="):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, R=np.ones((S, N, M, 1)))
    with pytest.raises(ValueError, match="sample_rate=False"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, sample_rate=False, **good)
    with pytest.raises(ValueError, match="1e\\+15|below"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, rate=np.full(S, 1e15))
    with pytest.raises(ValueError, match="1e\\+15|below"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, rate_init=np.full(S, 1e15), **good)       # a sampled rate is bounded where it starts
    # the Metropolis step
    for kw in (dict(nmetropolis=0), dict(nmetropolis=2.5), dict(rpropstdev=0.0), dict(rstdev=-1.0), dict(rpropstdev=np.nan)):
        with pytest.raises(ValueError, match="nmetropolis|rpropstdev"):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, **dict(good, **kw))
    utils_fixed = dict(rate=np.full(S, 2.0))
    # sizes, sweeps, q, transform
    with pytest.raises(ValueError, match="2\\^31"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, first_sample=2 ** 31 // R, **good)
    with pytest.raises(ValueError, match="2\\^31|first_sample"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, first_sample=-1, **good)
    big = np.broadcast_to(Vs[:1], (16385, M, T, K))
    with pytest.raises(ValueError, match="16384"):
        utils.negbin_fold_in_rows(Y, big, np.ones(16385), rate=np.full(16385, 2.0))
    for kw in (dict(sweeps=0), dict(sweeps=1.5), dict(sweeps=nf.MAX_ROW_SWEEPS + 1), dict(q=(5, 120)), dict(transform="cube")):
        with pytest.raises(ValueError):
            utils.negbin_fold_in_rows(Y, Vs, sigma2, **dict(utils_fixed, **kw))
    with pytest.raises(ValueError, match="nembeds"):
        utils.negbin_fold_in_rows(Y, rs.normal(size=(S, M, T, 11)), sigma2, **utils_fixed)
    # draws only together with omega; their shapes and ranges
    nm, sw = 4, 2
    draws = nf.random_draws_rows(rs, K, sw, nm, size=(S, R))
    omega = np.ones((S, R, sw, M, T))
    with pytest.raises(ValueError, match="omega"):
        utils.negbin_fold_in_rows(Y, Vs, sigma2, draws=draws, sweeps=sw, nmetropolis=nm, **good)
    z, mh, o, qs, tcode, sweeps, nmv = nf.check_args_rows(S, R, M, T, K, True, nm, draws=draws, omega=omega, sweeps=sw)
    assert z.shape == (S, R, sw, K) and mh.shape == (S, R, sw, 2, nm) and o.shape == omega.shape and (sweeps, nmv) == (sw, nm)
    d = draws.reshape(S, R, sw, 2 * nm + K)
    assert np.array_equal(z, d[..., 2 * nm:]) and np.array_equal(mh[:, :, :, 0], d[..., :nm]) and np.array_equal(mh[:, :, :, 1], d[..., nm:2 * nm])
    zf = nf.check_args_rows(S, R, M, T, K, False, nm, draws=draws[..., :sw * K], omega=omega, sweeps=sw)
    assert zf[0].shape == (S, R, sw, K) and zf[1] is None and zf[6] == 0
    hot = draws.copy()
    hot[0, 0, nm] = 1.5                                                    # a uniform outside (0, 1)
    for kw in (dict(draws=draws[..., :-1]), dict(draws=draws * np.nan), dict(draws=hot), dict(omega=omega[:, :, :1]), dict(omega=-omega),
               dict(omega=omega * np.nan)):
        with pytest.raises(ValueError):
            nf.check_args_rows(S, R, M, T, K, True, nm, **dict(dict(draws=draws, omega=omega, sweeps=sw), **kw))
    # the defaults of sweeps
    assert nf.check_args_rows(S, R, M, T, K, False)[5] == fold_in.DEFAULT_INNER_SWEEPS
    assert nf.check_args_rows(S, R, M, T, K, True)[5] == nf.DEFAULT_SWEEPS["rows"]
    assert nf.DEFAULT_SWEEPS["rows"] & (nf.DEFAULT_SWEEPS["rows"] - 1) == 0


class _NoDevice:
    device = 0

    def call(self, *a):
        raise AssertionError("a device call was made")


def _bare(world=1):
    m = object.__new__(NegativeBinomialBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.tf_order, m.stability = 6, 3, 5, 2, 2, 1e-6
    m.nmetropolis, m.rpropstdev, m.rstdev = 11, 0.25, 1.5
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    m._collected, m._draws, m._device_seed, m._callback = 0, 0, 1, False
    return m


def test_the_model_routes_to_the_module(monkeypatch):
    S = 4
    res = {"V": np.ones((S, 3, 5, 2)), "sigma2": np.ones((S, 1)), "R": np.full((S, 6, 1, 1), 2.0)}
    m = _bare()
    seen = []
    monkeypatch.setattr(nf, "evaluate_rows", lambda *a, **kw: seen.append((a, kw)) or {"W": None})
    m.negbin_fold_in_rows(np.ones((2, 3, 5)), res, seed=3, sweeps=7)
    a, kw = seen[-1]
    assert a[:5] == (S, 2, 3, 5, 2) and kw["rate"] is None and np.array_equal(kw["rate_init"], np.full((S, 2), 2.0))
    assert (kw["nmetropolis"], kw["rpropstdev"], kw["rstdev"], kw["seed"], kw["sweeps"]) == (11, 0.25, 1.5, 3, 7)
    m.negbin_fold_in_rows(np.ones((2, 3, 5)), dict(res, R=np.full((S, 1, 3, 1), 4.0)))
    assert seen[-1][1]["rate"].shape == (S, 1, 3, 1) and seen[-1][1]["rate_init"] is None
    m.negbin_fold_in_rows(np.ones((2, 3, 5)), res, rate=np.full((S, 2, 1, 1), 5.0))
    assert np.all(seen[-1][1]["rate"] == 5.0)
    with pytest.raises(ValueError, match="pass rate="):
        m.negbin_fold_in_rows(np.ones((2, 3, 5)), dict(res, R=np.ones((S, 6, 3, 1))))
    with pytest.raises(RuntimeError, match="keeps its samples on the host"):
        m.negbin_fold_in_rows(np.ones((2, 3, 5)), None)
    with pytest.raises(NotImplementedError, match="unsharded"):
        _bare(world=2).negbin_fold_in_rows(np.ones((2, 3, 5)), res)
    with pytest.raises(ValueError, match="results"):
        m.negbin_fold_in_rows(np.ones((2, 3, 5)), dict(res, V=np.ones((S, 4, 5, 2))))
    with pytest.raises(NotImplementedError, match="Negative-Binomial"):    # the Binomial call keeps refusing this model
        m.fold_in_rows(np.zeros((1, 3, 5)), results=dict(res, W=np.ones((S, 6, 2))))


def test_registration():
    """The header prototype's argument count equals SIGNATURES; the kernel lives in the existing unit, so the build still
    makes 32 compilations and counts fifteen kernel-time names."""
    with open(os.path.join(_native.ROOT, "include", "btf.h")) as f:
        text = f.read()
    proto = re.search(r"int btf_negbin_fold_in_rows\((.*?)\);", text, re.S)
    assert proto and len(proto.group(1).split(",")) == len(_native.SIGNATURES["btf_negbin_fold_in_rows"][1]) == 37
    assert len(_native.UNITS) + _native.INST_PARTS == 32 and len(_native.KERNEL_NAMES) == 15
    assert not any("negbin" in os.path.basename(src) for src, _ in _native.UNITS)
    with open(os.path.join(_native.CSRC, "btf_fold_in.hip")) as f:
        unit = f.read()
    assert '#include "btf_negbin_fold_rows.h"' in unit and "negbin_fold_rows_fn" in unit
    with open(os.path.join(_native.CSRC, "btf_fold_in.h")) as f:
        head = f.read()
    assert "constexpr int FOLD_PARTS = 4;" in head and "#pragma unroll 2" in head
    assert hasattr(_native.load(), "btf_negbin_fold_in_rows")


def test_every_gpu_replay_case_has_a_seed():
    """The replay cases of tests/test_gpu_negbin_fold_in_rows.py pick the first seed whose numpy chains keep cond(Q) < 1e9
    and every Metropolis decision clear of its threshold: such a seed exists for every case (conditions on numpy alone)."""
    import test_gpu_negbin_fold_in_rows as g
    cases = g.replay_cases()
    assert len(set(cases)) == len(cases)
    for case in cases:
        K, R, M, T, sampled, layout, nreps, special = case
        p, W, Wm, Rr, acc, cond = g.rows_numpy(K, R, M, T, sampled, layout, nreps, special)
        assert cond < g.COND_MAX and np.all(np.isfinite(W)) and W.shape == (g.S_REPLAY, R, K)
        if sampled:
            assert np.all(Rr > 0) and np.all((acc >= 0) & (acc <= 1))
    from conftest import load_golden
    o = load_golden(g.ORACLE)
    assert int(o["nchains"]) >= 8192 and o["mean_w"].shape == (2,) and o["mean_p"].shape == (12,) and np.all(o["se_p"] > 0)
