"""negbin_fold_in_rows on the GPU (csrc/btf_negbin_fold_rows.h: negbin_fold_rows_kernel<K, SAMPLED>).

Yardsticks: the numpy definition functionalmf_amd.negbin_fold_in.chain_rows on the same variates AND the same Polya-Gamma
weights (the siblings' 1e-6 * max(1, |W|) with cond(Q) < 1e9 asserted on the numpy side; the sampled rate to 1e-10
relative - per Metropolis step the state goes through one log and one exp, a few ulp each, and 12 steps leave a margin of
about 1e4; every accept decision of the numpy chain lies further than 1e-6 from its threshold, so rounding cannot flip
one), the Binomial fold_in_rows on (Y, Y + r) where the counts are small, the exact law where there is no data, and 32768
numpy chains where there is.  The case builders are plain numpy: tests/test_host_negbin_fold_in_rows.py runs them on the
CPU to show that every case has a seed.
"""
import numpy as np
import pytest
from conftest import load_golden

from functionalmf_amd import _native, fold_in, negbin_fold_in as nf, utils
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
R_TOL = 1e-10
COND_MAX = 1e9
DECISION_MARGIN = 1e-6
S_REPLAY, SWEEPS_REPLAY, NM_REPLAY = 3, 3, 4
RPROP_REPLAY, RSTDEV_REPLAY = 0.3, 1.0
S_STAT = 4096

# ---- measured constants ("Folding new rows into a Negative-Binomial fit"; scripts/negbin_fold_in_rows_rate.py
# --step oracle, on the CPU, writes them into profiles/r29_negbin_fold_in_rows_rate.jsonl and beside the oracle's means).
# The shift of the host stand-in sampler (fold_in_cols.polya_gamma cut at PG_TERMS = 200 terms): the largest |difference| of
# the oracle's means between 200 and 800 terms, 32768 numpy chains each - a property of the reference alone.  All three lie
# within 1.2 standard errors of that difference (0.00136 / 0.00197 / 0.00076): no shift is resolved at this size.
ORACLE = "negbin_fold_in_rows_oracle.npz"
ORACLE_SHIFT = {"logr": 0.00154,           # mean of log r: 1.7284 at 200 terms
                "w": 0.00132,              # largest over the K = 2 means of w
                "p": 0.00095}              # largest over the 12 means of ilogit(w . v)

FIXED_LAYOUTS = ("scalar", "column", "depth", "column_depth", "row")
EDGE_COUNTS = np.array([0, 1, 31, 32, 33, 34, 150, 195, 199, 201, 260, 1023, 1024, 1025, 5000], dtype=float)


def close(a, b, tol=W_TOL):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= tol


def fixed_rate(rs, layout, S, R, M, T):
    """rate= of a layout: (S,) plus a shape that broadcasts against (R,M,T)."""
    lead = {"scalar": (), "column": (1, M, 1), "depth": (1, 1, T), "column_depth": (1, M, T), "row": (R, 1, 1)}[layout]
    return rs.uniform(0.5, 6.0, size=(S,) + lead)


def rows_problem(K, R, M, T, seed, sampled, layout="scalar", nreps=1, special=None):
    rs = np.random.RandomState(seed)
    S, sw = S_REPLAY, SWEEPS_REPLAY
    nm = NM_REPLAY if sampled else 0
    Vs = 0.6 * rs.normal(size=(S, M, T, K))
    sigma2 = rs.uniform(0.5, 2.0, size=S)
    Y = rs.poisson(4.0, size=(R, M, T, nreps)).astype(float)
    if special == "edge_counts":                                          # both sides of 32 / 33, of 1024 and of pseudo-trials 200
        Y = rs.choice(EDGE_COUNTS, size=Y.shape)
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    if special == "holes":
        Y[R // 2] = np.nan                                                # a wholly missing row
        Y[0] = np.nan
        Y[0, M - 1, T - 1, 0] = 7.0                                       # a row whose only observed cell is the last
    rate = None if sampled else fixed_rate(rs, layout, S, R, M, T)
    rate_init = rs.uniform(1.2, 6.0, size=(S, R)) if sampled else None
    draws = nf.random_draws_rows(rs, K, sw, nm, size=(S, R))
    omega = rs.gamma(2.0, 0.4, size=(S, R, sw, M, T))
    return dict(Vs=Vs, sigma2=sigma2, Y=Y if nreps > 1 else Y[..., 0], rate=rate, rate_init=rate_init, draws=draws, omega=omega)


def rows_numpy(K, R, M, T, sampled, layout="scalar", nreps=1, special=None):
    """A case whose numpy chains keep cond(Q) under COND_MAX and every Metropolis decision further than DECISION_MARGIN from
    its threshold (u from prob, the candidate from the floor 1) - the first of a fixed sequence of seeds - and their
    results.  Conditions on the numpy side alone."""
    base = 100000 * K + 1000 * R + 10 * M * T + nreps + (5 if sampled else 0) + FIXED_LAYOUTS.index(layout) * 7 + (500 if special else 0)
    for k in range(50):
        p = rows_problem(K, R, M, T, base + 7919 * k, sampled, layout, nreps, special)
        S = S_REPLAY
        dense = None if sampled else np.broadcast_to(p["rate"].reshape((S,) + p["rate"].shape[1:] + (1,) * (4 - p["rate"].ndim)), (S, R, M, T))
        conds, margins, out = [], [], []
        for s in range(S):
            for r in range(R):
                out.append(nf.chain_rows(p["Y"][r], p["Vs"][s], p["sigma2"][s], None if sampled else dense[s, r], SWEEPS_REPLAY,
                                         p["draws"][s, r], omega=p["omega"][s, r], rate_init=p["rate_init"][s, r] if sampled else None,
                                         nmetropolis=NM_REPLAY, rpropstdev=RPROP_REPLAY, rstdev=RSTDEV_REPLAY,
                                         on_system=lambda Q: conds.append(np.linalg.cond(Q)),
                                         on_accept=lambda sw, st, prob, u, cand: margins.append(min(abs(u - prob), abs(cand - 1.0)))))
        if max(conds) < COND_MAX and (not sampled or min(margins) > DECISION_MARGIN):
            W = np.array([o[0] for o in out]).reshape(S, R, K)
            Wm = np.array([o[1] for o in out]).reshape(S, R, K)
            Rr = np.array([o[2] for o in out]).reshape(S, R) if sampled else None
            acc = np.array([o[3] for o in out]).reshape(S, R) if sampled else None
            return p, W, Wm, Rr, acc, max(conds)
    raise AssertionError("no seed with cond(Q) < %g and decisions clear of their thresholds" % COND_MAX)


def replay_cases():
    """(K, R, M, T, sampled, layout, nreps, special): the smallest cases that reach each edge."""
    cases = [(K, 65, 3, 3, sampled, FIXED_LAYOUTS[K % 5], 1, None) for K in range(1, 11) for sampled in (False, True)]   # every instantiation, a second block
    cases += [(2, R, 3, 3, sampled, "row", 1, None) for R in (1, 63, 64, 65, 129) for sampled in (False, True)]
    cases += [(3, 5, 1, MT, sampled, "depth", 1, None) for MT in (1, 3, 4, 5, 9) for sampled in (False, True)]   # waves without a cell, both unroll tails
    cases += [(3, 5, 3, 3, sampled, "column_depth", 3, None) for sampled in (False, True)]          # replicates
    cases += [(3, 5, 3, 3, sampled, "column", 1, "holes") for sampled in (False, True)]
    cases += [(3, 5, 3, 4, sampled, "scalar", 2, "edge_counts") for sampled in (False, True)]
    cases += [(4, 3, 2, 19, False, layout, 1, None) for layout in FIXED_LAYOUTS]                   # every fixed layout, more cells than a weight block
    cases += [(4, 3, 2, 19, True, "scalar", 1, None)]
    return cases


def run_replay(p, sampled):
    kw = dict(draws=p["draws"], omega=p["omega"], sweeps=SWEEPS_REPLAY, summary=False, nmetropolis=NM_REPLAY, rpropstdev=RPROP_REPLAY,
              rstdev=RSTDEV_REPLAY)
    if sampled:
        return utils.negbin_fold_in_rows(p["Y"], p["Vs"], p["sigma2"], sample_rate=True, rate_init=p["rate_init"], **kw)
    return utils.negbin_fold_in_rows(p["Y"], p["Vs"], p["sigma2"], rate=p["rate"], **kw)


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("case", replay_cases(), ids=lambda c: "K%d-R%d-M%d-T%d-%s-%s-n%d-%s" % (c[0], c[1], c[2], c[3], "sampled" if c[4] else "fixed", c[5], c[6], c[7]))
def test_replay_equals_numpy_chain(case):
    """1. With draws= and omega= the kernel equals chain_rows: S = 3, 3 sweeps, nmetropolis = 4."""
    K, R, M, T, sampled, layout, nreps, special = case
    p, W, Wm, Rr, acc, cond = rows_numpy(K, R, M, T, sampled, layout, nreps, special)
    out = run_replay(p, sampled)
    print("%r  max cond(Q) %.2e  max|W| %.2f  err W %.2e  W_mean %.2e" % (case, cond, np.abs(W).max(), np.abs(out["W"] - W).max(),
                                                                           np.abs(out["W_mean"] - Wm).max()))
    assert cond < COND_MAX
    assert close(out["W_mean"], Wm)
    assert close(out["W"], W)
    if sampled:
        print("   err R (rel) %.2e  accepted share %.3f" % (np.max(np.abs(out["R"] - Rr) / Rr), acc.mean()))
        assert np.array_equal(out["accept"], acc)
        assert float(np.max(np.abs(out["R"] - Rr) / Rr)) <= R_TOL
        assert 0 < acc.mean() < 1
    else:
        assert "R" not in out and "accept" not in out
    if special == "holes":
        assert np.isnan(p["Y"][R // 2]).all() and np.isfinite(out["W"]).all()


def keyed_problem(R, seed=11):
    rs = np.random.RandomState(seed)
    S, M, T, K = 3, 3, 4, 3
    Vs = 0.6 * rs.normal(size=(S, M, T, K))
    Y = rs.choice(np.array([0, 2, 5, 40, 190, 260], dtype=float), size=(R, M, T, 2))      # pseudo-trials on both sides of 200
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    return Vs, rs.uniform(0.5, 2.0, size=S), Y, rs.uniform(2.0, 4.0, size=(S, R))


@pytest.mark.parametrize("sampled", (False, True))
def test_keys_are_global(sampled):
    """2. With the device generators one call with S = 3 equals, bit for bit, a call with S = 2 followed by a call with
    first_sample=2; rows 0..63 of an R = 65 call equal an R = 64 call."""
    Vs, sigma2, Y, r0 = keyed_problem(65)
    keys = ("W", "W_mean") + (("R", "accept") if sampled else ())

    def call(sl, rows, first=0):
        kw = dict(seed=77, sweeps=3, summary=False, first_sample=first, nmetropolis=3, rpropstdev=0.4)
        if sampled:
            return utils.negbin_fold_in_rows(Y[:rows], Vs[sl], sigma2[sl], sample_rate=True, rate_init=r0[sl, :rows], **kw)
        return utils.negbin_fold_in_rows(Y[:rows], Vs[sl], sigma2[sl], rate=r0[sl, :rows, None, None], **kw)

    whole = call(slice(0, 3), 65)
    assert np.all(np.isfinite(whole["W"]))
    head, tail = call(slice(0, 2), 65), call(slice(2, 3), 65, first=2)
    for k in keys:
        assert np.array_equal(whole[k][:2], head[k]) and np.array_equal(whole[k][2:], tail[k]), k
    fewer = call(slice(0, 3), 64)
    for k in keys:
        assert np.array_equal(whole[k][:, :64], fewer[k]), k
    again = call(slice(0, 3), 65)
    assert all(np.array_equal(whole[k], again[k]) for k in keys)
    assert not np.array_equal(whole["W"][0], whole["W"][1])
    if sampled:
        assert 0 < whole["accept"].mean() < 1 and np.all(whole["R"] > 0)


def ilogit(x):
    return 1.0 / (1.0 + np.exp(-x))


def test_fixed_rate_against_the_binomial_fold_in_rows():
    """3. Integer rates 2 and 3 and counts with y + r <= 32: the chain has the law of the Binomial fold_in_rows on
    (Y, Y + r) at the same 4 sweeps.  One V tiled over S = 4096 samples, R = 2, (M,T) = (3,4), K = 2: every mean of w and
    of ilogit(w . v) - 28 comparisons - differs by at most 5 standard errors of the difference, computed from the two sets
    of draws (false-alarm rate below 2e-5; profiles/r28_negbin_fold_in_rate.jsonl records 0.00037 against 5 se of 0.00217
    for the same pair of samplers)."""
    rs = np.random.RandomState(5)
    S, R, M, T, K, sweeps = S_STAT, 2, 3, 4, 2, 4
    V = 0.8 * rs.normal(size=(M, T, K))
    Vs = np.ascontiguousarray(np.broadcast_to(V, (S, M, T, K)))
    sigma2 = np.full(S, 1.5)
    rates = np.array([2.0, 3.0])
    Y = rs.randint(0, 29, size=(R, M, T)).astype(float)
    Y[0, 1, 2] = Y[1, 0, 0] = np.nan
    assert np.nanmax(Y + rates[:, None, None]) <= fold_in.MAX_TRIALS
    nb = utils.negbin_fold_in_rows(Y, Vs, sigma2, rate=np.broadcast_to(rates[None, :, None, None], (S, R, 1, 1)), seed=3, sweeps=sweeps,
                                   summary=False)
    bi = utils.fold_in_rows((Y, Y + rates[:, None, None]), Vs, "binomial", sigma2=sigma2, seed=4, inner_sweeps=sweeps, summary=False)
    n = 0
    for name, a, b in (("w", nb["W"], bi["W"]), ("ilogit(w . v)", ilogit(np.einsum("srk,mtk->srmt", nb["W"], V)).reshape(S, R, -1),
                                                 ilogit(np.einsum("srk,mtk->srmt", bi["W"], V)).reshape(S, R, -1))):
        diff = np.abs(a.mean(axis=0) - b.mean(axis=0))
        se = np.sqrt(a.var(axis=0, ddof=1) / S + b.var(axis=0, ddof=1) / S)
        print("%s  largest |difference| %.5f  largest difference / se %.2f" % (name, diff.max(), (diff / se).max()))
        assert np.all(diff <= 5 * se), name
        n += diff.size
    assert n == 28


def test_no_data_with_a_sampled_rate_is_the_prior():
    """4. Every cell nan, rstdev = 1, rpropstdev = 1, nmetropolis = 8, 16 sweeps, S = 4096 independent chains: w has mean 0
    and variance sigma2 per component, and log r is half-normal - the floor cand > 1 truncates the symmetric walk's target
    N(0, 1) - with mean sqrt(2 / pi) and variance 1 - 2 / pi.  Each within 5 standard errors computed from the draws."""
    rs = np.random.RandomState(6)
    S, R, M, T, K = S_STAT, 2, 3, 4, 2
    Vs = rs.normal(size=(S, M, T, K))
    sigma2 = np.full(S, 1.7)
    out = utils.negbin_fold_in_rows(np.full((R, M, T), np.nan), Vs, sigma2, sample_rate=True, rate_init=np.full(S, 2.0), nmetropolis=8,
                                    rpropstdev=1.0, rstdev=1.0, seed=21, sweeps=16, summary=False)

    def within(x, mean, var, label):
        m, v = x.mean(axis=0), x.var(axis=0, ddof=1)
        se_m = np.sqrt(v / S)
        se_v = np.sqrt(((x - m) ** 4).mean(axis=0) - v * v) / np.sqrt(S)
        print("%s  mean %s (want %.4f, se %s)  variance %s (want %.4f, se %s)" % (label, m, mean, se_m, v, var, se_v))
        assert np.all(np.abs(m - mean) <= 5 * se_m) and np.all(np.abs(v - var) <= 5 * se_v), label

    within(out["W"].reshape(S, -1), 0.0, 1.7, "w")
    within(np.log(out["R"]), np.sqrt(2 / np.pi), 1 - 2 / np.pi, "log r")
    assert np.all(out["R"] > 1) and 0 < out["accept"].mean() < 1


def test_sampled_rate_with_data_against_the_numpy_chains():
    """5. (M,T) = (3,4), K = 2, 2 replicates, 8 sweeps, nmetropolis = 4: the means of log r, w and ilogit(w . v) over S = 4096
    device chains against the same finite chain run by chain_rows on 32768 numpy seeds (scripts/negbin_fold_in_rows_rate.py
    --step oracle; tests/golden/negbin_fold_in_rows_oracle.npz).  Bound: 5 combined standard errors plus twice the shift of
    the host stand-in sampler, which the script measures on the CPU between PG_TERMS and 4 PG_TERMS terms."""
    g = load_golden(ORACLE)
    S = S_STAT
    V, Y = g["V"], g["Y"]
    M, T, K = V.shape
    assert (M, T, K) == (3, 4, 2) and Y.shape == (M, T, 2) and int(g["sweeps"]) == 8 and int(g["nmetropolis"]) == 4 and int(g["nchains"]) >= 8192
    assert all(abs(float(g["shift_" + k]) - v) <= 5e-6 for k, v in ORACLE_SHIFT.items())          # the constants above are the stored run's
    Vs = np.ascontiguousarray(np.broadcast_to(V, (S, M, T, K)))
    out = utils.negbin_fold_in_rows(Y[None], Vs, np.full(S, float(g["sigma2"])), sample_rate=True, rate_init=np.full(S, float(g["rate_init"])),
                                    nmetropolis=4, rpropstdev=float(g["rpropstdev"]), rstdev=float(g["rstdev"]), seed=8, sweeps=8,
                                    summary=False)
    W = out["W"][:, 0]
    got = {"logr": np.log(out["R"][:, 0])[:, None], "w": W, "p": ilogit(np.einsum("sk,mtk->smt", W, V)).reshape(S, -1)}
    for name, x in got.items():
        shift = 2 * ORACLE_SHIFT[name]
        se = np.sqrt(x.var(axis=0, ddof=1) / S + g["se_" + name] ** 2)
        diff = np.abs(x.mean(axis=0) - g["mean_" + name])
        print("%s  largest |difference| %.5f  5 se %.5f  allowance for the stand-in sampler %.5f" % (name, diff.max(), 5 * se.max(), shift))
        assert np.all(diff <= 5 * se + shift), name


def test_failure_reporting_and_the_public_forms():
    """6. A non-finite sigma2 in one sample: BTF_ENOTPD with the failing index, nan for that sample, the clean call's bits for
    the others.  The mean of summary=True equals utils.posterior_summary on the same draws.  The model method equals the
    stateless call, and its draws go into posterior_predictive."""
    rs = np.random.RandomState(9)
    S, N, R, M, T, K = 3, 6, 70, 3, 4, 2
    Vs = 0.6 * rs.normal(size=(S, M, T, K))
    sigma2 = np.array([1.0, 2.0, 1.5])
    Y = rs.poisson(4.0, size=(R, M, T)).astype(float)
    Rfit = rs.uniform(2.0, 4.0, size=(S, N, 1, 1))
    q = (5, 50, 95)
    kw = dict(seed=5, sweeps=4, q=q, transform="ilogit")
    clean = utils.negbin_fold_in_rows(Y, Vs, sigma2, R=Rfit, **kw)
    assert np.all(np.isfinite(clean["W"])) and clean["R"].shape == (S, R) and clean["nsamples"] == S
    mean, quant = utils.posterior_summary(clean["W"], Vs, q=q, transform="ilogit")
    np.testing.assert_allclose(mean, clean["mean"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(quant, clean["quantiles"], rtol=0, atol=1e-12)
    for first in (0, 5):
        bad = sigma2.copy()
        bad[1] = np.nan
        with pytest.raises(_native.NotPositiveDefiniteError) as info:
            utils.negbin_fold_in_rows(Y, Vs, bad, R=Rfit, first_sample=first, **kw)
        assert info.value.code == _native.BTF_ENOTPD and info.value.index == (first + 1) * R + 0
        # the C entry point hands the outputs back beside the code: nan for the failing sample, the clean call's bits for the others
        lib, d = _native.load(), _native.dptr
        cnt, ys = nf.cell_statistics(Y, (R, M, T))
        yv, h = nf.row_histograms(Y)
        r0 = nf.resolve_rate_init(None, Rfit, S, R)
        W, Wm, Ro, acc = np.zeros((S, R, K)), np.zeros((S, R, K)), np.zeros((S, R)), np.zeros((S, R))
        rc = lib.btf_negbin_fold_in_rows(0, S, R, M, T, K, d(Vs), d(bad), d(cnt), d(ys), None, 0, 0, 0, 0, d(r0), d(yv), d(h), yv.shape[1], 30,
                                         0.1, 1.0, None, None, None, 5, 4, first, d(W), d(Wm), d(Ro), d(acc), 0, None, 0, None, None)
        assert rc == _native.BTF_ENOTPD and lib.btf_fail_index(None) == (first + 1) * R + 0
        assert np.all(np.isnan(W[1])) and np.all(np.isnan(Wm[1])) and np.all(np.isnan(Ro[1]))
        if first == 0:
            for got, key in ((W, "W"), (Wm, "W_mean"), (Ro, "R"), (acc, "accept")):
                assert np.array_equal(got[[0, 2]], clean[key][[0, 2]]), key
    again = utils.negbin_fold_in_rows(Y, Vs, sigma2, R=Rfit, **kw)                                 # the next call is served
    assert all(np.array_equal(again[k], clean[k]) for k in ("W", "W_mean", "R", "accept", "mean", "quantiles"))
    np.random.seed(0)
    m = NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, rdims=(1, 2), nmetropolis=7, rpropstdev=0.2, rstdev=1.5)
    res = {"W": rs.normal(size=(S, N, K)), "V": Vs, "sigma2": sigma2, "R": Rfit}
    via = m.negbin_fold_in_rows(Y, res, **kw)
    direct = utils.negbin_fold_in_rows(Y, Vs, sigma2, R=Rfit, nmetropolis=7, rpropstdev=0.2, rstdev=1.5, **kw)
    assert all(np.array_equal(via[k], direct[k]) for k in ("W", "W_mean", "R", "accept", "mean", "quantiles"))
    assert not np.array_equal(via["R"], clean["R"])
    pp = utils.posterior_predictive(via["W"], Vs, "negative_binomial", R=via["R"][:, :, None, None], seed=1)
    assert pp["mean"].shape == (R, M, T) and np.all(np.isfinite(pp["mean"]))
