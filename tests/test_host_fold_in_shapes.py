"""The case list of tests/test_gpu_fold_in_shapes.py and its admissibility, on the CPU alone.

The four fold-in kernels (csrc/btf_fold_in.h, btf_fold_in_cols.h, btf_slice_fold.h, btf_slice_fold_cols.h) are one template
each, instantiated for nembeds 1..10 times 2 or 6 families.  This module enumerates the shapes at which they are compared
with their numpy definitions ("Shape passes", the fold-in entry) and builds the inputs of every case; the GPU file
imports both.  Here every case is shown admissible by the reference alone - cond(Q) under the bound its tolerance is stated
for, both decision margins of a replayed slice chain above MARGIN_MIN, finite results, rounds.sum() > 0 - and the list is shown
complete: a case whose inputs are unsafe fails here, it is never dropped.  Inputs are chosen as the existing files choose
them: the first seed of a fixed sequence for which the definition alone meets the condition.  No GPU.

Geometry the cases are derived from: FOLD_PARTS = 4 waves per workgroup of fold_in_kernel (wave p takes the cells p, p + 4,
... under `#pragma unroll 2`), one lane per row and 64 rows per workgroup; SF_CHAINS = 4 chains per workgroup of
slice_fold_kernel, lanes over cells / constraints / features; one wave per chain in fold_cols_kernel and
slice_fold_cols_kernel, lanes over the N rows, over the nD penalty rows (nD = T, 2 T, 3 T - 1 for tf_order 0, 1, 2) and over
the T (tf_order + 2) entries of the prior band; WAVE = 64.
"""
import functools
import os

import numpy as np
import pytest

from functionalmf_amd import _native, fold_in
from functionalmf_amd import fold_in_cols as fc
from functionalmf_amd import slice_fold_in as sf
from functionalmf_amd import utils
from test_gpu_fold_in import COND_MAX as W_COND_MAX
from test_gpu_fold_in import W_TOL, gaussian_problem, numpy_fold_in
from test_gpu_fold_in_cols import COND_MAX as V_COND_MAX
from test_gpu_fold_in_cols import V_TOL, close, numpy_chains
from test_gpu_fold_in_cols import replay_problem as cols_problem
from test_gpu_slice_fold_in import MARGIN_MIN as ROWS_MARGIN_MIN
from test_gpu_slice_fold_in import REPLAY_CASES as ROWS_REPLAY_CASES
from test_gpu_slice_fold_in import replay_inputs as rows_replay_inputs
from test_host_slice_fold_in import FAMILY_NAMES, draw_rows
from test_host_slice_fold_in_cols import MARGIN_MIN as SCOLS_MARGIN_MIN
from test_host_slice_fold_in_cols import REPLAY_CASES as SCOLS_REPLAY_CASES
from test_host_slice_fold_in_cols import definition, safe
from test_host_slice_fold_in_cols import replay_inputs as scols_replay_inputs
from test_host_slice_fold_in_cols import replay_problem as scols_problem

WAVE, FOLD_PARTS, SF_CHAINS = 64, 4, 4
NSEEDS = 50                      # length of every seed sequence below
KS = tuple(range(1, 11))

# ------------------------------------------------------------------------------------------- 1. fold_in_rows, Gaussian, z
# (K, R, (M, T)); every case carries an empty row and a row whose only observed cell is the last one, jt = M T - 1
ROWS_K = [(K, 65, (1, 7)) for K in KS]                                                      # (a) every nembeds, two row blocks
ROWS_CELLS = [(K, 6, MT) for MT in ((1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (2, 4), (3, 3))  # (b) M T = 1, 2, 3, 4, 5, 8, 9:
              for K in (1, 4, 10)]                                                          # waves without a cell, both unroll tails
ROWS_R = [(K, R, (2, 3)) for R in (1, 63, 64, 65, 129) for K in (2, 7)]                     # (c) the clamped loads, a third block
ROWS_CASES = ROWS_K + ROWS_CELLS + ROWS_R
ROWS_BITS = (7, 129, (2, 3))     # the case of the one-row and split-S identities


def gaussian_rows(V0, R, seed, nreps=2):
    """R rows on the curves V0 (M,T,K) with the missing patterns of gaussian_problem by r % 6 (complete, 5 % missing, 90 %
    missing, empty, partial replicates, complete); then row R - 2 is emptied and row R - 1 keeps its last cell alone.
    Returns (Y (R,M,T,nreps), the empty row, the last-cell row)."""
    rs = np.random.RandomState(seed)
    M, T, K = V0.shape
    Y = np.einsum("rk,mtk->rmt", rs.normal(size=(R, K)), V0)[..., None] + rs.normal(0, 0.7, size=(R, M, T, nreps))
    empty, last = R - 2, R - 1
    keep = Y[last, M - 1, T - 1, 0]
    for r in range(R):
        kind = r % 6
        if kind == 1:
            Y[r][rs.uniform(size=(M, T)) < 0.05] = np.nan
        elif kind == 2:
            Y[r][rs.uniform(size=(M, T)) < 0.90] = np.nan
        elif kind == 3:
            Y[r] = np.nan
        elif kind == 4:
            Y[r, :, :, 0][rs.uniform(size=(M, T)) < 0.5] = np.nan
    Y[empty] = np.nan
    Y[last] = np.nan
    Y[last, M - 1, T - 1, 0] = keep
    return Y, empty, last


@functools.lru_cache(maxsize=None)
def rows_case(K, R, MT, S=3):
    """Inputs and the numpy result of one Gaussian row case.  R = 1 cannot hold three kinds of rows in one call: that case
    is three one-row calls (a row of 5 % missing cells, the empty row, the last-cell row), `one_row_calls`."""
    M, T = MT
    nrows = 3 if R == 1 else R
    base = 100000 * K + 100 * R + 10 * M + T
    for k in range(NSEEDS):
        seed = base + 7919 * k
        Vs, nu2, sigma2, _ = gaussian_problem(K, S=S, M=M, T=T, seed=seed)
        Y, empty, last = gaussian_rows(Vs[0], nrows, seed + 1)
        z = np.random.RandomState(seed + 2).normal(size=(S, nrows, K))
        W, Wm, cond = numpy_fold_in(Y, Vs, nu2, sigma2, z)
        if cond.max() < W_COND_MAX and np.all(np.isfinite(W)) and np.abs(W).max() < 10:
            for a in (Vs, Y, z, W, Wm):
                a.setflags(write=False)
            return dict(Vs=Vs, nu2=nu2, sigma2=sigma2, Y=Y, z=z, W=W, Wm=Wm, cond=float(cond.max()), empty=empty, last=last,
                        one_row_calls=R == 1, seed=seed)
    raise AssertionError("no seed with cond(Q) < %g" % W_COND_MAX)


# ------------------------------------------------------------------------------------------- 2. fold_in_rows, Binomial
BINOMIAL_R, BINOMIAL_MT, BINOMIAL_EMPTY = 65, (3, 3), 62


@functools.lru_cache(maxsize=None)
def binomial_case(K, S=3):
    """R = 65 rows of 9 cells with 1..8 trials, about a sixth missing, row 62 empty; no definition to replay (the entry
    point takes no Polya-Gamma variates): the GPU file checks exact properties."""
    rs = np.random.RandomState(300 + K)
    M, T = BINOMIAL_MT
    Vs = 0.8 * rs.normal(size=(S, M, T, K))
    sigma2 = rs.uniform(0.5, 2.0, size=S)
    N = rs.randint(1, 9, size=(BINOMIAL_R, M, T)).astype(float)
    p = utils.ilogit(np.einsum("rk,mtk->rmt", 0.7 * rs.normal(size=(BINOMIAL_R, K)), Vs[0]))
    Y = rs.binomial(N.astype(int), p).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.17] = np.nan
    Y[BINOMIAL_EMPTY] = np.nan
    for a in (Vs, Y, N):
        a.setflags(write=False)
    return dict(Vs=Vs, sigma2=sigma2, Y=Y, N=N)


# ------------------------------------------------------------------------------------------- 3. fold_in_cols, Gaussian, draws
ALL_COLUMNS = (0, 1, 2, 3, 4, 5)
# complete, 30 % missing, 90 % missing, partial replicates.  The empty and the single-cell column of replay_problem hang on
# the prior alone; at the depths of COLS_LEVELS numpy itself meets cond(Q) of 1e10 to 1e14 there, beyond the bound the V
# tolerance is stated for, so they are left out of those cases (and of those cases only).
OBSERVED_COLUMNS = (0, 1, 2, 5)
# (K, tf_order, T, N, columns)
COLS_K = [(K, tf, 9, 70, ALL_COLUMNS) for K in (2, 4, 6, 7, 9) for tf in (0, 1, 2)]        # (a) the nembeds no replay runs
COLS_TINY_N = 1                                                                            # (b) N = 1 at K = 1: a seed passes
COLS_N = [(3, 2, 9, N, ALL_COLUMNS) for N in (6, 63, 64, 65, 128, 129)] + [(1, 2, 9, COLS_TINY_N, ALL_COLUMNS)]
COLS_LEVELS = [(K, tf, T, 70, OBSERVED_COLUMNS) for tf, T in ((0, 65), (1, 33), (2, 23)) for K in (1, 2)]   # (c) second lane pass
COLS_CASES = COLS_K + COLS_N + COLS_LEVELS
COLS_SWEEPS = 2
# Beside the enumeration: the outermost level a reaches tau2 three sweeps after its update (tau2 <- c <- b <- a), so no replay
# of one to three sweeps sees the last line of the level update; one case of four sweeps here and one in SCOLS_DEEP do.
COLS_DEEP, DEEP_SWEEPS = (3, 2, 9, 70, ALL_COLUMNS), 4


def tiny_cols_problem(K, tf_order, T, seed, S=3, N=1, nreps=2):
    """replay_problem of tests/test_gpu_fold_in_cols.py for fewer than six rows: the same six columns, the single observed
    cell of column 4 in the last row (replay_problem puts it in row 5)."""
    rs = np.random.RandomState(seed)
    Ws = rs.normal(size=(S, N, K))
    nu2, lam2 = np.full(S, 0.5), np.full(S, 0.1)
    vt = 0.3 * np.cumsum(rs.normal(size=(6, T, K)), axis=1)
    Y = np.einsum("nk,ctk->cnt", Ws[0], vt)[..., None] + rs.normal(0, 0.7, size=(6, N, T, nreps))
    Y[1][rs.uniform(size=(N, T)) < 0.30] = np.nan
    Y[2][rs.uniform(size=(N, T)) < 0.90] = np.nan
    Y[3] = np.nan
    one = Y[4, N - 1, T // 2, 0]
    Y[4] = np.nan
    Y[4, N - 1, T // 2, 0] = one
    Y[5, :, :, 0][rs.uniform(size=(N, T)) < 0.5] = np.nan
    return Ws, nu2, lam2, Y


@functools.lru_cache(maxsize=None)
def cols_case(K, tf_order, T, N, columns, sweeps=COLS_SWEEPS):
    base = 1000 * K + 100 * tf_order + 10 * T + sweeps + 13 * N
    for k in range(NSEEDS):
        seed = base + 7919 * k
        problem = cols_problem if N >= 6 else tiny_cols_problem
        Ws, nu2, lam2, Y = problem(K, tf_order, T, seed, N=N)
        Y = np.ascontiguousarray(Y[list(columns)])
        draws = fc.random_draws(np.random.RandomState(seed + 1), T, K, tf_order, sweeps, size=(Ws.shape[0], Y.shape[0]))
        V, Vm, T2, cond = numpy_chains(Y, Ws, nu2, lam2, tf_order, sweeps, draws)
        if cond < V_COND_MAX and np.all(np.isfinite(V)) and np.all(np.isfinite(T2)):
            for a in (Ws, Y, draws, V, Vm, T2):
                a.setflags(write=False)
            return dict(Ws=Ws, nu2=nu2, lam2=lam2, Y=Y, draws=draws, V=V, Vm=Vm, T2=T2, cond=float(cond), seed=seed, tries=k + 1)
    raise AssertionError("no seed with cond(Q) < %g" % V_COND_MAX)


# ------------------------------------------------------------------------------------------- 4. slice_fold_in_rows, draws
def _missing_pairs(replayed):
    have = {(c[0], c[1]) for c in replayed}
    return [(f, K) for f in FAMILY_NAMES for K in KS if (f, K) not in have]


# (family, K, (M, T), constrained): (a) the 48 (family, K) pairs no replay runs, cells alternating 21 / 135 and, every other
# pair, the constraints; (b) 1, 2, 63, 64, 65, 128, 129 cells; the constrained gamma-grid cases need T >= 3
SROWS_PAIRS = [(f, K, ((3, 7), (9, 15))[i % 2], (i // 2) % 2 == 1) for i, (f, K) in enumerate(_missing_pairs(ROWS_REPLAY_CASES))]
SROWS_CELL_SHAPES = ((1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (16, 8), (3, 43))
SROWS_CELLS = [("poisson_identity", 4, MT, False) for MT in SROWS_CELL_SHAPES] + \
              [("gamma_grid", 2, MT, True) for MT in SROWS_CELL_SHAPES if MT[1] >= 3]
SROWS_CASES = SROWS_PAIRS + SROWS_CELLS
SROWS_FEATURES = (1, 63, 64, 65)                                                           # (c) F, lanes over f


def _rows_safe(want):
    return min(want["margin_ll"], want["margin_slack"]) > ROWS_MARGIN_MIN and np.all(np.isfinite(want["W"])) and \
        want["rounds"].sum() > 0


@functools.lru_cache(maxsize=None)
def srows_case(family, K, MT, constrained):
    for seed in range(NSEEDS):
        c = rows_replay_inputs(family, K, MT, constrained, seed)
        if _rows_safe(c["want"]):
            c["seed"] = seed
            for a in (c["Vs"], c["Y"], c["draws"], c["want"]["W"]):
                a.setflags(write=False)
            return c
    raise AssertionError("no seed with margins above %g" % ROWS_MARGIN_MIN)


@functools.lru_cache(maxsize=None)
def features_case(F, K=3, MT=(3, 7), S=3, R=3, sweeps=3, max_rounds=40):
    """poisson_identity rows with F binary features, about a fifth of the (row, feature) pairs missing: U ~ U(0.05, 0.6),
    every chain started at w = 0.3 (0 <= w . u_f <= 0.54); rows complete, half missing, empty (its features alone)."""
    M, T = MT
    for seed in range(NSEEDS):
        rs = np.random.RandomState(1000 * seed + F)
        falls = np.stack([np.linspace(1.0, 0.3 + 0.05 * k, T) for k in range(K)], axis=-1)
        Vs = 3.0 * rs.uniform(0.5, 1.5, size=(S, M, 1, K)) * falls[None, None]
        sigma2 = np.array([0.5, 1.0, 2.0])[:S] / K
        Us = rs.uniform(0.05, 0.6, size=(S, F, K))
        X = (rs.uniform(size=(R, F)) < 0.5).astype(float)
        X[rs.uniform(size=(R, F)) < 0.2] = np.nan
        w_true = rs.uniform(0.5, 1.0, size=(R, K)) / K
        Y = draw_rows("poisson_identity", None, np.einsum("rk,mtk->rmt", w_true, Vs[0]), 2, rs)
        Y[1][rs.uniform(size=Y[1].shape) < 0.5] = np.nan
        Y[2] = np.nan
        start = np.full(K, 0.3)
        rec = sf.record_length(K, max_rounds)
        draws = np.concatenate([rs.normal(size=(S, R, sweeps, K)), rs.uniform(size=(S, R, sweeps, rec - K))], axis=-1)
        codes = sf.feature_codes(X)
        _, S1, cnt, L = sf.row_statistics(Y, "poisson_identity", M, T)
        want = sf.chains(np.broadcast_to(start, (S, R, K)), Vs, sigma2, "poisson_identity", None, (S1, cnt, L), None, None, Us=Us,
                         x_codes=codes, draws=draws, sweeps=sweeps, max_rounds=max_rounds)
        if _rows_safe(want):
            for a in (Vs, Us, X, Y, draws, want["W"]):
                a.setflags(write=False)
            return dict(Vs=Vs, sigma2=sigma2, Us=Us, X=X, Y=Y, start=start, draws=draws, want=want, sweeps=sweeps, seed=seed,
                        Cons=None, Rc=None, param=None)
    raise AssertionError("no seed with margins above %g" % ROWS_MARGIN_MIN)


# ------------------------------------------------------------------------------------------- 5. slice_fold_in_cols, draws
# (family, K, tf_order, T, constrained, N): (a) the 48 missing pairs at S = 2, N = 65, tf_order cycling 0, 1, 2, T alternating
# 6 / 9, the constraints every other pair; (b) N = 63, 64, 129 at a constrained and an unconstrained pair
SCOLS_PAIRS = [(f, K, i % 3, (6, 9)[i % 2], (i // 2) % 2 == 1, 65) for i, (f, K) in enumerate(_missing_pairs(SCOLS_REPLAY_CASES))]
SCOLS_N = [(f, K, 2, 9, constrained, N) for N in (63, 64, 129) for f, K, constrained in (("poisson_identity", 3, True), ("gaussian", 4, False))]
SCOLS_CASES = SCOLS_PAIRS + SCOLS_N
# (family, K, tf_order, T, constrained, fixed scales): (c) the second lane pass of the level loops (tf 2: nD = 68, T (tf + 2)
# = 92; tf 0: nD = 65, T (tf + 2) = 130), on the complete and the half-missing column only (the single-cell and the empty column
# are beyond cond(Q) = 1e9 at these depths, as in COLS_LEVELS).  K = 1 Gaussian without constraints, K = 2 poisson_identity
# with them at T = 23 and without at T = 65: the 129 constraints of that depth on 70 rows leave the definition's smallest slack
# near 1e-7 at every seed, under MARGIN_MIN, and the feasibility loop runs over rows, not depths
SCOLS_LEVELS = [(("gaussian", "poisson_identity")[K - 1], K, tf, T, K == 2 and T == 23, fixed)
                for tf, T in ((2, 23), (0, 65)) for K in (1, 2) for fixed in (False, True)]
SCOLS_S = 2
SCOLS_DEEP = ("poisson_identity", 3, 2, 9, True, 65)     # at DEEP_SWEEPS sweeps (COLS_DEEP)


@functools.lru_cache(maxsize=None)
def scols_case(family, K, tf_order, T, constrained, N, sweeps=3):
    c = scols_replay_inputs(family, K, tf_order, T, constrained, S=SCOLS_S, N=N, sweeps=sweeps)
    for a in (c["Ws"], c["Y"], c["draws"], c["want"]["V"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def scols_levels_case(family, K, tf_order, T, constrained, fixed):
    base = 1000 * K + 100 * tf_order + 10 * T + (5 if constrained else 0)
    for k in range(NSEEDS):
        c = scols_problem(family, K, tf_order, T, constrained, base + 7919 * k, S=SCOLS_S, fixed=fixed)
        c["Y"], c["start"], c["draws"] = np.ascontiguousarray(c["Y"][:2]), c["start"][:2], np.ascontiguousarray(c["draws"][:, :2])
        if fixed:
            c["tau2"] = c["tau2"][:2]
        want = definition(c)
        if safe(want) and want["rounds"].sum() > 0:
            c["want"] = want
            for a in (c["Ws"], c["Y"], c["draws"], want["V"]):
                a.setflags(write=False)
            return c
    raise AssertionError("no seed with cond(Q) <= 1e9 and margins above %g" % SCOLS_MARGIN_MIN)


# ------------------------------------------------------------------------------------------- 6. failure reports
FAIL_FIRST_SAMPLES = (0, 5)


@functools.lru_cache(maxsize=None)
def rows_failure_case():
    """S = 3, R = 70; `bad` is Vs with one nan in sample 1 and one in sample 2 (0 v = nan for every row, observed or not:
    every row of those samples fails, the smallest index is sample 1, row 0)."""
    Vs, nu2, sigma2, _ = gaussian_problem(3, S=3, M=2, T=5, seed=61)
    Y, _, _ = gaussian_rows(Vs[0], 70, 62)
    bad = Vs.copy()
    bad[1, 1, 2, 0] = np.nan
    bad[2, 0, 4, 2] = np.nan
    return dict(Vs=Vs, bad=bad, nu2=nu2, sigma2=sigma2, Y=Y, z=np.random.RandomState(63).normal(size=(3, 70, 3)))


@functools.lru_cache(maxsize=None)
def cols_failure_case():
    """S = 3, C = 3, N = 70, T = 9, K = 3, tf_order 2; `bad` is Ws with one nan in sample 1."""
    Ws, nu2, lam2, Y = cols_problem(3, 2, 9, 71)
    bad = Ws.copy()
    bad[1, 17, 1] = np.nan
    return dict(Ws=Ws, bad=bad, nu2=nu2, lam2=lam2, Y=np.ascontiguousarray(Y[:3]), tf_order=2, sweeps=2)


# ------------------------------------------------------------------------------------------------------------------ tests
def test_the_list_is_the_enumeration():
    """Every group holds exactly the cases it is meant to hold: nothing dropped, nothing twice."""
    assert len(ROWS_CASES) == len(set(ROWS_CASES)) == 10 + 21 + 10
    assert {c[0] for c in ROWS_K} == set(KS) and {c[1:] for c in ROWS_K} == {(65, (1, 7))}
    assert {(c[0], c[2][0] * c[2][1]) for c in ROWS_CELLS} == {(K, n) for K in (1, 4, 10) for n in (1, 2, 3, 4, 5, 8, 9)}
    assert {c[1] for c in ROWS_CELLS} == {6}
    assert {(c[0], c[1]) for c in ROWS_R} == {(K, R) for K in (2, 7) for R in (1, 63, 64, 65, 129)} and {c[2] for c in ROWS_R} == {(2, 3)}
    assert ROWS_BITS in ROWS_CASES
    assert len(COLS_CASES) == len(set(COLS_CASES)) == 15 + 7 + 6
    assert {c[:3] for c in COLS_K} == {(K, tf, 9) for K in (2, 4, 6, 7, 9) for tf in (0, 1, 2)}
    assert all(c[3] == 70 and c[4] == ALL_COLUMNS for c in COLS_K)
    assert sorted(c[3] for c in COLS_N) == [1, 6, 63, 64, 65, 128, 129] and all(c[4] == ALL_COLUMNS for c in COLS_N)
    assert {c[:3] for c in COLS_N if c[3] >= 6} == {(3, 2, 9)} and {c[:3] for c in COLS_N if c[3] < 6} == {(1, 2, 9)}
    assert {c[:3] for c in COLS_LEVELS} == {(K, tf, T) for tf, T in ((0, 65), (1, 33), (2, 23)) for K in (1, 2)}
    assert all(c[4] == OBSERVED_COLUMNS for c in COLS_LEVELS)
    every = {(f, K) for f in FAMILY_NAMES for K in KS}
    for pairs, replayed in ((SROWS_PAIRS, ROWS_REPLAY_CASES), (SCOLS_PAIRS, SCOLS_REPLAY_CASES)):
        got = [(c[0], c[1]) for c in pairs]
        assert len(got) == len(set(got)) == 48
        assert set(got) | {(c[0], c[1]) for c in replayed} == every and not set(got) & {(c[0], c[1]) for c in replayed}
    assert {(c[2], c[3]) for c in SROWS_PAIRS} == {((3, 7), False), ((3, 7), True), ((9, 15), False), ((9, 15), True)}
    assert [c[2][0] * c[2][1] for c in SROWS_CELLS if c[0] == "poisson_identity"] == [1, 2, 63, 64, 65, 128, 129]
    assert [c[2][0] * c[2][1] for c in SROWS_CELLS if c[0] == "gamma_grid"] == [63, 64, 65, 128, 129]
    assert {c[:2] + c[3:] for c in SROWS_CELLS} == {("poisson_identity", 4, False), ("gamma_grid", 2, True)}
    assert len(SROWS_CASES) == len(set(SROWS_CASES)) == 48 + 12
    assert {c[2] for c in SCOLS_PAIRS} == {0, 1, 2} and {c[3] for c in SCOLS_PAIRS} == {6, 9} and {c[4] for c in SCOLS_PAIRS} == {False, True}
    assert {c[5] for c in SCOLS_PAIRS} == {65}
    assert sorted(c[5] for c in SCOLS_N) == [63, 63, 64, 64, 129, 129] and {c[4] for c in SCOLS_N} == {False, True}
    assert len(SCOLS_CASES) == len(set(SCOLS_CASES)) == 48 + 6
    assert {c[1:4] + c[5:] for c in SCOLS_LEVELS} == {(K, tf, T, fx) for tf, T in ((2, 23), (0, 65)) for K in (1, 2) for fx in (False, True)}
    assert len(SCOLS_LEVELS) == 8


def test_the_cases_sit_on_the_edges_they_are_meant_for():
    """The geometry constants, restated from the headers, against the shapes of the list."""
    src = open(os.path.join(_native.CSRC, "btf_fold_in.h")).read()
    assert "constexpr int FOLD_PARTS = %d;" % FOLD_PARTS in src and "#pragma unroll 2" in src
    src = open(os.path.join(_native.CSRC, "btf_slice_fold.h")).read()
    assert "constexpr int SF_CHAINS = %d;" % SF_CHAINS in src
    cells = sorted({c[2][0] * c[2][1] for c in ROWS_CELLS})
    assert min(cells) < FOLD_PARTS and FOLD_PARTS in cells                    # waves without a cell; one cell each
    assert {-(-(n - p) // FOLD_PARTS) % 2 for n in cells for p in range(FOLD_PARTS) if n > p} == {0, 1}   # both unroll tails
    assert {WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1} <= {c[1] for c in ROWS_R}
    for K, tf, T, N, _ in COLS_LEVELS:
        nD = fc.penalty(T, tf).shape[0]
        assert nD == (T, 2 * T, 3 * T - 1)[tf]
        assert nD > WAVE and T * (tf + 2) > WAVE                              # a second pass of both lane loops
    for _, K, tf, T, _, _ in SCOLS_LEVELS:
        assert fc.penalty(T, tf).shape[0] > WAVE and T * (tf + 2) > WAVE
    for K, tf, T, N, _ in COLS_K + COLS_N:
        assert fc.penalty(T, tf).shape[0] <= WAVE
    assert (3 * 3) % SF_CHAINS == 1                                           # S R = 9 chains: a last workgroup with one


@pytest.mark.parametrize("case", ROWS_CASES)
def test_gaussian_row_cases_are_admissible(case):
    K, R, MT = case
    c = rows_case(*case)
    nrows = 3 if R == 1 else R
    assert c["Y"].shape[:3] == (nrows,) + MT and c["Vs"].shape[1:] == MT + (K,) and 2 <= c["Vs"].shape[0] <= 3
    assert c["cond"] < W_COND_MAX and np.all(np.isfinite(c["W"])) and np.all(np.isfinite(c["Wm"])) and np.abs(c["W"]).max() < 10
    obs = ~np.isnan(c["Y"])
    assert not obs[c["empty"]].any()
    assert obs[c["last"]].sum() == 1 and obs[c["last"], MT[0] - 1, MT[1] - 1].any()
    assert np.all(c["Wm"][:, c["empty"]] == 0.0)


@pytest.mark.parametrize("K", KS)
def test_binomial_row_cases_are_admissible(K):
    c = binomial_case(K)
    R, n, y = fold_in.row_statistics((c["Y"], c["N"]), "binomial", *BINOMIAL_MT)
    assert R == BINOMIAL_R and BINOMIAL_MT[0] * BINOMIAL_MT[1] == 9 and not n[BINOMIAL_EMPTY].any() and n[0].any() and n[64].any()
    fold_in.check_args("binomial", c["Vs"].shape[0], R, K, summary=False, inner_sweeps=1)


@pytest.mark.parametrize("case", COLS_CASES)
def test_column_cases_are_admissible(case):
    K, tf, T, N, columns = case
    c = cols_case(*case, sweeps=COLS_SWEEPS)
    print("K=%d tf=%d T=%d N=%d columns=%r: seed %d (try %d), max cond(Q) %.2e" % (K, tf, T, N, columns, c["seed"], c["tries"], c["cond"]))
    assert c["Ws"].shape == (3, N, K) and c["Y"].shape[:3] == (len(columns), N, T)
    assert c["cond"] < V_COND_MAX and np.all(np.isfinite(c["V"])) and np.all(np.isfinite(c["Vm"])) and np.all(c["T2"] > 0)
    fc.check_args("gaussian", 3, len(columns), T, K, tf, c["draws"], COLS_SWEEPS, summary=False)


def test_the_four_sweep_cases_are_admissible():
    c = cols_case(*COLS_DEEP, sweeps=DEEP_SWEEPS)
    assert c["cond"] < V_COND_MAX and np.all(np.isfinite(c["V"])) and np.all(c["T2"] > 0)
    assert c["draws"].shape[-1] == fc.draws_length(COLS_DEEP[2], COLS_DEEP[0], COLS_DEEP[1], DEEP_SWEEPS)
    want = scols_case(*SCOLS_DEEP, sweeps=DEEP_SWEEPS)["want"]
    assert safe(want) and want["rounds"].sum() > 0
    assert COLS_DEEP not in COLS_CASES or DEEP_SWEEPS != COLS_SWEEPS


@pytest.mark.parametrize("case", SROWS_CASES)
def test_slice_row_cases_are_admissible(case):
    c = srows_case(*case)
    want = c["want"]
    assert min(want["margin_ll"], want["margin_slack"]) > ROWS_MARGIN_MIN, (want["margin_ll"], want["margin_slack"])
    assert np.all(np.isfinite(want["W"])) and want["rounds"].sum() > 0
    assert c["Vs"].shape[1:] == case[2] + (case[1],) and (c["Cons"] is not None) == case[3]


@pytest.mark.parametrize("F", SROWS_FEATURES)
def test_feature_cases_are_admissible(F):
    c = features_case(F)
    want = c["want"]
    assert min(want["margin_ll"], want["margin_slack"]) > ROWS_MARGIN_MIN, (want["margin_ll"], want["margin_slack"])
    assert np.all(np.isfinite(want["W"])) and want["rounds"].sum() > 0
    assert c["Us"].shape == (3, F, 3) and c["X"].shape == (3, F)
    assert np.all(c["Us"] @ c["start"] >= 0) and np.all(c["Us"] @ c["start"] <= 1)
    if F > 1:
        assert np.isnan(c["X"]).any() and (c["X"] == 0).any() and (c["X"] == 1).any()


@pytest.mark.parametrize("case", SCOLS_CASES)
def test_slice_column_cases_are_admissible(case):
    c = scols_case(*case)
    want = c["want"]
    assert safe(want) and want["rounds"].sum() > 0, (want["cond"], want["margin_ll"], want["margin_slack"])
    assert c["Ws"].shape == (SCOLS_S, case[5], case[1]) and c["Y"].shape[0] == 4 and (c["Cons"] is not None) == case[4]


@pytest.mark.parametrize("case", SCOLS_LEVELS)
def test_slice_column_level_cases_are_admissible(case):
    c = scols_levels_case(*case)
    want = c["want"]
    assert safe(want) and want["rounds"].sum() > 0, (want["cond"], want["margin_ll"], want["margin_slack"])
    assert c["Y"].shape[0] == 2 and (c["tau2"] is not None) == case[5] and (c["Cons"] is not None) == case[4]
    if case[5]:
        assert np.array_equal(want["Tau2"], np.broadcast_to(c["tau2"], want["Tau2"].shape))


def test_failure_cases_hold_what_they_say():
    r = rows_failure_case()
    assert r["Vs"].shape[0] == 3 and r["Y"].shape[0] == 70
    assert np.isnan(r["bad"][1]).sum() == 1 and np.isnan(r["bad"][2]).sum() == 1 and np.array_equal(r["bad"][0], r["Vs"][0])
    _, _, cond = numpy_fold_in(r["Y"], r["Vs"], r["nu2"], r["sigma2"])
    assert cond.max() < W_COND_MAX                                            # the clean call is an ordinary one
    c = cols_failure_case()
    assert c["Ws"].shape[0] == 3 and c["Y"].shape[0] == 3 and c["Ws"].shape[1] == 70
    assert np.isnan(c["bad"][1]).sum() == 1 and not np.isnan(c["bad"][[0, 2]]).any()


def test_tolerances_are_the_projects_own():
    assert W_TOL == 1e-10 and W_COND_MAX == 1e4 and V_TOL == 1e-6 and V_COND_MAX == 1e9
    assert ROWS_MARGIN_MIN == 1e-6 and SCOLS_MARGIN_MIN == 2e-6
    assert close(np.array([2.0 + 1e-6]), np.array([2.0])) and not close(np.array([1.0 + 3e-6]), np.array([1.0]))
