"""The four fold-in kernels (csrc/btf_fold_in.h, btf_fold_in_cols.h, btf_slice_fold.h, btf_slice_fold_cols.h) at every
nembeds, block edge and cell count, against their numpy definitions on supplied variates.

The cases, their inputs and the numpy results come from tests/test_host_fold_in_shapes.py, which shows on the CPU that
every case is admissible and that the list is complete.  Tolerances and the conditions attached to them are those of the
kernels' own test files: W to 1e-10 with cond(Q) < 1e4, V to 1e-6 max(1, |V|) with cond(Q) < 1e9, the slice chains with
rounds and unfinished equal and both decision margins above MARGIN_MIN.  The Binomial row kernel takes no supplied
variates: exact properties there.  The last group reaches the two documented failure reports of the Gaussian kernels
(BTF_ENOTPD of fold_in_rows, BTF_ESTATE of fold_in_cols) through non-finite states.
"""
import numpy as np
import pytest

from functionalmf_amd import _native, utils
from functionalmf_amd import fold_in
from functionalmf_amd import fold_in_cols as fc
from test_gpu_fold_in import COND_MAX as W_COND_MAX
from test_gpu_fold_in import W_TOL
from test_gpu_fold_in_cols import COND_MAX as V_COND_MAX
from test_gpu_fold_in_cols import V_TOL, close
from test_gpu_slice_fold_in import MARGIN_MIN as ROWS_MARGIN_MIN
from test_gpu_slice_fold_in import W_TOL as SLICE_W_TOL
from test_gpu_slice_fold_in import _call as rows_call
from test_gpu_slice_fold_in_cols import _check_replay
from test_host_fold_in_shapes import (BINOMIAL_EMPTY, COLS_CASES, COLS_DEEP, COLS_SWEEPS, DEEP_SWEEPS, FAIL_FIRST_SAMPLES, KS, ROWS_BITS,
                                      ROWS_CASES, SCOLS_CASES, SCOLS_DEEP, SCOLS_LEVELS, SROWS_CASES, SROWS_FEATURES, binomial_case,
                                      cols_case, cols_failure_case, features_case, rows_case, rows_failure_case, scols_case,
                                      scols_levels_case, srows_case)

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ------------------------------------------------------------------------------------------- 1. fold_in_rows, Gaussian, z
def _rows(c, rows=slice(None), samples=slice(None), **kw):
    args = dict(nu2=c["nu2"][samples], sigma2=c["sigma2"][samples], summary=False)
    args.update(kw)
    return utils.fold_in_rows(c["Y"][rows], c["Vs"][samples], "gaussian", **args)


@pytest.mark.parametrize("case", ROWS_CASES)
def test_gaussian_rows_equal_numpy(case):
    """1. W and W_mean against fold_in.conditional / draw: K = 1..10 at R = 65 and 7 cells; 1, 2, 3, 4, 5, 8, 9 cells (waves of
    the workgroup without a cell, odd and even trip counts of the unrolled cell loop) at K = 1, 4, 10; R = 1, 63, 64, 65, 129
    at K = 2, 7.  Every case holds an empty row and a row observed in its last cell alone."""
    c = rows_case(*case)
    if c["one_row_calls"]:
        outs = [_rows(c, rows=slice(r, r + 1), z=c["z"][:, r:r + 1]) for r in range(c["Y"].shape[0])]
        out = {k: np.concatenate([o[k] for o in outs], axis=1) for k in ("W", "W_mean")}
    else:
        out = _rows(c, z=c["z"])
    errw, errm = np.abs(out["W"] - c["W"]).max(), np.abs(out["W_mean"] - c["Wm"]).max()
    print("ERR rows K=%d R=%d cells=%d: W %.3e  W_mean %.3e  (tol %.0e)  max cond(Q) %.1f  max|w| %.2f"
          % (case[0], case[1], case[2][0] * case[2][1], errw, errm, W_TOL, c["cond"], np.abs(c["W"]).max()))
    assert c["cond"] < W_COND_MAX
    assert errm < W_TOL
    assert errw < W_TOL
    e = c["empty"]
    assert np.all(out["W_mean"][:, e] == 0.0)
    np.testing.assert_allclose(out["W"][:, e], c["z"][:, e] * np.sqrt(c["sigma2"])[:, None], rtol=0, atol=W_TOL)


def test_gaussian_rows_same_bits():
    """1. Rows 0, 63, 64 and 128 of the R = 129 call equal the four one-row calls (first and last lane of a block, first
    lane of the second and third), and the two parts of S with first_sample equal the whole call, bit for bit."""
    c = rows_case(*ROWS_BITS)
    full = _rows(c, z=c["z"])
    for r in (0, 63, 64, 128):
        one = _rows(c, rows=slice(r, r + 1), z=c["z"][:, r:r + 1])
        assert np.array_equal(one["W"][:, 0], full["W"][:, r]) and np.array_equal(one["W_mean"][:, 0], full["W_mean"][:, r]), r
    whole = _rows(c, seed=5)
    lo = _rows(c, samples=slice(0, 1), seed=5)
    hi = _rows(c, samples=slice(1, None), seed=5, first_sample=1)
    assert np.all(np.isfinite(whole["W"])) and not np.array_equal(whole["W"], full["W"])
    assert np.array_equal(np.concatenate([lo["W"], hi["W"]]), whole["W"])
    assert np.array_equal(np.concatenate([lo["W_mean"], hi["W_mean"]]), whole["W_mean"])
    assert np.array_equal(whole["W_mean"], full["W_mean"])


# ------------------------------------------------------------------------------------------- 2. fold_in_rows, Binomial
@pytest.mark.parametrize("K", KS)
def test_binomial_rows_exact_properties(K):
    """2. fold_in_kernel<K, Binomial> at K = 1..10, R = 65 (row 62 empty), 9 cells; the entry point takes no variates for
    this family, so: finite; the same bits from two calls, from S split with first_sample, and for rows 0, 63, 64 alone.
    The generator stream of a row is keyed by its index in the call, so a row other than 0 is alone in a call that keeps its
    index: the rows before it emptied, the rows after it cut off.  With inner_sweeps = 1 the empty row is, bit for bit, the
    empty row of the Gaussian call with the same seed, sigma2 and first_sample: both are sqrt(sigma2) times
    philox_normal(seed, stream, k) on an accumulation of exact zeros."""
    c = binomial_case(K)
    Y, N, Vs, s2 = c["Y"], c["N"], c["Vs"], c["sigma2"]
    kw = dict(seed=40 + K, summary=False)
    a = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, **kw)
    assert a["W"].shape == (Vs.shape[0], 65, K) and np.all(np.isfinite(a["W"])) and "W_mean" not in a
    b = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, **kw)
    assert np.array_equal(a["W"], b["W"])
    assert not np.array_equal(a["W"], utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, seed=41 + K, summary=False)["W"])
    lo = utils.fold_in_rows((Y, N), Vs[:1], "binomial", sigma2=s2[:1], **kw)
    hi = utils.fold_in_rows((Y, N), Vs[1:], "binomial", sigma2=s2[1:], first_sample=1, **kw)
    assert np.array_equal(np.concatenate([lo["W"], hi["W"]]), a["W"])
    one = utils.fold_in_rows((Y[:1], N[:1]), Vs, "binomial", sigma2=s2, **kw)
    assert np.array_equal(one["W"][:, 0], a["W"][:, 0])
    for r in (63, 64):
        Yr = np.full((r + 1,) + Y.shape[1:], np.nan)
        Yr[r] = Y[r]
        alone = utils.fold_in_rows((Yr, N[:r + 1]), Vs, "binomial", sigma2=s2, **kw)
        assert np.array_equal(alone["W"][:, r], a["W"][:, r]), r
    head = utils.fold_in_rows((Y[:64], N[:64]), Vs, "binomial", sigma2=s2, **kw)          # one block of rows against two
    assert np.array_equal(head["W"], a["W"][:, :64])
    e = BINOMIAL_EMPTY
    bn = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, inner_sweeps=1, first_sample=3, **kw)
    Yg = np.where(np.isnan(Y), np.nan, 0.5)
    ga = utils.fold_in_rows(Yg, Vs, "gaussian", nu2=np.ones(Vs.shape[0]), sigma2=s2, first_sample=3, **kw)
    assert np.all(ga["W_mean"][:, e] == 0.0) and np.all(bn["W"][:, e] != 0.0)
    assert np.array_equal(bn["W"][:, e], ga["W"][:, e])


# ------------------------------------------------------------------------------------------- 3. fold_in_cols, Gaussian, draws
def _check_columns(case, sweeps):
    K, tf, T, N, columns = case
    c = cols_case(*case, sweeps=sweeps)
    out = utils.fold_in_cols(c["Y"], c["Ws"], "gaussian", nu2=c["nu2"], lam2=c["lam2"], tf_order=tf, draws=c["draws"], sweeps=sweeps,
                             summary=False)
    errt = float(np.max(np.abs(out["Tau2"] - c["T2"]) / c["T2"]))
    print("ERR cols K=%d tf=%d T=%d N=%d ncols=%d sweeps=%d: V %.3e  V_mean %.3e  Tau2 %.3e  (tol %.0e)  max cond(Q) %.2e  max|V| %.2f"
          % (K, tf, T, N, len(columns), sweeps, _rel(out["V"], c["V"]), _rel(out["V_mean"], c["Vm"]), errt, V_TOL, c["cond"],
             np.abs(c["V"]).max()))
    assert c["cond"] < V_COND_MAX
    assert close(out["V_mean"], c["Vm"])
    assert close(out["V"], c["V"])
    assert errt <= V_TOL
    if 3 in columns:
        assert np.all(out["V_mean"][:, columns.index(3)] == 0.0)                # the empty column: the prior's mean


@pytest.mark.parametrize("case", COLS_CASES)
def test_columns_equal_numpy_chain(case):
    """3. V, V_mean and Tau2 against fold_in_cols.chain on supplied draws, 2 sweeps, S = 3: K = 2, 4, 6, 7, 9 at every
    tf_order (T = 9, N = 70, six columns); N = 1, 6, 63, 64, 65, 128, 129; (tf_order, T) = (0, 65), (1, 33), (2, 23), where
    the level loops, the 1 / (lam2 tau2) loop and the prior-band loop make a second lane pass (the four observed columns:
    the empty and the single-cell column are beyond cond(Q) = 1e9 there in numpy itself)."""
    _check_columns(case, COLS_SWEEPS)


@pytest.mark.parametrize("kernel", ["fold_cols", "slice_fold_cols"])
def test_every_level_update_reaches_the_output(kernel):
    """3 and 5, beside the enumeration.  The outermost level a reaches tau2 three sweeps after its update (tau2 <- c <- b <- a):
    replays of one to three sweeps never see the last line of the level update.  One case of four sweeps per column kernel."""
    if kernel == "fold_cols":
        _check_columns(COLS_DEEP, DEEP_SWEEPS)
    else:
        _check_replay(scols_case(*SCOLS_DEEP, sweeps=DEEP_SWEEPS), "ERR scols-deep %s K=%d tf=%d T=%d constrained=%s N=%d" % SCOLS_DEEP)


# ------------------------------------------------------------------------------------------- 4. slice_fold_in_rows, draws
def _check_rows(c, family, label, **kw):
    want = c["want"]
    assert min(want["margin_ll"], want["margin_slack"]) > ROWS_MARGIN_MIN, (want["margin_ll"], want["margin_slack"])
    assert np.all(np.isfinite(want["W"])) and want["rounds"].sum() > 0
    out = utils.slice_fold_in_rows(c["Y"], c["Vs"], family, **rows_call(c, draws=c["draws"], **kw))
    err = np.abs(out["W"] - want["W"]).max()
    print("ERR srows %s: W %.3e  (tol %.0e)  rounds %d  unfinished %d  margins %.2e %.2e"
          % (label, err, SLICE_W_TOL, want["rounds"].sum(), want["unfinished"].sum(), want["margin_ll"], want["margin_slack"]))
    assert np.array_equal(out["rounds"], want["rounds"]) and np.array_equal(out["unfinished"], want["unfinished"])
    assert err < SLICE_W_TOL
    assert np.array_equal(out["W_start"], np.broadcast_to(c["start"], out["W"].shape))


@pytest.mark.parametrize("case", SROWS_CASES)
def test_slice_rows_equal_the_definition(case):
    """4. W, rounds and unfinished against slice_fold_in.chains on supplied draws: the 48 (family, K) pairs the replay of
    tests/test_gpu_slice_fold_in.py leaves out, and 1, 2, 63, 64, 65, 128, 129 cells (lanes over cells: under one stride, one
    exactly, a tail of one; two; two and one) without constraints and, from T = 3 on, with them."""
    family, K, MT, constrained = case
    _check_rows(srows_case(*case), family, "%s K=%d cells=%d constrained=%s" % (family, K, MT[0] * MT[1], constrained))


@pytest.mark.parametrize("F", SROWS_FEATURES)
def test_slice_rows_with_features_equal_the_definition(F):
    """4. The row-feature loops (feasibility 0 <= w . u_f <= 1 and the feature term, lanes over f) at F = 1, 63, 64, 65
    against slice_fold_in.chains(..., Us=, x_codes=): K = 3, poisson_identity, a fifth of the pairs missing."""
    c = features_case(F)
    _check_rows(c, "poisson_identity", "features F=%d" % F, row_features=c["X"], Us=c["Us"])


# ------------------------------------------------------------------------------------------- 5. slice_fold_in_cols, draws
@pytest.mark.parametrize("case", SCOLS_CASES)
def test_slice_columns_equal_the_definition(case):
    """5. What the replay of tests/test_gpu_slice_fold_in_cols.py compares (rounds and unfinished equal, V and Tau2 within
    1e-6), at the 48 (family, K) pairs it leaves out (S = 2, N = 65) and at N = 63, 64, 129."""
    _check_replay(scols_case(*case), "ERR scols %s K=%d tf=%d T=%d constrained=%s N=%d" % case)


@pytest.mark.parametrize("case", SCOLS_LEVELS)
def test_slice_columns_second_pass_of_the_level_loops(case):
    """5. (tf_order, T) = (2, 23) and (0, 65), K = 1, 2, sampled and fixed scales: nD and T (tf_order + 2) beyond 64."""
    c = scols_levels_case(*case)
    out = _check_replay(c, "ERR scols-levels %s K=%d tf=%d T=%d constrained=%s fixed=%s" % case)
    if case[5]:
        assert np.array_equal(out["Tau2"], np.broadcast_to(c["tau2"], out["Tau2"].shape))


# ------------------------------------------------------------------------------------------- 6. failure reports
@pytest.mark.parametrize("first_sample", FAIL_FIRST_SAMPLES)
def test_fold_in_rows_names_the_first_failing_pair(first_sample):
    """6. A nan in Vs[1] and one in Vs[2] (S = 3, R = 70): NotPositiveDefiniteError with index (first_sample + 1) R + 0, the
    smallest failing sample * R + row over two blocks of rows and two samples; through the C entry point BTF_ENOTPD with
    sample 0 equal to the clean call bit for bit and nan in samples 1 and 2.  The documented error return of the Gaussian
    kernel, which has no data-dependent loop; nothing faults."""
    c = rows_failure_case()
    S, R, K = c["z"].shape
    M, T = c["Vs"].shape[1:3]
    kw = dict(nu2=c["nu2"], sigma2=c["sigma2"], z=c["z"], summary=False, first_sample=first_sample)
    clean = utils.fold_in_rows(c["Y"], c["Vs"], "gaussian", **kw)
    assert np.all(np.isfinite(clean["W"]))
    with pytest.raises(_native.NotPositiveDefiniteError) as info:
        utils.fold_in_rows(c["Y"], c["bad"], "gaussian", **kw)
    assert info.value.code == _native.BTF_ENOTPD and info.value.index == (first_sample + 1) * R + 0
    lib = _native.load()
    _, cnt, ysum = fold_in.row_statistics(c["Y"], "gaussian", M, T)
    W, Wm = np.zeros((S, R, K)), np.zeros((S, R, K))
    d = _native.dptr
    rc = lib.btf_fold_in_rows(0, 0, S, R, M, T, K, d(c["bad"]), d(c["nu2"]), d(c["sigma2"]), d(cnt), d(ysum), None, d(c["z"]), 0, 1,
                              first_sample, d(W), d(Wm), 0, None, 0, None, None)
    assert rc == _native.BTF_ENOTPD and lib.btf_fail_index(None) == (first_sample + 1) * R + 0
    assert b"not positive definite" in lib.btf_last_error(None)
    assert np.array_equal(W[0], clean["W"][0]) and np.array_equal(Wm[0], clean["W_mean"][0])
    assert np.all(np.isnan(W[1:])) and np.all(np.isnan(Wm[1:]))
    again = utils.fold_in_rows(c["Y"], c["Vs"], "gaussian", **kw)                          # the next call is served
    assert np.array_equal(again["W"], clean["W"])


@pytest.mark.parametrize("first_sample", FAIL_FIRST_SAMPLES)
def test_fold_in_cols_names_the_first_failing_pair(first_sample):
    """6. A nan in Ws[1] (S = 3, C = 3): BTF_ESTATE with btf_fail_index = (first_sample + 1) C + 0; samples 0 and 2 equal the
    clean call bit for bit, V, V_mean and Tau2 of sample 1 are nan.  banded_factor_forward returns at the first pivot that
    is not positive; nothing faults."""
    c = cols_failure_case()
    S, N, K = c["Ws"].shape
    C, T, tf, sweeps = c["Y"].shape[0], c["Y"].shape[2], c["tf_order"], c["sweeps"]
    kw = dict(nu2=c["nu2"], lam2=c["lam2"], tf_order=tf, seed=9, sweeps=sweeps, summary=False, first_sample=first_sample)
    clean = utils.fold_in_cols(c["Y"], c["Ws"], "gaussian", **kw)
    assert np.all(np.isfinite(clean["V"]))
    with pytest.raises(_native.BTFError, match="not positive definite") as info:
        utils.fold_in_cols(c["Y"], c["bad"], "gaussian", **kw)
    assert info.value.code == _native.BTF_ESTATE
    lib = _native.load()
    _, cnt, ysum = fc.column_statistics(c["Y"], "gaussian", N, T)
    nD = fc.penalty(T, tf).shape[0]
    V, Vm, T2 = np.zeros((S, C, T, K)), np.zeros((S, C, T, K)), np.zeros((S, C, nD))
    d = _native.dptr
    rc = lib.btf_fold_in_cols(0, 0, S, C, N, T, K, tf, d(c["bad"]), d(c["nu2"]), d(c["lam2"]), d(cnt), d(ysum), None, None, 9, sweeps,
                              first_sample, fc.STABILITY, d(V), d(Vm), d(T2), 0, None, 0, None, None)
    assert rc == _native.BTF_ESTATE and lib.btf_fail_index(None) == (first_sample + 1) * C + 0
    for got, want in ((V, clean["V"]), (Vm, clean["V_mean"]), (T2, clean["Tau2"])):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.all(np.isnan(got[1]))
    again = utils.fold_in_cols(c["Y"], c["Ws"], "gaussian", **kw)                          # the next call is served
    assert np.array_equal(again["V"], clean["V"])
