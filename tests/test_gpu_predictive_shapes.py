"""Shape pass of the predictive and summary kernels (csrc/btf_predict.h, posterior_summary_kernel of csrc/btf_kernels.h):
every sort geometry, every family, every nembeds, both passes of the percentile and list loops, every chunk count of the
scores, every rate layout ("Shape passes", the predictive entry).  The case lists, the inputs and the numpy
references are tests/test_host_predictive_shapes.py, which shows without a GPU that the lists are complete and every case
admissible.  Inputs go through the public forms (utils.posterior_predictive, utils.gamma_grid_predictive,
predictive.batch, predictive.gamma_grid_batch, utils.posterior_summary) with all cells listed, except in list 4.

A. the draws are where the header of btf_predict.h says: draw (cell, s, r) of a call is element g = (cell S + s) R + r of the
   batch run with the same seed on the host's eta and aux - bit for bit for the count families, to 1e-13 for the Gaussian
   family and the gamma grid (the bound of tests/test_gpu_gg_predictive.py for this identity);
B. the reductions against numpy on the device's own draws with the tolerances of test_reductions_against_numpy: 1e-12
   relative for quantiles, y_mean, y_var, pit_lo / pit_hi and mean, exact inside / nobs / coverage and nan pattern, 1e-10
   for rmse / mae; order statistics at integral positions (q = 0, q = 100, q = 50 at odd n) bit for bit;
C. the summary against einsum + mean + np.percentile within 1e-12 max(1, max|Mu|), the integral positions and the mean of
   the dyadic values (transform None, "square") bit for bit;
D. the two largest cases twice, the same bits.
"""
import numpy as np
import pytest

from functionalmf_amd import _native, predictive, utils

from test_host_predictive_shapes import (ALL_PRED_CASES, BATCH_FULL, BATCH_PREFIXES, COUNT_FAMILIES, DATA_CASES, FAMILIES, GG_TABLE,
                                         K_CASES, LIST_CASES, PARAM_CASES, POISON_CASES, PRED_SCORE_CELLS, Q_CASES, REPEAT_PRED,
                                         REPEAT_SUMMARY, SCORE_ALL_MISSING, SCORE_CASES, SCORE_CHUNK_MISSING, SEED, SORT_CASES,
                                         SUMMARY_CASES, SUMMARY_LIMIT, TOTAL_CASES, batch_case, batch_inputs, build, case_id,
                                         pred_geom, reference, summary_geom, summary_inputs, summary_reference)

pytestmark = pytest.mark.gpu

DRAW_TOL, RED_TOL, SCORE_TOL, SUMMARY_TOL = 1e-13, 1e-12, 1e-10, 1e-12
REDUCTIONS = ("quantiles", "y_mean", "y_var", "pit_lo", "pit_hi", "mean")


def rel(a, b):
    ok = ~np.isnan(b)
    return float(np.abs(a - b)[ok].max() / max(np.abs(b[ok]).max(), 1e-300)) if ok.any() else 0.0


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def predict(c, b, **over):
    kw = dict(data=b["Y"], q=c.q, draws_per_sample=c.R, seed=SEED, cells=b["cells"])
    kw.update(over)
    if c.fam == "gamma_grid":
        return utils.gamma_grid_predictive(b["Ws"], b["Vs"], GG_TABLE, **kw)
    return utils.posterior_predictive(b["Ws"], b["Vs"], c.fam, **kw, **b["kw"])


def batch(fam, eta, aux):
    if fam == "gamma_grid":
        return predictive.gamma_grid_batch(eta, GG_TABLE, seed=SEED)
    return predictive.batch(fam, eta, 0.0 if aux is None else aux, seed=SEED)


def check_draws(c, b, out):
    """A: out["draws"] against the batch at the global indices of the listed cells; returns the largest relative error."""
    eta, aux, idx = batch_inputs(c, b)
    want, got = batch(c.fam, eta, aux)[idx], out["draws"]
    assert got.shape == idx.shape == (len(b["cells"]), c.S * c.R)
    if c.fam in COUNT_FAMILIES:
        np.testing.assert_array_equal(got, want, err_msg="draws of %s (P, cells, lds = %r)" % (case_id(c), pred_geom(c.S * c.R)))
        return 0.0
    assert same_nan(got, want) and not np.isnan(want).any()
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert np.all(np.abs(got - want) <= DRAW_TOL * np.abs(want)), "draws of %s: %.3e" % (case_id(c), err.max())
    return float(err.max())


def check_reductions(c, b, out):
    """B: every reduction against numpy on the device's draws (all cells listed, in order); returns {name: error}."""
    n, geom = c.S * c.R, "%s (P, cells, lds = %r)" % (case_id(c), pred_geom(c.S * c.R))
    assert np.array_equal(b["cells"], np.arange(c.N * c.M * c.T)) and out["ndraws"] == n and out["nsamples"] == c.S
    ref = reference(c, b, out["draws"])
    errs = {}
    for name in REDUCTIONS:
        got, want = out[name], ref[name]
        assert got.shape == want.shape, name
        if want.size:
            errs[name] = rel(got, want)
            assert same_nan(got, want) and errs[name] <= RED_TOL, "%s of %s: %.3e" % (name, geom, errs[name])
    for qi, q in enumerate(c.q):
        if q in (0.0, 100.0) or (q == 50.0 and n % 2 == 1):            # an order statistic itself: the same bits
            np.testing.assert_array_equal(out["quantiles"][qi], ref["quantiles"][qi], err_msg="q = %g of %s" % (q, geom))
    np.testing.assert_array_equal(out["nobs"], ref["nobs"], err_msg="nobs of " + geom)
    np.testing.assert_array_equal(out["inside"], ref["inside"], err_msg="inside of " + geom)
    assert out["coverage"] == ref["coverage"] or (np.isnan(out["coverage"]) and np.isnan(ref["coverage"])), geom
    for name in ("rmse", "mae"):
        assert out[name].shape == (c.S,) and same_nan(out[name], ref[name]), "%s of %s" % (name, geom)
        errs[name] = rel(out[name], ref[name])
        assert errs[name] <= SCORE_TOL, "%s of %s: %.3e" % (name, geom, errs[name])
    return errs


def run_case(c, group):
    b = build(c)
    out = predict(c, b)
    errs = dict(draws=check_draws(c, b, out))
    errs.update(check_reductions(c, b, out))
    print("ERR %s %s: %s" % (group, case_id(c), "  ".join("%s %.2e" % kv for kv in errs.items())))
    return b, out


# ------------------------------------------------------------------------------------------- 1. sort geometry of pred_kernel
@pytest.mark.parametrize("c", SORT_CASES, ids=case_id)
def test_every_sort_geometry(c):
    run_case(c, "sort")


# ------------------------------------------------------------------------------------------- 2. nembeds
@pytest.mark.parametrize("c", K_CASES, ids=case_id)
def test_every_nembeds(c):
    run_case(c, "nembeds")


# ------------------------------------------------------------------------------------------- 3. percentiles
@pytest.mark.parametrize("c", Q_CASES, ids=case_id)
def test_percentile_passes(c):
    b, out = run_case(c, "percentiles")
    nq = len(c.q)
    assert out["quantiles"].shape == (nq, c.N, c.M, c.T)
    if nq < 2:
        assert np.isnan(out["inside"]).all() and np.isnan(out["coverage"]) and np.isnan(out["nominal"])
    else:
        assert out["nominal"] == (c.q[-1] - c.q[0]) / 100.0 and np.isfinite(out["inside"]).all()


# ------------------------------------------------------------------------------------------- 4. listed cells
@pytest.mark.parametrize("c", LIST_CASES, ids=case_id)
def test_listed_cells(c):
    b = build(c)
    cells = b["cells"]
    out = predict(c, b)
    every = predict(c, b, cells=np.arange(c.N * c.M * c.T, dtype=np.int32))
    err = check_draws(c, b, out)                                       # (the batch holds eta = 1 at the indices no draw uses)
    np.testing.assert_array_equal(out["draws"], every["draws"][cells])
    np.testing.assert_array_equal(out["cells"], cells)
    twice = [k for k in range(len(cells)) if (cells[:k] == cells[k]).any()]
    for k in twice:
        np.testing.assert_array_equal(out["draws"][k], out["draws"][int(np.flatnonzero(cells == cells[k])[0])])
    assert len(twice) == (1 if c.listed in (65, 129) else 0)
    for name in predictive.ARRAY_OUTPUTS:                              # what is listed changes nothing else
        if name != "draws":
            np.testing.assert_array_equal(out[name], every[name], err_msg=name)
    assert not np.isnan(every["draws"]).all(axis=1).any()
    print("ERR list %s: draws %.2e" % (case_id(c), err))


# ------------------------------------------------------------------------------------------- 5. data
@pytest.mark.parametrize("c", DATA_CASES, ids=case_id)
def test_replicates_and_missing_cells(c):
    b, out = run_case(c, "data")
    ncell = c.N * c.M * c.T
    flat = lambda name: out[name].reshape(ncell)
    assert flat("nobs")[ncell - 1] == 0 and np.isnan(flat("pit_lo")[ncell - 1]) and np.isnan(flat("pit_hi")[ncell - 1])
    assert flat("inside")[ncell - 1] == 0
    assert flat("nobs")[ncell - 2] == 1 and np.isfinite(flat("pit_lo")[ncell - 2])
    assert flat("nobs").max() == c.nreps
    if c.fam in COUNT_FAMILIES:
        assert (out["pit_lo"] < out["pit_hi"]).any()                   # a count equal to a draw


@pytest.mark.parametrize("c", POISON_CASES, ids=case_id)
def test_a_missing_trial_count_poisons_its_cell_alone(c):
    b, out = run_case(c, "poison")
    ncell, bad = c.N * c.M * c.T, c.param[1]
    trials = np.where(np.isnan(b["kw"]["trials"]), 5.0, b["kw"]["trials"])
    clean = predict(c, dict(b, kw=dict(trials=trials)))               # the same call with that one count given
    assert np.isnan(b["kw"]["trials"]).sum() == 1 and not np.isnan(clean["draws"]).any()
    others = np.arange(ncell) != bad
    for name in ("mean", "y_mean", "y_var", "pit_lo", "pit_hi", "inside", "nobs"):
        got, ref = out[name].reshape(ncell), clean[name].reshape(ncell)
        assert (name == "nobs") != bool(np.isnan(got[bad])), name
        np.testing.assert_array_equal(got[others], ref[others], err_msg=name)
    q, qc = out["quantiles"].reshape(len(c.q), ncell), clean["quantiles"].reshape(len(c.q), ncell)
    assert np.isnan(q[:, bad]).all()
    np.testing.assert_array_equal(q[:, others], qc[:, others])
    assert np.isnan(out["draws"][bad]).all()
    np.testing.assert_array_equal(out["draws"][others], clean["draws"][others])
    assert np.isfinite(out["coverage"])


# ------------------------------------------------------------------------------------------- 6. parameters
@pytest.mark.parametrize("c", PARAM_CASES, ids=case_id)
def test_parameter_layouts(c):
    run_case(c, "parameters")


# ------------------------------------------------------------------------------------------- 7. scores
@pytest.mark.parametrize("c", SCORE_CASES + SCORE_CHUNK_MISSING + TOTAL_CASES, ids=case_id)
def test_score_chunks_and_blocks(c):
    b, out = run_case(c, "scores")
    if c.data == "chunk_missing":
        assert out["nobs"].reshape(-1)[PRED_SCORE_CELLS:2 * PRED_SCORE_CELLS].sum() == 0 and out["nobs"].reshape(-1)[-1] > 0
    assert np.isfinite(out["rmse"]).all() and np.isfinite(out["mae"]).all()


@pytest.mark.parametrize("c", SCORE_ALL_MISSING, ids=case_id)
def test_scores_of_nothing_are_nan(c):
    b, out = run_case(c, "scores")
    assert np.isnan(out["rmse"]).all() and np.isnan(out["mae"]).all() and out["nobs"].sum() == 0 and np.isnan(out["coverage"])
    assert np.all(out["inside"] == 0) and np.isnan(out["pit_lo"]).all()


# ------------------------------------------------------------------------------------------- 8. pred_batch_kernel
@pytest.mark.parametrize("fam", FAMILIES)
def test_batch_prefixes(fam):
    eta, aux = batch_case(fam)
    full = batch(fam, eta, aux)
    assert full.shape == (BATCH_FULL,) and not np.isnan(full).any()
    for L in BATCH_PREFIXES:
        np.testing.assert_array_equal(batch(fam, eta[:L], None if aux is None else aux[:L]), full[:L], err_msg="%s prefix %d" % (fam, L))


# ------------------------------------------------------------------------------------------- 9. posterior_summary_kernel
def _summary_id(c):
    return "S%d-N%d-%dx%d-K%d-%s-nq%d" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4], len(c[5]))


@pytest.mark.parametrize("case", SUMMARY_CASES, ids=_summary_id)
def test_summary_equals_numpy(case):
    S, N, MT, K, transform, q = case
    Ws, Vs = summary_inputs(S, N, MT, K)
    geom = "%s (P, cells, lds = %r)" % (_summary_id(case), summary_geom(S))
    mean, quant = utils.posterior_summary(Ws, Vs, q=q, transform=transform)
    Mu, ref_mean, ref_q = summary_reference(Ws, Vs, transform, q)
    assert mean.shape == ref_mean.shape and quant.shape == ref_q.shape == (len(q), N) + MT
    bound = SUMMARY_TOL * max(1.0, np.abs(Mu).max())
    em, eq = np.abs(mean - ref_mean).max(), (np.abs(quant - ref_q).max() if len(q) else 0.0)
    print("ERR summary %s: mean %.2e  quantiles %.2e  (bound %.1e)" % (_summary_id(case), em, eq, bound))
    assert em <= bound and eq <= bound, geom
    if transform != "ilogit":                                          # dyadic values: exact sums, order statistics themselves
        np.testing.assert_array_equal(mean, ref_mean, err_msg="mean of " + geom)
        for qi, v in enumerate(q):
            if v in (0.0, 100.0) or (v == 50.0 and S % 2 == 1):
                np.testing.assert_array_equal(quant[qi], ref_q[qi], err_msg="q = %g of %s" % (v, geom))


def test_summary_refuses_more_than_its_row_holds():
    Ws, Vs = np.zeros((SUMMARY_LIMIT + 1, 1, 1)), np.zeros((SUMMARY_LIMIT + 1, 1, 2, 1))
    with pytest.raises(_native.BTFError, match="bad posterior_summary arguments") as e:
        utils.posterior_summary(Ws, Vs)
    assert e.value.code == _native.BTF_EINVAL


# ------------------------------------------------------------------------------------------- D. the largest cases twice
def test_the_largest_cases_give_the_same_bits_twice():
    c = REPEAT_PRED
    b = build(c)
    first, second = predict(c, b), predict(c, b)
    for name in predictive.ARRAY_OUTPUTS:
        np.testing.assert_array_equal(first[name], second[name], err_msg=name)
    S, N, MT, K, transform, q = REPEAT_SUMMARY
    Ws, Vs = summary_inputs(S, N, MT, K)
    a, bq = utils.posterior_summary(Ws, Vs, q=q, transform=transform)
    a2, bq2 = utils.posterior_summary(Ws, Vs, q=q, transform=transform)
    np.testing.assert_array_equal(a, a2)
    np.testing.assert_array_equal(bq, bq2)


def test_every_case_of_the_host_file_is_run_here():
    run = SORT_CASES + K_CASES + Q_CASES + LIST_CASES + DATA_CASES + POISON_CASES + PARAM_CASES + SCORE_CASES + SCORE_CHUNK_MISSING + \
        TOTAL_CASES + SCORE_ALL_MISSING
    assert set(run) == set(ALL_PRED_CASES) and len(run) == len(ALL_PRED_CASES)
