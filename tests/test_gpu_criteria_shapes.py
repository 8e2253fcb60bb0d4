"""Model-selection criteria on the GPU at every template instantiation and every chunk, block and tile edge of
csrc/btf_criteria.h (crit_kernel<K, FAM>, crit_plugin_kernel<FAM>, crit_total_kernel; launched by crit_run of
csrc/btf_analysis.hip), next to tests/test_gpu_criteria.py, whose comparison this is: scipy's elementwise log densities in
float64 on the host-formed einsum tensor (`_logdens`), NaN cells 0, summed per curve; the plug-in at Mu.mean(0) and the mean
variance; every scalar key against criteria.from_loglik - with that file's tolerances (loglik, ll_at_mean: rtol 1e-10 and
1e-10 of the largest finite magnitude; lppd rtol / atol 1e-10; p_waic rtol 1e-9, atol 1e-10; keys rtol 1e-10, atol 1e-9).

The geometry the cases are derived from:  one workgroup per (column j, WAVE = 64 rows), one lane per row, lanes past N
clamped to row N - 1 and masked;  CRIT_WAVES = 4 waves, wave w owning the depth chunks w, w + 4, ... of CRIT_TC = 16 cells
(nch = ceil(T / 16) chunks; the first chunk of a wave writes its LDS partial, later ones add to it: T > 64; waves with
w >= nch write zeros);  samples in blocks of CRIT_SB = 32, the plug-in sums read back and added from the second block on,
the Welford count s + 1 running across blocks;  ceil(N / 64) * M per-sample partial totals summed by crit_total_kernel
with 256 samples per thread block (S > 256: a second one).

Every case is built by `build` first, which asserts on the host that the reference is finite everywhere except the cells
the poisson_identity designs put a w . v = 0 under (tests/test_host_criteria.py runs every builder without a device).

Largest errors measured on an MI355X, per group of cases, as a share of the tolerance of each comparison (1 = at the
bound):
    instantiations   loglik 3.3e-06  ll_at_mean 3.4e-06  lppd 8.0e-06  p_waic 2.0e-05  per_sample 5.7e-06  keys 1.8e-04
    depth            loglik 2.6e-06  ll_at_mean 3.2e-06  lppd 6.4e-06  p_waic 2.6e-05  per_sample 4.1e-06  keys 5.3e-05
    sample blocks    loglik 3.8e-06  ll_at_mean 4.1e-06  lppd 6.5e-06  p_waic 9.1e-05  per_sample 4.7e-06  keys 4.6e-04
    rows, columns    loglik 2.5e-06  ll_at_mean 2.7e-06  lppd 8.6e-06  p_waic 6.1e-06  per_sample 5.3e-06  keys 1.3e-04
    infinities       loglik 2.0e-06  ll_at_mean 2.5e-06  lppd 4.1e-06  p_waic 5.1e-06  per_sample 3.5e-06  keys 3.4e-06
(The counts at T = 129 - poisson_log, nine chunks, wave 0 adding twice - are among the depth figures: nowhere near a
tolerance.)  The second run of the largest case of every group was bit-equal to the first."""
import numpy as np
import pytest
from scipy.special import logsumexp

from functionalmf_amd import criteria
from test_gpu_criteria import LINKS, _case, _logdens  # noqa: F401  (_logdens: the reference _case forms L and Lm with)

pytestmark = pytest.mark.gpu

KEYS = ("waic", "elpd_waic", "p_waic", "lppd", "waic_se", "dic", "p_dic", "mean_deviance", "deviance_at_mean")
CRIT_TC, CRIT_WAVES, CRIT_SB, WAVE, TOTAL_BLOCK = 16, 4, 32, 64, 256       # csrc/btf_criteria.h, crit_run


# ---------------------------------------------------------------- the poisson_identity designs (T = 70: chunks 0..4)
#   sample, row, column, depth cell:  chunk 0 | chunk 4, wave 0's second (the += branch) | the last cell of the partial
#   last chunk, in the second sample block and the second row tile
ZERO_CELLS = [(1, 3, 0, 3), (5, 10, 0, 65), (32, 64, 1, 69)]
ZERO_SAMPLE = (7, 1, 20)          # sample, column, depth cell: w . v = 0 in every row, so in both workgroups of the column


def _zero_cells(observed):
    """w_i^s = 0.7 e_0 and v_jt^s[0] = 0: w . v = 0 exactly at that cell of that sample alone (K = 2, positive factors)."""
    def prepare(Ws, Vs, Y4):
        for s, i, j, t in ZERO_CELLS:
            Ws[s, i, :] = 0.0
            Ws[s, i, 0] = 0.7
            Vs[s, j, t, 0] = 0.0
            Y4[i, j, t, :] = np.maximum(Y4[i, j, t, :], 1.0) if observed else np.nan       # (y >= 1: scipy's -inf too)
    return prepare


def _zero_sample(Ws, Vs, Y4):
    s, j, t = ZERO_SAMPLE
    Vs[s, j, t, :] = 0.0
    Y4[:, j, t, :] = np.maximum(Y4[:, j, t, :], 1.0)


DESIGNS = {"cells": _zero_cells(True), "cells-unobserved": _zero_cells(False), "sample": _zero_sample}


def _designed_minus_inf(design, S, N, M):
    """The (S,N,M) mask of the curve values the design makes -inf."""
    mask = np.zeros((S, N, M), dtype=bool)
    if design == "cells":
        for s, i, j, t in ZERO_CELLS:
            mask[s, i, j] = True
    elif design == "sample":
        mask[ZERO_SAMPLE[0], :, ZERO_SAMPLE[1]] = True
    return mask


# ---------------------------------------------------------------- the cases: (kind, N, M, T, R, K, S, form, design)
#   1  every crit_kernel<K, FAM>, and the two conjugate routes (family 3 with per-sample nu2, family 2 with trial counts)
INSTANCES = [(kind, 70, 2, 6, 2, K, 5, "complete", None) for K in range(1, 11) for kind in LINKS] + \
            [(kind, 70, 2, 6, 2, K, 5, "complete", None) for K in (1, 4, 7, 10) for kind in ("gauss", "binom")]
#   2  depth:  T     2  15  16  17  32  33  48  49  63  64  65  80  81  128  129
#              nch   1   1   1   2   2   3   3   4   4   4   5   5   6    8    9     (live waves min(nch, 4); += from nch = 5)
DEPTHS = (2, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80, 81, 128, 129)
DEPTH = [(kind, 65, 2, T, 2, 3, 5, "missing", None) for T in DEPTHS for kind in ("poisson_log", "gauss")]
#   3  sample blocks of 32 at two live waves (T = 20), and the block edges again at one (T = 12)
BLOCKS = [(kind, 33, 2, 20, 2, 4, S, "complete", None) for S in (1, 2, 31, 32, 33, 63, 64, 65, 96, 97) for kind in ("gauss", "negbin_logit")] + \
         [(kind, 33, 2, 12, 2, 4, S, "complete", None) for S in (31, 32, 33, 65) for kind in ("gauss", "negbin_logit")]
#   4  rows and columns: a tile of one lane, full tiles, a tile of one live lane behind full ones; then S = 257 over
#      3 x 3 workgroups: crit_total_kernel's second thread block sums nine partials
TILES = [(kind, N, M, 17, 2, 2, 33, "missing", None) for N in (1, 2, 63, 64, 65, 128, 129) for M in (1, 3) for kind in ("gauss", "bernoulli_logit")] + \
        [("poisson_log", 129, 3, 17, 2, 2, 257, "missing", None)]
#   5  w . v = 0 under poisson_identity
INFINITIES = [("poisson_identity", 65, 2, 70, 2, 2, 33, "complete", d) for d in ("cells", "cells-unobserved", "sample")]
GROUPS = {"instantiations": INSTANCES, "depth": DEPTH, "sample blocks": BLOCKS, "rows, columns": TILES, "infinities": INFINITIES}
LARGEST = {"instantiations": INSTANCES[-1], "depth": DEPTH[-1], "sample blocks": BLOCKS[19], "rows, columns": TILES[-1],
           "infinities": INFINITIES[0]}
ALL = [(g, spec) for g, specs in GROUPS.items() for spec in specs]


def _id(spec):
    kind, N, M, T, R, K, S, form, design = spec
    return "%s-N%d-M%d-T%d-K%d-S%d%s" % (kind, N, M, T, K, S, "-" + design if design else "")


def _seed(spec):
    """A seed of the case's own: no two cases share inputs, so the kernel of a neighbouring K or family cannot agree."""
    return 1 + [s for _, s in ALL].index(spec)


def build(spec, bind=True):
    """_case of the spec, with the builder's own conditions asserted on the host before any device call: the reference is
    finite everywhere but in the design's places, some curve is observed, the design's cells are what they claim."""
    kind, N, M, T, R, K, S, form, design = spec
    model, data, results, L, Lm, obs = _case(kind, N, M, T, R, K, S, seed=_seed(spec), form=form, bind=bind,
                                             prepare=DESIGNS.get(design))
    assert L.shape == (S, N, M) and Lm.shape == (N, M)
    assert obs.any() and (design is None or obs.all())
    assert not np.isnan(L).any() and np.isfinite(Lm).all()
    assert np.array_equal(L == -np.inf, _designed_minus_inf(design, S, N, M)) and not (L == np.inf).any()
    if design is not None:
        Mu = np.einsum("snk,smtk->snmt", results["W"], results["V"])
        assert (Mu >= 0).all()
        if design == "sample":
            s, j, t = ZERO_SAMPLE
            want = np.zeros(Mu.shape, dtype=bool)
            want[s, :, j, t] = True
        else:
            want = np.zeros(Mu.shape, dtype=bool)
            for s, i, j, t in ZERO_CELLS:
                want[s, i, j, t] = True
            Y4 = data
            gone = np.array([np.isnan(Y4[i, j, t]).all() for _, i, j, t in ZERO_CELLS])
            assert gone.all() == (design == "cells-unobserved") and gone.any() == gone.all()
        assert np.array_equal(Mu == 0, want)
    return model, results, L, Lm, obs


def _share(got, want, rtol, atol):
    """Largest |got - want| / (atol + rtol |want|) over the finite entries of the reference."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    return float((np.abs(got[fin] - want[fin]) / (atol + rtol * np.abs(want[fin]))).max()) if fin.any() else 0.0


def _finite_max(a):
    return float(np.abs(a[np.isfinite(a)]).max())


def _compare(ic, L, Lm, obs, label):
    """The comparison of test_pointwise_matches_scipy_and_keys_match_numpy, with the absolute terms scaled by the largest
    FINITE magnitude (the same number where everything is finite); inf and nan must sit in the reference's places."""
    S = L.shape[0]
    got = ic["loglik"]
    assert got.shape == L.shape
    ref = np.where(obs[None], L, 0.0)
    want = criteria.from_loglik(L, obs, Lm)
    with np.errstate(invalid="ignore"):
        figs = {"loglik": _share(got, ref, 1e-10, 1e-10 * _finite_max(ref)),
                "ll_at_mean": _share(ic["curves"]["ll_at_mean"], np.where(obs, Lm, 0.0), 1e-10, 1e-10 * _finite_max(Lm)),
                "lppd": _share(ic["curves"]["lppd"], want["curves"]["lppd"], 1e-10, 1e-10),
                "p_waic": _share(ic["curves"]["p_waic"], want["curves"]["p_waic"], 1e-9, 1e-10),
                "per_sample": _share(ic["loglik_per_sample"], want["loglik_per_sample"], 1e-10, 0.0),
                "keys": max(_share(ic[k], want[k], 1e-10, 1e-9) for k in KEYS)}
    print("CRIT-SHAPES", label, " ".join("%s=%.3g" % kv for kv in figs.items()))
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10 * _finite_max(ref))
    np.testing.assert_allclose(ic["curves"]["ll_at_mean"], np.where(obs, Lm, 0.0), rtol=1e-10, atol=1e-10 * _finite_max(Lm))
    for k in KEYS:
        np.testing.assert_allclose(ic[k], want[k], rtol=1e-10, atol=1e-9, err_msg=k)
    assert ic["n_curves"] == int(obs.sum()) and ic["nsamples"] == S
    np.testing.assert_allclose(ic["loglik_per_sample"], want["loglik_per_sample"], rtol=1e-10)
    np.testing.assert_allclose(ic["curves"]["lppd"], want["curves"]["lppd"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(ic["curves"]["p_waic"], want["curves"]["p_waic"], rtol=1e-9, atol=1e-10)
    return want


def _run(group, spec):
    model, results, L, Lm, obs = build(spec)
    ic = model.information_criteria(results, pointwise=True)
    want = _compare(ic, L, Lm, obs, "[%s] %s" % (group, _id(spec)))
    return ic, want, L


def _ids(specs):
    return [_id(s) for s in specs]


@pytest.mark.parametrize("spec", INSTANCES, ids=_ids(INSTANCES))
def test_every_instantiation(spec):
    _run("instantiations", spec)


@pytest.mark.parametrize("spec", DEPTH, ids=_ids(DEPTH))
def test_depth_chunks(spec):
    T = spec[3]
    nch = -(-T // CRIT_TC)
    assert (nch > CRIT_WAVES) == (T > 64)                   # the += branch runs from T = 65 on
    _run("depth", spec)


@pytest.mark.parametrize("spec", BLOCKS, ids=_ids(BLOCKS))
def test_sample_blocks(spec):
    assert min(-(-spec[3] // CRIT_TC), CRIT_WAVES) == (2 if spec[3] == 20 else 1)      # live waves
    _run("sample blocks", spec)


@pytest.mark.parametrize("spec", TILES, ids=_ids(TILES))
def test_row_tiles_and_columns(spec):
    kind, N, M, T, R, K, S = spec[:7]
    if S > TOTAL_BLOCK:
        assert -(-N // WAVE) * M > 1                        # several partials for the second block of crit_total_kernel
    _run("rows, columns", spec)


def test_zero_cells_give_minus_inf_in_the_references_places():
    spec = INFINITIES[0]
    ic, want, L = _run("infinities", spec)
    hit = np.zeros(L.shape[1:], dtype=bool)
    for s, i, j, t in ZERO_CELLS:
        assert ic["loglik"][s, i, j] == -np.inf
        hit[i, j] = True
    assert np.array_equal(ic["loglik"] == -np.inf, L == -np.inf) and np.isfinite(ic["loglik"][L != -np.inf]).all()
    # p_waic as np.var: nan on the three curves; lppd as scipy's logsumexp: finite, the -inf sample adds nothing
    assert np.array_equal(np.isnan(ic["curves"]["p_waic"]), hit) and np.isnan(ic["p_waic"]) and np.isnan(ic["waic"])
    assert np.isfinite(ic["curves"]["lppd"]).all()
    np.testing.assert_allclose(ic["curves"]["lppd"], logsumexp(L, axis=0) - np.log(L.shape[0]), rtol=1e-10, atol=1e-10)
    bad = sorted(s for s, _, _, _ in ZERO_CELLS)
    assert np.array_equal(np.flatnonzero(ic["loglik_per_sample"] == -np.inf), bad)
    assert np.isfinite(np.delete(ic["loglik_per_sample"], bad)).all()
    assert np.isfinite(ic["curves"]["ll_at_mean"]).all() and np.isfinite(ic["deviance_at_mean"])


def test_unobserved_zero_cells_contribute_nothing():
    ic, want, L = _run("infinities", INFINITIES[1])
    assert np.isfinite(ic["loglik"]).all() and np.isfinite(ic["loglik_per_sample"]).all()
    assert np.isfinite(ic["curves"]["p_waic"]).all() and np.isfinite(ic["waic"]) and np.isfinite(ic["dic"])


def test_a_sample_that_is_minus_inf_for_every_curve_of_a_workgroup():
    ic, want, L = _run("infinities", INFINITIES[2])
    s, j, t = ZERO_SAMPLE
    assert (ic["loglik"][s, :, j] == -np.inf).all() and np.isfinite(np.delete(ic["loglik"], s, axis=0)).all()
    assert np.isfinite(ic["loglik"][s, :, 1 - j]).all()
    assert ic["loglik_per_sample"][s] == -np.inf and np.isfinite(np.delete(ic["loglik_per_sample"], s)).all()
    assert np.isnan(ic["curves"]["p_waic"][:, j]).all() and np.isfinite(ic["curves"]["p_waic"][:, 1 - j]).all()
    assert np.isfinite(ic["curves"]["lppd"]).all()


def _bits(ic):
    out = {k: np.asarray(ic[k]) for k in KEYS + ("loglik", "loglik_per_sample")}
    out.update({"curves." + k: v for k, v in ic["curves"].items()})
    return out


@pytest.mark.parametrize("group", list(LARGEST), ids=[g.replace(", ", "-").replace(" ", "-") for g in LARGEST])
def test_twice(group):
    spec = LARGEST[group]
    assert spec in GROUPS[group]
    model, results, L, Lm, obs = build(spec)
    a = _bits(model.information_criteria(results, pointwise=True))
    b = _bits(model.information_criteria(results, pointwise=True))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
