"""PSIS-LOO on the GPU at every padding, tail-length and tile edge of csrc/btf_loo.h (loo_psis_kernel<WRITE_LW>,
loo_mean_kernel<K>; launched by btf_crit_loo of csrc/btf_analysis.hip), next to tests/test_gpu_loo.py, whose comparison
this is: criteria.psis_loo_host on the device's own pointwise matrix, the leave-curve-out mean against the host weights,
`_check` / `_rel` with the five figures of BOUND; inf and nan in the same places.

The geometry the cases are derived from:  one 64-lane workgroup per curve, the curve sorted by a bitonic network over
P = the power of two >= max(S, 64) slots (the S..P-1 pads are +inf with indices >= S), 18 P bytes of LDS (72 KiB at
P = 4096: the one launch above 64 KiB);  Mt = min(floor(S / 5), ceil(3 sqrt(S / r_eff))) largest ratios, a fit from
Mt >= 5 (S >= 25), the grid of 30 + floor(sqrt(n)) <= 64 points one per lane;  per_xcd = ceil(NM / 8), 8 per_xcd
workgroups, workgroup b on curve (b & 7) per_xcd + (b >> 3), idle when that is >= NM;  loo_mean_kernel: one workgroup per
(column, 64 rows), LOO_WAVES = 4 waves, wave w on the depth chunks w, w + 4, ... of LOO_TC = 16 cells (a wave wraps to a
second chunk from T = 65), lanes past N clamped to row N - 1 and masked.

Largest |device - host| / (1 + |host|) measured on an MI355X, per group of cases (MEASURED below).  Every group stays
under BOUND of tests/test_gpu_loo.py (elpd_loo 4.04e-15, pareto_k 9.67e-14, lppd 4.54e-15, log_weights 2.44e-14, mean
9.94e-15), pareto_k at S = 25..64 included, so BOUND is the bound of every case and no group has one of its own:
    sample counts  elpd_loo 5.62e-16  pareto_k 2.61e-15  lppd 3.83e-16  log_weights 1.60e-15  mean 5.63e-16
    curve map      elpd_loo 1.84e-16  pareto_k 1.40e-15  lppd 1.79e-16  log_weights 3.24e-16  mean 8.22e-16
    mean kernel    elpd_loo 3.86e-16  pareto_k 3.81e-15  lppd 2.10e-16  log_weights 6.25e-16  mean 4.97e-16
    ties           elpd_loo 2.26e-16  pareto_k 2.91e-15  lppd 1.80e-16  log_weights 3.50e-16  mean 4.08e-16
Should a figure ever exceed BOUND, the case prints the definition's own sensitivity (`_sensitivity`: its change under a
fixed-seed +-1 ulp perturbation of the matrix, up to 1.6e-13 for pareto_k at S = 25..64 on the host): a difference within
ten times that is rounding, anything above it a bug."""
import numpy as np
import pytest

from functionalmf_amd import criteria
from test_gpu_loo import BOUND, _case, _check, _reff, _rel

pytestmark = pytest.mark.gpu

FIGURES = ("elpd_loo", "pareto_k", "lppd", "log_weights", "mean")
NO_BOUND = dict.fromkeys(FIGURES, np.inf)          # `_check` as a measuring device: the figures are asserted by `_hold`
MEASURED = {          # on an MI355X; all under BOUND, which therefore holds for every group
    "sample counts": {"elpd_loo": 5.62e-16, "pareto_k": 2.61e-15, "lppd": 3.83e-16, "log_weights": 1.60e-15, "mean": 5.63e-16},
    "curve map": {"elpd_loo": 1.84e-16, "pareto_k": 1.40e-15, "lppd": 1.79e-16, "log_weights": 3.24e-16, "mean": 8.22e-16},
    "mean kernel": {"elpd_loo": 3.86e-16, "pareto_k": 3.81e-15, "lppd": 2.10e-16, "log_weights": 6.25e-16, "mean": 4.97e-16},
    "ties": {"elpd_loo": 2.26e-16, "pareto_k": 2.91e-15, "lppd": 1.80e-16, "log_weights": 3.50e-16, "mean": 4.08e-16},
}
assert all(v[k] <= BOUND[k] for v in MEASURED.values() for k in FIGURES)

TRANSFORMS = {None: lambda x: x, "ilogit": lambda x: 1.0 / (1.0 + np.exp(-x)), "square": lambda x: x * x}


def _padding(S):
    P = 64
    while P < S:
        P <<= 1
    return P


def _sensitivity(L, obs, r_eff, seed=0):
    """The host definition's own sensitivity: the change of its figures under a fixed-seed +-1 ulp perturbation of the
    matrix, measured as `_rel` measures the device against it."""
    up = np.random.RandomState(seed).randint(2, size=L.shape).astype(bool)
    Lp = np.where(up, np.nextafter(L, np.inf), np.nextafter(L, -np.inf))
    a = criteria.psis_loo_host(L, obs, r_eff=r_eff, log_weights=True)
    b = criteria.psis_loo_host(Lp, obs, r_eff=r_eff, log_weights=True)
    out = {k: _rel(b["curves"][k], a["curves"][k]) for k in ("elpd_loo", "pareto_k", "lppd")}
    out["log_weights"] = _rel(b["log_weights"], a["log_weights"])
    return out


def _measure(model, results, obs, r_eff, transform, label, ic=None):
    """One loo() call against the host definition on the device's own matrix: (figures, device result, host result)."""
    if ic is None:
        ic = model.information_criteria(results, pointwise=True)
    res = model.loo(results, r_eff=r_eff, mean=True, transform=transform, log_weights=True)
    host = criteria.psis_loo_host(ic["loglik"], obs, r_eff=1.0 if r_eff is None else r_eff, log_weights=True)
    figs = _check(res, host, "", label, bound=NO_BOUND)
    Mu = np.einsum("snk,smtk->snmt", results["W"], results["V"])
    want = np.einsum("snm,snmt->nmt", np.exp(host["log_weights"]), TRANSFORMS[transform](Mu))
    figs["mean"] = _rel(res["mean"], want)
    assert np.array_equal(res["curves"]["lppd"], ic["curves"]["lppd"])
    return figs, res, host


def _hold(group, figs, label):
    print("LOO-SHAPES [%s] %s" % (group, label), " ".join("%s=%.3g" % (k, figs[k]) for k in FIGURES))
    for k in FIGURES:
        assert figs[k] <= BOUND[k], (group, label, k, figs[k], BOUND[k])


# ---------------------------------------------------------------- sample counts
#   S      5  24  25  26  29  30  63  64  65  127  128  129  255  256  257  511  512  513  2048  2049  4095
#   P     64  64  64  64  64  64  64  64 128  128  128  256  256  256  512  512  512 1024  2048  4096  4096
#   Mt, r_eff None   1   4   5   5   5   6  12  12  13   25   25   25   48   48   49   68   68   68   136   136   192
#   Mt, r_eff 0.3    1   4   5   5   5   6  12  12  13   25   25   25   51   51   51  102  102  102   248   248   351
#   Mt, r_eff 3.0    1   4   5   5   5   6  12  12  13   20   20   20   28   28   28   40   40   40    79    79   111
SAMPLE_COUNTS = (5, 24, 25, 26, 29, 30, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2048, 2049, 4095)
R_EFFS = (None, 0.3, 3.0)


def _count_case(S):
    N, M, T = (9, 3, 5) if S < 2048 else (5, 1, 2)
    return _case("gauss", N, M, T, 2, 3, S, "complete", seed=7000 + S)


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_sample_counts(S):
    model, results, obs = _count_case(S)
    assert obs.all()
    ic = model.information_criteria(results, pointwise=True)
    worst = dict.fromkeys(FIGURES, 0.0)
    for r_eff in R_EFFS:
        re = 1.0 if r_eff is None else r_eff
        Mt = criteria.tail_length(S, re)
        figs, res, host = _measure(model, results, obs, r_eff, "square", "S=%d P=%d r_eff=%s Mt=%d" % (S, _padding(S), r_eff, Mt), ic=ic)
        kk = host["curves"]["pareto_k"]
        assert np.all(np.isinf(kk)) if S <= 24 else np.all(np.isfinite(kk)), "a condition of the inputs"
        if figs["pareto_k"] > BOUND["pareto_k"]:
            print("LOO-SHAPES sensitivity of the definition, S=%d r_eff=%s:" % (S, r_eff), _sensitivity(ic["loglik"], obs, re))
        worst = {k: max(worst[k], figs[k]) for k in FIGURES}
    _hold("sample counts", worst, "S=%d" % S)


def test_tail_length_takes_both_arms_of_its_min():
    """A condition of the cases, on the host: Mt is floor(S / 5) in some and ceil(3 sqrt(S / r_eff)) in others."""
    arms = {(S, r): S // 5 < np.ceil(3.0 * np.sqrt(S / (r or 1.0))) for S in SAMPLE_COUNTS for r in R_EFFS}
    assert set(arms.values()) == {True, False}
    assert all(arms[S, 0.3] and not arms[S, 3.0] for S in (127, 128, 129, 255, 256, 257, 511, 512, 513))


def test_both_write_lw_variants_give_the_same_estimate():
    S = 257
    model, results, obs = _count_case(S)
    full = model.loo(results, r_eff=0.3, mean=True, log_weights=True)
    lean = model.loo(results, r_eff=0.3)
    assert "mean" not in lean and "log_weights" not in lean
    assert np.array_equal(lean["curves"]["elpd_loo"], full["curves"]["elpd_loo"])
    assert np.array_equal(lean["curves"]["pareto_k"], full["curves"]["pareto_k"]) and np.isfinite(full["curves"]["pareto_k"]).all()
    assert lean["elpd_loo"] == full["elpd_loo"]


# ---------------------------------------------------------------- curve map
#   N M      1x1  7x1  1x7  8x1  3x3  5x3  16x1  17x1  4x4
#   NM         1    7    7    8    9   15    16    17    16
#   per_xcd    1    1    1    1    2    2     2     3     2
#   idle       7    1    1    0    7    1     0     7     0      workgroups of the 8 per_xcd
CURVE_MAP = [(1, 1), (7, 1), (1, 7), (8, 1), (3, 3), (5, 3), (16, 1), (17, 1), (4, 4)]


@pytest.mark.parametrize("N,M", CURVE_MAP, ids=["%dx%d" % nm for nm in CURVE_MAP])
def test_curve_map(N, M):
    S = 64
    model, results, obs = _case("gauss", N, M, 5, 2, 3, S, "complete", seed=8000 + 10 * N + M)
    re = _reff("grid", N, M, seed=N * M)
    figs, res, host = _measure(model, results, obs, re, None, "%dx%d" % (N, M))
    for k in ("elpd_loo", "pareto_k"):                       # every curve's reference value differs: a swap would show
        assert len(np.unique(host["curves"][k])) == N * M and np.isfinite(host["curves"][k]).all(), k
    assert len(np.unique(re)) == N * M
    _hold("curve map", figs, "%dx%d" % (N, M))


# ---------------------------------------------------------------- loo_mean_kernel
@pytest.mark.parametrize("K", range(1, 11))
def test_mean_at_every_nembeds_and_transform(K):
    model, results, obs = _case("gauss", 70, 2, 6, 2, K, 30, "complete", seed=9000 + K)
    ic = model.information_criteria(results, pointwise=True)
    for transform in TRANSFORMS:
        figs, res, host = _measure(model, results, obs, None, transform, "K=%d %s" % (K, transform), ic=ic)
        assert np.isfinite(res["mean"]).all()
        _hold("mean kernel", figs, "K=%d transform=%s" % (K, transform))


#   T     15  16  17  48  49  64  65  129
#   nch    1   1   2   3   4   4   5    9     (a wave's second chunk from T = 65; T = 129: wave 0 owns chunks 0, 4, 8)
MEAN_TILES = [(T, N) for T in (15, 16, 17, 48, 49, 64, 65, 129) for N in (1, 64, 65)]


@pytest.mark.parametrize("T,N", MEAN_TILES, ids=["T%d-N%d" % tn for tn in MEAN_TILES])
def test_mean_at_every_depth_chunk_and_row_tile(T, N):
    model, results, obs = _case("gauss", N, 2, T, 2, 3, 30, "complete", seed=9500 + 10 * T + N)
    figs, res, host = _measure(model, results, obs, 0.5, "ilogit", "T=%d N=%d" % (T, N))
    assert res["mean"].shape == (N, 2, T) and np.isfinite(res["mean"]).all()
    _hold("mean kernel", figs, "T=%d N=%d" % (T, N))


# ---------------------------------------------------------------- ties
def _tied(copies, seed):
    """20 distinct states (W, V and nu2), each `copies` times, in a fixed random order."""
    model, results, obs = _case("gauss", 9, 3, 5, 2, 3, 20, "complete", seed=seed)
    idx = np.random.RandomState(seed).permutation(np.repeat(np.arange(20), copies))
    return model, {k: np.ascontiguousarray(v[idx]) for k, v in results.items()}, obs, idx


#   r_eff None: Mt = 20, the cut-off is the last sample of a group of five;  3.0: Mt = 18, the cut-off sits inside a group,
#   whose five samples all stay outside the tail (n = 15);  "grid": a tail length per curve
@pytest.mark.parametrize("r_eff", [None, 3.0, "grid"])
def test_ties_follow_the_definitions_rules(r_eff):
    model, results, obs, idx = _tied(5, seed=31)
    S = idx.shape[0]
    assert criteria.tail_length(S, 1.0) == 20 and criteria.tail_length(S, 3.0) == 18
    ic = model.information_criteria(results, pointwise=True)
    L = ic["loglik"]
    for g in range(20):                                      # equal states: bit-equal log-likelihoods
        assert (L[idx == g] == L[idx == g][:1]).all(), g
    assert all(len(np.unique(L[:, i, j])) == 20 for i in range(9) for j in range(3))
    re = _reff(r_eff, 9, 3, seed=5)
    figs, res, host = _measure(model, results, obs, re, "square", "ties r_eff=%s" % (r_eff,), ic=ic)
    lw = host["log_weights"]
    assert np.isfinite(host["curves"]["pareto_k"]).all()
    # the rules bite: in every curve some group of tied samples lies in the tail with five different smoothed weights
    assert all(max(len(np.unique(lw[idx == g, i, j])) for g in range(20)) == 5 for i in range(9) for j in range(3))
    if r_eff == 3.0:                                         # the cut-off's own group stays outside: its weights are equal
        order = np.argsort(-L[:, 0, 0], kind="stable")       # ascending log ratio, ties by sample index
        assert len(np.unique(lw[order[80:85], 0, 0])) == 1 and len(np.unique(lw[order[85:90], 0, 0])) == 5
    _hold("ties", figs, "r_eff=%s" % (r_eff,))


def test_all_samples_equal():
    model, results, obs, idx = _tied(1, seed=32)
    S = 30
    results = {k: np.ascontiguousarray(np.repeat(v[:1], S, axis=0)) for k, v in results.items()}
    ic = model.information_criteria(results, pointwise=True)
    assert (ic["loglik"] == ic["loglik"][:1]).all()
    figs, res, host = _measure(model, results, obs, None, None, "all equal", ic=ic)
    assert np.all(res["curves"]["pareto_k"] == np.inf) and np.all(host["curves"]["pareto_k"] == np.inf)
    # uniform weights: elpd_loo is lppd, up to the rounding the definition itself shows between the two
    own = _rel(host["curves"]["elpd_loo"], host["curves"]["lppd"])
    assert _rel(res["curves"]["elpd_loo"], host["curves"]["lppd"]) <= BOUND["elpd_loo"] + own
    np.testing.assert_allclose(res["log_weights"], -np.log(S), rtol=0, atol=BOUND["log_weights"] * (1 + np.log(S)))
    _hold("ties", figs, "all equal")
