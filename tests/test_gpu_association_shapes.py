"""Posterior feature association on the GPU at every tile geometry of csrc/btf_assoc.h (launched by assoc_run of
csrc/btf_analysis.hip), next to tests/test_gpu_association.py, whose comparison this is: association.reference on the
device's own posterior_functionals(pointwise=True) values, _check_summaries / _check_of_means / _well_conditioned of that
module with its tolerances R_TOL = 1e-12 (r, absolute) and REL_TOL = 1e-11 (slope, intercept, of the largest magnitude); the
sets and counts (defined, n_mean, prob_positive, n) exact.

The geometry, from assoc_run:  P = the power of two >= max(S, 2);  cells = max(1, min(min(16, 64 KiB / 8 P) / nstats, F))
features per reduce workgroup, ceil(F / cells) feature tiles per column, cells * nstats * 8 P bytes of LDS (128 KiB at
P = 8192 with both statistics: the one launch above 64 KiB);  rb = ceil(N / 256) row blocks of assoc_pbar_kernel and
assoc_gbar_kernel;  ceil(F / 8) feature blocks of assoc_pbar_kernel;  ceil(M / 4) column blocks of assoc_cross_kernel.

Every shape was first checked on the host: the float64 moment route in numpy (association.moments + from_moments, the
device's route) agrees with association.statistics to a tenth of the tolerances (1e-13 for r, 1e-12 of the scale for
slope and intercept) on these very inputs (`_moment_route_error`, asserted by every case before the device is called).

Largest errors measured on an MI355X, per group of cases: r and its summaries, absolute (held to R_TOL = 1e-12), and the
worst slope / intercept / stderr / sd figure as a share of its bound (REL_TOL = 1e-11 of the largest magnitude):
    feature tiles   r 6.7e-16    others 5.3e-05 of the bound
    sample counts   r 2.7e-14    others 9.9e-04 of the bound      (regressions over n = 3..6 rows)
    rows            r 1.0e-15    others 1.6e-04 of the bound
    columns         r 4.4e-16    others 3.7e-05 of the bound
    nembeds         r 5.6e-16    others 7.0e-05 of the bound
    chunking        r 5.6e-16    others 6.5e-05 of the bound      (chunked against whole: bit-equal)
On the host the moment route itself was at most 4.3e-14 (r) and 1.4e-14 of the scale (slope, intercept) from the direct
definition over all these cases."""
import numpy as np
import pytest

from functionalmf_amd import association
from functionalmf_amd.utils import posterior_feature_association, posterior_functionals
from test_gpu_association import R_TOL, REL_TOL, STATS, _check_of_means, _check_summaries, _same, _states, _well_conditioned

pytestmark = pytest.mark.gpu

Q = (0, 100, 33.3, 50)            # the two ends and a position between two samples


def _cells(S, nstats, F):
    """(P, cells, feature tiles, bytes of LDS) of assoc_run."""
    P = 2
    while P < S:
        P <<= 1
    cells = max(1, min(max(1, min(16, 65536 // (8 * P))) // nstats, F))
    return P, cells, -(-F // cells), cells * nstats * P * 8


def _moment_route_error(y, Ws, Us):
    """(largest |r| difference, largest slope / intercept difference over their scale) between the moment route in float64
    numpy and the direct definition; the defined sets must be equal."""
    st = association.statistics(y, Ws, Us)
    S, F, M = st["r"].shape
    got = np.full((3, S, F, M), np.nan)
    for s in range(S):
        for j in range(M):
            mom = association.moments(y[s, :, j], Ws[s])
            for f in range(F):
                got[:, s, f, j] = association.from_moments(mom, Us[s, f])
    ref = np.stack([st["r"], st["slope"], st["intercept"]])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref[0])
    if not ok.any():
        return 0.0, 0.0
    scale = max(np.abs(ref[1][ok]).max(), np.abs(ref[2][ok]).max())
    return float(np.abs(got[0] - ref[0])[ok].max()), float(max(np.abs(got[1] - ref[1])[ok].max(), np.abs(got[2] - ref[2])[ok].max()) / scale)


def _run(dims, which="auc", stats=STATS, level=None, zero_feature=None, seed=3, q=Q, scratch=0, prepare=None):
    """One case: inputs, their own conditions, the device call and the comparison.  Returns (inputs, values, result)."""
    Ws, Vs, Us = _states(seed=seed, **dims)
    if zero_feature is not None:
        Us[:, zero_feature] = 0.0
    if prepare is not None:
        prepare(Ws, Vs, Us)
    F, M = dims["F"], dims["M"]
    allpairs = np.array([(f, j) for f in range(F) for j in range(M)])
    y = posterior_functionals(Ws, Vs, which=(which,), level=level, pointwise=True)[which]["pointwise"]
    _well_conditioned(y, Ws, Us)
    er, es = _moment_route_error(y, Ws, Us)
    print("moment route on the host: r %.3g, slope / intercept %.3g of the scale" % (er, es))
    assert er <= 0.1 * R_TOL and es <= 0.1 * REL_TOL, (er, es)
    got = posterior_feature_association(Ws, Vs, Us, which=which, stats=stats, level=level, q=q, pairs=allpairs, _scratch_bytes=scratch)
    ref = association.reference(y, Ws, Us, which=which, stats=stats, q=q, pairs=allpairs)
    what = "%s %s %s" % (sorted(dims.items()), which, stats)
    _check_summaries(got, ref, what)
    _check_of_means(got["of_means"], ref["of_means"], what)
    return (Ws, Vs, Us), y, got


def _undefined_feature(got, f, stats, F, M, S):
    """Feature f is constant (all zero): undefined in every sample, for every column; every other feature is defined."""
    others = [g for g in range(F) if g != f]
    assert (got["defined"][f] == 0).all() and (got["defined"][others] == 1).all()
    for k in stats:
        v = got[k]["values"].reshape(F, M, S)
        assert np.isnan(v[f]).all() and np.isfinite(v[others]).all(), k
        for key in ("mean", "var", "prob_positive"):
            assert np.isnan(got[k][key][f]).all() and np.isfinite(got[k][key][others]).all(), (k, key)
        assert np.isnan(got[k]["quantiles"][:, f]).all() and np.isfinite(got[k]["quantiles"][:, others]).all(), k
    assert np.isnan(got["of_means"]["r"][f]).all() and np.isfinite(got["of_means"]["r"][others]).all()


# ---------------------------------------------------------------- feature tiles
#   stats        F    cells  tiles  (S = 37: P = 64, 16 rows of 512 bytes fit)
#   r, slope     8      8      1
#   r, slope     9      8      2    a last tile of one feature
#   r, slope    17      8      3
#   one         16     16      1
#   one         17     16      2    a last tile of one feature
#   one         33     16      3
TILES = [(STATS, 8, 8, 1), (STATS, 9, 8, 2), (STATS, 17, 8, 3), (("r",), 16, 16, 1), (("r",), 17, 16, 2), (("r",), 33, 16, 3),
         (("slope",), 17, 16, 2), (("slope",), 33, 16, 3)]


@pytest.mark.parametrize("stats,F,cells,tiles", TILES, ids=["%s-F%d-cells%d-tiles%d" % ("+".join(t[0]), t[1], t[2], t[3]) for t in TILES])
def test_feature_tiles(stats, F, cells, tiles):
    dims = dict(S=37, N=20, M=2, T=3, K=2, F=F)
    assert _cells(37, len(stats), F)[:3] == (64, cells, tiles)
    _, _, got = _run(dims, stats=stats, zero_feature=F - 1)          # the zero feature lies in the last (partial) tile
    assert got["stats"] == tuple(stats) and set(got) >= set(stats) and not (set(STATS) - set(stats)) & set(got)
    _undefined_feature(got, F - 1, stats, F, 2, 37)
    assert (got["n_mean"] == 20).all()


def test_one_statistic_alone_is_that_statistic_of_the_pair_at_every_tiling():
    Ws, Vs, Us = _states(seed=3, S=37, N=20, M=2, T=3, K=2, F=17)
    Us[:, 16] = 0.0
    both = posterior_feature_association(Ws, Vs, Us, stats=STATS, q=Q)             # tiles of 8
    for k in STATS:
        _same(posterior_feature_association(Ws, Vs, Us, stats=(k,), q=Q)[k], both[k], k)       # tiles of 16


# ---------------------------------------------------------------- sample counts
#   S        P    stats  cells  LDS
#   2        2      2      3     96 B
#   3        4      2      3    192 B
#   1024  1024      2      3     48 KiB   (4 rows fit beside F = 3)
#   1025  2048      2      2     64 KiB   two feature tiles
#   2049  4096      2      1     64 KiB   three feature tiles
#   4096  4096      2      1     64 KiB
#   4097  8192      2      1    128 KiB   (1 / 2 = 0 cells, clamped to one: two rows of 64 KiB)
#   8192  8192      2      1    128 KiB
#   4097  8192      1      1     64 KiB
SAMPLES = [(2, STATS, 2, 3, 96), (3, STATS, 4, 3, 192), (1024, STATS, 1024, 3, 48 << 10), (1025, STATS, 2048, 2, 64 << 10),
           (2049, STATS, 4096, 1, 64 << 10), (4096, STATS, 4096, 1, 64 << 10), (4097, STATS, 8192, 1, 128 << 10),
           (8192, STATS, 8192, 1, 128 << 10), (4097, ("r",), 8192, 1, 64 << 10)]
SAMPLES_LEVEL = 0.25


def _sample_count_inputs(Ws, Vs, Us):
    """Positive factors, curves (0, w . v, 0): column 0 crosses the level in every row of every sample, column 1 in some
    rows only (n = 2..6, so the defined count differs between the columns), and in no row of every fifth sample."""
    S, N, K = Ws.shape
    rs = np.random.RandomState(S)
    Ws[:] = rs.uniform(0.5, 1.5, size=Ws.shape)
    Vs[:] = 0.0
    Vs[:, 0, 1] = rs.uniform(0.5, 1.5, size=(S, K))
    Vs[:, 1, 1] = rs.uniform(0.05, 0.35, size=(S, K))
    Vs[::5, 1, 1] *= 1e-3


@pytest.mark.parametrize("S,stats,P,cells,lds", SAMPLES, ids=["S%d-%s-P%d-cells%d" % (t[0], "+".join(t[1]), t[2], t[3]) for t in SAMPLES])
def test_sample_counts(S, stats, P, cells, lds):
    dims = dict(S=S, N=6, M=2, T=3, K=2, F=3)
    g = _cells(S, len(stats), 3)
    assert (g[0], g[1], g[3]) == (P, cells, lds)
    (Ws, Vs, Us), y, got = _run(dims, which="crossing", stats=stats, level=SAMPLES_LEVEL, prepare=_sample_count_inputs)
    n = (~np.isnan(y)).sum(axis=1)                                    # (S,M)
    assert (n[:, 0] == 6).all() and (n[::5, 1] == 0).all()
    assert (got["defined"][:, 0] == 1).all() and (got["defined"][:, 1] < 1).all() and (got["defined"][:, 1] > 0).all()
    if S >= 1024:
        assert set(np.unique(n[:, 1])) >= {0, 2, 3, 4, 5, 6}          # n < 3 (undefined), n = 3 and everything above
    assert np.array_equal(got["defined"][:, 1], np.full(3, (n[:, 1] >= 3).sum() / S))


# ---------------------------------------------------------------- rows, columns
#   N      rb  (F = 3: one feature block of assoc_pbar_kernel; F = 9: two, the second with one feature)
ROWS = [(3, 3), (63, 3), (64, 3), (65, 3), (256, 3), (257, 3), (600, 3), (257, 9), (600, 9)]


@pytest.mark.parametrize("N,F", ROWS, ids=["N%d-F%d-rb%d" % (n, f, -(-n // 256)) for n, f in ROWS])
def test_rows(N, F):
    _, _, got = _run(dict(S=5, N=N, M=2, T=3, K=2, F=F), seed=3 + N)
    assert (got["n_mean"] == N).all() and (got["of_means"]["n"] == N).all() and (got["defined"] == 1).all()


@pytest.mark.parametrize("M", [4, 5, 8, 9])
def test_columns(M):
    _, _, got = _run(dict(S=5, N=20, M=M, T=3, K=2, F=3), seed=30 + M)
    assert got["of_means"]["r"].shape == (3, M) and np.isfinite(got["of_means"]["r"]).all() and got["of_means"]["sd_y"].shape == (M,)


# ---------------------------------------------------------------- nembeds
NEMBEDS_LEVEL = 1.0


@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds(nembeds):
    dims = dict(S=8, N=70, M=3, T=5, K=nembeds, F=4)
    _, y, got = _run(dims, which="crossing", level=NEMBEDS_LEVEL, seed=50 + nembeds)
    n = (~np.isnan(y)).sum(axis=1)
    assert n.min() >= 3 and n.max() < 70                              # the level leaves rows out of every regression
    assert np.array_equal(got["n_mean"], n.mean(axis=0)) and (got["defined"] == 1).all()


# ---------------------------------------------------------------- chunking
@pytest.fixture(scope="module")
def chunk_case():
    dims = dict(S=37, N=300, M=2, T=3, K=2, F=3)
    (Ws, Vs, Us), y, got = _run(dims, which="crossing", level=NEMBEDS_LEVEL, seed=7)
    undefined = np.isnan(y)
    assert undefined.any() and (undefined.any(axis=0) & ~undefined.all(axis=0)).any()
    return Ws, Vs, Us, got


@pytest.mark.parametrize("nchunk_samples", [1, 3, 10])
def test_chunking_reloads_the_running_sums_of_two_row_blocks(chunk_case, nchunk_samples):
    Ws, Vs, Us, whole = chunk_case
    assert nchunk_samples == 1 or 37 % nchunk_samples != 0
    allpairs = np.array([(f, j) for f in range(3) for j in range(2)])
    got = posterior_feature_association(Ws, Vs, Us, which="crossing", stats=STATS, level=NEMBEDS_LEVEL, q=Q, pairs=allpairs,
                                        _scratch_bytes=nchunk_samples * 300 * 2 * 8)
    _same(got, whole, nchunk_samples)
