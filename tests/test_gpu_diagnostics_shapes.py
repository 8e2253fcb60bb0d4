"""diag_kernel<K> (csrc/btf_diag.h, through diagnostics.convergence) at every draw count, chain count and nembeds at which
its mapping onto threads, waves and LDS changes, next to tests/test_gpu_diagnostics.py, whose bounds these are.

Reference: `spec` of tests/test_host_diagnostics.py, the transcription of the definition that shares nothing with the
package, on bit-equal draws; the mean against x.mean().  Every cell of every case is compared in all five outputs:
rhat and mcse_mean to 1e-10 relative, ess_bulk and ess_tail to 1e-8 relative, the mean to 1e-12 max(1, |x|max); nan and
inf sit in the same places.

Feeding a series to a cell: with K = 1, V all ones and W[c][s, i, 0] = x_i[c, s], cell (i, 0, 0) is the series x_i, so one
call diagnoses N chosen series.  All draws are multiples of 2^-8 (squares: 2^-16), and with K > 1 the factors are, so the
device's draws and numpy's are the same bits (identity and square only).

Conditions on the inputs, asserted by every case before the comparison and by test_host_diagnostics.py on the same
builders without a GPU (`conditions`): Geyer's rule branches on the sign of each pair sum and of the last even term, so
every series here keeps |even + odd| and |even| above 1e-6 in all four of its sequences (`geyer_margin`); and at least one
half-chain of the draws, and of the folded draws, is not constant, so that no R-hat is a ratio of two rounding errors.
Seeds that miss a condition are replaced by the next (`RESEED`, found on the host).

The groups and what they reach in the kernel:
  A  K = 1..10 x {identity, square}: every instantiation, each with factors of its own
  B  one chain, S = 4..9 and the edges of 256, 512, 1024, 2048, 4096: one to sixteen passes of the strided loops and
     z-score registers, the second compare-exchange per thread (P >= 1024), n == P (no +inf pads), 64 KiB of LDS
  C  four chains at the same pooled edges (S = 64 .. 1024)
  D  C in {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 43, 63, 64} at S = 4, 5, 41, 4096 // C: every group width of diag_seg_sum
     (128 by red[], 64, 32, 16, 8, 4, 2, idle tail threads), the strided cm normalisation (C > 32), the odd-S loop
  E  every S = 4..72 at C = 1 and S = 4..24 at C = 3: the quantile index, both parities, every h from 2 up
  F  Geyer: sequences that end on the lag bound (h = 5..9), hundreds of passes, four different stopping lags, antithetic
  G  cell geometry (N, M, T) at K = 2
  H  a non-finite draw that only a later pass of the load loop sees, at the dropped middle draw of an odd S; constant cells
  I  the two largest cases twice: the same bits

Largest relative differences measured on an MI355X over the whole file, 914 series (bound):
    rhat       5.6e-16    (1e-10)
    ess_bulk   1.1e-14    (1e-8)
    ess_tail   1.4e-14    (1e-8)
    mcse_mean  3.3e-15    (1e-10)
    mean       0          of max(1, |x|max): sums of multiples of 2^-16 are exact in any order  (1e-12)
"""
import numpy as np
import pytest

from functionalmf_amd import diagnostics

from test_gpu_diagnostics import _cells, _chains
from test_host_diagnostics import ar1, pairs_margin, spec

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
REL = {"rhat": 1e-10, "ess_bulk": 1e-8, "ess_tail": 1e-8, "mcse_mean": 1e-10}
MEAN_TOL = 1e-12
OUT4 = ("rhat", "ess_bulk", "ess_tail", "mcse_mean")
KINDS = ("ar09", "iid", "ints", "squares", "q95", "anti")
WORST = dict.fromkeys(OUT4 + ("mean",), 0.0)


# ---------------------------------------------------------------- the inputs (no GPU needed)
def _grid(x):
    return np.round(x * 256) / 256


def draw(kind, C, S, seed, offsets=False, phi=None):
    """One (C, S) series of the kind, multiples of 2^-8; offsets: chain c is moved by c / 64."""
    rs = np.random.RandomState(seed)
    if kind == "ar09":
        x = _grid(ar1(rs, C, S, 0.9 if phi is None else phi))
    elif kind == "iid":
        x = _grid(rs.normal(size=(C, S)))
    elif kind == "ints":                                   # heavy ties
        x = rs.randint(0, 4, size=(C, S)).astype(float)
    elif kind == "squares":                                # folded ties
        x = rs.randint(-3, 4, size=(C, S)).astype(float) ** 2
    elif kind == "q95":                                    # heavy_ties_q95 of the host test: the q95 indicator is constant
        x = np.minimum(rs.randint(0, 10, size=(C, S)), 7).astype(float)
    elif kind == "anti":
        x = _grid(ar1(rs, C, S, -0.8))
    elif kind == "trend":
        x = _grid(0.25 * np.arange(S)[None, :] + np.arange(C)[:, None] + 0.25 * rs.normal(size=(C, S)))
    else:
        raise KeyError(kind)
    if offsets:
        x = x + np.arange(C)[:, None] / 64.0
    return x


def _halves(x):
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, x.shape[1] - h:]], axis=0)


def conditions(x):
    """(reference outputs, pairs, margin, well posed) of one (C, S) series."""
    pairs = []
    with np.errstate(divide="ignore", invalid="ignore"):
        want = spec(x, pairs)
    posed = all(np.ptp(_halves(y), axis=1).max() > 0 for y in (x, np.abs(x - np.median(x))))
    return want, pairs, pairs_margin(pairs), bool(posed)


# seeds replaced because the first choice misses a condition: (group, kind, C, S) -> how many steps of 7919 further
RESEED = {("B", "q95", 1, 4): 1, ("D", "q95", 1, 4): 1, ("E", "ints", 1, 5): 1}


def series(group, kind, C, S, **kw):
    base = 1000 * (1 + (KINDS + ("trend",)).index(kind)) + 37 * C + S + 100000 * "ABCDEFGHI".index(group[0])
    return draw(kind, C, S, base + 7919 * RESEED.get((group, kind, C, S), 0), **kw)


def as_chains(xs):
    """Result dicts (K = 1, M = T = 1, V all ones) whose cell (i, 0, 0) is the series xs[i] of (C, S)."""
    xs = np.asarray(xs, dtype=float)                       # (ncell, C, S)
    ncell, C, S = xs.shape
    return [{"W": np.ascontiguousarray(xs[:, c, :].T[:, :, None]), "V": np.ones((S, 1, 1, 1))} for c in range(C)]


B_SIZES = (4, 5, 6, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
C_SIZES = (64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)
D_CHAINS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 43, 63, 64)
D_CASES = [(C, S) for C in D_CHAINS for S in sorted({4, 5, 41, 4096 // C}) if C * S <= 4096]
E_CASES = [(1, S) for S in range(4, 73)] + [(3, S) for S in range(4, 25)]
E_KINDS = ("ints", "ar09")
F1_SIZES = tuple(range(10, 20))
G_SHAPES = ((1, 1, 1), (1, 1, 5), (1, 4, 1), (5, 1, 1), (5, 3, 1), (2, 1, 5), (3, 5, 2))
F3_SEED = 4244               # the first seed from 4242 on whose four sequences stop at four different lags


def kinds_case(group, C, S, kinds=KINDS, **kw):
    return np.stack([series(group, k, C, S, **kw) for k in kinds])


def factor_case(group, K, transform, N, M, T, C=2, S=9):
    """(chains, (ncell, C, S) series) with dyadic factors at nembeds K."""
    seed = 500 + 11 * K + 100000 * "ABCDEFGHI".index(group) + 97 * (N + 10 * M + 100 * T) + (transform == "square")
    seed += 7919 * RESEED.get((group, K, transform, N, M, T), 0)
    chains = _chains(C, S, N, M, T, K, seed=seed, dyadic=True)
    return chains, _cells(chains, transform).reshape(N * M * T, C, S)


def host_cases():
    """Every series of the file, as (id, (ncell, C, S) array): what the conditions are asserted on."""
    for K in range(1, 11):
        for tr in ("identity", "square"):
            yield "A-K%d-%s" % (K, tr), factor_case("A", K, tr, 2, 1, 3)[1]
    for S in B_SIZES:
        yield "B-S%d" % S, kinds_case("B", 1, S)
    for S in C_SIZES:
        yield "C-S%d" % S, kinds_case("C", 4, S)
    for C, S in D_CASES:
        yield "D-C%d-S%d" % (C, S), kinds_case("D", C, S, offsets=True)
    for C, S in E_CASES:
        yield "E-C%d-S%d" % (C, S), kinds_case("E", C, S, kinds=E_KINDS)
    for S in F1_SIZES:
        yield "F1-S%d" % S, kinds_case("F1", 2, S, kinds=("trend",))
    yield "F2", kinds_case("F2", 4, 1000, kinds=("ar09",), phi=0.98)
    yield "F3", f3_case()
    for S in (40, 41):
        yield "F4-S%d" % S, kinds_case("F4", 3, S, kinds=("anti",))
    for shape in G_SHAPES:
        yield "G-%d-%d-%d" % shape, factor_case("G", 2, "identity", *shape, S=12)[1]
    yield "H-C1", h_case(1, 300, 299)[1][2:]
    yield "H-C3", h_case(3, 101, 50)[1][2:]
    yield "I-C64", kinds_case("I", 64, 64, offsets=True)
    yield "I-C1", kinds_case("I", 1, 4096)


def f3_case():
    return draw("ar09", 2, 200, F3_SEED)[None]


def h_case(C, S, s_bad):
    """Three cells: a non-finite draw (in the last chain at s_bad), a constant cell, an ordinary one."""
    xs = np.stack([series("H", "ar09", C, S), np.full((C, S), 1.5), series("H", "iid", C, S)])
    xs[0, C - 1, s_bad] = np.nan if C == 1 else np.inf
    return as_chains(xs), xs


# ---------------------------------------------------------------- the comparison
def _rel(got, want):
    """Relative difference; 0 where both are the same nan or inf, inf where they are not."""
    if np.isnan(want) or np.isinf(want):
        return 0.0 if (np.isnan(got) if np.isnan(want) else got == want) else np.inf
    if want == 0.0:
        return 0.0 if got == 0.0 else np.inf
    return abs(got / want - 1.0)


def compare(res, xs, what):
    """Every cell of res (row-major over (N, M, T)) against spec of its series xs[cell]; returns the pairs per cell."""
    xs = np.asarray(xs)
    got = {k: np.asarray(res[k]).reshape(-1) for k in diagnostics.OUTPUTS}
    assert got["rhat"].size == len(xs)
    all_pairs, fails = [], []
    for i, x in enumerate(xs):
        want, pairs, margin, posed = conditions(x)
        assert margin > MARGIN and posed, ("a condition on the input", what, i, margin, posed)
        all_pairs.append(pairs)
        for j, k in enumerate(OUT4):
            d = _rel(got[k][i], want[j])
            WORST[k] = max(WORST[k], d)
            if not d <= REL[k]:
                fails.append((what, i, k, got[k][i], want[j], d))
        dm = abs(got["mean"][i] - x.mean()) / max(1.0, np.abs(x).max())
        WORST["mean"] = max(WORST["mean"], dm)
        if not dm <= MEAN_TOL:
            fails.append((what, i, "mean", got["mean"][i], x.mean(), dm))
    print("%s: %d cells; largest so far %s" % (what, len(xs), " ".join("%s %.3g" % kv for kv in WORST.items())))
    assert not fails, fails
    return all_pairs


def run_series(xs, what):
    xs = np.asarray(xs)
    res = diagnostics.convergence(as_chains(xs), scalars=())
    assert res["nchains"] == xs.shape[1] and res["ndraws"] == xs.shape[2] and res["rhat"].shape == (len(xs), 1, 1)
    return res, compare(res, xs, what)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest relative differences over the file: " + "  ".join("%s %.3g" % kv for kv in WORST.items()))


# ---------------------------------------------------------------- A: every instantiation
@pytest.mark.parametrize("transform", ["identity", "square"])
@pytest.mark.parametrize("K", range(1, 11))
def test_every_nembeds(K, transform):
    chains, xs = factor_case("A", K, transform, 2, 1, 3)
    compare(diagnostics.convergence(chains, transform=transform, scalars=()), xs, "A K=%d %s" % (K, transform))


# ---------------------------------------------------------------- B, C: pooled-draw edges
@pytest.mark.parametrize("S", B_SIZES)
def test_pooled_draw_edges_one_chain(S):
    run_series(kinds_case("B", 1, S), "B C=1 S=%d" % S)


@pytest.mark.parametrize("S", C_SIZES)
def test_pooled_draw_edges_four_chains(S):
    run_series(kinds_case("C", 4, S), "C C=4 S=%d" % S)


# ---------------------------------------------------------------- D: chain-count edges
def _group_width(C):
    G = 256 // (2 * C)
    return 1 << (G.bit_length() - 1)


def test_the_chain_counts_reach_every_group_width():
    assert {_group_width(C) for C in D_CHAINS} == {128, 64, 32, 16, 8, 4, 2}
    assert 2 * 43 * _group_width(43) < 256 and 4 * 2 * 33 > 256        # idle tail threads; a second cm pass
    assert (64, 64) in D_CASES and (1, 4096) in D_CASES


@pytest.mark.parametrize("C,S", D_CASES, ids=["C%d-S%d" % cs for cs in D_CASES])
def test_chain_count_edges(C, S):
    xs = kinds_case("D", C, S, offsets=True)
    assert C == 1 or np.unique(xs[0].mean(axis=1)).size > 1
    run_series(xs, "D C=%d S=%d" % (C, S))


# ---------------------------------------------------------------- E: every small size
@pytest.mark.parametrize("C,S", E_CASES, ids=["C%d-S%d" % cs for cs in E_CASES])
def test_every_small_size(C, S):
    run_series(kinds_case("E", C, S, kinds=E_KINDS), "E C=%d S=%d" % (C, S))


# ---------------------------------------------------------------- F: Geyer's sequences
@pytest.mark.parametrize("S", F1_SIZES)
def test_geyer_ends_on_the_lag_bound(S):
    h = S // 2
    _, pairs = run_series(kinds_case("F1", 2, S, kinds=("trend",)), "F1 S=%d" % S)
    for v in (0, 3):                                       # bulk and raw: every pair up to the bound, the last one accepted
        p = pairs[0][v]
        assert len(p) - 1 == (h - 3) // 2 >= 1 and p[-1][0] + p[-1][1] > 0, (v, p)


def test_geyer_long_sequences():
    _, pairs = run_series(kinds_case("F2", 4, 1000, kinds=("ar09",), phi=0.98), "F2")
    assert len(pairs[0][0]) - 1 > 20, len(pairs[0][0])


def test_geyer_four_series_stop_at_four_lags():
    _, pairs = run_series(f3_case(), "F3")
    stops = [len(p) for p in pairs[0]]
    assert len(set(stops)) == 4, stops


@pytest.mark.parametrize("S", [40, 41])
def test_geyer_antithetic_chains(S):
    run_series(kinds_case("F4", 3, S, kinds=("anti",)), "F4 S=%d" % S)


# ---------------------------------------------------------------- G: cell geometry
@pytest.mark.parametrize("N,M,T", G_SHAPES)
def test_cell_geometry(N, M, T):
    chains, xs = factor_case("G", 2, "identity", N, M, T, S=12)
    assert len({x.tobytes() for x in xs}) == N * M * T     # all cells distinct
    res = diagnostics.convergence(chains, scalars=())
    assert res["rhat"].shape == (N, M, T)
    compare(res, xs, "G %s" % ((N, M, T),))


# ---------------------------------------------------------------- H: nan rules beyond the first pass
@pytest.mark.parametrize("C,S,s_bad", [(1, 300, 299), (3, 101, 50)])
def test_non_finite_draw_in_a_late_pass_and_constant_cell(C, S, s_bad):
    chains, xs = h_case(C, S, s_bad)
    assert ((C - 1) * S + s_bad >= 256 if C == 1 else s_bad == S // 2) and not np.isfinite(xs[0]).all()
    res = diagnostics.convergence(chains, scalars=())
    for k in diagnostics.OUTPUTS:
        assert np.isnan(res[k][:2]).all(), k
    compare({k: res[k][2:] for k in diagnostics.OUTPUTS}, xs[2:], "H C=%d S=%d" % (C, S))


# ---------------------------------------------------------------- I: same bits twice
@pytest.mark.parametrize("C,S", [(64, 64), (1, 4096)])
def test_two_calls_same_bits(C, S):
    xs = kinds_case("I", C, S, offsets=C > 1)
    a, _ = run_series(xs, "I C=%d S=%d" % (C, S))
    b = diagnostics.convergence(as_chains(xs), scalars=())
    for k in diagnostics.OUTPUTS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
