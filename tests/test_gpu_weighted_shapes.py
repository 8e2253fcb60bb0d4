"""Parity against the oracle for the weighted half-sweeps - the streaming accumulation's MODE 1 (every output its own
weights: Gaussian data with missing cells or replicates, Binomial data under compat="exact") and MODE 2 (the stale
cached weights of compat="reference", quirks Q1 / Q2) - over nembeds 1..10, both outputs-per-lane forms (one output
per lane from nembeds 9), 8-wave instances (nembeds >= 6), several 128-output tiles and row chunks, every form of
the source-weight load, byte and f64 pseudo-data, byte replicate counts, and the first tile with its source outputs in
one 64-output half only.  The weights are set from a host draw that varies from cell to cell, so that stale and own
weights differ; each case also proves it ran the path it names.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

TF = 2
W_TOL, V_TOL = 1e-10, 1e-8
MODE2_GAP = 1e-4              # stale against own weights: far above the tolerances (guards against a silent MODE 1)


def _state(rs, N, M, T, K):
    st = dict(W=rs.normal(size=(N, K)), V=0.2 * rs.normal(size=(M, T, K)), Tau2=np.exp(rs.normal(size=(M, 3 * T - 1))),
              lam2=0.3, sigma2=0.8)
    if N > 1:
        st["W"][np.triu_indices(N, 1, K)] = 0
    return st


def _copy(st):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in st.items()}


def _probabilities(rs, N, M, T, K):
    Wt = rs.normal(size=(N, K))
    Vt = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    return 1 / (1 + np.exp(-np.einsum("nk,mtk->nmt", Wt, Vt)))


def _binomial_data(rs, N, M, T, K, trials):
    """(Ysucc, Ntrials) and the accumulation's bytes per cell for that kind of count."""
    p = _probabilities(rs, N, M, T, K)
    if trials == "mixed":                                   # every count 1..127 somewhere: 2 kappa = 2Y - N in [-127, 127]
        Ntr = rs.randint(1, 128, size=(N, M, T)).astype(float)
        Ntr.flat[:127] = np.arange(1, 128)
        return rs.binomial(Ntr.astype(int), p).astype(float), Ntr, 9.0
    if trials == "2.5":                                     # non-integer counts: f64 pseudo-data
        return rs.binomial(3, p).astype(float) * (2.5 / 3), np.full((N, M, T), 2.5), 16.0
    n = int(trials)
    Ys = rs.binomial(n, p).astype(float)
    if n == 127:                                            # the byte range's ends: 2 kappa = -127 and +127
        Ys[0, 0, :3] = 0.0
        Ys[1, 0, :3] = 127.0
    if n == 128:                                            # one 2 kappa = -128: outside what the byte form takes
        Ys[Ys == 0] = 1.0
        Ys[Ys == 128] = 127.0
        Ys[N // 2, M // 2, T // 2] = 0.0
    return Ys, np.full((N, M, T), float(n)), (9.0 if n <= 127 else 16.0)


def _column_patterns(rs, N, M, T, changes):
    """Missing-cell mask whose ybar NaN pattern changes exactly at the columns `changes` (column 0 included): the
    columns between two changes share the pattern of the first (quirk Q2: they reuse its weights)."""
    miss = np.zeros((N, M, T), bool)
    ch = sorted(set(changes) | {0})
    for a, (j0, j1) in enumerate(zip(ch, ch[1:] + [M])):
        pat = rs.rand(N, T) < 0.08
        pat[a % N, a % T] = True                            # distinct from every other pattern
        pat[(a + 1) % N, :] = False                         # and never a whole column of the row empty
        miss[:, j0:j1] = pat[:, None, :]
    return miss


def _half_tile(own):
    """The first 128-output tile holds source outputs in exactly one 64-output half."""
    t = np.zeros(128, bool)
    t[:min(128, own.size)] = own[:128]
    return t[:64].any() != t[64:].any()


def _expect_sampler(variant, K, T):
    # (the twisted layout of weighted data fits 160 KB of LDS except at nembeds 10 with ndepth 40: the single chain)
    if variant == "chain" or (K, T) == (10, 40):
        return "chain"
    return variant


def _bytes_per_cell(model):
    b = ctypes.c_double()
    model._ctx.call("btf_get_accum_bytes_per_cell", ctypes.byref(b))
    return b.value


def _check_sides(compat, N, K, any_nan, src_col, half, T):
    """Sources of both half-sweeps; under compat="reference" the tile condition the case names."""
    from functionalmf_amd.factor import stale_row_sources
    src_row = stale_row_sources(N, K, any_nan)
    own_w = src_row == np.arange(N)
    own_v = np.repeat(src_col == np.arange(src_col.size), T)
    if compat == "reference":
        if "W" in half:
            assert N > 64 and _half_tile(own_w)
        if "V" in half:
            assert _half_tile(own_v)
    return not own_w.all(), not own_v.all()


def _compare(model, data, ost, compat, stale_w, stale_v, variant, K, T, w_step, v_step):
    """Both half-sweeps on the GPU from the state in `ost` (weights already set) and the oracle's, same normals; under
    compat="reference" the own-weights oracle must be far away wherever a side has a stale output."""
    from oracle import btf_oracle as orc
    N, M = ost["W"].shape[0], ost["V"].shape[0]
    Delta = orc.trend_penalty(T, TF)
    np.random.seed(9)
    zw = np.random.normal(size=sum(min(i + 1, K) for i in range(N)))
    zv = np.random.normal(size=(M, K * T))
    np.random.seed(9)
    model._resample_W(data)
    model._resample_V(data)
    assert model.v_sampler() == _expect_sampler(variant, K, T)
    perm = orc.perm_from_order(model.v_order(), K, T)
    st0 = _copy(ost)
    w_step(ost, z=zw, compat=compat)
    assert relerr(model.W, ost["W"]) < W_TOL
    st1 = _copy(ost)
    v_step(ost, Delta, z=zv, compat=compat, perm=perm)
    assert relerr(model.V, ost["V"]) < V_TOL
    if compat == "reference":
        if stale_w:
            assert relerr(w_step(_copy(st0), z=zw, compat="exact"), ost["W"]) > MODE2_GAP
        if stale_v:
            assert relerr(v_step(_copy(st1), Delta, z=zv, compat="exact", perm=perm), ost["V"]) > MODE2_GAP


def _binomial_case(N, M, T, K, compat, variant, trials="4", changes=None, half=(), seed=0):
    from functionalmf_amd.factor import BinomialBayesianTensorFiltering, stale_col_sources
    from oracle import btf_oracle as orc
    rs = np.random.RandomState(seed)
    Ys, Ntr, bpc = _binomial_data(rs, N, M, T, K, trials)
    if changes is not None:
        miss = _column_patterns(rs, N, M, T, changes)
        Ys[miss] = np.nan
        Ntr[miss] = np.nan
    miss = np.isnan(Ys)
    st = _state(rs, N, M, T, K)
    model = BinomialBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=TF, sigma2_init=st["sigma2"], lam2_init=st["lam2"],
                                            W_init=st["W"], V_init=st["V"], Tau2_init=st["Tau2"], compat=compat, sampler=variant)
    data = (Ys, Ntr)
    model._bind_data(data)
    assert _bytes_per_cell(model) == bpc
    omega = rs.gamma(2.0, 0.2, size=(N, M, T))             # Polya-Gamma-like weights, different in every cell
    with np.errstate(divide="ignore"):
        nu2 = np.where(miss, np.inf, 1.0 / omega)
    model.nu2 = nu2
    src_col = stale_col_sources(miss)
    if changes is not None:
        assert sorted(np.flatnonzero(src_col == np.arange(M))) == sorted(set(changes) | {0})
    stale_w, stale_v = _check_sides(compat, N, K, bool(miss.any()), src_col, half, T)
    _compare(model, data, dict(st, nu2=nu2), compat, stale_w, stale_v, variant, K, T,
             lambda s, **kw: orc.binomial_w_step(s, Ys, Ntr, **kw),
             lambda s, D, **kw: orc.binomial_v_step(s, Ys, Ntr, D, **kw))


COMPATS = ["reference", "exact"]
VARIANTS = ["banded", "chain", "banded_nopanel"]

# no NaN: quirk Q1 on every row >= K, Q2 on every column after the first
FULL = [
    # N,    M,  T,  K, half
    (20, 3, 12, 1, ""),
    (20, 3, 12, 2, ""),
    (20, 4, 12, 5, ""),
    (20, 4, 12, 8, ""),           # 8-wave instance, two outputs per lane
    (20, 3, 12, 9, ""),           # one output per lane
    (20, 3, 12, 10, ""),
    (200, 5, 40, 9, "WV"),        # first tile: W rows 0..8 and V column 0 (outputs 0..39) in half 0 only
    (200, 5, 40, 10, "WV"),
    (5, 4, 12, 5, ""),            # N = K: no stale row
    (6, 4, 12, 5, ""),            # N = K + 1: one
    (9, 3, 10, 9, ""),
    (10, 3, 10, 9, ""),
    (600, 2, 10, 3, ""),          # 16 rows per w_solve workgroup, several V chunks per tile
    (1100, 2, 8, 5, ""),          # 32
    (30, 12, 20, 6, ""),          # 240 outputs: two V tiles, the second without a source
    (30, 15, 20, 9, "V"),         # 300 outputs at one output per lane
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("N,M,T,K,half", FULL)
def test_binomial_complete_half_sweeps(N, M, T, K, half, compat, variant):
    _binomial_case(N, M, T, K, compat, variant, half=half, seed=N * 7 + K)


# NaN (Q1 off): the column pattern changes where a source column's outputs straddle the 64-output boundary and a tile
# boundary; odd T pairs outputs of two columns in one lane (two gathers of the source weight), even T keeps them in one
# column (one 16-byte load)
NAN = [
    # N,  M,  T, K, changes
    (24, 30, 10, 6, (6, 12, 25)),      # outputs 60..69 and 120..129
    (24, 30, 9, 6, (7, 14, 22)),       # 63..71 and 126..134
    (24, 30, 10, 9, (6, 12, 25)),
    (24, 30, 9, 9, (7, 14, 22)),
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("N,M,T,K,changes", NAN)
def test_binomial_missing_pattern_half_sweeps(N, M, T, K, changes, compat, variant):
    _binomial_case(N, M, T, K, compat, variant, changes=changes, seed=T * 13 + K)


TRIALS = [
    # trials, N, M, T, K, half
    ("4", 70, 6, 12, 5, "W"),          # bytes; W tile 0: rows 0..4 in half 0, none of 64..69
    ("mixed", 70, 6, 12, 9, "W"),      # bytes, every count 1..127
    ("127", 40, 5, 12, 6, ""),         # bytes at 2 kappa = -127 / +127
    ("128", 40, 5, 12, 6, ""),         # 2 kappa = -128: the f64 pseudo-data
    ("2.5", 70, 6, 12, 9, "W"),        # f64
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("trials,N,M,T,K,half", TRIALS)
def test_binomial_trial_counts_half_sweeps(trials, N, M, T, K, half, compat, variant):
    _binomial_case(N, M, T, K, compat, variant, trials=trials, half=half, seed=len(trials) * 5 + K)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("K", [3, 9, 10])
def test_gaussian_byte_counts_stale_columns(K, compat, variant):
    """Gaussian data, R = 3 with partial replicates (byte counts that vary along the depth axis): two whole rows
    missing give every column one ybar pattern, one more missing cell from column 7 on (outputs 63..71) changes it once
    in the middle of the first tile - MODE 2 in the V half-sweep, MODE 1 (any NaN) in the W half-sweep."""
    from functionalmf_amd.factor import GaussianBayesianTensorFiltering, stale_col_sources
    from oracle import btf_oracle as orc
    N, M, T, R = 22, 20, 9, 3
    rs = np.random.RandomState(40 + K)
    p = _probabilities(rs, N, M, T, K)
    Y = np.log(p / (1 - p))[..., None] + rs.normal(0, 0.7, size=(N, M, T, R))
    Y[rs.rand(N, M, T, R) < 0.3] = np.nan
    Y[..., 0] = np.where(rs.rand(N, M, T) < 0.9, rs.normal(size=(N, M, T)), Y[..., 0])
    Y[:, :, :, 0][np.isnan(Y).all(-1)] = 0.5                 # every cell observed at least once ...
    Y[3] = np.nan                                            # ... but two whole rows
    Y[11] = np.nan
    Y[5, 7:, 2] = np.nan                                     # the one pattern change
    st = _state(rs, N, M, T, K)
    st["nu2"] = 0.6
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=TF, sigma2_init=st["sigma2"], lam2_init=st["lam2"],
                                            nu2_init=st["nu2"], W_init=st["W"], V_init=st["V"], Tau2_init=st["Tau2"],
                                            compat=compat, sampler=variant)
    model._bind_data(Y)
    assert _bytes_per_cell(model) == 9.0 and model.likelihood_form() == "weighted"
    src_col = stale_col_sources(np.isnan(Y).all(-1))
    assert list(np.flatnonzero(src_col == np.arange(M))) == [0, 7]
    stale_w, stale_v = _check_sides(compat, N, K, True, src_col, "", T)
    assert not stale_w and stale_v
    _compare(model, Y, st, compat, stale_w, stale_v, variant, K, T,
             lambda s, **kw: orc.w_step(s, Y, **kw), lambda s, D, **kw: orc.v_step(s, Y, D, **kw))
