"""Host halves of the convergence diagnostics (functionalmf_amd/diagnostics.py): chain_diagnostics against the numpy
statement of Vehtari et al. (2021), its behaviour on known chains and edge cases, and the refusals convergence() makes
before any device call.  No GPU."""
import types

import numpy as np
import pytest
from scipy.stats import norm, rankdata

from functionalmf_amd import _native, diagnostics
from functionalmf_amd.factor import GaussianBayesianTensorFiltering


# ---- the definition, transcribed on its own (split / zscale / rhat / ess / diag)
def _split(x):
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, x.shape[1] - h:]], axis=0)


def _zscale(x):
    r = rankdata(x, method="average").reshape(x.shape)
    return norm.ppf((r - 0.375) / (x.size + 0.25))


def _rhat(x):
    C, n = x.shape
    B = n * np.var(x.mean(1), ddof=1)
    W = np.mean(np.var(x, axis=1, ddof=1))
    return np.sqrt((B / W + n - 1) / n)


def _ess(x, pairs=None):
    """pairs: a list that receives every (even, odd) the rule reads, the first (1, rho[1]) included."""
    C, n = x.shape
    xc = x - x.mean(1, keepdims=True)
    acov = np.array([[np.dot(xc[c, :n - t], xc[c, t:]) / n for t in range(n)] for c in range(C)])
    mean_var = acov[:, 0].mean() * n / (n - 1)
    var_plus = mean_var * (n - 1) / n + (np.var(x.mean(1), ddof=1) if C > 1 else 0.0)
    rho = np.zeros(n)
    rho[0] = even = 1.0
    rho[1] = odd = 1.0 - (mean_var - acov[:, 1].mean()) / var_plus
    if pairs is not None:
        pairs.append((even, odd))
    t = 1
    while t < n - 3 and even + odd > 0:
        even = 1.0 - (mean_var - acov[:, t + 1].mean()) / var_plus
        odd = 1.0 - (mean_var - acov[:, t + 2].mean()) / var_plus
        if pairs is not None:
            pairs.append((even, odd))
        if even + odd >= 0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2
        t += 2
    tau = -1 + 2 * rho[:max_t + 1].sum() + rho[max_t + 1:max_t + 2].sum()
    tau = max(tau, 1 / np.log10(C * n))
    return C * n / tau


def spec(x, pairs=None):
    """pairs: a list that receives four lists, the (even, odd) pairs of the bulk, q05, q95 and raw series (see _ess)."""
    p = [None] * 4 if pairs is None else [[] for _ in range(4)]
    s = _split(x)
    folded = np.abs(x - np.median(x))
    r = max(_rhat(_zscale(s)), _rhat(_zscale(_split(folded))))
    eb = _ess(_zscale(s), p[0])
    q05, q95 = np.quantile(x, [0.05, 0.95])
    et = min(_ess(_split((x <= q05).astype(float)), p[1]), _ess(_split((x <= q95).astype(float)), p[2]))
    mcse = np.std(x, ddof=1) / np.sqrt(_ess(s, p[3]))
    if pairs is not None:
        pairs.extend(p)
    return np.array([r, eb, et, mcse])


def pairs_margin(pairs):
    """The smallest |even + odd| and |even| over the pairs of the four series, as spec(x, pairs) lists them.  Geyer's rule
    branches on the sign of exactly these values, so a series with a small margin may legitimately come out differently
    from two correct float64 evaluations.  A pair of a constant series is nan (0 / 0, exactly, in any order of summation)
    and compares false either way: it is left out."""
    with np.errstate(invalid="ignore"):
        v = np.array([[abs(e + o), abs(e)] for series in pairs for e, o in series])
    return float(np.nanmin(v))


def geyer_margin(x):
    pairs = []
    with np.errstate(divide="ignore", invalid="ignore"):
        spec(x, pairs)
    return pairs_margin(pairs)


def got(x):
    d = diagnostics.chain_diagnostics(x)
    return np.array([d["rhat"], d["ess_bulk"], d["ess_tail"], d["mcse_mean"]])


def ar1(rs, C, S, phi, shift=0.0):
    e = rs.normal(size=(C, S))
    x = np.zeros((C, S))
    x[:, 0] = e[:, 0] / np.sqrt(1 - phi * phi)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x + shift


CASES = {
    "iid_4x1000": lambda rs: rs.normal(size=(4, 1000)),
    "ar09_4x400": lambda rs: ar1(rs, 4, 400, 0.9),
    "odd_S": lambda rs: ar1(rs, 3, 101, 0.3),
    "S4": lambda rs: rs.normal(size=(2, 4)),
    "S5_one_chain": lambda rs: rs.normal(size=(1, 5)),
    "ties": lambda rs: rs.randint(0, 4, size=(4, 60)).astype(float),
    "heavy_ties_q95": lambda rs: np.minimum(rs.randint(0, 10, size=(2, 40)), 7).astype(float),
    "one_chain": lambda rs: ar1(rs, 1, 300, 0.6),
    "shifted": lambda rs: rs.normal(size=(4, 200)) + np.array([0.0, 0.0, 0.0, 1.0])[:, None],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_chain_diagnostics_match_the_definition(case):
    x = CASES[case](np.random.RandomState(sorted(CASES).index(case) + 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        want = spec(x)
    assert np.allclose(got(x), want, rtol=1e-12, atol=0.0, equal_nan=True), (got(x), want)


def test_reported_values_of_the_definition():
    rs = np.random.RandomState(0)
    d = diagnostics.chain_diagnostics(rs.normal(size=(4, 1000)))
    assert abs(d["rhat"] - 1.0) < 0.01 and 3000 < d["ess_bulk"] < 5000


def test_ar1_bulk_ess_near_theory():
    phi, C, S = 0.5, 4, 2000
    x = ar1(np.random.RandomState(1), C, S, phi)
    want = C * S * (1 - phi) / (1 + phi)
    assert abs(diagnostics.chain_diagnostics(x)["ess_bulk"] / want - 1.0) < 0.25


def test_shifted_chain_is_flagged():
    x = np.random.RandomState(2).normal(size=(4, 1000))
    x[3] += 1.0
    assert diagnostics.chain_diagnostics(x)["rhat"] > 1.05
    assert diagnostics.chain_diagnostics(x[:3])["rhat"] < 1.01


def test_constant_and_non_finite_series_give_nan():
    for x in (np.full((2, 10), 3.5), np.r_[np.ones(9), np.nan][None], np.r_[np.zeros(7), np.inf][None]):
        assert all(np.isnan(v) for v in diagnostics.chain_diagnostics(x).values())


def test_one_dimensional_input_is_one_chain():
    x = np.random.RandomState(4).normal(size=51)
    assert np.array_equal(got(x), got(x[None]))
    with pytest.raises(ValueError):
        diagnostics.chain_diagnostics(np.ones((2, 3)))


def test_geyer_margin_counts_every_pair_and_skips_a_constant_series():
    x = ar1(np.random.RandomState(7), 2, 40, 0.9)
    pairs = []
    spec(x, pairs)
    assert len(pairs) == 4 and all(p[0][0] == 1.0 and len(p) >= 2 for p in pairs)
    assert geyer_margin(x) == min(min(abs(e + o), abs(e)) for p in pairs for e, o in p) > 0
    y = CASES["heavy_ties_q95"](np.random.RandomState(7))           # the q95 indicator is constant: its one pair is nan
    assert np.isfinite(geyer_margin(y))


def test_every_series_of_the_gpu_shape_suite_meets_its_conditions():
    """tests/test_gpu_diagnostics_shapes.py compares the kernel with spec only on series where Geyer's rule is away from
    its branch points and no R-hat is 0 / 0; the same builders, the same assertion, no GPU."""
    import test_gpu_diagnostics_shapes as shapes
    count = 0
    for cid, xs in shapes.host_cases():
        for i, x in enumerate(xs):
            want, _, margin, posed = shapes.conditions(x)
            assert margin > shapes.MARGIN and posed and np.all(np.isfinite(want)), (cid, i, margin, posed, want)
            count += 1
    assert count > 800


# ---- refusals before any device call
class _NoDevice:
    """Stands in for the native library: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def _res(S=6, N=3, M=2, T=4, K=2):
    return {"W": np.zeros((S, N, K)), "V": np.zeros((S, M, T, K))}


def _model(collected=6, N=3, M=2, T=4, K=2, device=0, world=1):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.device = N, M, T, K, device
    m._collected = collected
    m._plan = types.SimpleNamespace(world=world)
    m._exchange = types.SimpleNamespace(active=False)
    return m


def test_refusals_before_any_device_call(no_device):
    conv = diagnostics.convergence
    bad = [
        [_res(S=6), _res(S=7)],                      # different S
        [_res(N=3), _res(N=4)],                      # different shapes
        [_res(K=2), _res(K=3)],
        [_res(S=3)],                                 # S < 4
        [_res(S=3), _res(S=3)],
        [_res(K=11)],                                # nembeds outside 1..10
        [_res(S=1000, N=1, M=1, T=1)] * 5,           # 5000 pooled draws
        [_res(S=4, N=1, M=1, T=1)] * 65,             # 65 chains
        [_model(device=0), _model(device=1)],        # models on different devices
        [{"V": np.zeros((6, 2, 4, 2))}],             # no W
        [{"W": np.zeros((6, 3)), "V": np.zeros((6, 2, 4, 2))}],
        ["not a chain"],
        [],
    ]
    for chains in bad:
        with pytest.raises(ValueError):
            conv(chains)
    for t in ("log", "Identity", 1):
        with pytest.raises(ValueError):
            conv(_res(), transform=t)
    with pytest.raises(ValueError):
        conv([_model(), _res(S=7)])
    with pytest.raises(ValueError):
        conv([_model(K=11)])
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        conv([_model(collected=0), _res()])
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        _model(collected=0).convergence_diagnostics(_res())
    with pytest.raises(NotImplementedError):
        conv([_model(world=2)])
    with pytest.raises(ValueError):
        _model().convergence_diagnostics(_res(), transform="exp")


def test_the_documented_limit_admits_four_chains_of_1000():
    assert diagnostics.MAX_POOLED_DRAWS >= 4096 and diagnostics.MAX_CHAINS >= 4
