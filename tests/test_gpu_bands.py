"""Simultaneous credible bands on the GPU (csrc/btf_bands.h via utils.posterior_bands and
BayesianTensorFiltering.posterior_bands) against the numpy definition (functionalmf_amd/bands.py) on the host-formed
(S,N,M,T) tensor: both methods, with and without a depth mask, at every row-block, padding and tile edge; every nembeds and
transform; exact ties and zero scales with integer factors; determinism across calls, column chunks and the origin of the
samples; an undisturbed chain; the property the call exists for; the library's own refusals.

Tolerances (the conventions of test_gpu_functionals.py): values of the curve 1e-12 * max(1, max|m|) (center, the rank band:
order statistics of m itself); scale 1e-10 relative; the supt crit, stat, lower and upper 1e-8 relative - an absolute error of
2e-12 max|m| in m - center over a scale of at least 1e-3 max|m|, plus the scale's 1e-10 - on inputs for which the test itself
checks that bound on the scale.  The rank inputs keep adjacent sorted values of every cell at least 1e-9 max(1, max|m|)
apart (checked), so no comparison can flip and depth, k and the two shares are equal exactly."""
import numpy as np
import pytest

from functionalmf_amd import bands
from functionalmf_amd.factor import GaussianBayesianTensorFiltering
from functionalmf_amd.utils import posterior_bands

pytestmark = pytest.mark.gpu


def _tensor(Ws, Vs, transform):
    Mu = np.einsum("znk,zmtk->znmt", Ws, Vs)
    if transform == "ilogit":
        Mu = 1 / (1 + np.exp(-Mu))
    elif transform == "square":
        Mu = Mu ** 2
    return Mu


def _inputs_ok(Mu):
    """The inputs' own conditions: every per-cell sd at least 1e-3 max|m|, adjacent sorted values of every cell at least
    1e-9 max(1, max|m|) apart."""
    top = np.abs(Mu).max()
    return Mu.std(0, ddof=1).min() >= 1e-3 * top and np.diff(np.sort(Mu, axis=0), axis=0).min() >= 1e-9 * max(1.0, top)


def _factors(seed, S, N, M, T, K, transform=None, smooth=False):
    """Random factors whose tensor meets _inputs_ok: the first of a fixed sequence of seeds that does (the conditions
    are asserted by the caller all the same)."""
    for k in range(50):
        rs = np.random.RandomState(1000 * seed + k)
        Ws = rs.normal(size=(S, N, K))
        Vs = rs.normal(size=(S, M, T, K))
        if smooth:
            Vs = 0.4 * np.cumsum(Vs, axis=2)
        if transform == "ilogit":
            Ws *= 0.6
        Mu = _tensor(Ws, Vs, transform)
        if _inputs_ok(Mu):
            break
    return Ws, Vs, Mu


def _close(got, ref, tol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max() if ref.size else 0.0
    print("%s: max abs err %.3e (tol %.3e)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _rel(got, ref, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / np.abs(ref))
    print("%s: max rel err %.3e (tol %.3e)" % (what, rel.max(), rtol))
    assert rel.max() <= rtol, (what, rel.max())


def _check_supt(out, ref, Mu, what):
    base = 1e-12 * max(1.0, np.abs(Mu).max())
    _close(out["center"], ref["center"], base, what + " center")
    _rel(out["scale"], ref["scale"], 1e-10, what + " scale")
    _rel(out["crit"], ref["crit"], 1e-8, what + " crit")
    _rel(out["lower"], ref["lower"], 1e-8, what + " lower")
    _rel(out["upper"], ref["upper"], 1e-8, what + " upper")
    assert out["need"] == ref["need"] and np.all(out["inside"] >= ref["need"] / Mu.shape[0])
    assert np.array_equal(out["inside"], ref["inside"]), what


def _check_rank(out, ref, Mu, what):
    base = 1e-12 * max(1.0, np.abs(Mu).max())
    assert out["need"] == ref["need"] and out["k_pointwise"] == ref["k_pointwise"]
    assert np.array_equal(out["k"], ref["k"]), what
    assert np.array_equal(out["inside"], ref["inside"]), what
    assert np.array_equal(out["pointwise_inside"], ref["pointwise_inside"]), what
    _close(out["lower"], ref["lower"], base, what + " lower")
    _close(out["upper"], ref["upper"], base, what + " upper")


def _curves(N, M):
    return sorted({(0, 0), (N - 1, M - 1), (N // 2, M // 2), (min(N - 1, 15), 0), (min(N - 1, 16), M - 1)})


def _mask(T, seed):
    use = np.ones(T, dtype=bool)
    if T > 1:
        use[np.random.RandomState(seed).choice(T, max(1, T // 3), replace=False)] = False
    return use


# S, N, M, T, K, transform, smooth, levels, k expected on the unmasked rank band at the first level ("pos": >= 1 somewhere,
# "zero": 0 somewhere, "both").  N: one lane, a full row block less one, a block and one row; S: 2 (need = S), a power of
# two and its neighbours, two padded rows; T: a single depth, fewer than and more than a moments block (8 depths).
CASES = [(2, 1, 1, 1, 1, None, False, (95, 80), "zero"),
         (2, 63, 1, 2, 3, None, False, (95,), "zero"),
         (63, 63, 3, 2, 2, None, False, (95, 99.9), "both"),
         (64, 65, 1, 7, 5, "ilogit", False, (80, 95), "pos"),
         (65, 65, 3, 70, 4, None, True, (80, 95), "both"),
         (65, 1, 1, 2, 10, "square", False, (80, 95), "pos"),
         (257, 63, 3, 7, 3, None, False, (95, 80), "pos"),
         (257, 1, 3, 70, 2, None, True, (95, 80), "both"),
         # the rank kernels slice the depth axis until 2048 workgroups: every depth a slice above, 2 or 3 depths a slice
         # (65 row tiles x columns) and one slice (2048 of them) here
         (33, 65, 13, 70, 2, None, True, (80,), None),
         (5, 1024, 32, 3, 1, None, False, (60,), None)]


@pytest.mark.parametrize("S,N,M,T,K,transform,smooth,levels,expect_k", CASES)
def test_bands_match_numpy(S, N, M, T, K, transform, smooth, levels, expect_k):
    Ws, Vs, Mu = _factors(S + N + T, S, N, M, T, K, transform, smooth)
    assert _inputs_ok(Mu)
    curves = _curves(N, M)
    for level in levels:
        for depths in (None, _mask(T, S + T)):
            what = "S=%d N=%d M=%d T=%d level=%g mask=%s" % (S, N, M, T, level, depths is not None)
            ref = bands.supt_band(Mu, level, depths)
            out = posterior_bands(Ws, Vs, method="supt", level=level, depths=depths, transform=transform, curves=curves)
            _check_supt(out, ref, Mu, what)
            raw = np.stack([ref["stat"][:, i, j] for i, j in curves])
            _close(out["stat"], raw, 1e-8 * max(1.0, raw.max()), what + " stat")
            ref = bands.rank_band(Mu, level, depths)
            out = posterior_bands(Ws, Vs, method="rank", level=level, depths=depths, transform=transform, curves=curves)
            _check_rank(out, ref, Mu, what)
            assert np.array_equal(out["stat"], np.stack([ref["stat"][:, i, j] for i, j in curves])), what
            if level == levels[0] and depths is None:
                if S == 2 or level == 99.9:
                    assert ref["need"] == S
                assert expect_k not in ("pos", "both") or (ref["k"] >= 1).any()
                assert expect_k not in ("zero", "both") or (ref["k"] == 0).any()


@pytest.mark.parametrize("transform", [None, "ilogit", "square"])
@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds_and_transform(nembeds, transform):
    """All thirty instantiations of the moments, sweep and rank kernels, each on inputs of its own: a kernel of another
    nembeds reads W and V at another stride."""
    S, N, M, T = 33, 70, 2, 5                    # a full 64-row block and a partial one
    Ws, Vs, Mu = _factors(100 * nembeds + len(transform or ""), S, N, M, T, nembeds, transform)
    assert _inputs_ok(Mu)
    what = "K=%d %s" % (nembeds, transform)
    _check_supt(posterior_bands(Ws, Vs, method="supt", level=90, transform=transform), bands.supt_band(Mu, 90), Mu, what)
    _check_rank(posterior_bands(Ws, Vs, method="rank", level=90, transform=transform), bands.rank_band(Mu, 90), Mu, what)


def test_exact_ties_and_zero_scales_with_integer_factors():
    """Integer W and V: every dot product and comparison is exact, so the strict counts of tied values and the depths
    that supt skips are tested as such.  S a power of two: the mean is exact too."""
    rs = np.random.RandomState(3)
    S, N, M, T, K = 64, 6, 5, 8, 3
    Ws = rs.randint(-2, 3, size=(S, N, K)).astype(float)
    Vs = rs.randint(-2, 3, size=(S, M, T, K)).astype(float)
    Vs[:, 0, 2] = 0.0                                        # column 0: scale == 0 at depth 2
    Vs[:, 1] = 0.0                                           # column 1: scale == 0 everywhere
    Mu = _tensor(Ws, Vs, None)
    srt = np.sort(Mu, axis=0)
    assert (srt[1:] == srt[:-1]).any() and Mu.std(0, ddof=1)[:, 2].min() > 0
    curves = [(0, 0), (3, 1), (5, 4)]
    only = np.zeros(T, dtype=bool)
    only[2] = True
    for depths in (None, only):
        ref = bands.rank_band(Mu, 80, depths)
        out = posterior_bands(Ws, Vs, method="rank", level=80, depths=depths, curves=curves)
        for key in ("lower", "upper", "k", "inside", "pointwise_inside"):
            assert np.array_equal(out[key], ref[key]), key
        assert np.array_equal(out["stat"], np.stack([ref["stat"][:, i, j] for i, j in curves]))
        assert np.all(out["stat"][1] == 0) and np.all(out["k"][:, 1] == 0) and np.all(out["inside"][:, 1] == 1.0)
        ref = bands.supt_band(Mu, 80, depths)
        out = posterior_bands(Ws, Vs, method="supt", level=80, depths=depths, curves=curves)
        assert np.array_equal(out["center"], ref["center"])
        assert np.array_equal(out["scale"] == 0, ref["scale"] == 0) and np.all(out["scale"][:, 0, 2] == 0)
        assert np.all(out["scale"][:, 1] == 0) and np.all(out["crit"][:, 1] == 0) and np.all(out["inside"][:, 1] == 1.0)
        assert np.array_equal(out["lower"][:, 1], ref["center"][:, 1]) and np.array_equal(out["upper"][:, 1], ref["center"][:, 1])
        assert np.all(out["stat"][1] == 0)                   # every depth of (3, 1) is skipped: D = 0
        if depths is only:                                   # column 0: the only used depth is skipped
            assert np.all(out["stat"][0] == 0) and np.all(out["crit"][:, 0] == 0)
            assert np.array_equal(out["lower"][:, 0], ref["center"][:, 0])
        _rel(out["scale"], ref["scale"], 1e-10, "scale")
        _rel(out["crit"], ref["crit"], 1e-8, "crit")
        _rel(out["lower"], ref["lower"], 1e-8, "lower")
        _rel(out["upper"], ref["upper"], 1e-8, "upper")
        assert np.array_equal(out["inside"], ref["inside"])
        print("scale bits equal: %s, crit bits equal: %s" % (np.array_equal(out["scale"], ref["scale"]),
                                                             np.array_equal(out["crit"], ref["crit"])))


def _bits_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=k in ("covered", "coverage")), k


def test_same_bits_twice_and_across_column_chunks():
    rs = np.random.RandomState(5)
    S, N, M, T, K = 100, 70, 5, 20, 4
    Ws, Vs = rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K))
    depths = _mask(T, 1)
    for method in ("supt", "rank"):
        kw = dict(method=method, level=90, depths=depths, curves=[(3, 2), (69, 4), (0, 0)])
        a = posterior_bands(Ws, Vs, **kw)
        _bits_equal(a, posterior_bands(Ws, Vs, **kw))
        # the stage of one column (btf_analysis.hip: bands_run): supt (S + 2 T) N doubles, rank T slices of N S integers
        per_col = (S + 2 * T) * N * 8 if method == "supt" else T * N * S * 4
        for cap in (1, per_col, 2 * per_col + 8):            # chunks of 1, 1 and 2 columns: 5, 5 and 3 chunks
            _bits_equal(a, posterior_bands(Ws, Vs, _scratch_bytes=cap, **kw))


def _gauss_data(N=30, M=6, T=12, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W, V = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Mu = np.einsum("nk,mtk->nmt", W, V)
    return Mu, Mu[..., None] + rs.normal(0, 0.4, size=(N, M, T, 2))


def test_device_collected_equals_uploaded_bit_for_bit():
    truth, Y = _gauss_data()
    truth[0, 0, :] = np.nan
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=5)
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        m.posterior_bands()
    res = m.run_gibbs(Y, nburn=10, nsamples=20, verbose=False)
    Mu = _tensor(res["W"], res["V"], None)
    for method in ("supt", "rank"):
        kw = dict(method=method, level=90, curves=[(0, 0), (29, 5)], truth=truth)
        a = m.posterior_bands(**kw)
        _bits_equal(a, m.posterior_bands(res, **kw))
        _bits_equal(a, posterior_bands(res["W"], res["V"], **kw))
        _bits_equal(a, m.posterior_bands(_scratch_bytes=1, **kw))
        ref = (bands.supt_band if method == "supt" else bands.rank_band)(Mu, 90)
        _close(a["lower"], ref["lower"], 1e-8 * np.abs(ref["lower"]).max(), method + " lower")
        covered, cov = bands.coverage(a["lower"], a["upper"], truth)
        assert np.array_equal(a["covered"], covered, equal_nan=True) and a["coverage"] == cov and np.isnan(covered[0, 0])
    with pytest.raises(ValueError, match="unknown method"):
        m.posterior_bands(res, method="bonferroni")
    with pytest.raises(ValueError, match="no depth"):
        m.posterior_bands(depths=np.zeros(12, dtype=bool))


def test_chain_is_undisturbed():
    Y = _gauss_data(seed=1)[1]
    Y[:3, :3] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=7))
    a, b = models
    for m in models:
        res = m.run_gibbs(Y, nburn=4, nsamples=3, verbose=False)
    a.posterior_bands(method="supt", curves=[(1, 1)])
    a.posterior_bands(method="rank", level=60, curves=[(1, 1)])
    a.posterior_bands(res, method="rank")
    for m in models:
        m.run_gibbs(Y, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def smooth_posterior(S=300, N=6, M=2, T=40, K=2, seed=4):
    """Kept samples around a smooth surface: the factors of a fit plus a random walk over depth in V and noise in W."""
    rs = np.random.RandomState(seed)
    W0, V0 = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Ws = W0[None] + 0.1 * rs.normal(size=(S, N, K))
    Vs = V0[None] + 0.05 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2) + 0.1 * rs.normal(size=(S, M, 1, K))
    return Ws, Vs


def test_simultaneous_bands_hold_the_curve_where_the_pointwise_band_does_not():
    Ws, Vs = smooth_posterior()
    S, level = Ws.shape[0], 95
    ref = bands.rank_band(_tensor(Ws, Vs, None), level)
    assert ref["pointwise_inside"].max() < 0.90                      # numpy alone, with margin
    rk = posterior_bands(Ws, Vs, method="rank", level=level)
    sup = posterior_bands(Ws, Vs, method="supt", level=level)
    print("pointwise_inside %.3f..%.3f, rank inside %.3f..%.3f, supt inside %.3f..%.3f" % (
        rk["pointwise_inside"].min(), rk["pointwise_inside"].max(), rk["inside"].min(), rk["inside"].max(),
        sup["inside"].min(), sup["inside"].max()))
    assert np.all(rk["inside"] >= level / 100) and np.all(sup["inside"] >= level / 100)
    assert np.all(rk["pointwise_inside"] < level / 100)
    assert np.all(rk["k"] < rk["k_pointwise"]) and np.all(rk["upper"] >= rk["lower"]) and np.all(sup["upper"] >= sup["lower"])


def test_the_library_refuses_too_many_and_too_few_samples():
    import ctypes as C
    from functionalmf_amd import _native
    lib = _native.load()

    def call(S, method, level=95.0):
        Ws, Vs = np.zeros((S, 1, 1)), np.zeros((S, 1, 2, 1))
        lower, upper, crit, inside = np.zeros((1, 1, 2)), np.zeros((1, 1, 2)), np.zeros((1, 1)), np.zeros((1, 1))
        rc = lib.btf_posterior_bands(0, S, 1, 1, 2, 1, _native.dptr(Ws), _native.dptr(Vs), 0, method, level, None, None, 0, None, None,
                                     _native.dptr(lower), _native.dptr(upper), _native.dptr(crit), _native.dptr(inside), None, None, 0)
        return rc, lib.btf_last_error(None)

    for method, name in ((0, "supt"), (1, "rank")):
        rc, msg = call(bands.MAX_SAMPLES[name] + 1, method)
        assert rc == _native.BTF_EINVAL and b"samples" in msg
        rc, msg = call(1, method)
        assert rc == _native.BTF_EINVAL and b"two samples" in msg
        rc, msg = call(5, method, level=100.0)
        assert rc == _native.BTF_EINVAL and b"level" in msg
    rc, msg = call(5, 2)
    assert rc == _native.BTF_EINVAL and b"method" in msg
    flags = np.zeros(2, dtype=np.int32)
    Ws, Vs, out = np.zeros((5, 1, 1)), np.zeros((5, 1, 2, 1)), np.zeros((1, 1, 2))
    rc = lib.btf_posterior_bands(0, 5, 1, 1, 2, 1, _native.dptr(Ws), _native.dptr(Vs), 0, 0, 95.0, flags.ctypes.data_as(C.POINTER(C.c_int32)),
                                 None, 0, None, None, _native.dptr(out), None, None, None, None, None, 0)
    assert rc == _native.BTF_EINVAL and b"depth" in lib.btf_last_error(None)
    # the limits themselves run: one padded row fills the workgroup's 64 KiB
    for name in ("supt", "rank"):
        S = bands.MAX_SAMPLES[name]
        Ws, Vs = np.ones((S, 1, 1)), np.ones((S, 1, 2, 1))
        Ws[: S // 2] = 2.0                                            # two values, each S / 2 times
        out = posterior_bands(Ws, Vs, method=name, level=50)
        if name == "rank":
            assert out["k"][0, 0] == 0 and out["inside"][0, 0] == 1.0 and out["pointwise_inside"][0, 0] == 0.0
            assert np.all(out["lower"] == 1.0) and np.all(out["upper"] == 2.0)
        else:
            ref = bands.supt_band(_tensor(Ws, Vs, None), 50)
            assert np.all(out["center"] == 1.5) and out["inside"][0, 0] == 1.0
            _rel(out["crit"], ref["crit"], 1e-8, "crit at the limit")
