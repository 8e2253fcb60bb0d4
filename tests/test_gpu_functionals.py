"""Posterior curve functionals on the GPU (csrc/btf_functionals.h via utils.posterior_functionals and
BayesianTensorFiltering.posterior_functionals) against numpy on the host-formed (S,N,M,T) tensor: every functional's mean,
variance, percentiles, raw curve values and pointwise array; exact ties and zeros with integer factors; censoring of the
crossing; determinism, device-collected against uploaded states, an undisturbed chain; the reference application's AUC;
one full-size run.

Tolerances: 1e-12 * max(1, max|m|) for values of the curve (as test_posterior_summary_matches_numpy), times the x range
for auc and times T for rise (sums of T terms); variances 1e-10 relative; positions (argmax, argmin, crossing) 1e-9 of
the x range, on inputs for which the test itself checks that no comparison can flip by rounding."""
import warnings

import numpy as np
import pytest

from functionalmf_amd import functionals
from functionalmf_amd.factor import GaussianBayesianTensorFiltering
from functionalmf_amd.utils import posterior_functionals

pytestmark = pytest.mark.gpu

ALL = functionals.NAMES
Q = (5, 50, 95, 0, 100, 33.3)


def _tensor(Ws, Vs, transform):
    Mu = np.einsum("znk,zmtk->znmt", Ws, Vs)
    if transform == "ilogit":
        Mu = 1 / (1 + np.exp(-Mu))
    elif transform == "square":
        Mu = Mu ** 2
    return Mu


def _tols(Mu, x):
    base = 1e-12 * max(1.0, np.abs(Mu).max())
    span = x[-1] - x[0]
    pos = 1e-9 * span
    return {"auc": base * span, "max": base, "min": base, "rise": base * Mu.shape[-1],
            "argmax": pos, "argmin": pos, "crossing": pos}


def _assert_no_branch_can_flip(Mu, level):
    """The inputs' own condition: top two and bottom two values of every sampled curve differ by more than 1e-9 and no
    |m_t - level| is below 1e-9."""
    srt = np.sort(Mu, axis=-1)
    assert (srt[..., -1] - srt[..., -2]).min() > 1e-9
    assert (srt[..., 1] - srt[..., 0]).min() > 1e-9
    assert np.abs(Mu - level).min() > 1e-9


def _close(got, ref, tol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    if ok.any():
        err = np.abs(got[ok] - ref[ok]).max()
        print("%s: max abs err %.3e (tol %.3e)" % (what, err, tol))
        assert err <= tol, (what, err, tol)


def _rel(got, ref, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    if ok.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(ref[ok] == 0, np.where(got[ok] == 0, 0.0, np.inf), np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))
        print("%s: max rel err %.3e (tol %.3e)" % (what, rel.max(), rtol))
        assert rel.max() <= rtol, (what, rel.max())


def _check_summaries(out, ref, tols, q, exceed=None):
    """out: the device dict; ref: {name: (S,N,M)} from numpy."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for name, v in ref.items():
            o, tol = out[name], tols[name]
            S = v.shape[0]
            if name == "crossing":
                n = (~np.isnan(v)).sum(0)
                assert np.array_equal(o["defined"], n / S)
                mean = np.where(n > 0, np.nanmean(v, axis=0), np.nan)
                var = np.where(n > 1, np.nanvar(v, axis=0, ddof=1), np.nan)
                quant = functionals.censored_percentile(v, q, axis=0)
            else:
                mean = v.mean(0)
                var = v.var(0, ddof=1) if S > 1 else np.full(v.shape[1:], np.nan)
                quant = np.percentile(v, q, axis=0)
            _close(o["mean"], mean, tol, name + " mean")
            _rel(o["var"], var, 1e-10, name + " var")
            _close(o["quantiles"], quant, tol, name + " quantiles")
            if exceed is not None:
                assert np.array_equal(o["prob_above"], (v > exceed).sum(0) / S), name


CASES = [(37, 5, 4, 6, 3, None, False), (200, 9, 7, 5, 2, "ilogit", True), (1000, 3, 5, 11, 5, None, True),
         (1025, 9, 7, 370, 5, None, False), (2, 4, 3, 2, 4, None, False), (1, 3, 2, 2, 2, "ilogit", False),
         (64, 70, 1, 9, 10, "square", True), (33, 130, 2, 7, 1, None, False), (1025, 2, 3, 4, 1, "square", False)]


@pytest.mark.parametrize("S,N,M,T,K,transform,own_x", CASES)
def test_functionals_match_numpy(S, N, M, T, K, transform, own_x):
    rs = np.random.RandomState(0 if S == 1025 and T == 370 else S + N)
    Ws = rs.normal(size=(S, N, K))
    Vs = rs.normal(size=(S, M, T, K))
    x = np.cumsum(rs.uniform(0.2, 3.0, size=T)) if own_x else None
    level = {None: 0.3, "ilogit": 0.55, "square": 0.3}[transform]
    Mu = _tensor(Ws, Vs, transform)
    _assert_no_branch_can_flip(Mu, level)
    xs = functionals.default_x(T) if x is None else x
    ref = functionals.curve_functionals(Mu, xs, level=level)
    tols = _tols(Mu, xs)
    curves = [(0, 0), (N - 1, M - 1), (N // 2, M // 2)]
    exceed = 0.4
    small = S * N * M <= 100000
    out = posterior_functionals(Ws, Vs, which=ALL, q=Q, transform=transform, x=x, level=level, exceed=exceed, curves=curves,
                                pointwise=small)
    assert set(out) == set(ALL)
    _check_summaries(out, ref, tols, Q, exceed=exceed)
    for name in ALL:
        raw = np.stack([ref[name][:, i, j] for i, j in curves])
        _close(out[name]["curves"], raw, tols[name], name + " curves")
        if small:
            _close(out[name]["pointwise"], ref[name], tols[name], name + " pointwise")


@pytest.mark.parametrize("transform", [None, "ilogit", "square"])
@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds_and_transform(nembeds, transform):
    """All thirty instantiations of func_sweep_kernel<K, transform> behind func_sweep_fn, each on inputs of its own: a kernel
    of another nembeds reads W and V at another stride, and every functional of every curve is then wrong."""
    S, N, M, T = 5, 70, 2, 6                     # a full 64-row block and a partial one
    rs = np.random.RandomState(100 * nembeds + len(transform or ""))
    Ws, Vs = rs.normal(size=(S, N, nembeds)), rs.normal(size=(S, M, T, nembeds))
    x = np.cumsum(rs.uniform(0.2, 3.0, size=T))
    level = {None: 0.3, "ilogit": 0.55, "square": 0.3}[transform]
    Mu = _tensor(Ws, Vs, transform)
    _assert_no_branch_can_flip(Mu, level)
    ref = functionals.curve_functionals(Mu, x, level=level)
    assert np.isnan(ref["crossing"]).any() and not np.isnan(ref["crossing"]).all()
    tols = _tols(Mu, x)
    out = posterior_functionals(Ws, Vs, which=ALL, q=Q, transform=transform, x=x, level=level, exceed=0.4, pointwise=True)
    assert set(out) == set(ALL)
    for name in ALL:
        _close(out[name]["pointwise"], ref[name], tols[name], "K=%d %s %s pointwise" % (nembeds, transform, name))
    _check_summaries(out, ref, tols, Q, exceed=0.4)


def test_exact_ties_and_zeros_with_integer_factors():
    """Integer W, V, x and level: every dot product, difference and comparison is exact, so the first-occurrence and
    the d == 0 rules are tested as such."""
    rs = np.random.RandomState(3)
    S, N, M, T, K = 50, 6, 5, 8, 3
    Ws = rs.randint(-2, 3, size=(S, N, K)).astype(float)
    Vs = rs.randint(-2, 3, size=(S, M, T, K)).astype(float)
    x = np.cumsum(rs.randint(1, 4, size=T)).astype(float)
    level = 1.0
    Mu = _tensor(Ws, Vs, None)
    srt = np.sort(Mu, axis=-1)
    assert (srt[..., -1] == srt[..., -2]).any() and (srt[..., 0] == srt[..., 1]).any()       # ties in both extremes
    assert (Mu[..., 0] == level).any() and (Mu[..., 1:] == level).any() and (Mu == Mu[..., :1]).all(-1).any()
    ref = functionals.curve_functionals(Mu, x, level=level)
    assert np.isnan(ref["crossing"]).any() and not np.isnan(ref["crossing"]).all()
    out = posterior_functionals(Ws, Vs, which=ALL, q=Q, x=x, level=level, pointwise=True)
    for name in ("max", "min", "argmax", "argmin", "rise", "auc"):
        assert np.array_equal(out[name]["pointwise"], ref[name]), name
    _close(out["crossing"]["pointwise"], ref["crossing"], 1e-12 * x[-1], "crossing pointwise")
    _check_summaries(out, ref, _tols(Mu, x), Q)


def test_crossing_censoring():
    S, S_cross, N, T = 20, 12, 3, 9
    x = functionals.default_x(T)
    rs = np.random.RandomState(1)
    a = rs.uniform(0.8, 1.2, size=S)
    Ws = np.ones((S, N, 1)) * (1.0 + 0.1 * np.arange(N))[None, :, None]
    Vs = np.zeros((S, 3, T, 1))
    Vs[:S_cross, 0, :, 0] = a[:S_cross, None] * (1.0 - 0.9 * x)[None]            # falls through 0.5 inside the range
    Vs[S_cross:, 0, :, 0] = a[S_cross:, None] * (1.0 - 0.1 * x)[None]            # stays above 0.7: never crosses
    Vs[:, 1, :, 0] = a[:, None] * (2.0 + x)[None]                               # never crosses in any sample
    Vs[:, 2, :, 0] = a[:, None] * (1.0 - 0.95 * x)[None]                        # crosses in every sample
    perm = rs.permutation(S)                                                    # censored samples anywhere in the order
    Ws, Vs = Ws[perm], Vs[perm]
    level = 0.5
    Mu = _tensor(Ws, Vs, None)
    ref = functionals.curve_functionals(Mu, x, level=level)["crossing"]
    share = (~np.isnan(ref)).mean(0)
    assert np.array_equal(share, np.tile([S_cross / S, 0.0, 1.0], (N, 1)))       # the constructed shares, on the numpy side
    q = (5, 25, 50, 55, 60, 75, 100)
    rq = functionals.censored_percentile(ref, q, axis=0)
    assert np.isfinite(rq[:4, :, 0]).all() and np.isnan(rq[4:, :, 0]).all() and np.isfinite(rq[:, :, 2]).all()
    out = posterior_functionals(Ws, Vs, which=("crossing",), q=q, level=level, exceed=0.5, curves=[(0, 0), (1, 1)])["crossing"]
    assert np.array_equal(out["defined"], share)
    with np.errstate(invalid="ignore"):
        numpy_inf = np.percentile(np.where(np.isnan(ref), np.inf, ref), q, axis=0)
    _close(out["quantiles"][:4, :, 0], numpy_inf[:4, :, 0], 1e-9, "quantiles below the share")
    assert np.isnan(out["quantiles"][4:, :, 0]).all()
    _close(out["quantiles"][:, :, 2], numpy_inf[:, :, 2], 1e-9, "quantiles of the always-crossing column")
    assert np.isnan(out["quantiles"][:, :, 1]).all() and np.isnan(out["mean"][:, 1]).all() and np.isnan(out["var"][:, 1]).all()
    assert np.all(out["defined"][:, 1] == 0.0) and np.all(out["prob_above"][:, 1] == 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        _close(out["mean"], np.nanmean(ref, axis=0), 1e-9, "mean over the defined samples")
        _rel(out["var"], np.where(share > 0, np.nanvar(ref, axis=0, ddof=1), np.nan), 1e-10, "var over the defined samples")
    assert np.array_equal(out["prob_above"], (ref > 0.5).mean(0))
    assert np.array_equal(np.isnan(out["curves"][0]), np.isnan(ref[:, 0, 0])) and np.isnan(out["curves"][1]).all()


def _bits_equal(a, b):
    assert set(a) == set(b)
    for name in a:
        assert set(a[name]) == set(b[name]), name
        for k in a[name]:
            assert np.array_equal(a[name][k], b[name][k], equal_nan=True), (name, k)


def test_same_bits_twice_and_one_functional_equals_all():
    rs = np.random.RandomState(5)
    S, N, M, T, K = 300, 70, 5, 20, 4
    Ws, Vs = rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K))
    kw = dict(q=Q, level=0.2, exceed=0.1, curves=[(3, 2), (69, 4)], pointwise=True)
    a = posterior_functionals(Ws, Vs, which=ALL, **kw)
    b = posterior_functionals(Ws, Vs, which=ALL, **kw)
    _bits_equal(a, b)
    for name in ALL:
        one = posterior_functionals(Ws, Vs, which=(name,), **kw)
        _bits_equal(one, {name: a[name]})
    rev = posterior_functionals(Ws, Vs, which=ALL[::-1], **kw)
    _bits_equal(rev, a)


def _gauss_data(N=30, M=6, T=12, K=3, seed=0):
    rs = np.random.RandomState(seed)
    W, V = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    return np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.4, size=(N, M, T, 2))


def test_device_collected_equals_uploaded_bit_for_bit():
    Y = _gauss_data()
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=5)
    with pytest.raises(RuntimeError, match="no samples collected on the device"):
        m.posterior_functionals()
    res = m.run_gibbs(Y, nburn=10, nsamples=20, verbose=False)
    kw = dict(which=ALL, q=Q, level=0.1, exceed=0.0, curves=[(0, 0), (29, 5)], pointwise=True)
    a = m.posterior_functionals(**kw)
    b = m.posterior_functionals(res, **kw)
    c = posterior_functionals(res["W"], res["V"], **kw)
    _bits_equal(a, b)
    _bits_equal(a, c)
    Mu = _tensor(res["W"], res["V"], None)
    _close(a["auc"]["mean"], functionals.curve_functionals(Mu)["auc"].mean(0), 1e-12 * max(1.0, np.abs(Mu).max()), "auc mean")
    with pytest.raises(ValueError, match="level"):
        m.posterior_functionals(which=("crossing",))
    with pytest.raises(ValueError, match="unknown functional"):
        m.posterior_functionals(res, which=("area",))


def test_chain_is_undisturbed():
    Y = _gauss_data(seed=1)
    Y[:3, :3] = np.nan
    models = []
    for _ in range(2):
        np.random.seed(11)
        models.append(GaussianBayesianTensorFiltering(30, 6, 12, nembeds=3, rng="device", device_seed=7))
    a, b = models
    for m in models:
        res = m.run_gibbs(Y, nburn=4, nsamples=3, verbose=False)
    a.posterior_functionals(which=ALL, level=0.0, exceed=0.0, curves=[(1, 1)], pointwise=True)
    a.posterior_functionals(res, which=("auc", "crossing"), level=0.0)
    for m in models:
        m.run_gibbs(Y, nburn=3, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2)
    for k in ("nu2", "sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_auc_mean_is_the_reference_applications_quantity():
    """doseresponse/feature_importance.py:40 on the same samples (default x, no transform)."""
    rs = np.random.RandomState(8)
    S, N, M, T, K = 120, 40, 6, 9, 4
    Ws, Vs = rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    Mu = np.einsum('znk,zmtk->znmt', Ws, Vs)
    want = trapz(Mu, dx=1 / (T - 1), axis=-1).mean(axis=0)
    got = posterior_functionals(Ws, Vs)["auc"]["mean"]
    _close(got, want, 1e-12 * max(1.0, np.abs(Mu).max()), "auc mean against feature_importance.py:40")


def test_too_many_samples_is_refused_by_the_library():
    import ctypes as C
    from functionalmf_amd import _native
    lib = _native.load()
    S = functionals.MAX_SAMPLES + 1
    Ws, Vs, x = np.zeros((S, 1, 1)), np.zeros((S, 1, 2, 1)), np.array([0.0, 1.0])
    which = np.zeros(1, dtype=np.int32)
    mean = np.zeros((1, 1, 1))
    rc = lib.btf_posterior_functionals(0, S, 1, 1, 2, 1, _native.dptr(Ws), _native.dptr(Vs), 0, which.ctypes.data_as(C.POINTER(C.c_int32)),
                                       1, _native.dptr(x), float("nan"), float("nan"), None, 0, None, 0, _native.dptr(mean), None, None,
                                       None, None, None, None)
    assert rc == _native.BTF_EINVAL and b"samples" in lib.btf_last_error(None)
    # the limit itself runs
    Ws, Vs = np.ones((S - 1, 1, 1)), np.ones((S - 1, 1, 2, 1))
    out = posterior_functionals(Ws, Vs, which=("auc", "max"), q=(50,))
    assert out["auc"]["mean"][0, 0] == 1.0 and out["max"]["quantiles"][0, 0, 0] == 1.0 and out["auc"]["var"][0, 0] == 0.0


def test_full_size_run():
    """(512, 256, 64), K = 5, S = 1000 uploaded samples: finishes; spot curves agree with numpy computed for them alone."""
    S, N, M, T, K = 1000, 512, 256, 64, 5
    rs = np.random.RandomState(0)
    Ws = rs.normal(size=(S, N, K))
    Vs = rs.standard_normal(size=(S, M, T, K))
    curves = [(0, 0), (511, 255), (100, 7), (63, 128), (64, 129), (300, 200)]
    level, q = 0.3, (5, 50, 95)
    which = ("auc", "argmax", "crossing")
    out = posterior_functionals(Ws, Vs, which=which, q=q, level=level, curves=curves)
    x = functionals.default_x(T)
    for c, (i, j) in enumerate(curves):
        Mu = np.einsum("zk,ztk->zt", Ws[:, i], Vs[:, j])
        _assert_no_branch_can_flip(Mu, level)
        ref = functionals.curve_functionals(Mu, x, level=level)
        tols = _tols(Mu, x)
        for name in which:
            _close(out[name]["curves"][c], ref[name], tols[name], "%s curve %r" % (name, (i, j)))
        one = {name: {k: (v[:, i, j][:, None, None] if k == "quantiles" else v[i, j][None, None]) for k, v in out[name].items()
                      if k != "curves"} for name in which}
        _check_summaries(one, {name: ref[name][:, None, None] for name in which}, tols, q)
