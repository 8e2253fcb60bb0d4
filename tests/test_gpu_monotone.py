"""Monotone projection of the posterior on the GPU (csrc/btf_monotone.h via utils.posterior_monotone and
BayesianTensorFiltering.posterior_monotone): bit for bit against utils.factor_pav per sample (nmf_pav_kernel), against the
reference's factor_pav (tests/golden/g17_monotone.npz, written by tests/golden/make_golden_monotone.py) to the 1e-12
relative tests/test_gpu_nmf.py holds factor_pav to, and the summary of the projected states bit for bit against
utils.posterior_summary on them.

Inputs, per case, with rs = RandomState(seed):  Ws = rs.gamma(1, 1, (S,N,K)),
Vs = 0.2 * rs.gamma(1, 1, (S,M,T,K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, noise, (S,M,T,K)): decreasing trends with
noise, so the pools are rich (6 to 9 of 12, 7 to 13 of 20, ...) and the smallest non-zero step of a projected curve is
5.9e-6 of its scale - no vote can flip between numpy's dot product and the device's FMA chain.  The five fixture cases, and
GPU-only: N above the register-resident bound at K <= 5 (1024) and at K >= 6 (512), T = 1, and M = 1 with S = 1."""
import ctypes as C
import os

import numpy as np
import pytest

from functionalmf_amd import _native, monotone, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_monotone.npz")
Q = (5, 95)
# name -> (S, N, M, T, K), noise, seed; the first five are the fixture's
CASES = {
    "c0": ((6, 70, 3, 12, 3), 0.15, 1),
    "c1": ((3, 300, 2, 9, 5), 0.1, 2),
    "c2": ((4, 37, 5, 20, 2), 0.3, 3),
    "c3": ((2, 5, 2, 2, 1), 0.5, 4),
    "c4": ((3, 130, 2, 16, 10), 0.05, 5),
    "N1100_K2": ((2, 1100, 2, 8, 2), 0.15, 6),       # 76 rows beyond the 1024 a workgroup keeps in registers at K <= 5
    "N600_K6": ((2, 600, 2, 8, 6), 0.15, 7),         # 88 rows beyond the 512 at K >= 6
    "T1": ((3, 20, 2, 1, 3), 0.15, 8),
    "M1_S1": ((1, 40, 1, 10, 3), 0.3, 9),
}
FIXTURE_CASES = ["c0", "c1", "c2", "c3", "c4"]


def _recipe(dims, noise, seed):
    S, N, M, T, K = dims
    rs = np.random.RandomState(seed)
    Ws = rs.gamma(1, 1, (S, N, K))
    Vs = np.ascontiguousarray(0.2 * rs.gamma(1, 1, (S, M, T, K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, noise, (S, M, T, K)))
    Ws.setflags(write=False)
    Vs.setflags(write=False)
    return Ws, Vs


def _inputs(name):
    return _recipe(*CASES[name])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs():
    """{(name, increasing): (Ws, Vs, the call's dict)}: every case projected once in both directions."""
    out = {}
    for name in CASES:
        Ws, Vs = _inputs(name)
        for inc in (False, True):
            r = utils.posterior_monotone(Ws, Vs, q=Q, increasing=inc)
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            out[name, inc] = (Ws, Vs, r)
    return out


BOTH = [(n, inc) for n in CASES for inc in (False, True)]
IDS = ["%s-%s" % (n, "inc" if inc else "dec") for n, inc in BOTH]


@pytest.mark.parametrize("name,inc", BOTH, ids=IDS)
def test_bit_for_bit_against_factor_pav_per_sample(runs, name, inc):
    Ws, Vs, out = runs[name, inc]
    (S, N, M, T, K) = CASES[name][0]
    assert out["V"].shape == (S, M, T, K) and out["pools"].shape == (S, M) and out["pools"].dtype == np.int32
    assert out["nsamples"] == S
    for s in range(S):
        ref = -utils.factor_pav(Ws[s], -Vs[s]) if inc else utils.factor_pav(Ws[s], Vs[s])
        assert np.array_equal(out["V"][s], ref), (name, inc, s)
    # pools = the runs of equal consecutive depths of the projected block (the inputs have no two equal depths)
    runs_ = 1 + np.any(out["V"][:, :, 1:] != out["V"][:, :, :-1], axis=3).sum(axis=2)
    assert np.array_equal(out["pools"], runs_)
    if name in ("c0", "c2") and not inc:
        assert out["pools"].min() < T - 2 and out["pools"].max() < T      # rich pool structures, not a trivial pass


@pytest.mark.parametrize("name", FIXTURE_CASES)
@pytest.mark.parametrize("inc", [False, True], ids=["dec", "inc"])
def test_against_the_reference_fixture(runs, golden, name, inc):
    Ws, Vs, out = runs[name, inc]
    p = name + "_"
    assert np.array_equal(golden[p + "Ws"], Ws) and np.array_equal(golden[p + "Vs"], Vs)      # the recipe is the fixture's
    ref = golden[p + ("Pinc" if inc else "P")]
    err = np.abs(out["V"] - ref).max() / np.abs(ref).max()
    print("%s increasing=%s: relative error %.3g" % (name, inc, err))
    assert err <= 1e-12
    assert np.array_equal(out["pools"], golden[p + ("pools_inc" if inc else "pools")])


@pytest.mark.parametrize("name", ["N1100_K2", "N600_K6", "T1", "M1_S1"])
def test_gpu_only_cases_against_the_numpy_definition(runs, name):
    for inc in (False, True):
        Ws, Vs, out = runs[name, inc]
        ref, pools = monotone.project_host(Ws, Vs, increasing=inc)
        assert np.abs(out["V"] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(out["pools"], pools)
    if name == "T1":
        assert np.array_equal(out["V"], Vs) and (out["pools"] == 1).all() and (out["changed"] == 0).all()
    else:
        assert (runs[name, False][2]["pools"] < CASES[name][0][3]).any()


# ---------------------------------------------------------------- every nembeds, register-row bound and depth loop
# mono_project_kernel<K> keeps nr = min(mono_rows(K), ceil(N / 256)) rows of W per thread in registers (mono_rows = 4 at
# K <= 5, 2 at K >= 6) and reads the rows from 256 * mono_rows(K) on from global memory at every vote; its loops over the
# depths step by 256 threads.  name -> (S, N, M, T, K), noise, seed: the module's recipe.
SHAPES = {}
for _k in range(1, 11):
    SHAPES["K%d" % _k] = ((2, 70, 2, 12, _k), 0.15, 20 + _k)
for _k, _ns in ((1, (255, 256, 257, 512, 513, 768, 769, 1024, 1025)), (5, (255, 256, 257, 512, 513, 768, 769, 1024, 1025)),
                (6, (256, 257, 512, 513)), (10, (256, 257, 512, 513))):
    for _n in _ns:                               # nr = 1 | 2 | 3 | 4 | 4 + fallback (K <= 5);  1 | 2 | 2 + fallback (K >= 6)
        SHAPES["N%d_K%d" % (_n, _k)] = ((2, _n, 2, 8, _k), 0.15, 1000 * _k + _n)
for _t in (2, 257, 300):                         # one trip of the depth loops, a second trip of one thread, of 44
    SHAPES["T%d" % _t] = ((2, 20, 2, _t, 3), 0.15, 40 + _t)


def _nr(N, K):
    """(register rows in use, rows read from global memory at every vote)."""
    rows = 4 if K <= 5 else 2
    return min(rows, -(-N // 256)), max(0, N - 256 * rows)


def _host_with_margin(Ws, Vs, inc):
    """monotone.project_host's walk once more, recording the smallest non-zero |w_i . v_t - w_i . v_{t+1}| any vote saw, over
    the largest |w_i . v_t|: a vote can differ between numpy's dot product and the device's FMA chain (about 1e-16 of the
    scale apart) only below it.  Exact zeros are the pairs inside a pool: bit-identical depths on both sides.
    Returns (V', pools, margin)."""
    out, pools, margin = np.empty_like(Vs), np.empty(Vs.shape[:2], dtype=np.int32), np.inf
    for s in range(Vs.shape[0]):
        W = Ws[s]
        for j in range(Vs.shape[1]):
            V = np.array(Vs[s, j])
            T = V.shape[0]
            scale = np.abs(W @ V.T).max()
            first, merges, merged = np.arange(T), 0, True
            while merged:
                merged, t = False, 0
                while t < T - 1:
                    step = (W @ V[t + 1] - W @ V[t]) if inc else (W @ V[t] - W @ V[t + 1])
                    nz = np.abs(step[step != 0])
                    if nz.size:
                        margin = min(margin, nz.min() / scale)
                    if np.any(step < 0):
                        mine, next_ = first == first[t], first == first[t + 1]
                        w0, w1 = int(mine.sum()), int(next_.sum())
                        V[mine | next_] = (w0 * V[t] + w1 * V[t + 1]) / (w0 + w1)
                        first[next_] = first[t]
                        merges, merged, t = merges + 1, True, t + w1
                    else:
                        t += 1
            out[s, j], pools[s, j] = V, T - merges
    return out, pools, margin


def test_the_shapes_reach_every_register_row_count():
    assert {_nr(SHAPES[n][0][1], SHAPES[n][0][4]) for n in SHAPES if n.startswith("N") and n.endswith(("_K1", "_K5"))} == \
        {(1, 0), (2, 0), (3, 0), (4, 0), (4, 1)}
    assert {_nr(SHAPES[n][0][1], SHAPES[n][0][4]) for n in SHAPES if n.endswith(("_K6", "_K10"))} == {(1, 0), (2, 0), (2, 1)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bit_for_bit_against_the_numpy_definition(name):
    dims, noise, seed = SHAPES[name]
    S, N, M, T, K = dims
    Ws, Vs = _recipe(dims, noise, seed)
    for inc in (False, True):
        ref, pools = monotone.project_host(Ws, Vs, increasing=inc)
        again, pools2, margin = _host_with_margin(Ws, Vs, inc)
        assert np.array_equal(again, ref) and np.array_equal(pools2, pools)          # the walk above is the definition's
        print("%s increasing=%s: smallest non-zero step of a vote %.3g of the scale, pools %d..%d of %d"
              % (name, inc, margin, pools.min(), pools.max(), T))
        assert margin > 1e-9, (name, inc, margin)                                    # no vote can flip
        out = utils.posterior_monotone(Ws, Vs, q=None, increasing=inc)
        print("%s increasing=%s: largest difference %.3g" % (name, inc, np.abs(out["V"] - ref).max()))
        assert np.array_equal(out["pools"], pools), (name, inc)
        assert np.array_equal(out["V"], ref), (name, inc)
        assert pools.min() >= 1 and (pools < T).any()
        if T > 256:                                   # merges among the depths a thread reaches on its second trip
            assert (ref[:, :, 256:] != Vs[:, :, 256:]).any(), (name, inc)


def test_monotone_columns_stay_as_they_are_and_the_other_direction_is_one_pool():
    """Positive W and a V that falls in every component: decreasing already (pools == T, the bits of the input; the stateless
    entry point projects its device copy where it lies, so this is the kernel's in-place path that writes nothing), and
    increasing=True merges every column into a single pool, the mean of its depths built up pair by pair."""
    S, N, M, T, K = 2, 300, 3, 9, 4
    rs = np.random.RandomState(12)
    Ws = rs.gamma(1, 1, (S, N, K))
    Vs = np.ascontiguousarray(rs.gamma(1, 1, (S, M, T, K)).cumsum(axis=2)[:, :, ::-1])
    same = utils.posterior_monotone(Ws, Vs, q=None, increasing=False)
    assert (same["pools"] == T).all() and np.array_equal(same["V"], Vs) and (same["changed"] == 0).all()
    ref, pools, margin = _host_with_margin(Ws, Vs, True)
    assert (pools == 1).all() and margin > 1e-9
    assert np.array_equal(ref, monotone.project_host(Ws, Vs, increasing=True)[0])
    one = utils.posterior_monotone(Ws, Vs, q=None, increasing=True)
    assert (one["pools"] == 1).all() and np.array_equal(one["V"], ref) and (one["changed"] == 1).all()
    assert (one["V"] == one["V"][:, :, :1]).all()
    assert np.abs(one["V"][:, :, 0] - Vs.mean(axis=2)).max() <= 1e-12 * np.abs(Vs).max()


@pytest.mark.parametrize("name,inc", [("c0", False), ("c4", True), ("N1100_K2", False), ("T1", False), ("M1_S1", True)])
@pytest.mark.parametrize("transform", [None, "square", "ilogit"])
def test_summary_is_posterior_summary_of_the_projected_states(runs, name, inc, transform):
    Ws, Vs, out0 = runs[name, inc]
    T = CASES[name][0][3]
    out = out0 if transform is None else utils.posterior_monotone(Ws, Vs, q=Q, transform=transform, increasing=inc)
    assert np.array_equal(out["V"], out0["V"])
    mean, quant = utils.posterior_summary(Ws, out["V"], Q, transform)
    assert np.array_equal(out["mean"], mean) and np.array_equal(out["quantiles"], quant)
    assert np.array_equal(out["changed"], (out["pools"] < T).mean(axis=0)) and out["changed"].shape == (CASES[name][0][2],)
    none = utils.posterior_monotone(Ws, Vs, q=None, increasing=inc, return_V=False)
    assert set(none) == {"pools", "changed", "nsamples"} and np.array_equal(none["pools"], out["pools"])


@pytest.mark.parametrize("name,inc", BOTH, ids=IDS)
def test_every_projected_curve_is_monotone(runs, name, inc):
    Ws, Vs, out = runs[name, inc]
    for s in range(len(Ws)):
        for j in range(Vs.shape[1]):
            curves = Ws[s] @ out["V"][s, j].T                  # (N,T)
            steps = np.diff(curves, axis=1)
            scale = np.abs(curves).max()
            assert ((-steps if inc else steps) <= 1e-12 * scale).all(), (name, inc, s, j)


def test_two_calls_return_identical_bits(runs):
    for name, inc in (("c0", False), ("c2", True), ("N600_K6", False)):
        Ws, Vs, out = runs[name, inc]
        again = utils.posterior_monotone(Ws, Vs, q=Q, increasing=inc)
        assert set(again) == set(out)
        for k, v in out.items():
            assert np.array_equal(again[k], v), (name, k)


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k, v in b.items():
        assert np.array_equal(a[k], v), (what, k)


def test_model_method_on_the_collected_samples():
    N, M, T, K, S = 12, 3, 10, 3, 5
    rs = np.random.RandomState(1)
    W, V = rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, 0.4, size=(N, M, T, 2))
    np.random.seed(0)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=5)
    with pytest.raises(RuntimeError, match="no samples collected"):
        m.posterior_monotone()
    res = m.run_gibbs(Y, nburn=20, nsamples=S, verbose=False)
    W0, V0 = np.array(m.W, copy=True), np.array(m.V, copy=True)
    before = m.posterior_summary(Q)
    a = m.posterior_monotone(return_V=True)
    ref = utils.posterior_monotone(res["W"], res["V"], q=Q)
    _same(a, ref, "collected against stateless")
    _same(m.posterior_monotone(results=res, return_V=True), ref, "results= against stateless")
    assert "V" not in m.posterior_monotone() and (a["pools"] < T).any() and a["nsamples"] == S
    after = m.posterior_summary(Q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # not in place: nothing changed
    assert np.array_equal(m.W, W0) and np.array_equal(m.V, V0)
    with pytest.raises(ValueError, match="in_place"):
        m.posterior_monotone(results=res, in_place=True)
    host_V = np.array(res["V"], copy=True)

    b = m.posterior_monotone(in_place=True)
    assert np.array_equal(b["mean"], a["mean"]) and np.array_equal(b["quantiles"], a["quantiles"])
    assert np.array_equal(b["pools"], a["pools"]) and np.array_equal(res["V"], host_V)        # the host dict is not touched
    mean, quant = m.posterior_summary(Q)
    assert np.array_equal(mean, b["mean"]) and np.array_equal(quant, b["quantiles"])
    c = m.posterior_monotone(return_V=True)
    assert np.array_equal(c["V"], a["V"]) and (c["pools"] == T).all() and (c["changed"] == 0).all()
    rise = m.posterior_functionals(which=("rise",))["rise"]
    assert (rise["mean"] == 0).all() and (rise["quantiles"] == 0).all()                      # no upward step in any sample
    assert (m.posterior_functionals(results=res, which=("rise",))["rise"]["mean"] > 0).any()
    assert np.array_equal(m.W, W0) and np.array_equal(m.V, V0)

    res2 = m.run_gibbs(Y, nburn=0, nsamples=S, verbose=False)                                 # a fresh, unprojected set
    mean2, quant2 = m.posterior_summary(Q)
    ref2 = utils.posterior_summary(res2["W"], res2["V"], Q)
    assert np.array_equal(mean2, ref2[0]) and np.array_equal(quant2, ref2[1])
    assert (m.posterior_monotone()["pools"] < T).any()

    # the C entry points refuse before anything is read or launched
    lib = _native.load()
    d, pools = _native.dptr, np.zeros((S + 1, M), dtype=np.int32)
    ip = pools.ctypes.data_as(C.POINTER(C.c_int32))
    m._ctx.kernel_times()                                        # (reading the counters resets them)
    assert lib.btf_collect_monotone(m._ctx.h, S + 1, None, None, 0, 0, 0, None, 0, None, ip, None, None) == _native.BTF_EINVAL
    assert b"collected" in lib.btf_last_error(m._ctx.h)
    Wc, Vc = _native.as_f64(res["W"]), _native.as_f64(res["V"])
    assert lib.btf_collect_monotone(m._ctx.h, S, d(Wc), d(Vc), 0, 1, 0, None, 0, None, ip, None, None) == _native.BTF_EINVAL
    assert b"in_place" in lib.btf_last_error(m._ctx.h)
    buf = np.zeros(8)
    assert lib.btf_posterior_monotone(0, 1, 1, 1, 1000, 10, d(buf), d(buf), 0, 0, None, 0, None, ip, None, None) == _native.BTF_EINVAL
    assert b"pav_fits" in lib.btf_last_error(None)
    assert m._ctx.kernel_times()["criteria"][1] == 0 and (pools == 0).all()
    assert lib.btf_collect_monotone(m._ctx.h, S, None, None, 0, 0, 0, None, 0, None, ip, None, None) == _native.BTF_OK
    assert m._ctx.kernel_times()["criteria"][1] == 1             # the one projection launch, counted under BTF_K_CRITERIA
    assert (pools[:S] >= 1).all() and (pools[:S] <= T).all()


def test_the_example_projects_an_unconstrained_fit():
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("monotone_posterior", os.path.join(ROOT, "examples", "monotone_posterior.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, rows = mod.main(verbose=False, nburn=20, nsamples=20, N=12, M=3, T=9)
    assert out["nsamples"] == 20 and out["pools"].shape == (20, 3) and out["mean"].shape == (12, 3, 9)
    assert rows["p_monotone"][0] < 1.0 and rows["p_monotone"][1] == 1.0          # every projected curve is monotone
    assert np.isfinite(rows["waic"]).all() and np.isfinite(rows["dic"]).all() and rows["pools_mean"] < 9
