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


def _inputs(name):
    (S, N, M, T, K), noise, seed = CASES[name]
    rs = np.random.RandomState(seed)
    Ws = rs.gamma(1, 1, (S, N, K))
    Vs = np.ascontiguousarray(0.2 * rs.gamma(1, 1, (S, M, T, K)).cumsum(axis=2)[:, :, ::-1] + rs.gamma(1.0, noise, (S, M, T, K)))
    Ws.setflags(write=False)
    Vs.setflags(write=False)
    return Ws, Vs


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
