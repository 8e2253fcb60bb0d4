"""The host half of the Negative-Binomial criteria (functionalmf_amd/criteria.py: negbin_loglik, negbin_statistics,
negbin_rates): the written definition against a brute-force loop over scipy.stats.nbinom.logpmf for every rate layout, the
statistics, R-bar, the ValueErrors, the registration of the unit and the refusals that stay."""
import itertools
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, criteria
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

N, M, T, R, K, S = 4, 3, 5, 2, 2, 3
LAYOUTS = list(itertools.product((False, True), repeat=3))        # rate full along (rows, columns, depth)?


def _problem(seed=0):
    rs = np.random.RandomState(seed)
    Y = rs.poisson(6.0, size=(N, M, T, R)).astype(float)
    Y[0, 0, 0, 0] = 0.0
    Y[1, 1, 1, 0] = 40.0
    Y[2, 0, 3, 1] = np.nan                  # a missing replicate
    Y[3, 2, 4] = np.nan                     # a cell without observations inside an observed curve
    Y[1, 2] = np.nan                        # a curve without observations
    Ws = 0.6 * rs.normal(size=(S, N, K))
    Vs = 0.8 * rs.normal(size=(S, M, T, K))
    return Y, Ws, Vs, rs


def _rates(rs, layout, S=S):
    tail = tuple(full if on else 1 for full, on in zip((N, M, T), layout))
    return rs.uniform(0.5, 30.0, size=(S,) + tail)


def _brute(Y, Ws, Vs, Rs):
    from scipy.stats import nbinom
    Sn = Ws.shape[0]
    R4 = np.broadcast_to(np.reshape(Rs, (Sn,) + ((1, 1, 1) if Rs.ndim < 4 else Rs.shape[1:])), (Sn, N, M, T))
    Rbar = np.mean(R4, axis=0)
    eta = np.einsum("snk,smtk->snmt", Ws, Vs)
    L, Lm = np.zeros((Sn, N, M)), np.zeros((N, M))
    for i, j, t, r in itertools.product(range(N), range(M), range(T), range(Y.shape[3])):
        y = Y[i, j, t, r]
        if np.isnan(y):
            continue
        for s in range(Sn):
            L[s, i, j] += nbinom.logpmf(y, R4[s, i, j, t], 1.0 - 1.0 / (1.0 + np.exp(-eta[s, i, j, t])))
        Lm[i, j] += nbinom.logpmf(y, Rbar[i, j, t], 1.0 - 1.0 / (1.0 + np.exp(-eta[:, i, j, t].mean())))
    return L, Lm


@pytest.mark.parametrize("layout", LAYOUTS)
def test_negbin_loglik_is_the_sum_of_nbinom_logpmf(layout):
    Y, Ws, Vs, rs = _problem(seed=1 + LAYOUTS.index(layout))
    Rs = _rates(rs, layout)
    L, L_at_mean, obs = criteria.negbin_loglik(Y, Ws, Vs, Rs)
    want, want_mean = _brute(Y, Ws, Vs, Rs)
    assert L.shape == (S, N, M) and obs.sum() == N * M - 1 and not obs[1, 2]
    np.testing.assert_allclose(L, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(L_at_mean, want_mean, rtol=1e-12, atol=1e-12)
    assert np.all(L[:, 1, 2] == 0.0) and L_at_mean[1, 2] == 0.0
    # from_loglik and psis_loo_host take the matrix as it is
    ic = criteria.from_loglik(L, obs, L_at_mean)
    assert ic["n_curves"] == N * M - 1 and np.isfinite(ic["waic"]) and np.isfinite(ic["dic"])
    assert criteria.psis_loo_host(L, obs)["n_curves"] == N * M - 1


def test_scalar_rate_forms_and_a_three_tensor():
    Y, Ws, Vs, rs = _problem(seed=20)
    r = rs.uniform(1.0, 5.0, size=S)
    a = criteria.negbin_loglik(Y, Ws, Vs, r)
    b = criteria.negbin_loglik(Y, Ws, Vs, r[:, None])
    c = criteria.negbin_loglik(Y, Ws, Vs, r.reshape(S, 1, 1, 1))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    np.testing.assert_allclose(a[0], _brute(Y, Ws, Vs, r)[0], rtol=1e-12, atol=1e-12)
    L3 = criteria.negbin_loglik(Y[..., 0], Ws, Vs, r)[0]
    Y1 = np.full_like(Y, np.nan)
    Y1[..., 0] = Y[..., 0]
    np.testing.assert_allclose(L3, criteria.negbin_loglik(Y1, Ws, Vs, r)[0], rtol=1e-14, atol=1e-14)


def test_statistics_mask_and_constant():
    from scipy.special import gammaln
    Y = _problem()[0]
    S1, cnt, c0, Y4, obs = criteria.negbin_statistics(Y, (N, M, T))
    o4 = ~np.isnan(Y)
    assert np.array_equal(obs, o4.any(axis=(2, 3))) and not obs[1, 2] and obs[3, 2] and obs.sum() == N * M - 1
    assert S1.shape == cnt.shape == (M, T, N) and S1.flags.c_contiguous and cnt.flags.c_contiguous
    assert np.array_equal(S1, np.nansum(Y, axis=3).transpose(1, 2, 0))
    assert np.array_equal(cnt, o4.sum(axis=3).astype(float).transpose(1, 2, 0))
    assert cnt[2, 4, 3] == 0.0 and cnt[0, 3, 2] == 1.0
    want = np.zeros((N, M))
    for i, j in itertools.product(range(N), range(M)):
        want[i, j] = -sum(gammaln(y + 1.0) for y in Y[i, j].ravel() if not np.isnan(y))
    np.testing.assert_allclose(c0, want, rtol=1e-14, atol=0)
    assert c0[1, 2] == 0.0
    assert Y4.shape == (N, M, T, R) and Y4.flags.c_contiguous and np.array_equal(Y4, Y, equal_nan=True)
    assert criteria.negbin_statistics(Y[..., 0], (N, M, T))[3].shape == (N, M, T, 1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rates_append_the_mean_and_carry_the_axis_flags(layout):
    rs = np.random.RandomState(3)
    Rs = _rates(rs, layout)
    rates, flags = criteria.negbin_rates(Rs, S, (N, M, T))
    ext = int(np.prod(Rs.shape[1:]))
    assert rates.shape == (S + 1, ext) and rates.flags.c_contiguous and rates.dtype == np.float64
    assert np.array_equal(rates[:S], Rs.reshape(S, -1))
    assert np.array_equal(rates[S], np.mean(Rs, axis=0).ravel())
    bits = (_native.PRED_AUX_ROWS, _native.PRED_AUX_COLS, _native.PRED_AUX_DEPTH)
    assert flags == _native.PRED_AUX_PER_SAMPLE | sum(b for b, on in zip(bits, layout) if on)


def test_value_errors():
    Y, Ws, Vs, rs = _problem(seed=4)
    good = rs.uniform(1.0, 3.0, size=(S, N, 1, 1))
    criteria.negbin_loglik(Y, Ws, Vs, good)
    Yb = Y.copy()
    Yb[0, 1, 2, 0] = -1.0
    with pytest.raises(ValueError, match=">= 0"):
        criteria.negbin_loglik(Yb, Ws, Vs, good)
    with pytest.raises(ValueError, match=">= 0"):
        criteria.negbin_statistics(Yb, (N, M, T))
    for bad in (0.0, -2.0, np.inf, np.nan):
        Rb = good.copy()
        Rb[1, 2] = bad
        with pytest.raises(ValueError, match="rate"):
            criteria.negbin_loglik(Y, Ws, Vs, Rb)
        with pytest.raises(ValueError, match="rate"):
            criteria.negbin_rates(Rb, S, (N, M, T))
    with pytest.raises(ValueError, match="leading dimension"):
        criteria.negbin_loglik(Y, Ws, Vs, good[:2])
    with pytest.raises(ValueError, match="leading dimension"):
        criteria.negbin_rates(good[:2], S, (N, M, T))
    with pytest.raises(ValueError):
        criteria.negbin_loglik(Y, Ws, Vs, np.ones((S, 2, 1, 1)))          # an axis neither full nor 1
    with pytest.raises(ValueError):
        criteria.negbin_loglik(Y, Ws[:, :3], Vs, good)
    with pytest.raises(ValueError, match="pair"):
        criteria.negbin_statistics((Y[..., 0], Y[..., 0]), (N, M, T))


def test_unit_header_and_abi_are_registered():
    from conftest import ROOT
    assert any(src == os.path.join(_native.CSRC, "btf_nb_criteria.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_nb_criteria.h") in _native.HEADERS
    assert os.path.join(_native.CSRC, "btf_lgamma.h") in _native.HEADERS
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name, nargs in (("btf_crit_set_counts", 4), ("btf_nb_crit_eval", 11), ("btf_nb_crit_loo", 12)):
        assert re.search(r"int %s\(btf_ctx\* ctx, int slot," % name, text), name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
    # unchanged: the counter table and the signatures of the five-plus-one families
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    assert len(_native.SIGNATURES["btf_crit_eval"][1]) == 12 and len(_native.SIGNATURES["btf_crit_loo"][1]) == 14
    # one copy of the lgamma helpers: the sampler's header includes the shared one and defines none of them itself
    kern = open(os.path.join(_native.CSRC, "btf_kernels.h")).read()
    assert '#include "btf_lgamma.h"' in kern
    for fn in ("double lgamma_big(", "double lgamma_diff(", "double nb_count_part("):
        assert fn not in kern, fn


def test_no_spills_or_scratch_in_the_negbin_criteria_kernels():
    """Code-object notes (scripts/kernel_notes.py): nb_crit_kernel exists at every nembeds 1..10 with a per-lane and a
    wave-uniform rate; none of the new kernels spills VGPRs or uses scratch; static LDS stays within the 64 KiB limit and
    the registers within the 256 per lane that two waves per SIMD allow."""
    import importlib.util
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"nb_crit_(const_tab_|const_|plugin_)?kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    main = [r for r in rows if re.search(r"nb_crit_kernelILi", r["mangled"])]
    ks = sorted(int(m) for r in main for m in re.findall(r"nb_crit_kernelILi(\d+)E", r["mangled"]))
    assert ks == sorted(list(range(1, 11)) * 2), ks
    assert sum("nb_crit_const_kernel" in r["mangled"] for r in rows) == 2
    assert sum("nb_crit_const_tab_kernel" in r["mangled"] for r in rows) == 1
    assert sum("nb_crit_plugin_kernel" in r["mangled"] for r in rows) == 2
    for r in rows:
        assert r["lds"] <= 64 * 1024 and r["vgpr"] + r["agpr"] <= 256, r


class _NoDevice:
    """Stands in for a context: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


def _bare(world=1):
    m = object.__new__(NegativeBinomialBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds = N, M, T, K
    m._plan = types.SimpleNamespace(world=world)
    m._exchange = types.SimpleNamespace(active=False)
    m._ctx = _NoDevice()
    m._collected = 0
    m._shared = (0, 1, 2)
    m._R, m._R_dev_new = np.full((1, 1, 1), 2.0), False
    return m


def test_the_pinned_refusals_still_raise_and_the_new_methods_refuse_before_any_device_call():
    Y, Ws, Vs, rs = _problem(seed=5)
    res = {"W": Ws, "V": Vs, "R": np.full((S, 1, 1, 1), 2.0)}
    m = _bare()
    for call in (lambda: m.information_criteria(res, data=Y), lambda: m.loo(res, data=Y), lambda: m.logprob(Y),
                 lambda: m.fold_in_rows(Y[:2], results={"V": Vs, "sigma2": np.ones((S, 1))})):
        with pytest.raises(NotImplementedError):
            call()
    sharded = _bare(world=2)
    for call in (lambda: sharded.negbin_criteria(res, data=Y), lambda: sharded.negbin_loo(res, data=Y),
                 lambda: sharded.negbin_logprob(Y)):
        with pytest.raises(NotImplementedError, match="unsharded"):
            call()
    for call in (lambda: m.negbin_criteria(None, data=Y), lambda: m.negbin_loo(None, data=Y)):
        with pytest.raises(RuntimeError, match="no samples collected"):
            call()
    with pytest.raises(ValueError, match="leading dimension"):
        m.negbin_criteria(dict(res, R=np.full((S + 1, 1, 1, 1), 2.0)), data=Y)
    with pytest.raises(ValueError, match="rate"):
        m.negbin_criteria(dict(res, R=np.zeros((S, 1, 1, 1))), data=Y)
    with pytest.raises(ValueError, match="r_eff"):
        m.negbin_loo(res, data=Y, r_eff=0.0)
    with pytest.raises(ValueError, match="reduce"):
        m.negbin_logprob(Y, reduce="cell")
