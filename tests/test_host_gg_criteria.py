"""Host halves of the gamma-grid model-selection criteria (gamma_grid_criteria / gamma_grid_loo): the written definition
criteria.gamma_grid_loglik against the reference's own logpdf, mu_loglikelihood and dic (tests/golden/g18_gamma_grid_dic.npz),
the statistics the kernel reads, the ABI symbol, and the register budget of the new kernels.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native, criteria

TABLES = ("norm", "raw")          # weights summing to one (what estimate_likelihood produces), and weights that do not


def _definition(g, name):
    lik = (g["mean_grid"], g[name + "_probs"], float(g["variance"]))
    return criteria.gamma_grid_loglik(g["Y"], g["Ws"], g["Vs"], lik)


def test_fixture_is_what_the_issue_describes(golden):
    g = golden("g18_gamma_grid_dic.npz")
    N, M, T, R, K, S, G = [int(x) for x in g["dims"]]
    assert (N, M, T, R, K, S, G) == (6, 4, 7, 3, 2, 12, 9)
    Y = g["Y"]
    obs = ~np.isnan(Y)
    assert Y.shape == (N, M, T, R) and 0 < (~obs).sum()
    assert (~obs.any(axis=(2, 3))).sum() == 1                        # one curve without observations
    assert (~obs.any(axis=3) & obs.any(axis=(2, 3))[..., None]).sum() >= 1      # a cell without, inside an observed curve
    assert np.all(g["Ws"] > 0) and np.all(g["Vs"] > 0)
    assert abs(g["norm_probs"].sum() - 1.0) < 1e-14 and abs(g["raw_probs"].sum() - 1.0) > 0.1


@pytest.mark.parametrize("name", TABLES)
def test_loglik_equals_the_references_per_curve(golden, name):
    g = golden("g18_gamma_grid_dic.npz")
    L, L_at_mean, obs = _definition(g, name)
    want = g[name + "_logpdf"].sum(axis=-1)                          # (S,N,M): the reference's cells summed over depth
    np.testing.assert_allclose(L[:, obs], want[:, obs], rtol=1e-12, atol=0)
    assert np.all(L[:, ~obs] == 0.0) and np.all(L_at_mean[~obs] == 0.0)
    assert np.array_equal(obs, np.any(~np.isnan(g["Y"]), axis=(2, 3)))
    # an unobserved curve holds T log sum_g p_g in the reference
    lsp, T = np.log(g[name + "_probs"].sum()), g["Y"].shape[2]
    np.testing.assert_allclose(want[:, ~obs], T * lsp, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name", TABLES)
def test_dic_equals_the_references_through_the_identity(golden, name):
    """reference DIC = ours - 2 lsp T (number of unobserved curves), lsp = log sum_g p_g (0 for normalised weights)."""
    g = golden("g18_gamma_grid_dic.npz")
    L, L_at_mean, obs = _definition(g, name)
    res = criteria.from_loglik(L, obs, L_at_mean)
    lsp, T, nun = np.log(g[name + "_probs"].sum()), g["Y"].shape[2], int((~obs).sum())
    np.testing.assert_allclose(res["dic"] - 2.0 * lsp * T * nun, float(g[name + "_dic"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["loglik_per_sample"] + lsp * T * nun, g[name + "_mu_loglikelihood"], rtol=1e-12, atol=0)
    if name == "norm":
        np.testing.assert_allclose(res["dic"], float(g["norm_dic"]), rtol=1e-12, atol=0)
    assert res["n_curves"] == int(obs.sum()) == obs.size - 1


def test_negated_row_gives_minus_inf_in_the_definition(golden):
    g = golden("g18_gamma_grid_dic.npz")
    Ws = g["Ws"].copy()
    Ws[3, 2] = -Ws[3, 2]
    L, L_at_mean, obs = criteria.gamma_grid_loglik(g["Y"], Ws, g["Vs"], (g["mean_grid"], g["raw_probs"], float(g["variance"])))
    assert np.all(L[3, 2][obs[2]] == -np.inf) and np.all(np.isfinite(np.delete(L, 3, axis=0)))
    assert np.all(np.isfinite(L_at_mean))
    res = criteria.from_loglik(L, obs, L_at_mean)
    assert np.all(np.isnan(res["curves"]["p_waic"][2][obs[2]])) and np.all(np.isfinite(res["curves"]["lppd"]))


def test_statistics_layout_mask_and_refusal():
    rs = np.random.RandomState(0)
    N, M, T, R = 5, 3, 4, 3
    Y = rs.gamma(3.0, 0.3, size=(N, M, T, R))
    Y[rs.rand(N, M, T, R) < 0.3] = np.nan
    Y[2, 1] = np.nan
    Y[0, 0, 1] = np.nan
    S1, cnt, L, obs = criteria.gamma_grid_statistics(Y, (N, M, T))
    for a in (S1, cnt, L):
        assert a.shape == (M, T, N) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(cnt, (~np.isnan(Y)).sum(axis=3).transpose(1, 2, 0))
    np.testing.assert_allclose(S1, np.nansum(Y, axis=3).transpose(1, 2, 0), rtol=1e-15)
    np.testing.assert_allclose(L, np.nansum(np.log(Y), axis=3).transpose(1, 2, 0), rtol=1e-15, atol=1e-15)
    assert S1[0, 1, 0] == 0.0 and cnt[0, 1, 0] == 0.0 and L[0, 1, 0] == 0.0
    assert obs.shape == (N, M) and obs.dtype == bool and not obs[2, 1] and obs.sum() == N * M - 1
    # the statistics of criteria.statistics, which the other families upload, agree on S1 and cnt
    s1, c, _, _, o = criteria.statistics(criteria.FAMILY_POISSON_IDENTITY, Y, (N, M, T))
    assert np.array_equal(s1, S1) and np.array_equal(c, cnt) and np.array_equal(o, obs)
    # a 3-tensor is one replicate per cell
    S1b, cntb, Lb, _ = criteria.gamma_grid_statistics(Y[..., 0], (N, M, T))
    assert np.array_equal(cntb, (~np.isnan(Y[..., 0])).astype(float).transpose(1, 2, 0))
    for bad in (0.0, -0.2):
        Yb = Y.copy()
        Yb[4, 2, 3, 0] = bad
        with pytest.raises(ValueError, match="the gamma_grid likelihood needs every observed y > 0"):
            criteria.gamma_grid_statistics(Yb, (N, M, T))
    with pytest.raises(ValueError):
        criteria.gamma_grid_statistics(Y, (N, M, T + 1))


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    assert re.search(r"int btf_crit_set_logsum\(btf_ctx\* ctx, int slot, const double\* L\);", text)
    assert "btf_crit_set_logsum" in _native.SIGNATURES and len(_native.SIGNATURES["btf_crit_set_logsum"][1]) == 3
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_crit_set_logsum")
    assert any(src == os.path.join(_native.CSRC, "btf_gg_criteria.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_gg_criteria.h") in _native.HEADERS
    # unchanged: the counter table, the signatures family 5 enters through
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    assert len(_native.SIGNATURES["btf_crit_eval"][1]) == 12 and len(_native.SIGNATURES["btf_crit_loo"][1]) == 14
    assert criteria.FAMILY_GAMMA_GRID == _native.CRIT_FAMILY_GAMMA_GRID == 5
    # one copy of the cell formula: the criteria kernels call gg_term of btf_gamma_grid.h
    gg = open(os.path.join(_native.CSRC, "btf_gg_criteria.h")).read()
    assert gg.count("gg_term(") == 2 and "exp_tab(" not in gg and "log_tab(" not in gg


def test_no_spills_or_scratch_in_the_gamma_grid_criteria_kernels():
    """Code-object notes (scripts/kernel_notes.py): gg_crit_kernel exists at every nembeds 1..10; neither it nor the plug-in
    kernel spills VGPRs or uses scratch.  The static LDS (the tables and the block of 16 samples' partial sums) lets two
    workgroups share a CU's 160 KiB, and so do the registers (at most 256 per lane: two waves per SIMD)."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"gg_crit(_plugin)?_kernel", r["mangled"])]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    main = [r for r in rows if "gg_crit_kernel" in r["mangled"]]
    ks = sorted(int(m) for r in main for m in re.findall(r"gg_crit_kernelILi(\d+)E", r["mangled"]))
    assert ks == list(range(1, 11)), ks
    assert sum("gg_crit_plugin_kernel" in r["mangled"] for r in rows) == 1
    for r in main:
        assert 2 * r["lds"] <= 160 * 1024 and r["lds"] <= 64 * 1024, r
        assert r["vgpr"] + r["agpr"] <= 256, r


def test_models_with_another_likelihood_are_refused_before_any_device_call():
    from functionalmf_amd.factor import NonconjugateBayesianTensorFiltering

    class _NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device entry point %s called" % name)

    model = NonconjugateBayesianTensorFiltering.__new__(NonconjugateBayesianTensorFiltering)
    model._link, model._callback, model.loglikelihood = 1, False, "poisson_identity"
    model._ctx = _NoDevice()
    model._plan = type("P", (), {"world": 1})()
    model._exchange = type("E", (), {"active": False})()
    with pytest.raises(ValueError, match="information_criteria"):
        model.gamma_grid_criteria({"W": np.zeros((2, 3, 1)), "V": np.zeros((2, 2, 4, 1))})
    with pytest.raises(ValueError, match=r"use loo\b"):
        model.gamma_grid_loo({"W": np.zeros((2, 3, 1)), "V": np.zeros((2, 2, 4, 1))})
