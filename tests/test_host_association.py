"""Host halves of the posterior feature association (functionalmf_amd/association.py): the numpy definition against a direct
per-triple loop with np.corrcoef, the moment route the kernels take against it, the plug-in table against
scipy.stats.linregress, the argument checks made before any device call, the refusal order of the model method, the ABI
symbols and the register budget of the new kernels.  No GPU."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, association, functionals, utils
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

nan = np.nan
S, N, M, T, K, F = 9, 23, 4, 6, 3, 5
LEVEL = 1.0


class _NoDevice:
    """Stands in for the native library and the context: any call into them fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(11)
    Ws, Vs, Us = rs.normal(size=(S, N, K)), rs.normal(size=(S, M, T, K)), rs.normal(size=(S, F, K))
    Us[:, 2] = 0.0                                            # a constant x: undefined in every sample
    Vs[:3, 0] *= 1e-3                                         # column 0 never crosses in three samples: n = 0
    Mu = np.einsum("snk,smtk->snmt", Ws, Vs)
    f = functionals.curve_functionals(Mu, level=LEVEL)
    return Ws, Us, {"auc": f["auc"], "crossing": f["crossing"]}


@pytest.mark.parametrize("which", ["auc", "crossing"])
def test_definition_against_a_direct_loop_with_corrcoef(case, which):
    Ws, Us, f = case
    y = f[which]
    st = association.statistics(y, Ws, Us)
    if which == "crossing":
        assert np.isnan(y).any() and (st["n"] == 0).any() and (st["n"] >= 3).any()
    nchecked = 0
    for s in range(S):
        for j in range(M):
            I = ~np.isnan(y[s, :, j])
            assert st["n"][s, j] == I.sum()
            for ft in range(F):
                x = Ws[s, I] @ Us[s, ft]
                r = st["r"][s, ft, j]
                if I.sum() < 3 or ft == 2:
                    assert np.isnan(r) and np.isnan(st["slope"][s, ft, j]) and np.isnan(st["intercept"][s, ft, j])
                    continue
                assert abs(r - np.corrcoef(x, y[s, I, j])[0, 1]) < 1e-13
                slope, icpt = np.polyfit(x, y[s, I, j], 1)
                scale = max(abs(slope), abs(icpt), 1.0)
                assert abs(st["slope"][s, ft, j] - slope) < 1e-11 * scale and abs(st["intercept"][s, ft, j] - icpt) < 1e-11 * scale
                nchecked += 1
    assert nchecked > S * M * (F - 1) // 3


@pytest.mark.parametrize("which", ["auc", "crossing"])
def test_the_moment_route_of_the_kernels_is_the_definition(case, which):
    Ws, Us, f = case
    y = f[which]
    st = association.statistics(y, Ws, Us)
    worst = 0.0
    for s in range(S):
        for j in range(M):
            mom = association.moments(y[s, :, j], Ws[s])
            assert mom[0] == st["n"][s, j]
            for ft in range(F):
                r, slope, icpt = association.from_moments(mom, Us[s, ft])
                assert np.isnan(r) == np.isnan(st["r"][s, ft, j])
                if not np.isnan(r):
                    worst = max(worst, abs(r - st["r"][s, ft, j]))
                    assert abs(slope - st["slope"][s, ft, j]) <= 1e-11 * max(1.0, abs(slope))
                    assert abs(icpt - st["intercept"][s, ft, j]) <= 1e-11 * max(1.0, abs(icpt))
    assert worst < 1e-13, worst


def test_summaries_by_hand():
    v = np.array([0.5, nan, -0.25, 0.75, nan, 0.0]).reshape(6, 1, 1)
    out = association.summarize(v, q=(0, 50, 100))
    d = np.array([0.5, -0.25, 0.75, 0.0])
    assert out["defined"].tolist() == [[4 / 6]] and out["prob_positive"].tolist() == [[0.5]]
    assert out["mean"][0, 0] == d.mean() and abs(out["var"][0, 0] - d.var(ddof=1)) < 1e-16
    assert out["quantiles"][:, 0, 0].tolist() == [-0.25, 0.25, 0.75]
    one = association.summarize(np.array([nan, 0.3]).reshape(2, 1, 1), q=(5, 95))
    assert one["var"].tolist() == [[0.0]] and one["quantiles"][:, 0, 0].tolist() == [0.3, 0.3] and one["prob_positive"].tolist() == [[1.0]]
    none = association.summarize(np.full((3, 1, 2), nan))
    assert np.isnan(none["mean"]).all() and np.isnan(none["var"]).all() and np.isnan(none["quantiles"]).all()
    assert np.isnan(none["prob_positive"]).all() and none["defined"].tolist() == [[0.0, 0.0]]


def test_reference_dictionary(case):
    Ws, Us, f = case
    pairs = [(0, 1), (2, 0), (4, 3)]
    out = association.reference(f["crossing"], Ws, Us, which="crossing", stats=("slope", "r"), q=(10, 90), pairs=pairs)
    assert out["which"] == "crossing" and out["stats"] == ("slope", "r") and out["nsamples"] == S
    assert out["n_mean"].shape == (M,) and out["defined"].shape == (F, M) and out["defined"][2].max() == 0
    assert out["defined"][0, 0] <= (S - 3) / S                    # the three samples in which column 0 never crosses
    for k in ("r", "slope"):
        assert out[k]["mean"].shape == (F, M) and out[k]["quantiles"].shape == (2, F, M) and out[k]["values"].shape == (3, S)
        assert np.isnan(out[k]["values"][1]).all()                # feature 2: constant
    assert np.nanmax(np.abs(out["r"]["values"])) <= 1 + 1e-12
    assert set(out["of_means"]) == {"r", "slope", "intercept", "stderr", "n", "sd_x", "sd_y"}
    assert "of_means" not in association.reference(f["auc"], Ws, Us, of_means=False)


def test_of_means_against_scipy_linregress(case):
    stats = pytest.importorskip("scipy.stats")
    Ws, Us, f = case
    for which in ("auc", "crossing"):
        y = f[which]
        om = association.plug_in_table(y, Ws, Us)
        Pbar = np.einsum("snk,sfk->snf", Ws, Us).mean(axis=0)
        with np.errstate(invalid="ignore"):
            gbar = np.where(np.isnan(y).all(axis=0), nan, np.nanmean(np.where(np.isnan(y).all(axis=0), 0.0, y), axis=0))
        assert np.allclose(om["sd_x"], Pbar.std(axis=0), rtol=1e-12, atol=0)
        for j in range(M):
            I = ~np.isnan(gbar[:, j])
            assert (om["n"][:, j] == I.sum()).all() and I.sum() >= 3
            assert abs(om["sd_y"][j] - gbar[I, j].std()) < 1e-12 * gbar[I, j].std()
            for ft in range(F):
                if ft == 2:
                    assert np.isnan([om[k][ft, j] for k in ("r", "slope", "intercept", "stderr")]).all()
                    continue
                fit = stats.linregress(Pbar[I, ft], gbar[I, j])
                assert abs(om["r"][ft, j] - fit.rvalue) < 1e-12
                scale = max(abs(fit.slope), abs(fit.intercept))
                assert abs(om["slope"][ft, j] - fit.slope) < 1e-11 * scale and abs(om["intercept"][ft, j] - fit.intercept) < 1e-11 * scale
                assert abs(om["stderr"][ft, j] - fit.stderr) < 1e-11 * max(fit.stderr, scale)


BAD = [
    (dict(which="area"), "unknown functional"),
    (dict(which=("auc",)), "unknown functional"),
    (dict(stats=("tau",)), "stats"),
    (dict(stats=()), "stats"),
    (dict(stats=("r", "r")), "stats"),
    (dict(stats="intercept"), "stats"),
    (dict(q=(5, 101)), "percentiles"),
    (dict(which="crossing"), "level"),
    (dict(which="crossing", level=np.inf), "level"),
    (dict(transform="log"), "transform"),
    (dict(x=np.array([0.0, 0.5, 0.5, 1.0])), "strictly increasing"),
    (dict(x=np.linspace(0, 1, 5)), "ndepth"),
    (dict(pairs=[(6, 0)]), "pairs"),
    (dict(pairs=[(0, 4)]), "pairs"),
    (dict(pairs=[(-1, 0)]), "pairs"),
    (dict(pairs=[(0, 0, 1)]), "pairs"),
    (dict(pairs=[(0.0, 1.0)]), "pairs"),
    (dict(pairs=np.zeros((0, 2), dtype=int)), "pairs"),
]
GOOD = dict(Ws=np.zeros((3, 5, 2)), Vs=np.zeros((3, 4, 4, 2)), Us=np.zeros((3, 6, 2)))


@pytest.mark.parametrize("kw,msg", BAD)
def test_argument_checks_raise_before_the_library_is_loaded(no_device, kw, msg):
    with pytest.raises(ValueError, match=msg):
        utils.posterior_feature_association(GOOD["Ws"], GOOD["Vs"], GOOD["Us"], **kw)


def test_shape_and_size_checks_raise_before_the_library_is_loaded(no_device):
    Ws, Vs, Us = GOOD["Ws"], GOOD["Vs"], GOOD["Us"]
    for bad in (np.zeros((2, 6, 2)), np.zeros((3, 6, 3)), np.zeros((3, 0, 2)), np.zeros((3, 6)), np.zeros((3, 6, 2, 1))):
        with pytest.raises(ValueError, match=r"U must be \(S,F,nembeds\)"):
            utils.posterior_feature_association(Ws, Vs, bad)
    for bad in (nan, np.inf):
        U = Us.copy()
        U[1, 2, 0] = bad
        with pytest.raises(ValueError, match="U must be finite"):
            utils.posterior_feature_association(Ws, Vs, U)
    with pytest.raises(ValueError, match="needs the feature embeddings"):
        utils.posterior_feature_association(Ws, Vs, None)
    with pytest.raises(ValueError, match="ndepth >= 2"):
        utils.posterior_feature_association(np.zeros((3, 5, 2)), np.zeros((3, 4, 1, 2)), Us)
    with pytest.raises(ValueError, match="Ws must be"):
        utils.posterior_feature_association(np.zeros((3, 5, 2)), np.zeros((2, 4, 4, 2)), Us)
    big = association.MAX_SAMPLES + 1
    with pytest.raises(ValueError, match="exceed %d" % association.MAX_SAMPLES):
        utils.posterior_feature_association(np.zeros((big, 1, 1)), np.zeros((big, 1, 2, 1)), np.zeros((big, 1, 1)))
    with pytest.raises(ValueError, match="_scratch_bytes"):
        utils.posterior_feature_association(Ws, Vs, Us, _scratch_bytes=-1)
    assert association.MAX_SAMPLES == 8192 and association.STATS == ("r", "slope")


def _model_without_a_device(N=5, M=4, T=4, K=2, world=1):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds = N, M, T, K
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    return m


@pytest.mark.parametrize("kw,msg", BAD)
def test_the_model_method_checks_its_arguments_before_its_samples(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model_without_a_device().posterior_feature_association(U=GOOD["Us"], **kw)     # (no samples collected: the arguments come first)


def test_refusal_order_of_the_model_method():
    good = dict(W=GOOD["Ws"], V=GOOD["Vs"], U=GOOD["Us"])
    with pytest.raises(NotImplementedError, match="unsharded"):
        _model_without_a_device(world=2).posterior_feature_association(which="area", results=good)
    with pytest.raises(ValueError, match="needs the feature embeddings"):
        _model_without_a_device().posterior_feature_association()
    with pytest.raises(ValueError, match="needs the feature embeddings"):
        _model_without_a_device().posterior_feature_association(results=dict(W=good["W"], V=good["V"]))
    with pytest.raises(ValueError, match=r"U must be \(S,F,nembeds\)"):
        _model_without_a_device().posterior_feature_association(U=np.zeros((3, 6, 3)))
    with pytest.raises(ValueError, match="U must be finite"):
        _model_without_a_device().posterior_feature_association(U=np.full((3, 6, 2), nan))
    with pytest.raises(ValueError, match="stats"):
        _model_without_a_device().posterior_feature_association(stats=("x",), results=good)
    with pytest.raises(RuntimeError, match="no samples collected"):
        _model_without_a_device().posterior_feature_association(U=good["U"])
    with pytest.raises(ValueError, match="results"):
        _model_without_a_device().posterior_feature_association(results={"V": good["V"], "U": good["U"]})
    with pytest.raises(ValueError, match=r"U must be \(S,F,nembeds\)"):                # S of U against S of the samples
        _model_without_a_device().posterior_feature_association(U=np.zeros((2, 6, 2)), results=good)


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    for name in ("btf_posterior_association", "btf_collect_association"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    assert hasattr(lib, "btf_posterior_association") and hasattr(lib, "btf_collect_association")
    assert len(_native.SIGNATURES["btf_posterior_association"][1]) == 31
    assert len(_native.SIGNATURES["btf_collect_association"][1]) == 25
    assert any(src == os.path.join(_native.CSRC, "btf_assoc.hip") for src, _ in _native.UNITS)
    assert os.path.join(_native.CSRC, "btf_assoc.h") in _native.HEADERS
    # the launches are counted under BTF_K_CRITERIA: the counter table keeps its length
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    abi = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    assert abi.count("assoc_run(s, ") == 2 and abi.count("assoc_check(") == 3      # one of each, behind both entry points


def test_no_spills_or_scratch_in_the_association_kernels():
    """Code-object notes (scripts/kernel_notes.py): none of the association kernels spills VGPRs or uses scratch, at K = 10
    (55 Gram sums in registers) included; the moments kernel has no LDS; the reduce kernel's static LDS beside its 64 KiB of
    dynamic rows leaves room for two workgroups in a CU's 160 KiB."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"assoc_\w+_kernel", r["mangled"])]
    assert len(rows) == 4 * 10 + 3, [r["mangled"] for r in rows]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    for r in rows:
        if "assoc_moments_kernel" in r["mangled"]:
            assert r["lds"] == 0, r
        if "assoc_reduce_kernel" in r["mangled"]:
            assert 2 * (r["lds"] + 64 * 1024) <= 160 * 1024 and r["vgpr"] <= 128, r
