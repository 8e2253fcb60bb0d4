"""Binary row features of the constrained model: the argument checks (before any device context exists), the new entry
points in the header, the binding and the built library, and the code-object notes of the new kernels."""
import importlib.util
import os
import re

import numpy as np
import pytest

from functionalmf_amd import _native
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering as Model


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was created before the arguments were checked")
    monkeypatch.setattr(_native, "Context", boom)


N, M, T, K, F = 6, 3, 5, 3, 4
CONS = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)


def _build(**kw):
    return Model(N, M, T, "poisson_identity", CONS, nembeds=K, **kw)


def _good():
    rs = np.random.RandomState(1)
    X = (rs.rand(N, F) < 0.5).astype(float)
    X[1, 2] = np.nan
    return X, rs.uniform(0.01, 0.1, (F, K))


@pytest.mark.parametrize("bad", [0.5, 2.0, -1.0, np.inf])
def test_non_binary_features_raise(no_device, bad):
    X, U = _good()
    X[0, 0] = bad
    with pytest.raises(ValueError, match="0, 1 or nan"):
        _build(row_features=X, feature_embeddings=U)


def test_wrong_shapes_raise(no_device):
    X, U = _good()
    with pytest.raises(ValueError, match="row_features must be"):
        _build(row_features=X[:-1], feature_embeddings=U)
    with pytest.raises(ValueError, match="row_features must be"):
        _build(row_features=X[:, :0], feature_embeddings=U[:0])
    with pytest.raises(ValueError, match="row_features must be"):
        _build(row_features=X[:, 0], feature_embeddings=U[:1])
    with pytest.raises(ValueError, match="feature_embeddings must be"):
        _build(row_features=X, feature_embeddings=U[:-1])
    with pytest.raises(ValueError, match="feature_embeddings must be"):
        _build(row_features=X, feature_embeddings=U[:, :-1])
    with pytest.raises(ValueError, match="finite"):
        _build(row_features=X, feature_embeddings=np.where(np.arange(K) == 1, np.nan, U))


def test_one_without_the_other_raises(no_device):
    X, U = _good()
    with pytest.raises(ValueError, match="without row_features"):
        _build(feature_embeddings=U)
    with pytest.raises(ValueError, match="needs feature_embeddings"):
        _build(row_features=X)


def test_an_infeasible_start_names_the_worst_pair(no_device):
    X, U = _good()
    W = np.full((N, K), 0.5)
    U2 = U.copy()
    U2[1] = 0.5                       # 0.75 everywhere: fine
    U2[3] = [1.0, 1.0, 0.4]           # 1.2 > 1
    W[4] = [0.5, 0.5, 1.5]            # row 4: 1.6, the worst
    with pytest.raises(ValueError, match=r"w_4 \. u_3 = 1\.6.*row 4, feature 3"):
        _build(row_features=X, feature_embeddings=U2, W_init=W)
    U3 = U.copy()
    U3[2, 0] = -1.0                   # negative product
    with pytest.raises(ValueError, match=r"u_2 .*outside \[0, 1\]"):
        _build(row_features=X, feature_embeddings=U3, W_init=np.full((N, K), 0.5))
    Model._check_feature_start(np.full((N, K), 0.5), U)          # feasible: no exception
    codes, Uc = Model._check_features(X, U, N, K)
    assert codes.dtype == np.uint8 and codes[1, 2] == 2 and set(np.unique(codes)) <= {0, 1, 2}
    assert np.array_equal(codes[X == 1], np.ones((X == 1).sum(), dtype=np.uint8)) and Uc.flags["C_CONTIGUOUS"]


def test_new_abi_is_declared_exported_and_bound():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    names = ("btf_gass_set_row_features", "btf_gass_set_U", "btf_gass_get_U")
    for name in names:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _native.SIGNATURES
    _native.build()
    lib = _native.load()
    for name in names:
        assert hasattr(lib, name)
    assert len(_native.SIGNATURES["btf_gass_set_row_features"][1]) == 4
    assert os.path.join(_native.CSRC, "btf_gass_features.h") in _native.HEADERS
    # no new unit, no new counter: the kernels live in btf_gass_ep.hip and are counted under BTF_K_ESS
    assert any(src == os.path.join(_native.CSRC, "btf_gass_ep.hip") for src, _ in _native.UNITS)
    assert not any("features" in os.path.basename(src) for src, _ in _native.UNITS)
    assert len(_native.KERNEL_NAMES) == 15 and re.search(r"BTF_K_COUNT = 15\b", text)
    unit = open(os.path.join(_native.CSRC, "btf_gass_ep.hip")).read()
    assert '#include "btf_gass_features.h"' in unit


def test_no_spills_or_scratch_in_the_feature_kernels():
    """Code-object notes (scripts/kernel_notes.py): the Bernoulli evaluation (three instances), the feature-chain analysis
    and the derived-constraints kernel neither spill VGPRs nor use scratch.  The analysis kernel's static LDS is
    GassScratch alone: (10000 + 8) + 256 ints, 2 x 256 doubles, 256 ints = 46176 bytes; the evaluation kernel stages 1024
    cells as (e0, e1[, em], code) beside 4 x 128 partial sums: within 33 KB."""
    from conftest import ROOT
    _native.build()
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(ROOT, "scripts", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    rows = [r for r in kn.kernels() if re.search(r"gass_(feat_rc|feat_analyse|bern_eval)_kernel", r["mangled"])]
    assert len(rows) == 5, [r["mangled"] for r in rows]
    bad = [(r["mangled"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] or r["scratch"]]
    assert not bad, bad
    scratch_bytes = (10000 + 8) * 4 + 256 * 4 + 2 * 256 * 8 + 256 * 4          # sizeof(GassScratch)
    ana = [r for r in rows if "feat_analyse" in r["mangled"]]
    assert len(ana) == 1 and scratch_bytes <= ana[0]["lds"] < scratch_bytes + 1024, ana[0]["lds"]
    rows_ana = [r for r in kn.kernels() if re.search(r"gass_analyse_rows_kernelILb0E", r["mangled"])]
    assert ana[0]["lds"] == rows_ana[0]["lds"]                                  # the same scratch as the row analysis
    for r in rows:
        if "bern_eval" in r["mangled"]:
            assert r["lds"] <= 33 * 1024 and r["vgpr"] <= 128 and r["sgpr_spill"] == 0, r
