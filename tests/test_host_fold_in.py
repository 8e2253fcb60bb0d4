"""Host halves of fold_in_rows (functionalmf_amd/fold_in.py): the numpy definition against a brute-force dense
least-squares formulation, every refusal before the library is loaded, and the wiring of the new unit and symbols.  No GPU."""
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _native, utils
from functionalmf_amd import fold_in
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering,
                                     GaussianBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """Stands in for the native library and for a context: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device entry point %s called" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoDevice())


def _bare(cls, M=3, T=4, K=2, world=1, collected=0):
    m = object.__new__(cls)
    m.nrows, m.ncols, m.ndepth, m.nembeds = 5, M, T, K
    m._plan = types.SimpleNamespace(world=world)
    m._exchange = types.SimpleNamespace(active=False)
    m._ctx = _NoDevice()
    m._collected = collected
    m._draws, m._device_seed = 0, 1
    return m


@pytest.mark.parametrize("K,nreps", [(1, 1), (3, 1), (5, 3), (10, 2)])
def test_conditional_equals_dense_least_squares(K, nreps):
    """Q and Q^-1 b are the normal equations of the stacked regression  [y_obs / nu; 0] = [X_obs / nu; I / sigma] w: one row
    of X per OBSERVED replicate (a missing one contributes no row), solved by a dense least-squares routine."""
    rs = np.random.RandomState(10 + K)
    M, T = 4, 6
    V = rs.normal(size=(M, T, K))
    Y = rs.normal(size=(M, T, nreps))
    Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    Y[1] = np.nan                                             # a column without any observation
    nu2, sigma2 = 0.7, 1.9
    mean, Q = fold_in.conditional(Y if nreps > 1 else Y[..., 0], V, nu2, sigma2)
    rows, rhs = [], []
    for j in range(M):
        for t in range(T):
            for r in range(nreps):
                if not np.isnan(Y[j, t, r]):
                    rows.append(V[j, t] / np.sqrt(nu2))
                    rhs.append(Y[j, t, r] / np.sqrt(nu2))
    X = np.vstack(rows + [np.eye(K) / np.sqrt(sigma2)])
    y = np.concatenate([np.array(rhs), np.zeros(K)])
    w_ls = np.linalg.lstsq(X, y, rcond=None)[0]
    np.testing.assert_allclose(mean, w_ls, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Q, X.T.dot(X), rtol=0, atol=1e-12)
    # an empty row: the prior
    m0, Q0 = fold_in.conditional(np.full((M, T), np.nan), V, nu2, sigma2)
    assert np.all(m0 == 0) and np.array_equal(Q0, np.eye(K) / sigma2)
    # draw: covariance factor L^-T, so that (w - mean) has precision Q
    z = rs.normal(size=K)
    w = fold_in.draw(mean, Q, z)
    L = np.linalg.cholesky(Q)
    np.testing.assert_allclose(L.T.dot(w - mean), z, rtol=0, atol=1e-12)


def test_row_statistics():
    Y = np.array([[[1.0, np.nan], [2.0, 3.0]]])[..., None] * np.ones(3)     # (1,2,2,3)
    Y[0, 1, 0, 1] = np.nan
    R, c, s = fold_in.row_statistics(Y, "gaussian", 2, 2)
    assert R == 1 and c.tolist() == [[[3, 0], [2, 3]]] and s.tolist() == [[[3, 0], [4, 9]]]
    Yb, Nb = np.array([[[1.0, np.nan, 0.0]]]), np.array([[[2.0, 3.0, 0.0]]])
    R, n, y = fold_in.row_statistics((Yb, Nb), "binomial", 1, 3)
    assert n.tolist() == [[[2, 0, 0]]] and y.tolist() == [[[1, 0, 0]]]
    R, n, y = fold_in.row_statistics(np.array([[[1.0, 0.0, np.nan]]]), "binomial", 1, 3)     # Bernoulli tensor
    assert n.tolist() == [[[1, 1, 0]]]


def test_model_refusals_raise_before_any_device_call(no_device):
    Y = np.zeros((2, 3, 4))
    res = {"V": np.ones((6, 3, 4, 2)), "sigma2": np.ones((6, 1)), "nu2": np.ones((6, 1))}
    for cls in (NegativeBinomialBayesianTensorFiltering, NonconjugateBayesianTensorFiltering,
                ConstrainedNonconjugateBayesianTensorFiltering):
        with pytest.raises(NotImplementedError):
            _bare(cls).fold_in_rows(Y, results=res)
    with pytest.raises(NotImplementedError):
        _bare(GaussianBayesianTensorFiltering, world=2).fold_in_rows(Y, results=res)
    g = _bare(GaussianBayesianTensorFiltering)
    with pytest.raises(RuntimeError):
        g.fold_in_rows(Y)                                      # nothing collected, no results
    for bad_Y in (np.zeros((2, 3, 5)), np.zeros((3, 4)), np.zeros((2, 4, 4, 1)), (Y, Y)):
        with pytest.raises(ValueError):
            g.fold_in_rows(bad_Y, results=res)
    for key, val in (("V", np.ones((6, 3, 4, 3))), ("V", np.ones((3, 4, 2))), ("sigma2", np.ones(5)), ("nu2", np.ones(7)),
                     ("nu2", np.array([1, 1, 0, 1, 1, 1.0])), ("nu2", np.array([1, 1, np.nan, 1, 1, 1.0])),
                     ("sigma2", np.array([1, 1, -1, 1, 1, 1.0])), ("sigma2", np.array([1, 1, np.inf, 1, 1, 1.0]))):
        with pytest.raises(ValueError):
            g.fold_in_rows(Y, results=dict(res, **{key: val}))
    with pytest.raises(ValueError):
        g.fold_in_rows(Y, results={"V": res["V"], "sigma2": res["sigma2"]})          # Gaussian without nu2
    with pytest.raises(ValueError):
        g.fold_in_rows(Y, results=res, z=np.zeros((6, 2, 3)))
    with pytest.raises(ValueError):
        g.fold_in_rows(Y, results=res, transform="log")
    with pytest.raises(ValueError):
        g.fold_in_rows(Y, results=res, q=(5, 101))
    big = {"V": np.ones((fold_in.MAX_SUMMARY_SAMPLES + 1, 1, 2, 1)), "sigma2": np.ones(fold_in.MAX_SUMMARY_SAMPLES + 1),
           "nu2": np.ones(fold_in.MAX_SUMMARY_SAMPLES + 1)}
    with pytest.raises(ValueError):
        _bare(GaussianBayesianTensorFiltering, M=1, T=2, K=1).fold_in_rows(np.zeros((1, 1, 2)), results=big)
    b = _bare(BinomialBayesianTensorFiltering)
    Yb = (np.ones((2, 3, 4)), 2 * np.ones((2, 3, 4)))
    with pytest.raises(ValueError):
        b.fold_in_rows(Yb, results=res, z=np.zeros((6, 2, 2)))                       # z with a Binomial model
    with pytest.raises(ValueError):
        b.fold_in_rows((Yb[0], 40 * Yb[1]), results=res)                              # counts beyond the exact sampler
    with pytest.raises(ValueError):
        b.fold_in_rows((3 * Yb[1], Yb[1]), results=res)                               # more successes than trials
    with pytest.raises(ValueError):
        b.fold_in_rows(Yb, results=res, inner_sweeps=0)
    with pytest.raises(RuntimeError):
        b.fold_in_rows(Yb)
    assert g._draws == 0 and b._draws == 0                     # a refused call takes no seed


def test_stateless_refusals_raise_before_any_device_call(no_device):
    V = np.ones((6, 3, 4, 2))
    Y = np.zeros((2, 3, 4))
    one = np.ones(6)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V, "poisson", nu2=one, sigma2=one)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V[0], "gaussian", nu2=one, sigma2=one)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V, "gaussian", sigma2=one)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V, "gaussian", nu2=one, sigma2=-one)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y[:, :2], V, "gaussian", nu2=one, sigma2=one)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V, "gaussian", nu2=one, sigma2=one, first_sample=-1)
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, V, "binomial", sigma2=one, z=np.zeros((6, 2, 2)))
    with pytest.raises(ValueError):
        utils.fold_in_rows(Y, np.ones((6, 3, 4, 11)), "gaussian", nu2=one, sigma2=one)


def test_the_unit_and_the_symbols_are_wired():
    assert os.path.join(_native.CSRC, "btf_fold_in.hip") in _native.SOURCES
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("btf_fold_in_rows", "btf_collect_fold_in"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["btf_fold_in_rows"][1]) == 24 and len(_native.SIGNATURES["btf_collect_fold_in"][1]) == 18
    assert fold_in.MAX_TRIALS == 32 and fold_in.DEFAULT_INNER_SWEEPS >= 1
