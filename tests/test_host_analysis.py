"""The front end the posterior analysis features share (functionalmf_amd/_analysis.py, _native.check): the argument checks
tested directly, and the refusals of every analysis method of a model - no samples, a sharded model, a malformed results
dict - made before any device call.  No GPU."""
import os
import re
import types

import numpy as np
import pytest

from functionalmf_amd import _analysis, _native
from functionalmf_amd.factor import GaussianBayesianTensorFiltering


# ---- the shared checks
def test_transform_code():
    assert [_analysis.transform_code(t) for t in (None, "identity", "ilogit", "square")] == [0, 0, 1, 2]
    assert set(_analysis.TRANSFORMS) == {None, "identity", "ilogit", "square"}
    for bad in ("cube", 3, ["ilogit"]):
        with pytest.raises(ValueError, match="transform must be"):
            _analysis.transform_code(bad)


def test_check_q():
    for q, want in ((50, [50.0]), ([2.5, 97.5], [2.5, 97.5]), ([], []), ((0, 100), [0.0, 100.0])):
        qs = _analysis.check_q(q)
        assert qs.dtype == np.float64 and qs.ndim == 1 and qs.flags.c_contiguous and qs.tolist() == want
    for bad in (-1, 101, [5, 101], np.array([[5.0, 95.0]]), [np.nan]):
        with pytest.raises(ValueError, match=r"\[0, 100\]"):
            _analysis.check_q(bad)
    with pytest.raises(ValueError):
        _analysis.check_q(None)
    qs = _analysis.check_q(None, allow_none=True)
    assert qs.shape == (0,) and qs.dtype == np.float64
    with pytest.raises(ValueError):
        _analysis.check_q([101], allow_none=True)


def test_check_states():
    shape, K = (5, 3, 4), 2
    W, V = np.zeros((6, 5, 2)), np.zeros((6, 3, 4, 2))
    for model in ((), (shape, K)):
        Ws, Vs = _analysis.check_states(W, V, *model)
        assert Ws.shape == W.shape and Vs.shape == V.shape
        bad = [(np.zeros((6, 5, 3)), V),                       # a wrong K
               (np.zeros((7, 5, 2)), V), (W, V[:5]),           # a wrong S between W and V
               (W[0], V), (W, V[0]), (W, V[..., None])]        # a wrong ndim
        for w, v in bad:
            with pytest.raises(ValueError, match="Ws must be"):
                _analysis.check_states(w, v, *model)
    # against a model: its own N, M, T, K, named in the message, and at least one sample
    for w, v in ((np.zeros((6, 4, 2)), V), (W, np.zeros((6, 3, 5, 2))), (np.zeros((6, 5, 3)), np.zeros((6, 3, 4, 3)))):
        _analysis.check_states(w, v)                            # consistent with each other
        with pytest.raises(ValueError, match=r"results: Ws must be \(S,5,2\) and Vs \(S,3,4,2\), got"):
            _analysis.check_states(w, v, shape, K, what="results: ")
    with pytest.raises(ValueError):
        _analysis.check_states(W[:0], V[:0], shape, K)
    Ws, Vs = _analysis.check_states(W[:0], V[:0])               # S = 0 without a model: the entry point's refusal, as before
    assert Ws.shape == (0, 5, 2) and Vs.shape == (0, 3, 4, 2)
    # V alone (fold_in_rows): at least one sample with or without a model
    assert _analysis.check_states(None, V)[0] is None and _analysis.check_states(None, V, shape, K)[1].shape == V.shape
    for v, model in ((V[:0], ()), (V[0], ()), (V[:0], (shape, K)), (np.zeros((6, 3, 4, 3)), (shape, K))):
        with pytest.raises(ValueError, match="Vs must be"):
            _analysis.check_states(None, v, *model)
    # non-contiguous and float32 inputs come back contiguous float64 with equal values
    rs = np.random.RandomState(0)
    W32 = rs.normal(size=(6, 2, 5)).astype(np.float32).transpose(0, 2, 1)
    V32 = rs.normal(size=(6, 3, 8, 2)).astype(np.float32)[:, :, ::2]
    assert not W32.flags.c_contiguous and not V32.flags.c_contiguous
    for model in ((), (shape, K)):
        Ws, Vs = _analysis.check_states(W32, V32, *model)
        assert Ws.dtype == Vs.dtype == np.float64 and Ws.flags.c_contiguous and Vs.flags.c_contiguous
        assert np.array_equal(Ws, W32) and np.array_equal(Vs, V32)


def test_check_scalars():
    a = _analysis.check_scalars("nu2", np.full((4, 1), 2.0, dtype=np.float32), 4)
    assert a.shape == (4,) and a.dtype == np.float64 and a.flags.c_contiguous and np.all(a == 2.0)
    for bad in (None, np.ones(3), np.ones((4, 2))):
        for positive in (True, False):
            with pytest.raises(ValueError, match="sigma2"):
                _analysis.check_scalars("sigma2", bad, 4, positive=positive)
    for bad in ([1, 1, 0, 1], [1, -1, 1, 1], [1, 1, np.nan, 1], [np.inf, 1, 1, 1]):
        with pytest.raises(ValueError, match="finite and positive"):
            _analysis.check_scalars("sigma2", bad, 4)
        assert _analysis.check_scalars("sigma2", bad, 4, positive=False).shape == (4,)      # only counted


class _Lib:
    """Stands in for the library: the texts and failing index it keeps for a context and for the stateless entry points."""

    def btf_last_error(self, handle):
        return b"text of the context" if handle else b"text of the stateless call"

    def btf_fail_index(self, handle):
        return 7 if handle else 3


def test_return_code_check():
    lib = _Lib()
    assert _native.check(_native.BTF_OK, lib) is None and _native.check(_native.BTF_OK, lib, object()) is None
    for code in (_native.BTF_EINVAL, _native.BTF_EHIP, _native.BTF_ESTATE):
        with pytest.raises(_native.BTFError, match="text of the stateless call") as err:
            _native.check(code, lib)
        assert err.value.code == code and not isinstance(err.value, np.linalg.LinAlgError)
    with pytest.raises(_native.BTFError, match="text of the context") as err:
        _native.check(_native.BTF_EINVAL, lib, object())
    assert err.value.code == _native.BTF_EINVAL
    for handle, index, text in ((None, 3, "stateless call"), (object(), 7, "context")):
        with pytest.raises(_native.NotPositiveDefiniteError, match=text) as err:
            _native.check(_native.BTF_ENOTPD, lib, handle)
        assert isinstance(err.value, np.linalg.LinAlgError) and isinstance(err.value, _native.BTFError)
        assert err.value.code == _native.BTF_ENOTPD and err.value.index == index
    with pytest.raises(_native.NotPositiveDefiniteError) as err:          # an entry point that records no failing system
        _native.check(_native.BTF_ENOTPD, lib, fail_index=False)
    assert err.value.index == -1


# ---- a model with no device behind it: every refusal comes before any device call
class _NoDevice:
    """Stands in for the context: any call into the library fails the test."""

    def call(self, name, *args):
        raise AssertionError("device entry point %s called" % name)


N, M, T, K, S = 5, 3, 4, 2, 6


def _model_without_a_device(world=1, collected=None):
    m = object.__new__(GaussianBayesianTensorFiltering)
    m.nrows, m.ncols, m.ndepth, m.nembeds, m.device = N, M, T, K, 0
    m._plan, m._exchange, m._ctx = types.SimpleNamespace(world=world), types.SimpleNamespace(active=False), _NoDevice()
    if collected is not None:
        m._collected = collected
    return m


Y, Y_NEW = np.zeros((N, M, T)), np.zeros((2, M, T))
FROM_COLLECTED = {
    "posterior_summary": lambda m: m.posterior_summary(),
    "information_criteria": lambda m: m.information_criteria(data=Y),
    "loo": lambda m: m.loo(data=Y),
    "posterior_predictive": lambda m: m.posterior_predictive(),
    "posterior_functionals": lambda m: m.posterior_functionals(),
    "fold_in_rows": lambda m: m.fold_in_rows(Y_NEW),
    "convergence_diagnostics": lambda m: m.convergence_diagnostics(),
}
FROM_RESULTS = {
    "information_criteria": lambda m, res: m.information_criteria(res, data=Y),
    "loo": lambda m, res: m.loo(res, data=Y),
    "posterior_predictive": lambda m, res: m.posterior_predictive(res),
    "posterior_functionals": lambda m, res: m.posterior_functionals(res),
    "fold_in_rows": lambda m, res: m.fold_in_rows(Y_NEW, results=res),
    "convergence_diagnostics": lambda m, res: m.convergence_diagnostics(res),      # the model's own samples beside the dict
}


@pytest.mark.parametrize("name", sorted(FROM_COLLECTED))
def test_nothing_collected_is_a_runtime_error(name):
    for collected in (None, 0):
        with pytest.raises(RuntimeError, match="no samples collected on the device"):
            FROM_COLLECTED[name](_model_without_a_device(collected=collected))


@pytest.mark.parametrize("name", sorted(FROM_COLLECTED))
def test_a_sharded_model_is_refused(name):
    good = dict(W=np.zeros((S, N, K)), V=np.zeros((S, M, T, K)), nu2=np.ones((S, 1)), sigma2=np.ones((S, 1)))
    for collected in (0, S):
        with pytest.raises(NotImplementedError, match="unsharded"):
            FROM_COLLECTED[name](_model_without_a_device(world=2, collected=collected))
    if name in FROM_RESULTS:
        with pytest.raises(NotImplementedError, match="unsharded"):
            FROM_RESULTS[name](_model_without_a_device(world=2, collected=S), good)


@pytest.mark.parametrize("name", sorted(FROM_RESULTS))
def test_malformed_results_are_a_value_error(name):
    one = np.ones((S, 1))
    wrong_K = dict(W=np.zeros((S, N, K + 1)), V=np.zeros((S, M, T, K + 1)), nu2=one, sigma2=one)
    short_V = dict(W=np.zeros((S, N, K)), V=np.zeros((S - 1, M, T, K)), nu2=one, sigma2=one)
    for bad in (wrong_K, short_V, {}):
        with pytest.raises(ValueError):
            FROM_RESULTS[name](_model_without_a_device(collected=S), bad)


# ---- the C++ side: the analysis entry points have a compilation unit of their own
def test_analysis_entry_points_live_in_their_own_unit():
    pattern = re.compile(r"btf_posterior_\w+|btf_collect_(summary|functionals|ranking|association|monotone|fold_in)|btf_crit_\w+|"
                         r"btf_predict_\w+|btf_fold_in_rows|btf_diag_eval")
    names = sorted(n for n in _native.SIGNATURES if pattern.fullmatch(n))
    assert len(names) >= 19 and "btf_collect_begin" not in names and "btf_collect_end" not in names
    unit = os.path.join(_native.CSRC, "btf_analysis.hip")
    assert unit in _native.SOURCES
    analysis, abi = open(unit).read(), open(os.path.join(_native.CSRC, "btf_abi.hip")).read()
    for name in names:
        definition = re.compile(r"^int %s\(" % name, re.M)
        assert len(definition.findall(analysis)) == 1, name
        assert not definition.search(abi), name
