"""Host halves of slice_fold_in_cols (functionalmf_amd/slice_fold_in_cols.py): the numpy definition against the stored
moments of the exact Gibbs chain, the exact fit, fixed scales, every refusal before the library is loaded, the wiring of the
new unit and symbols, and the safety of the replay inputs.  No GPU.  The problem builders are shared with
tests/test_gpu_slice_fold_in_cols.py."""
import functools
import os
import re

import numpy as np
import pytest
from conftest import load_golden

from functionalmf_amd import _native, utils
from functionalmf_amd import fold_in_cols as fc
from functionalmf_amd import slice_fold_in as sf
from functionalmf_amd import slice_fold_in_cols as sc
from functionalmf_amd.factor import (ConstrainedNonconjugateBayesianTensorFiltering, NegativeBinomialBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)
from test_gpu_fold_in_cols import z_problem
from test_host_slice_fold_in import _bare, draw_rows, fit_constraints, gamma_table, no_device  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e9                   # the project's bound on cond(Q) for a replay against numpy
# Every decision of a replayed chain (r(v') against the slice height, every constraint slack against 0) is further than
# this from its edge.  A relative 1e-6 on nu moves a proposal by 1e-6 |nu sin phi|, a slack (coefficients of order one on
# curves of order one, |nu| well below one) by less than 1e-6, and r by 1e-6 times its slope along nu; the smallest of the
# ~1e5 slacks a case meets is of order 1e-5, so a larger bound would leave no seed.  test_replay_inputs_are_safe shows
# that scaling every nu of the definition by 1 + 1e-6 changes no rounds / unfinished count at this bound; the device's
# rounding (1e-15 relative) is nine orders below that perturbation.
MARGIN_MIN = 2e-6
Z_SWEEPS = 256                   # the sweeps of the replicates below (largest |z| seen: 0.97 exact fit, 2.37 doubled variance)

# family, K, tf_order, T, constrained: every family with and without constraints, K in {1, 3, 5, 8, 10}, tf_order in
# {0, 1, 2}, T in {6, 9}
REPLAY_CASES = [
    ("poisson_log", 1, 0, 6, False), ("poisson_log", 5, 2, 9, True),
    ("poisson_identity", 3, 1, 9, False), ("poisson_identity", 10, 2, 6, True),
    ("bernoulli_logit", 5, 0, 6, False), ("bernoulli_logit", 8, 1, 9, True),
    ("gaussian", 8, 2, 9, False), ("gaussian", 1, 1, 6, True),
    ("negbin_logit", 10, 0, 6, False), ("negbin_logit", 3, 2, 9, True),
    ("gamma_grid", 3, 1, 6, False), ("gamma_grid", 5, 2, 9, True),
]


def replay_problem(family, K, tf_order, T, constrained, seed, S=3, N=70, sweeps=3, max_rounds=40, fixed=False):
    """S states on N = 70 rows (one full pass of 64 lanes and a tail) and four new columns: complete, half missing, a
    single observed cell, empty.  Every row of W is positive and every factor of the true curve falls along the depth
    axis, so the curves are positive and falling: feasible under the constraints."""
    rs = np.random.RandomState(seed)
    falls = np.stack([np.linspace(1.0, 0.3 + 0.05 * k, T) for k in range(K)], axis=-1)              # (T,K)
    scale = 3.0 if family == "poisson_identity" else 1.0
    Ws = rs.uniform(0.5, 1.5, size=(S, N, K)) / K
    v_true = scale * rs.uniform(0.5, 1.5, size=(4, 1, K)) * falls[None]                             # (C,T,K)
    lam2 = np.resize([0.05, 0.1, 0.2], S)
    lik = gamma_table(6, rs)
    param = {"gaussian": 0.3, "negbin_logit": 4.0, "gamma_grid": lik}.get(family)
    Y = draw_rows(family, param, np.einsum("nk,ctk->cnt", Ws[0], v_true), 2, rs)
    Y[1][rs.uniform(size=Y[1].shape) < 0.5] = np.nan
    one = Y[2, 5, T // 2, 0]
    Y[2] = np.nan
    Y[2, 5, T // 2, 0] = one
    Y[3] = np.nan
    start = 0.9 * v_true                                                                             # (C,T,K)
    Cons = fit_constraints(T) if constrained else None
    nD = fc.penalty(T, tf_order).shape[0]
    tau2 = rs.uniform(0.5, 2.0, size=(4, nD)) if fixed else None
    draws = sc.random_draws(rs, T, K, tf_order, sweeps, max_rounds, size=(S, 4))
    return dict(family=family, K=K, tf_order=tf_order, T=T, Ws=Ws, lam2=lam2, Y=Y, start=start, Cons=Cons, tau2=tau2, draws=draws,
                param=param, sweeps=sweeps, max_rounds=max_rounds)


def definition(c, nu_scale=1.0):
    """The numpy definition on the inputs of replay_problem, with the default fit."""
    S, N = c["Ws"].shape[:2]
    p = sf.check_param(c["family"], c["param"])
    C, S1, cnt, L = sc.column_statistics(c["Y"], c["family"], N, c["T"])
    a, b = sc.fit_weights(sc.gaussian_fit(c["Y"], c["family"], c["param"]), C, N, c["T"])
    tau2 = None if c["tau2"] is None else np.broadcast_to(c["tau2"], (S,) + c["tau2"].shape)
    return sc.chains(np.broadcast_to(c["start"], (S,) + c["start"].shape), c["Ws"], c["lam2"], c["tf_order"], c["family"], p,
                     (S1, cnt, L), a, b, c["Cons"], tau2, c["draws"], sweeps=c["sweeps"], max_rounds=c["max_rounds"],
                     nu_scale=nu_scale)


def safe(want):
    return want["cond"] <= COND_MAX and min(want["margin_ll"], want["margin_slack"]) > MARGIN_MIN and np.all(np.isfinite(want["V"]))


def replay_inputs(family, K, tf_order, T, constrained, need_unfinished=False, **kw):
    """The inputs of a replay case, chosen by the definition alone: the first seed of a fixed sequence whose chains keep
    cond(Q) <= COND_MAX and both decision margins above MARGIN_MIN (and, need_unfinished, leave a sweep at the cap)."""
    base = 1000 * K + 100 * tf_order + 10 * T + (5 if constrained else 0)
    for k in range(200):
        c = replay_problem(family, K, tf_order, T, constrained, base + 7919 * k, **kw)
        want = definition(c)
        if safe(want) and (not need_unfinished or want["unfinished"].sum() > 0):
            c["want"] = want
            return c
    raise AssertionError("no seed with cond(Q) <= %g and margins above %g" % (COND_MAX, MARGIN_MIN))


@functools.lru_cache(maxsize=None)
def replay_case(idx):
    c = replay_inputs(*REPLAY_CASES[idx])
    for a in (c["Ws"], c["Y"], c["draws"], c["want"]["V"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def capped_case():
    """max_rounds = 2: the definition has unfinished sweeps."""
    return replay_inputs("poisson_identity", 3, 1, 6, True, need_unfinished=True, max_rounds=2)


@functools.lru_cache(maxsize=None)
def fixed_case():
    """tau2= fixed."""
    return replay_inputs("gamma_grid", 3, 2, 6, True, fixed=True)


def z_inputs(multiplier):
    """z_problem as a slice_fold_in_cols problem of the Gaussian family: (W, lam2, nu2, stats, weights, sums)."""
    W, Y, nu2, lam2 = z_problem()
    N, T = Y.shape
    _, S1, cnt, L = sc.column_statistics(Y[None], "gaussian", N, T)
    a, b = sc.fit_weights(sc.gaussian_fit(Y[None], "gaussian", nu2, multiplier=multiplier), 1, N, T)
    return W, lam2, nu2, (S1[0], cnt[0], None), a[0], b[0]


def z_replicates(multiplier, R, seed, sweeps=Z_SWEEPS):
    """R replicates of `chain` on z_problem under numpy's generator from v = 0; returns (V (R,T,K), rounds, unfinished)."""
    W, lam2, nu2, stats, a, b = z_inputs(multiplier)
    rng = np.random.default_rng(seed)
    V, rounds, unf = [], 0, 0
    for _ in range(R):
        o = sc.chain(np.zeros((stats[0].shape[1], W.shape[1])), W, lam2, 2, "gaussian", nu2, stats, a, b, rng=rng, sweeps=sweeps,
                     track_cond=False)
        V.append(o["v"])
        rounds, unf = rounds + o["rounds"], unf + o["unfinished"]
    return np.array(V), rounds, unf


def z_against_gibbs(V):
    """Largest two-sample |z| of the per-coordinate means of V (replicates along axis 0) against the stored moments of the
    exact Gibbs chain (tests/golden/fold_in_cols_numpy_replicates.npz), the standard error from both variances."""
    g = load_golden("fold_in_cols_numpy_replicates.npz")
    se = np.sqrt(V.var(axis=0, ddof=1) / V.shape[0] + g["var"] / int(g["nsamples"]))
    return float(np.max(np.abs(V.mean(axis=0) - g["mean"]) / se))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("multiplier", [1.0, np.sqrt(2.0)])
def test_definition_against_stored_gibbs_moments(multiplier):
    """300 replicates of `chain` on z_problem, Gaussian family, with the exact fit (multiplier 1) and with a fit of doubled
    variance: each reproduces the stored moments of the exact Gibbs chain, largest two-sample |z| below 5.  With the exact
    fit every sweep accepts its first proposal."""
    V, rounds, unf = z_replicates(multiplier, 300, seed=11)
    z = z_against_gibbs(V)
    print("multiplier %.3f: largest |z| %.2f, proposals per sweep %.2f, unfinished %d" % (multiplier, z, rounds / (300.0 * Z_SWEEPS), unf))
    assert unf == 0
    if multiplier == 1.0:
        assert rounds == 300 * Z_SWEEPS
    assert z < 5


def test_exact_fit_is_the_gibbs_draw_of_fold_in_cols():
    """With the exact fit and phi = pi / 2 (u_a = 1 / 4) the accepted proposal is m + nu: the chain on the record of
    fold_in_cols.chain (same normals and gammas) walks the Gibbs chain's path."""
    W, lam2, nu2, stats, a, b = z_inputs(1.0)
    _, Y, _, _ = z_problem()
    T, K, sweeps = Y.shape[1], W.shape[1], 5
    nD, n = fc.penalty(T, 2).shape[0], T * K
    rs = np.random.RandomState(3)
    d = sc.random_draws(rs, T, K, 2, sweeps).copy()
    body = d[4 * nD:].reshape(sweeps, -1)
    body[:, n + 1] = 0.25
    gibbs = np.concatenate([d[:4 * nD]] + [np.concatenate([body[r, :n], body[r, n + 1 + sc.DEFAULT_MAX_ROUNDS:]]) for r in range(sweeps)])
    v, _, tau2 = fc.chain(Y, W, nu2, lam2, 2, sweeps, gibbs)
    o = sc.chain(np.zeros((T, K)), W, lam2, 2, "gaussian", nu2, stats, a, b, draws=d, sweeps=sweeps)
    assert o["rounds"] == sweeps and o["unfinished"] == 0
    np.testing.assert_allclose(o["v"], v, rtol=0, atol=1e-10)
    np.testing.assert_allclose(o["tau2"], tau2, rtol=1e-9)


def test_fixed_scales_never_move():
    c = fixed_case()
    want = c["want"]
    assert np.array_equal(want["Tau2"], np.broadcast_to(c["tau2"], want["Tau2"].shape))
    free = definition(dict(c, tau2=None))
    assert not np.allclose(free["Tau2"], want["Tau2"]) and not np.allclose(free["V"], want["V"])


def test_chain_refuses_a_bad_start_and_replays():
    c = replay_case(3)
    S, N = c["Ws"].shape[:2]
    again = definition(c)
    assert np.array_equal(again["V"], c["want"]["V"]) and np.array_equal(again["rounds"], c["want"]["rounds"])
    p = sf.check_param(c["family"], c["param"])
    _, S1, cnt, L = sc.column_statistics(c["Y"], c["family"], N, c["T"])
    bad = sc.chain(-c["start"][0], c["Ws"][0], 0.1, c["tf_order"], c["family"], p, (S1[0], cnt[0], None), Constraints=c["Cons"],
                   draws=c["draws"][0, 0], sweeps=c["sweeps"])
    assert bad["failed"] and np.all(np.isnan(bad["v"])) and bad["rounds"] == 0


@pytest.mark.parametrize("which", list(range(len(REPLAY_CASES))) + ["capped", "fixed"])
def test_replay_inputs_are_safe(which):
    """The inputs of every replay case are chosen by the definition alone (cond(Q) <= COND_MAX, margins above MARGIN_MIN),
    and with such margins scaling every nu by 1 + 1e-6 changes no rounds / unfinished count."""
    c = capped_case() if which == "capped" else fixed_case() if which == "fixed" else replay_case(which)
    want = c["want"]
    assert safe(want), (want["cond"], want["margin_ll"], want["margin_slack"])
    assert want["rounds"].sum() > 0
    if which == "capped":
        assert want["unfinished"].sum() > 0
    moved = definition(c, nu_scale=1.0 + 1e-6)
    assert np.array_equal(moved["rounds"], want["rounds"]) and np.array_equal(moved["unfinished"], want["unfinished"])
    assert np.max(np.abs(moved["V"] - want["V"]) / np.maximum(1.0, np.abs(want["V"]))) < 1e-4


def test_gaussian_fit_and_fit_weights():
    rs = np.random.RandomState(0)
    lik = gamma_table(5, rs)
    for family, param in (("poisson_log", None), ("poisson_identity", None), ("bernoulli_logit", None), ("gaussian", 0.4),
                          ("negbin_logit", 3.0), ("gamma_grid", lik)):
        eta = rs.uniform(0.3, 1.2, size=(2, 6, 4))
        Y = draw_rows(family, param, eta, 3, rs)
        Y[0, 1] = np.nan
        Y[1, 2, 3, :2] = np.nan
        mu, sd = sc.gaussian_fit(Y, family, param)
        assert mu.shape == sd.shape == (2, 6, 4)
        assert np.all(np.isnan(mu[0, 1])) and np.all(np.isnan(sd[0, 1]))
        ok = ~np.isnan(mu)
        assert ok.sum() == 2 * 6 * 4 - 4 and np.all(sd[ok] > 0) and np.all(np.isfinite(mu[ok]))
        wide = sc.gaussian_fit(Y, family, param, multiplier=4)[1]
        np.testing.assert_allclose(wide[ok], 2 * sd[ok])
        a, b = sc.fit_weights((mu, sd), 2, 6, 4)
        assert np.all(a[~ok] == 0) and np.all(b[~ok] == 0)
        np.testing.assert_allclose(a[ok], 1 / sd[ok] ** 2)
        np.testing.assert_allclose(b[ok], mu[ok] / sd[ok] ** 2)
    Yg = 0.7 + 0.1 * rs.normal(size=(1, 3, 2, 5))
    mu, sd = sc.gaussian_fit(Yg, "gaussian", 0.4, multiplier=1)
    np.testing.assert_allclose(mu, Yg.mean(axis=3))
    np.testing.assert_allclose(sd, np.sqrt(0.4 / 5))
    z, z2 = sc.fit_weights(False, 1, 3, 2)
    assert not z.any() and not z2.any()
    sd[0, 0, 0] = -1.0
    assert sc.fit_weights((mu, sd), 1, 3, 2)[0][0, 0, 0] == 0
    with pytest.raises(ValueError):
        sc.fit_weights((mu, sd[:, :2]), 1, 3, 2)
    with pytest.raises(ValueError):
        sc.fit_weights((mu, np.full(sd.shape, np.inf)), 1, 3, 2)


def _cols_bare(cls, **kw):
    m = _bare(cls, **kw)
    m.tf_order, m.stability = 2, 1e-6
    return m


def test_model_refusals_raise_before_any_device_call(no_device):
    """Bad shapes, an LDS refusal, draws of the wrong shape or range, a callable likelihood, a sharded model, nothing
    collected, the Negative-Binomial model - each before any device call, and without taking a seed."""
    Y = np.ones((2, 5, 4))
    res = {"W": np.ones((6, 5, 2)), "V": np.ones((6, 3, 4, 2)), "lam2": np.ones((6, 1))}
    L = sc.record_length(4, 2, 2, 3)
    nD = fc.penalty(4, 2).shape[0]
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        g = _cols_bare(cls)
        with pytest.raises(NotImplementedError):
            _cols_bare(cls, world=2).slice_fold_in_cols(Y, results=res)
        with pytest.raises(NotImplementedError):
            _cols_bare(cls, family=lambda W, V, d: 0.0).slice_fold_in_cols(Y, results=res)
        with pytest.raises(RuntimeError):
            g.slice_fold_in_cols(Y)                            # nothing collected, no results
        for bad_Y in (np.ones((2, 5, 5)), np.ones((5, 4)), np.ones((2, 4, 4, 1)), (Y, Y), np.full((2, 5, 4), np.inf)):
            with pytest.raises(ValueError):
                g.slice_fold_in_cols(bad_Y, results=res)
        for key, val in (("W", np.ones((6, 5, 3))), ("V", np.ones((6, 3, 4, 3))), ("lam2", np.ones(5)),
                         ("lam2", np.array([1, 1, -1, 1, 1, 1.0])), ("lam2", None)):
            with pytest.raises(ValueError):
                g.slice_fold_in_cols(Y, results=dict(res, **{key: val}))
        for kw in (dict(start=np.zeros(3)), dict(start=np.full((4, 2), np.nan)), dict(tau2=np.ones((2, nD + 1))),
                   dict(tau2=-np.ones((2, nD))), dict(sweeps=3, draws=np.full((6, 2, L - 1), 0.5)),
                   dict(sweeps=3, draws=np.full((6, 2, L), 1.5)), dict(sweeps=3, draws=np.full((6, 2, L), -0.5)),
                   dict(fit=(np.ones((2, 5, 4)),)), dict(fit=(np.ones((2, 5, 3)), np.ones((2, 5, 3)))),
                   dict(sweeps=0), dict(max_rounds=0), dict(transform="log"), dict(q=(5, 101)), dict(sweeps=2.5)):
            with pytest.raises(ValueError):
                g.slice_fold_in_cols(Y, results=res, **kw)
        assert g._draws == 0                                   # a refused call takes no seed
    big = _cols_bare(NonconjugateBayesianTensorFiltering, M=3, T=370, K=10)
    with pytest.raises(ValueError, match="LDS"):
        big.slice_fold_in_cols(np.ones((1, 5, 370)), results={"W": np.ones((2, 5, 10)), "V": np.ones((2, 3, 370, 10)), "lam2": np.ones(2)})
    gg = _cols_bare(NonconjugateBayesianTensorFiltering, family="gamma_grid")
    gg._gg_table = sf.check_param("gamma_grid", gamma_table(4, np.random.RandomState(0)))
    with pytest.raises(ValueError, match="y > 0"):
        gg.slice_fold_in_cols(np.zeros((2, 5, 4)), results=res)
    assert not hasattr(NegativeBinomialBayesianTensorFiltering, "slice_fold_in_cols")
    for cls in (NonconjugateBayesianTensorFiltering, ConstrainedNonconjugateBayesianTensorFiltering):
        with pytest.raises(NotImplementedError, match="slice-sampled.*slice_fold_in_cols"):
            _cols_bare(cls).fold_in_cols(Y, results=res)


def test_stateless_refusals_raise_before_any_device_call(no_device):
    W = np.ones((6, 5, 2))
    V = np.ones((6, 3, 4, 2))
    Y = np.ones((2, 5, 4))
    one = np.ones(6)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "binomial", lam2=one, Vs=V)
    with pytest.raises(NotImplementedError):
        utils.slice_fold_in_cols(Y, W, lambda W, V, d: 0.0, lam2=one, Vs=V)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W[0], "poisson", lam2=one, Vs=V)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", Vs=V)                                   # no lam2
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=-one, Vs=V)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one)                               # neither Vs nor start
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one, Vs=V[:, :, :3])
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y[:, :4], W, "poisson", lam2=one, Vs=V)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one, Vs=V, first_sample=-1)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one, Vs=V, first_sample=2 ** 31 // 2)
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "gaussian", lam2=one, Vs=V)                        # no variance
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one, Vs=V, Constraints=np.ones((3, 4)))
    with pytest.raises(ValueError):
        utils.slice_fold_in_cols(Y, W, "poisson", lam2=one, Vs=V, stability=0.0)
    with pytest.raises(ValueError, match="LDS"):
        utils.slice_fold_in_cols(np.ones((1, 5, 370)), np.ones((2, 5, 10)), "poisson", lam2=np.ones(2), start=np.zeros((370, 10)))
    with pytest.raises(ValueError, match="below 64"):
        utils.slice_fold_in_cols(np.ones((1, 5, 4)), np.ones((2, 5, 10)), "poisson", lam2=np.ones(2), start=np.zeros((4, 10)), tf_order=6)


def test_lds_count():
    """The count of the header, restated: the dose-response shape fits, and so does the flu shape of fold_in_cols's table."""
    T, K, tf = 9, 5, 2
    nD = fc.penalty(T, tf).shape[0]
    n, bw = T * K, 3 * K
    assert sc.lds_bytes(T, K, tf) == 8 * (n * (bw + 1) + 6 * n + T * 15 + 5 * nD + T * 4) + 8 * ((bw * (bw + 1) // 2 + 3) // 4) + 8192
    assert sc.lds_bytes(T, K, tf) < sc.LDS_LIMIT == fc.LDS_LIMIT
    assert sc.lds_bytes(370, 10, 2) > sc.LDS_LIMIT
    assert sc.record_length(T, K, tf, 3, 40) == 4 * nD + 3 * (n + 41 + 4 * nD)


def test_the_unit_and_the_symbols_are_wired():
    assert os.path.join(_native.CSRC, "btf_slice_fold_cols.hip") in _native.SOURCES
    assert os.path.exists(os.path.join(_native.CSRC, "btf_slice_fold_cols.h"))
    text = open(os.path.join(ROOT, "include", "btf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    analysis = open(os.path.join(_native.CSRC, "btf_analysis.hip")).read()
    for name in ("btf_slice_fold_cols", "btf_collect_slice_fold_cols"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _native.SIGNATURES
        assert re.search(r"^int\s+%s\s*\(" % name, analysis, flags=re.M), name + " is defined beside the analysis entry points"
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_native.SIGNATURES[name][1]), name
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load()
        assert hasattr(lib, "btf_slice_fold_cols") and hasattr(lib, "btf_collect_slice_fold_cols")
    assert sc.DEFAULT_SWEEPS & (sc.DEFAULT_SWEEPS - 1) == 0 and sc.DEFAULT_MAX_ROUNDS == 40
