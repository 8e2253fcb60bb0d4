"""Posterior predictive checks on the GPU (csrc/btf_checks.h via BayesianTensorFiltering.posterior_checks,
utils.posterior_checks and checks.evaluate) against the written definition, functionalmf_amd/checks.py.

The replicated curves are the documented draws: every case rebuilds T_rep and T_obs in numpy (checks.reference) from the
draws utils.posterior_predictive returns for the same seed with draws_per_sample = reps * nreps.  Tolerances are those of
the project's fixed-order fp64 reductions: relative 1e-12 of max |T| for chisq, max, total; absolute 1e-12 for lag1
(|lag1| <= 1 by Cauchy-Schwarz); zeros exact.  The integer counts are compared exactly, which presupposes that no
comparison is decided by rounding: a comparison is ambiguous when |T_rep - T_obs| <= 1e-9 max(1, |T_obs|) while the
replicated curve differs from the observed one (identical curves tie exactly on both sides), and every fixed seed of this
file is asserted to have none.  Three kinds of tie between different curves are exact on both sides as well and are not
counted: `zeros` and, for count data, `total` (sums of integers below 2^53 are exact in any order), and a `max` that is
bitwise equal on the two sides (the maximum selects one term |y - mu| / sqrt(v), computed alike for y_rep and y: equal
bits mean the same slot holds the same count).  What remains is genuine: lag1 of count data depends on the replicates of
a depth through their sum alone, so a replicated curve with the data's sum at every depth ties with it up to the rounding
of the plain adds.  The count families therefore get levels of ten to twenty counts a slot, which keeps such a curve
improbable at the few depths of these shapes (and takes the samplers through both their inversion and rejection paths).
Statistical thresholds as in tests/test_gpu_predictive.py: Z = 5.5, p-value floor 1e-6."""
import numpy as np
import pytest
from scipy import stats

from functionalmf_amd import _native, checks, predictive, utils
from functionalmf_amd.factor import (BinomialBayesianTensorFiltering, GaussianBayesianTensorFiltering,
                                     NonconjugateBayesianTensorFiltering)

pytestmark = pytest.mark.gpu

Z = 5.5
PFLOOR = 1e-6
FAMS = ["poisson", "poisson_identity", "binomial", "gaussian", "negbin"]
ALL = checks.DISCREPANCIES
PER_CURVE = ("p_ge", "p_gt", "defined", "t_obs", "t_rep")


LEVEL = {"poisson": 3.0, "negbin": 2.5}          # added to eta: tens of counts a slot (see the docstring)


def _states(rs, S, N, M, T, K, fam="gaussian", scale=0.6):
    if fam == "poisson_identity":
        return rs.uniform(1.0, 3.0, size=(S, N, K)), rs.uniform(1.0, 3.0, size=(S, M, T, K))
    Ws, Vs = rs.normal(0, scale, size=(S, N, K)), rs.normal(0, scale, size=(S, M, T, K))
    if fam in LEVEL:
        Ws[..., 0] = 1.0
        Vs[..., 0] += LEVEL[fam]
    return Ws, Vs


def _eta(Ws, Vs):
    return np.einsum("znk,zmtk->znmt", Ws, Vs)


def _family_args(fam, rs, S, shape):
    """keyword arguments of utils.posterior_checks / posterior_predictive and the (S,N,M,T)-broadcastable aux"""
    if fam == "gaussian":
        nu2 = rs.uniform(0.2, 0.6, size=S)
        return dict(nu2=nu2), nu2[:, None, None, None]
    if fam == "negbin":
        R = rs.uniform(0.5, 4.0, size=(S,) + (shape[0], 1, shape[2]))
        return dict(R=R), R
    if fam == "binomial":
        tr = rs.randint(0, 60, size=shape).astype(float)
        return dict(trials=tr), tr[None]
    return {}, None


def _data(fam, rs, Mu0, nreps):
    Y = np.nan_to_num(Mu0)[..., None] + rs.normal(size=Mu0.shape + (nreps,))
    return Y if fam == "gaussian" else np.round(np.abs(Y))


def _moments(fam, Ws, Vs, aux):
    code = predictive.family_code(fam)
    eta = _eta(Ws, Vs)
    with np.errstate(invalid="ignore"):
        return predictive.mean_function(code, eta, aux), checks.variance_function(code, eta, aux)


def _arrays(out):
    """every array of a result dict, by name"""
    flat = {"nobs": out["nobs"]}
    for name in out["which"]:
        for k in PER_CURVE:
            flat[name + "." + k] = out[name][k]
        for k in ("T_obs", "T_rep"):
            flat["overall." + name + "." + k] = out["overall"][name][k]
        flat["overall." + name + ".p"] = np.array([out["overall"][name][k] for k in ("p_ge", "p_gt", "defined")], dtype=float)
    if "curves" in out:
        flat["curves.T_obs"], flat["curves.T_rep"] = out["curves"]["T_obs"], out["curves"]["T_rep"]
    return flat


def _assert_same_bits(a, b, names=None):
    fa, fb = _arrays(a), _arrays(b)
    for k in (fa if names is None else names):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)


def _close(name, got, ref, what):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, name, "nan pattern")
    ok = ~np.isnan(ref)
    if not ok.any():
        return
    err = np.abs(got - ref)[ok].max()
    if name == "zeros":
        assert err == 0.0, (what, name, err)
    else:
        bound = 1e-12 if name == "lag1" else 1e-12 * max(np.abs(ref[ok]).max(), 1e-300)
        assert err <= bound, (what, name, err, bound)


def _ambiguous(name, fam, T_obs, T_rep, reps, identical=None):
    """comparisons that rounding could decide: close values of curves that are not the same vector (see the docstring of
    the file for the ties that are exact on both sides)"""
    if name == "zeros" or (name == "total" and fam != "gaussian"):
        return 0
    to = np.repeat(T_obs, reps, axis=-1)
    with np.errstate(invalid="ignore"):
        near = np.abs(T_rep - to) <= 1e-9 * np.maximum(1.0, np.abs(to))
        if name == "max":
            near &= T_rep != to
    if identical is not None:
        near &= ~identical
    return int(near.sum())


def _check_case(fam, Ws, Vs, kw, aux, Y, reps, seed, what, call=None):
    """utils.posterior_checks (or `call`) on every curve against checks.reference on the documented draws: the raw T
    values, the nan pattern, the counts (exactly, after asserting that no comparison is ambiguous), the means and the pool."""
    S, N = Ws.shape[:2]
    M, T = Vs.shape[1:3]
    Y4 = Y[..., None] if Y.ndim == 3 else Y
    nreps = Y4.shape[3]
    curves = np.arange(N * M, dtype=np.int32)
    out = (call or utils.posterior_checks)(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=seed, curves=curves, **kw)
    cells = np.arange(N * M * T, dtype=np.int32)
    draws = utils.posterior_predictive(Ws, Vs, fam, draws_per_sample=reps * nreps, seed=seed, cells=cells, **kw)["draws"]
    Mu, Var = _moments(fam, Ws, Vs, aux)
    ref = checks.reference(Y, Mu, Var, draws, reps=reps, which=ALL, curves=curves)
    assert out["which"] == ALL and out["nsets"] == S * reps == ref["nsets"] and out["ndraws"] == S * reps * nreps
    assert out["curves"]["T_obs"].shape == (N * M, 5, S) and out["curves"]["T_rep"].shape == (N * M, 5, S * reps)
    np.testing.assert_array_equal(out["curves"]["index"], ref["curves"]["index"])
    # identical[l, e]: the replicated curve of set e equals the observed curve l slot for slot
    d = draws.reshape(N * M, T, S, reps, nreps).transpose(0, 2, 3, 1, 4).reshape(N * M, S * reps, T, nreps)
    obs = ~np.isnan(Y4).reshape(N * M, 1, T, nreps)
    identical = ((d == Y4.reshape(N * M, 1, T, nreps)) | ~obs).all(axis=(2, 3))
    for k, name in enumerate(ALL):
        _close(name, out["curves"]["T_obs"][:, k], ref["curves"]["T_obs"][:, k], what + " T_obs")
        _close(name, out["curves"]["T_rep"][:, k], ref["curves"]["T_rep"][:, k], what + " T_rep")
        _close(name, out[name]["t_obs"], ref[name]["t_obs"], what + " t_obs")
        _close(name, out[name]["t_rep"], ref[name]["t_rep"], what + " t_rep")
        assert _ambiguous(name, fam, ref["curves"]["T_obs"][:, k], ref["curves"]["T_rep"][:, k], reps, identical) == 0, \
            (what, name, "an ambiguous comparison: pick another seed")
        np.testing.assert_array_equal(out[name]["defined"], ref[name]["defined"], err_msg="%s %s defined" % (what, name))
        for key in ("p_ge", "p_gt"):
            with np.errstate(invalid="ignore"):
                got, want = np.rint(out[name][key] * out[name]["defined"]), np.rint(ref[name][key] * ref[name]["defined"])
            np.testing.assert_array_equal(got, want, err_msg="%s %s %s * defined" % (what, name, key))
            np.testing.assert_array_equal(out[name][key], ref[name][key], err_msg="%s %s %s" % (what, name, key))
        go, ro = out["overall"][name], ref["overall"][name]
        _close(name, go["T_obs"], ro["T_obs"], what + " pooled T_obs")
        _close(name, go["T_rep"], ro["T_rep"], what + " pooled T_rep")
        assert _ambiguous(name, fam, ro["T_obs"], ro["T_rep"], reps) == 0, (what, name, "an ambiguous pooled comparison: pick another seed")
        assert go["defined"] == ro["defined"], (what, name)
        for key in ("p_ge", "p_gt"):
            assert go[key] == ro[key] or (ro["defined"] == 0 and np.isnan(go[key]) and np.isnan(ro[key])), (what, name, key, go[key], ro[key])
    np.testing.assert_array_equal(out["nobs"], ref["nobs"])
    return out, ref


# ---------------------------------------------------------------- 1. + 2. the documented draws, exact counts
def _patterns(Y, pattern, rs):
    Y = Y.copy()
    if pattern == "depth_tail":
        Y[:, :, -3:] = np.nan
    elif pattern == "replicates":
        Y[rs.uniform(size=Y.shape) < 0.3] = np.nan
    elif pattern == "empty_curve":
        Y[1, 2] = np.nan
        Y[0, 0, 0, 0] = np.nan
    elif pattern == "alternating":
        Y[::2, :, 1::2] = np.nan                     # rows 0, 2, 4: no adjacent depths, lag1 is nan
        Y[1, 1, 3] = np.nan                          # a gap between observed depths
    return Y


PATTERNS = ["complete", "depth_tail", "replicates", "empty_curve", "alternating"]


@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_replicates_are_the_documented_draws_and_counts_are_exact(fam, pattern, reps):
    N, M, T, K, S, nreps = 5, 4, 7, 3, 37, 3
    shape = (N, M, T)
    rs = np.random.RandomState(1000 + 100 * FAMS.index(fam) + 10 * PATTERNS.index(pattern) + reps)
    Ws, Vs = _states(rs, S, N, M, T, K, fam)
    kw, aux = _family_args(fam, rs, S, shape)
    if fam == "binomial":
        kw["trials"][2, 1, 4] = np.nan                 # a missing trial count: the curve (2,1) is bad
    Mu, _ = _moments(fam, Ws, Vs, aux)
    Y = _patterns(_data(fam, rs, Mu[0], nreps), pattern, rs)
    out, ref = _check_case(fam, Ws, Vs, kw, aux, Y, reps, 21 + reps, "%s %s reps=%d" % (fam, pattern, reps))
    skipped = np.isnan(out["nobs"])
    want = np.zeros((N, M), dtype=bool)
    if pattern == "empty_curve":
        want[1, 2] = True
    if fam == "binomial" and pattern != "depth_tail":        # (there the missing count lies under unobserved slots: nothing is drawn)
        want[2, 1] = True
    np.testing.assert_array_equal(skipped, want)
    for name in ALL:
        for k in PER_CURVE:
            assert np.isnan(out[name][k][skipped]).all()
    if pattern == "alternating":
        assert np.isnan(out["lag1"]["p_ge"][::2]).all() and (out["lag1"]["defined"][::2][~skipped[::2]] == 0).all()
        assert not np.isnan(out["lag1"]["p_ge"][1::2][~skipped[1::2]]).any()
    if pattern == "complete" and fam != "binomial":
        assert (out["chisq"]["defined"] == S * reps).all() and (out["nobs"] == T * nreps).all()


# ---------------------------------------------------------------- 3. geometry and source independence, bit for bit
@pytest.fixture(scope="module")
def collected():
    N, M, T, K, S = 7, 5, 9, 3, 12
    rs = np.random.RandomState(0)
    Y = rs.normal(size=(N, M, T, 2))
    Y[:2, :2] = np.nan
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=5)
    res = model.run_gibbs(Y, nburn=3, nthin=1, nsamples=S, verbose=False)
    assert model._collected == S
    return model, Y, res


@pytest.mark.parametrize("fam", FAMS)
def test_uploaded_and_collected_states(collected, fam):
    model, Y, res = collected
    S, shape, K = res["W"].shape[0], (model.nrows, model.ncols, model.ndepth), model.nembeds
    rs = np.random.RandomState(2)
    code = predictive.family_code(fam)
    Yc = Y if fam == "gaussian" else np.round(np.abs(3 * Y))
    kw = dict(param=0.7 if fam in ("gaussian", "negbin") else None,
              trials=rs.randint(1, 9, size=shape).astype(float) if fam == "binomial" else None)
    up = checks.evaluate(model._ctx, shape, K, code, S, res["W"], res["V"], Y=Yc, which=ALL, reps=2, seed=11, curves=[0, 17], **kw)
    co = checks.evaluate(model._ctx, shape, K, code, S, None, None, Y=Yc, which=ALL, reps=2, seed=11, curves=[0, 17], **kw)
    _assert_same_bits(up, co)
    if fam == "poisson_identity":                # signed states: curves with w.v <= 0 somewhere are bad
        assert np.isnan(up["nobs"]).any()
    else:
        assert np.array_equal(np.isnan(up["nobs"]), np.isnan(Y).all(axis=(2, 3)))


@pytest.mark.parametrize("fam", FAMS)
def test_subset_chunks_and_seed(fam):
    N, M, T, K, S, nreps, reps = 5, 11, 4, 2, 30, 2, 2
    rs = np.random.RandomState(40 + FAMS.index(fam))
    Ws, Vs = _states(rs, S, N, M, T, K, fam)
    kw, aux = _family_args(fam, rs, S, (N, M, T))
    Y = _data(fam, rs, _moments(fam, Ws, Vs, aux)[0][0], nreps)
    Y[rs.uniform(size=Y.shape) < 0.2] = np.nan
    curves = [(4, 10), (0, 0), (2, 7), (0, 0)]
    full = utils.posterior_checks(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=99, curves=curves, **kw)
    again = utils.posterior_checks(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=99, curves=curves, **kw)
    _assert_same_bits(full, again)
    np.testing.assert_array_equal(full["curves"]["T_rep"][1], full["curves"]["T_rep"][3])       # a curve listed twice
    # a subset of the discrepancies, in another order
    sub = utils.posterior_checks(Ws, Vs, fam, Y, which=("zeros", "lag1"), reps=reps, seed=99, curves=curves, **kw)
    assert sub["which"] == ("zeros", "lag1")
    fs, ff = _arrays(sub), _arrays(full)
    for k in fs:
        if not k.startswith("curves."):
            np.testing.assert_array_equal(fs[k], ff[k], err_msg=k)
    np.testing.assert_array_equal(sub["curves"]["T_rep"], full["curves"]["T_rep"][:, [4, 2]])
    np.testing.assert_array_equal(sub["curves"]["T_obs"], full["curves"]["T_obs"][:, [4, 2]])
    # the rows in chunks of 2 and of 1: other launches, the same bits
    for rows in (2, 1):
        _assert_same_bits(full, utils.posterior_checks(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=99, curves=curves, _chunk_rows=rows, **kw))
    other = utils.posterior_checks(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=100, curves=curves, **kw)
    assert not np.array_equal(other["curves"]["T_rep"], full["curves"]["T_rep"])
    np.testing.assert_array_equal(other["curves"]["T_obs"], full["curves"]["T_obs"])             # the data side draws nothing


# ---------------------------------------------------------------- 4. edges
def _edge_case(fam, seed, S, shape, K, nreps, reps, what, missing=0.2, mutate=None, rate_shape=None, fix_Y=None):
    N, M, T = shape
    rs = np.random.RandomState(seed)
    Ws, Vs = _states(rs, S, N, M, T, K, fam)
    kw, aux = _family_args(fam, rs, S, shape)
    if rate_shape is not None:
        R = rs.uniform(0.5, 4.0, size=(S,) + rate_shape)
        kw, aux = dict(R=R), (R.reshape(S, 1, 1, 1) if len(rate_shape) == 0 else R)
    if mutate is not None:
        mutate(Ws, Vs, kw)
    Y = _data(fam, rs, _moments(fam, Ws, Vs, aux)[0][0], nreps)
    Y[rs.uniform(size=Y.shape) < missing] = np.nan
    if fix_Y is not None:
        fix_Y(Y)
    return _check_case(fam, Ws, Vs, kw, aux, Y, reps, seed + 7, what)


@pytest.mark.parametrize("fam", ["gaussian", "poisson"])
@pytest.mark.parametrize("S,reps", [(1, 1), (85, 3), (128, 2), (257, 1)])
def test_lane_block_edges(fam, S, reps):
    """nsets = 1, 255, 256, 257: under, at and over one block of lanes"""
    out, _ = _edge_case(fam, 50 + S, S, (3, 2, 4), 2, 1, reps, "%s nsets=%d" % (fam, S * reps))
    assert out["nsets"] == S * reps


@pytest.mark.parametrize("fam", ["gaussian", "binomial"])
@pytest.mark.parametrize("M", [checks.POOL_TILE - 1, checks.POOL_TILE, checks.POOL_TILE + 1, 2 * checks.POOL_TILE + 1])
def test_column_tile_edges(fam, M):
    assert checks.POOL_TILE == 8
    _edge_case(fam, 60 + M, 6, (2, M, 5), 2, 2, 1, "%s M=%d" % (fam, M))


@pytest.mark.parametrize("fam,nreps", [("gaussian", 2), ("negbin", 1), ("poisson", 1)])
def test_two_depths_and_one_observed_depth(fam, nreps):
    """T = 2, and T = 2 with the second depth unobserved - the one-depth curve a context can hold (it needs ndepth >= 2;
    T = 1 of the definition is tested in test_host_checks.py).  Count data with one replicate: curves this short tie
    only when they are identical."""
    _edge_case(fam, 70, 9, (3, 3, 2), 2, nreps, 2, fam + " T=2", missing=0.0)
    N, M, T, S, K = 3, 3, 2, 9, 2
    rs = np.random.RandomState(71)
    Ws, Vs = _states(rs, S, N, M, T, K, fam)
    kw, aux = _family_args(fam, rs, S, (N, M, T))
    Y = _data(fam, rs, _moments(fam, Ws, Vs, aux)[0][0], nreps)
    Y[:, :, 1] = np.nan
    out, _ = _check_case(fam, Ws, Vs, kw, aux, Y, 2, 72, fam + " one depth")
    assert np.isnan(out["lag1"]["p_ge"]).all() and (out["lag1"]["defined"] == 0).all() and (out["chisq"]["defined"] == S * 2).all()


@pytest.mark.parametrize("fam,K", [("gaussian", 1), ("poisson_identity", 5), ("negbin", 10), ("gaussian", 10)])
def test_nembeds(fam, K):
    _edge_case(fam, 80 + K, 7, (3, 3, 4), K, 2, 1, "%s K=%d" % (fam, K))


@pytest.mark.parametrize("fam", FAMS)
def test_three_dimensional_data(fam):
    N, M, T, S, K = 4, 3, 5, 8, 2
    rs = np.random.RandomState(90 + FAMS.index(fam))
    Ws, Vs = _states(rs, S, N, M, T, K, fam)
    kw, aux = _family_args(fam, rs, S, (N, M, T))
    Y = _data(fam, rs, _moments(fam, Ws, Vs, aux)[0][0], 1)[..., 0]
    Y[0, 1, 2] = np.nan
    assert Y.ndim == 3
    out, _ = _check_case(fam, Ws, Vs, kw, aux, Y, 3, 91, fam + " 3-D data")
    assert out["ndraws"] == S * 3


@pytest.mark.parametrize("rate_shape", [(), (4, 1, 1), (1, 3, 1), (1, 1, 5), (4, 3, 5), (4, 1, 5), (1, 3, 5), (4, 3, 1)])
def test_negative_binomial_rate_layouts(rate_shape):
    _edge_case("negbin", 100 + len(rate_shape) + sum(rate_shape), 6, (4, 3, 5), 2, 2, 1, "negbin R %r" % (rate_shape,), rate_shape=rate_shape)


def test_binomial_trials_zero_and_missing():
    def mutate(Ws, Vs, kw):
        kw["trials"][:] = np.maximum(kw["trials"], 1.0)
        kw["trials"][0, 0, 1] = 0.0                 # v == 0: out of chisq / max / lag1, and it breaks the adjacency
        kw["trials"][1, 2, :] = 0.0                 # no slot left at all: chisq = max = 0, lag1 nan
        kw["trials"][2, 1, 3] = np.nan              # a bad curve

    def fix_Y(Y):
        Y[1, 2] = 0.0                               # (no trials, no successes: every replicate of it is the same curve)
    out, ref = _edge_case("binomial", 110, 8, (3, 3, 5), 2, 2, 2, "binomial trials", missing=0.0, mutate=mutate, fix_Y=fix_Y)
    assert np.isnan(out["nobs"][2, 1]) and np.isnan(out["nobs"]).sum() == 1
    assert out["lag1"]["defined"][1, 2] == 0 and out["chisq"]["defined"][1, 2] == 16 and out["chisq"]["t_rep"][1, 2] == 0.0
    assert out["chisq"]["p_ge"][1, 2] == 1.0 and out["chisq"]["p_gt"][1, 2] == 0.0 and out["max"]["t_obs"][1, 2] == 0.0


def test_identity_link_with_a_non_positive_eta():
    def mutate(Ws, Vs, kw):
        Ws[3, 1] = -Ws[3, 1]                        # sample 3, row 1: eta < 0 at every cell of the row
    out, _ = _edge_case("poisson_identity", 120, 8, (3, 9, 4), 2, 2, 1, "identity eta <= 0", mutate=mutate)
    np.testing.assert_array_equal(np.isnan(out["nobs"]), np.arange(3)[:, None] == np.ones(9, dtype=int)[None, :])
    assert np.isfinite(out["overall"]["chisq"]["T_rep"]).all()       # the bad row is left out of the pool


@pytest.mark.parametrize("fam", ["gaussian", "poisson"])
def test_more_draws_a_cell_than_the_predictive_call_sorts(fam):
    """S * reps * nreps = 16400 > 16384: no limit here.  The reference draws come from predictive.batch at the global
    indices cell * n + d, consecutive on this (1,1,2) tensor; K = 1, so that eta = w v is the device's to the bit."""
    S, reps, N, M, T = 8200, 2, 1, 1, 2
    n = S * reps
    assert n > predictive.MAX_DRAWS
    rs = np.random.RandomState(130)
    Ws, Vs = rs.uniform(0.5, 1.5, size=(S, N, 1)), rs.uniform(0.5, 1.5, size=(S, M, T, 1))
    nu2 = rs.uniform(0.2, 0.6, size=S)
    kw = dict(nu2=nu2) if fam == "gaussian" else {}
    eta = _eta(Ws, Vs)                                              # (S,1,1,2)
    code = predictive.family_code(fam)
    aux = nu2[:, None, None, None] if fam == "gaussian" else None
    Mu = predictive.mean_function(code, eta, aux)
    Var = checks.variance_function(code, eta, aux)
    Y = _data(fam, rs, Mu[0], 1)[..., 0]
    eta_g = np.repeat(eta.reshape(S, T).T, reps, axis=1).reshape(-1)          # cell-major, then d = s * reps + rho
    aux_g = np.tile(np.repeat(nu2, reps), T) if fam == "gaussian" else np.zeros(T * n)
    draws = predictive.batch(code, eta_g, aux_g, seed=131).reshape(T, n)
    ref = checks.reference(Y, Mu, Var, draws, reps=reps, which=ALL, curves=[0])
    out = utils.posterior_checks(Ws, Vs, fam, Y, which=ALL, reps=reps, seed=131, curves=[0], **kw)
    assert out["nsets"] == n and out["ndraws"] == n
    d = draws.T                                                      # (n, T)
    identical = (d == Y.reshape(1, T)).all(axis=1)[None]
    for k, name in enumerate(ALL):
        _close(name, out["curves"]["T_rep"][:, k], ref["curves"]["T_rep"][:, k], fam + " big T_rep")
        _close(name, out["curves"]["T_obs"][:, k], ref["curves"]["T_obs"][:, k], fam + " big T_obs")
        assert _ambiguous(name, fam, ref["curves"]["T_obs"][:, k], ref["curves"]["T_rep"][:, k], reps, identical) == 0, name
        for key in PER_CURVE[:3]:
            np.testing.assert_array_equal(out[name][key], ref[name][key], err_msg=name + key)
        _close(name, out[name]["t_rep"], ref[name]["t_rep"], fam + " big t_rep")


def test_the_entry_point_refuses_on_its_own():
    N, M, T, K, S = 4, 3, 5, 2, 3
    np.random.seed(0)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K)
    lib, h, dp = _native.load(), model._ctx.h, _native.dptr
    W, V, Y = np.zeros((S, N, K)), np.zeros((S, M, T, K)), np.zeros((N, M, T, 1))
    which = np.array([0, 2], dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(_native._c_ip)
    counts, nobs, po, pr = np.zeros((5, 2, N, M)), np.zeros((N, M)), np.zeros((2, S)), np.zeros((2, S))

    def call(family=3, param=1.0, S_=S, Ws=W, Vs=V, Y_=Y, reps=1, wh=which, nw=2):
        return lib.btf_predict_check(h, family, param, S_, dp(Ws), dp(Vs), None, 0, None, dp(Y_), 1, reps, 5, ip(wh), nw, None, 0, 0,
                                     dp(counts), dp(nobs), dp(po), dp(pr), None, None)
    assert call() == _native.BTF_OK
    assert call(reps=0) == _native.BTF_EINVAL and b"reps must be >= 1" in lib.btf_last_error(h)
    assert call(wh=np.array([2, 2], dtype=np.int32)) == _native.BTF_EINVAL and b"distinct" in lib.btf_last_error(h)
    assert call(wh=np.array([0, 5], dtype=np.int32)) == _native.BTF_EINVAL and b"0..4" in lib.btf_last_error(h)
    assert call(family=5) == _native.BTF_EINVAL and call(Y_=None) == _native.BTF_EINVAL
    assert call(param=0.0) == _native.BTF_EINVAL and b"param > 0" in lib.btf_last_error(h)
    assert call(Ws=None, Vs=None) == _native.BTF_ESTATE                       # nothing collected
    assert call(reps=2 ** 30) == _native.BTF_EINVAL and b"draw index" in lib.btf_last_error(h)


# ---------------------------------------------------------------- 5. statistics
def _randomised_rank(res, name, rs):
    """(count_gt + u (count_ge - count_gt + 1)) / (n + 1): uniform when T_obs is exchangeable with its n replicates."""
    d = res[name]
    n = d["defined"]
    gt, ge = np.rint(d["p_gt"] * n), np.rint(d["p_ge"] * n)
    ok = n > 0
    u = rs.uniform(size=n.shape)
    return ((gt + u * (ge - gt + 1.0)) / (n + 1.0))[ok]


def _truth(rs, N, M, T, K, shift):
    W = rs.normal(0, 0.5, size=(1, N, K))
    V = 0.3 * np.cumsum(rs.normal(size=(1, M, T, K)), axis=2)
    V[..., 0] += shift                                  # (with W's first column near 1 below: a common level)
    W[..., 0] = 1.0
    return W, V


@pytest.mark.parametrize("fam", ["gaussian", "poisson"])
def test_well_specified_ranks_are_uniform(fam):
    """Every kept state equals the truth the data was drawn from: T_obs is exchangeable with its n = 199 replicates, so its
    randomised rank is uniform over the 1200 curves (KS against U(0,1), p > 1e-6)."""
    N, M, T, K, n = 40, 30, 12, 3, 199
    rs = np.random.RandomState(7 if fam == "gaussian" else 8)
    W, V = _truth(rs, N, M, T, K, 1.0 if fam == "poisson" else 0.0)
    eta = _eta(W, V)[0]
    if fam == "gaussian":
        Y, kw = eta + np.sqrt(0.5) * rs.normal(size=eta.shape), dict(nu2=np.array([0.5]))
    else:
        Y, kw = rs.poisson(np.exp(eta)).astype(float), {}
    res = utils.posterior_checks(W, V, fam, Y, which=("chisq", "lag1"), reps=n, seed=17, **kw)
    assert res["nsets"] == n
    for name in ("chisq", "lag1"):
        r = _randomised_rank(res, name, rs)
        assert r.size == N * M
        p = stats.kstest(r, "uniform").pvalue
        print(fam, name, "KS p", p, "overall p_ge", res["overall"][name]["p_ge"])
        assert p > PFLOOR


def test_misspecified_fits_are_flagged():
    N, M, T, K, n = 40, 30, 12, 3, 199
    rs = np.random.RandomState(9)
    W, V = _truth(rs, N, M, T, K, 1.0)
    eta = _eta(W, V)[0]
    lam = np.exp(eta)
    # Negative-Binomial data with r = 0.5, scored as Poisson at the truth: over-dispersion, chi-square far out in the tail
    Ynb = rs.poisson(rs.gamma(0.5, lam / 0.5)).astype(float)
    res = utils.posterior_checks(W, V, "poisson", Ynb, which=("chisq", "zeros"), reps=n, seed=18)
    print("negbin as poisson: overall chisq p_ge", res["overall"]["chisq"]["p_ge"], "zeros p_ge", res["overall"]["zeros"]["p_ge"])
    assert res["overall"]["chisq"]["p_ge"] < 0.01
    # Gaussian data with AR(1) noise along depth, coefficient 0.8, scored with independent noise of the same variance
    z = rs.normal(size=eta.shape)
    for t in range(1, T):
        z[..., t] = 0.8 * z[..., t - 1] + np.sqrt(1 - 0.64) * z[..., t]
    Yar = eta + np.sqrt(0.5) * z
    res = utils.posterior_checks(W, V, "gaussian", Yar, which=("lag1",), reps=n, seed=19, nu2=np.array([0.5]))
    print("AR(1) as white noise: overall lag1 p_ge", res["overall"]["lag1"]["p_ge"])
    assert res["overall"]["lag1"]["p_ge"] < 0.01


# ---------------------------------------------------------------- 6. the model methods
def test_model_method_gaussian(collected):
    model, Y, res = collected
    a = model.posterior_checks(seed=3, curves=[(2, 3)], reps=2)
    b = model.posterior_checks(results=res, seed=3, curves=[(2, 3)], reps=2)
    c = utils.posterior_checks(res["W"], res["V"], "gaussian", Y, nu2=res["nu2"], seed=3, curves=[(2, 3)], reps=2)
    assert a["which"] == ALL[:4] == c["which"]
    _assert_same_bits(a, b)
    _assert_same_bits(a, c)
    assert a["nsamples"] == res["W"].shape[0] and a["nsets"] == 2 * a["nsamples"] and a["ndraws"] == 2 * a["nsets"]
    np.testing.assert_array_equal(a["curves"]["index"], [[2, 3]])
    d0 = model._draws
    model.posterior_checks()                          # seed=None: the model's next device seed
    assert model._draws == d0 + 1
    model.posterior_checks(seed=4)
    assert model._draws == d0 + 1


def test_model_method_binomial_pair():
    N, M, T, K, S = 6, 4, 8, 2, 10
    rs = np.random.RandomState(12)
    tr = rs.randint(1, 20, size=(N, M, T)).astype(float)
    Yb = rs.binomial(tr.astype(int), 0.4).astype(float)
    np.random.seed(0)
    bm = BinomialBayesianTensorFiltering(N, M, T, nembeds=K, rng="device", device_seed=3)
    res = bm.run_gibbs((Yb, tr), nburn=2, nthin=1, nsamples=S, verbose=False)
    a = bm.posterior_checks(results=res, seed=6)      # the bound (Y, N) pair
    b = utils.posterior_checks(res["W"], res["V"], "binomial", (Yb, tr), seed=6)
    assert a["which"] == ALL
    _assert_same_bits(a, b)
    _assert_same_bits(a, bm.posterior_checks(results=res, data=(Yb, tr), seed=6))
    _assert_same_bits(a, bm.posterior_checks(results=res, data=Yb, trials=tr, seed=6))
    assert (a["nobs"] == T).all() and (a["chisq"]["defined"] == S).all()


def test_gamma_grid_is_refused():
    N, M, T, K = 4, 3, 5, 2
    np.random.seed(0)
    model = NonconjugateBayesianTensorFiltering(N, M, T, loglikelihood="poisson_log", nembeds=K)
    model._link = 5                                    # the gamma_grid link id (LINKS["gamma_grid"])
    assert NonconjugateBayesianTensorFiltering.LINKS["gamma_grid"] == 5
    with pytest.raises(NotImplementedError, match="gamma_grid"):
        model.posterior_checks(results=dict(W=np.zeros((2, N, K)), V=np.zeros((2, M, T, K))), data=np.ones((N, M, T)))
