"""WAIC, DIC and PSIS-LOO of the conjugate Negative-Binomial model with its sampled rate on the GPU (csrc/btf_nb_criteria.h
via negbin_criteria / negbin_loo / negbin_logprob) against the written definition criteria.negbin_loglik: parity at the
smallest shapes where the kernels can go wrong, the sampler's own btf_nb_loglik, the PSIS stage, bit-identities, an
undisturbed chain, select_hyperparams_DIC and the refusals.

Geometry the cases are derived from (csrc/btf_criteria.h, btf_nb_criteria.h): one workgroup per (column, 64 rows), one lane
per row (N = 1, 63, 65: one lane, a short tile, a second tile of one lane); 4 waves over depth chunks of 16 cells
(T = 16, 17, 33: one full chunk, a second of one cell, a third) and, in the constant kernel, over chunks of 16 (t,r)
observations (T nreps = 99: seven chunks, three waves adding a second); samples in blocks of 32 (S = 1, 2, 32, 33; the
constant kernel runs S + 1 rate tensors: 33 and 34 cross its block edge).  The context refuses ndepth < 2 (btf_create), so
the smallest depth here is T = 2, not 1.

Tolerances: those of tests/test_gpu_gg_criteria.py - relative 1e-10 on waic, dic, lppd and the per-curve lppd, 1e-9 on
p_waic, the pointwise matrix rtol = atol = 1e-10.  Every figure is printed before it is asserted (NB-PARITY lines).
Measured on an MI355X: pointwise matrix, plug-in and per-sample totals at most 1.2e-4 of that tolerance (counts up to 5003,
rates up to 1e3 included, so no bound of its own was needed); dic, lppd to 1.6e-15 relative, waic to 3.3e-14, p_waic to 4.1e-14; against
btf_nb_loglik 5.4e-16 (scalar rate) and 4.9e-13 (one rate per row) relative, bound 1e-9; the PSIS stage inside the bounds
of tests/test_gpu_loo.py (largest: log weights 3.1e-15)."""
import functools

import numpy as np
import pytest

from functionalmf_amd import _native, criteria, utils
from functionalmf_amd.factor import NegativeBinomialBayesianTensorFiltering

pytestmark = pytest.mark.gpu

COUNTS = (0.0, 32.0, 33.0, 1023.0, 1024.0, 5003.0)      # the edges of the product form (32 | 33) and of the sampler's table
RATES = (1.0001, 2.5, 40.0, 1e3)                        # 40 and 1e3: above the Stirling threshold, no shift

# N, M, T, nreps, K, S, rate full along (rows, columns, depth)
SHAPES = [
    (1, 2, 2, 1, 1, 1, (0, 0, 0)),
    (63, 2, 16, 3, 5, 2, (1, 0, 0)),
    (65, 3, 17, 1, 10, 32, (0, 1, 0)),
    (65, 2, 33, 3, 5, 33, (0, 0, 1)),
    (63, 3, 17, 3, 1, 33, (1, 1, 0)),
    (1, 3, 33, 3, 10, 32, (1, 0, 1)),
    (65, 2, 16, 1, 5, 2, (0, 1, 1)),
    (63, 2, 33, 3, 10, 33, (1, 1, 1)),
]


def _inputs(N, M, T, nreps, K, S, layout, seed, counts=COUNTS, fractional=True):
    """Counts with the edge values of COUNTS, a non-integer count, NaN replicates, a cell without observations inside an
    observed curve and (M > 1) a curve without any; W, V with |w.v| well under 10; every element of the rate tensor one of
    RATES (a scalar rate: RATES[seed % 4]), jittered by 5 % between samples (sample 0 keeps the exact values)."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K)) * (0.8 / np.sqrt(K))
    V = rs.normal(size=(M, T, K))
    Y = rs.poisson(5.0, size=(N, M, T, nreps)).astype(float)
    flat = Y.reshape(-1)
    pos = rs.choice(flat.size, size=min(flat.size, len(counts) + 1), replace=False)
    for p, c in zip(pos, counts + ((7.25,) if fractional else ())):
        flat[p] = c
    if nreps > 1:
        Y[rs.rand(N, M, T, nreps) < 0.08] = np.nan
    Y[N // 2, 0, T - 1] = np.nan
    if M > 1:
        Y[N - 1, M - 1] = np.nan
    Ws = W[None] + 0.1 * rs.normal(size=(S, N, K)) / np.sqrt(K)
    Vs = V[None] + 0.1 * rs.normal(size=(S, M, T, K))
    tail = tuple(full if on else 1 for full, on in zip((N, M, T), layout))
    base = rs.choice(RATES, size=tail) if np.prod(tail) > 1 else np.full(tail, RATES[seed % len(RATES)])
    Rs = base[None] * np.exp(0.05 * rs.normal(size=(S,) + tail) * (np.arange(S) > 0).reshape(S, 1, 1, 1))
    assert np.abs(np.einsum("snk,smtk->snmt", Ws, Vs)).max() < 10.0
    return W, V, Y, Ws, Vs, Rs


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(inputs, host definition) of SHAPES[idx], computed once and shared; nothing writes to it."""
    N, M, T, nreps, K, S, layout = SHAPES[idx]
    W, V, Y, Ws, Vs, Rs = _inputs(N, M, T, nreps, K, S, layout, seed=70 + idx)
    L, L_at_mean, obs = criteria.negbin_loglik(Y, Ws, Vs, Rs)
    for a in (W, V, Y, Ws, Vs, Rs, L, L_at_mean, obs):
        a.setflags(write=False)
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(L_at_mean)) and obs.sum() == N * M - (1 if M > 1 else 0)
    return dict(W=W, V=V, Y=Y, Ws=Ws, Vs=Vs, Rs=Rs, L=L, L_at_mean=L_at_mean, obs=obs)


def _model(N, M, T, K, layout, W, V, R, seed=1, **kw):
    np.random.seed(seed)
    rdims = tuple(d for d in range(3) if not layout[d])
    return NegativeBinomialBayesianTensorFiltering(N, M, T, nembeds=K, rdims=rdims, W_init=np.array(W), V_init=np.array(V),
                                                   R_init=np.array(R), **kw)


def _parity(res, L, L_at_mean, obs, label):
    host = criteria.from_loglik(L, obs, L_at_mean)
    scale = lambda got, want: float(np.max(np.abs(got - want) / (1e-10 + 1e-10 * np.abs(want)))) if want.size else 0.0
    print("NB-PARITY", label, "share of the tolerance: pointwise %.3g ll_at_mean %.3g per_sample %.3g" % (
        scale(res["loglik"], L), scale(res["curves"]["ll_at_mean"], L_at_mean), scale(res["loglik_per_sample"], host["loglik_per_sample"])))
    for k in ("waic", "dic", "lppd", "p_waic"):
        print("NB-PARITY", label, k, res[k], host[k], abs(res[k] - host[k]) / max(abs(host[k]), 1e-300))
    np.testing.assert_allclose(res["loglik"], L, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["curves"]["ll_at_mean"], L_at_mean, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["loglik_per_sample"], host["loglik_per_sample"], rtol=1e-10, atol=1e-10)
    assert np.all(res["loglik"][:, ~obs] == 0.0) and np.all(res["curves"]["ll_at_mean"][~obs] == 0.0)
    assert res["n_curves"] == host["n_curves"] and res["nsamples"] == L.shape[0]
    for k, rtol in (("waic", 1e-10), ("dic", 1e-10), ("lppd", 1e-10), ("p_waic", 1e-9)):
        assert abs(res[k] - host[k]) <= rtol * abs(host[k]), (k, res[k], host[k])
    np.testing.assert_allclose(res["curves"]["lppd"], host["curves"]["lppd"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["curves"]["p_waic"], host["curves"]["p_waic"], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_parity_with_the_host_definition(idx):
    c = _case(idx)
    N, M, T, nreps, K, S, layout = SHAPES[idx]
    model = _model(N, M, T, K, layout, c["W"], c["V"], c["Rs"][0])
    model.set_data(np.array(c["Y"]))
    results = {"W": c["Ws"], "V": c["Vs"], "R": c["Rs"]}
    res = model.negbin_criteria(results, pointwise=True)
    label = "shape %r" % (SHAPES[idx],)
    _parity(res, c["L"], c["L_at_mean"], c["obs"], label)
    s = S - 1
    got = model.negbin_logprob(c["Y"], reduce="curve", W=c["Ws"][s], V=c["Vs"][s], R=c["Rs"][s])
    np.testing.assert_allclose(got, c["L"][s], rtol=1e-10, atol=1e-10)
    tot = model.negbin_logprob(c["Y"], W=c["Ws"][s], V=c["Vs"][s], R=c["Rs"][s])
    assert tot == res["loglik_per_sample"][s]
    # the current state and rate: what the model was built with
    cur = model.negbin_logprob(c["Y"], reduce="curve")
    want = criteria.negbin_loglik(c["Y"], c["W"][None], c["V"][None], c["Rs"][:1])[0][0]
    np.testing.assert_allclose(cur, want, rtol=1e-10, atol=1e-10)
    # without "R" in the results the current rate stands for every sample
    nor = model.negbin_criteria({"W": c["Ws"], "V": c["Vs"]}, pointwise=True)
    Lr = criteria.negbin_loglik(c["Y"], c["Ws"], c["Vs"], np.broadcast_to(c["Rs"][0], c["Rs"].shape))[0]
    np.testing.assert_allclose(nor["loglik"], Lr, rtol=1e-10, atol=1e-10)
    cmp = criteria.compare(res, res)
    assert cmp["elpd_diff"] == 0.0 and cmp["n_curves"] == res["n_curves"]


@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds(nembeds):
    """nb_crit_kernel<K, ROWS> for every K, alternating the per-lane and the wave-uniform rate, each K on inputs of its own."""
    layout = (nembeds % 2, 1, (nembeds // 2) % 2)
    N, M, T, nreps, S = 20, 3, 9, 2, 5
    W, V, Y, Ws, Vs, Rs = _inputs(N, M, T, nreps, nembeds, S, layout, seed=100 + nembeds)
    L, L_at_mean, obs = criteria.negbin_loglik(Y, Ws, Vs, Rs)
    model = _model(N, M, T, nembeds, layout, W, V, Rs[0])
    res = model.negbin_criteria({"W": Ws, "V": Vs, "R": Rs}, data=Y, pointwise=True)
    _parity(res, L, L_at_mean, obs, "nembeds %d" % nembeds)


@pytest.mark.parametrize("layout", [(0, 0, 0), (1, 0, 0)])
def test_rate_difference_equals_the_samplers_own_kernel(layout):
    """negbin_logprob(R=C) - negbin_logprob(R=R) per curve, summed over the axes the rate is shared across, is what
    btf_nb_loglik (the likelihood ratio of the rate's MH step) returns for the same W, V: relative 1e-9."""
    N, M, T, nreps, K = 40, 3, 17, 3, 4
    W, V, Y, _, _, Rs = _inputs(N, M, T, nreps, K, 2, layout, seed=130 + layout[0])
    R, C = Rs[0], Rs[0] * np.exp(0.3 * np.random.RandomState(5).normal(size=Rs[0].shape))
    model = _model(N, M, T, K, layout, W, V, R)
    model._bind_data(Y)
    model._push_state()
    ll = np.zeros(R.shape)
    model._ctx.call("btf_nb_loglik", _native.dptr(_native.as_f64(R)), _native.dptr(_native.as_f64(C)),
                    model._shared_flags().ctypes.data_as(_native._c_ip), _native.dptr(ll))
    diff = model.negbin_logprob(Y, reduce="curve", R=C) - model.negbin_logprob(Y, reduce="curve", R=R)
    got = diff.sum(axis=1) if layout[0] else diff.sum()
    err = np.max(np.abs(got - ll.reshape(np.shape(got))) / np.abs(ll.reshape(np.shape(got))))
    print("NB-PARITY btf_nb_loglik layout", layout, "max relative error %.3g" % err)
    assert err <= 1e-9


def _loo_inputs(S, layout, seed):
    N, M, T, nreps, K = 33, 3, 9, 2, 3
    return (N, M, T, K), _inputs(N, M, T, nreps, K, S, layout, seed, counts=(0.0, 33.0, 1024.0))


@pytest.mark.parametrize("S,r_eff,layout", [(33, None, (0, 0, 0)), (33, 0.5, (1, 0, 1)), (200, None, (1, 1, 0)), (200, 0.5, (0, 1, 1))])
def test_loo_against_the_host_psis_on_the_devices_own_matrix(S, r_eff, layout):
    """Only the unchanged PSIS stage differs: criteria.psis_loo_host is fed the device's pointwise matrix."""
    from test_gpu_loo import BOUND, _check, _rel
    (N, M, T, K), (W, V, Y, Ws, Vs, Rs) = _loo_inputs(S, layout, seed=150 + S + layout[0])
    model = _model(N, M, T, K, layout, W, V, Rs[0])
    model.set_data(Y)
    results = {"W": Ws, "V": Vs, "R": Rs}
    ic = model.negbin_criteria(results, pointwise=True)
    res = model.negbin_loo(results, r_eff=r_eff, mean=True, log_weights=True)
    obs = np.any(~np.isnan(Y), axis=(2, 3))
    host = criteria.psis_loo_host(ic["loglik"], obs, r_eff=1.0 if r_eff is None else r_eff, log_weights=True)
    kk = res["curves"]["pareto_k"]
    assert np.all(np.isnan(kk[~obs])) and np.all(res["curves"]["elpd_loo"][~obs] == 0)
    figs = _check(res, host, "", "negbin S=%d r_eff=%s" % (S, r_eff))
    Mu = np.einsum("snk,smtk->snmt", Ws, Vs)
    figs["mean"] = _rel(res["mean"], np.einsum("snm,snmt->nmt", np.exp(host["log_weights"]), Mu))
    print("LOO-PARITY negbin", S, r_eff, "mean=%.3g" % figs["mean"])
    assert figs["mean"] <= BOUND["mean"], figs
    assert np.array_equal(res["curves"]["lppd"], ic["curves"]["lppd"])
    assert criteria.compare(res, res)["n_curves"] == res["n_curves"] == int(obs.sum())


def _same_ic(a, b):
    for k in ("waic", "elpd_waic", "p_waic", "lppd", "waic_se", "dic", "p_dic", "mean_deviance", "deviance_at_mean", "n_curves"):
        assert a[k] == b[k], k
    assert np.array_equal(a["loglik_per_sample"], b["loglik_per_sample"])
    for k in a["curves"]:
        assert np.array_equal(a["curves"][k], b["curves"][k]), k
    if "loglik" in a:
        assert np.array_equal(a["loglik"], b["loglik"])


def test_two_calls_the_model_free_form_and_the_held_out_slot():
    from test_gpu_loo import _same
    layout = (1, 0, 1)
    (N, M, T, K), (W, V, Y, Ws, Vs, Rs) = _loo_inputs(40, layout, seed=170)
    model = _model(N, M, T, K, layout, W, V, Rs[0])
    model.set_data(Y)
    results = {"W": Ws, "V": Vs, "R": Rs}
    a = model.negbin_criteria(results, pointwise=True)
    la = model.negbin_loo(results, mean=True, log_weights=True)
    b = model.negbin_criteria(results, pointwise=True)
    lb = model.negbin_loo(results, mean=True, log_weights=True)
    _same_ic(a, b)
    _same(la, lb)
    assert np.array_equal(la["curves"]["lppd"], a["curves"]["lppd"])
    _same_ic(a, utils.negbin_criteria(Ws, Vs, Rs, Y, pointwise=True))
    _same(la, utils.negbin_loo(Ws, Vs, Rs, Y, mean=True, log_weights=True))
    # held-out counts through data=: another tensor, its own slot, against the definition; slot 0 is untouched
    Yh = np.full_like(Y, np.nan)
    Yh[::3, ::2] = Y[::3, ::2]
    h = model.negbin_criteria(results, data=Yh, pointwise=True)
    Lh, _, obs_h = criteria.negbin_loglik(Yh, Ws, Vs, Rs)
    np.testing.assert_allclose(h["loglik"], Lh, rtol=1e-10, atol=1e-10)
    assert h["n_curves"] == int(obs_h.sum()) < a["n_curves"]
    _same_ic(a, model.negbin_criteria(results, pointwise=True))
    _same_ic(h, model.negbin_criteria(results, data=Yh, pointwise=True))


def _chain_problem(seed):
    rs = np.random.RandomState(seed)
    N, M, T, nreps, K = 16, 5, 8, 2, 2
    P = 1 / (1 + np.exp(-np.einsum("nk,mtk->nmt", 0.7 * rs.normal(size=(N, K)), 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1))))
    Y = rs.negative_binomial(4.0, 1 - P[..., None].repeat(nreps, -1)).astype(float)
    Y[:2, :2] = np.nan
    return (N, M, T, K), Y


def _chain_model(dims, seed, **kw):
    np.random.seed(seed)
    return NegativeBinomialBayesianTensorFiltering(*dims[:3], nembeds=dims[3], tf_order=1, sigma2_init=0.5, lam2_init=0.1, nmetropolis=3,
                                                   rng="device", device_seed=7, **kw)


def test_chain_is_undisturbed():
    dims, Y = _chain_problem(9)
    a, b = (_chain_model(dims, seed=11, rdims=(1, 2)) for _ in range(2))
    np.random.seed(13)
    res = a.run_gibbs(Y, nburn=2, nsamples=6, verbose=False)
    np.random.seed(13)
    b.run_gibbs(Y, nburn=2, nsamples=6, verbose=False)
    assert res["R"].shape == (6, dims[0], 1, 1)
    ic = a.negbin_criteria(res, pointwise=True)
    a.negbin_loo(res, mean=True)
    a.negbin_logprob(Y)
    L = criteria.negbin_loglik(Y, res["W"], res["V"], res["R"])[0]
    np.testing.assert_allclose(ic["loglik"], L, rtol=1e-10, atol=1e-10)
    for m in (a, b):
        np.random.seed(14)
        m.run_gibbs(Y, nburn=2, nsamples=2, verbose=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V) and np.array_equal(a.Tau2, b.Tau2) and np.array_equal(a.R, b.R)
    for k in ("sigma2", "lam2"):
        assert getattr(a, k) == getattr(b, k), k


def test_select_hyperparams_DIC_scores_through_negbin_criteria():
    dims, Y = _chain_problem(12)
    m = _chain_model(dims, seed=4)
    out = m.select_hyperparams_DIC(Y, verbose=False, lam2=[0.1, 0.01], nburn=3, nsamples=6)
    assert out["scores"].shape == (2,) and np.all(np.isfinite(out["scores"]))
    best = int(np.argmin(out["scores"]))
    assert out["best"]["lam2"] == [0.1, 0.01][best]
    assert out["scores"][best] == m.negbin_criteria(out["fit"])["dic"]


def test_refusals():
    N, M, T, nreps, K, S = 6, 3, 4, 2, 2, 3
    W, V, Y, Ws, Vs, Rs = _inputs(N, M, T, nreps, K, S, (0, 0, 0), seed=190)
    S1, cnt, c0, Y4, obs = criteria.negbin_statistics(Y, (N, M, T))
    zero = np.zeros((N, M))
    curve, tot = np.zeros((5, N, M)), np.zeros(S)
    dp = _native.dptr
    rates, flags = criteria.negbin_rates(Rs, S, (N, M, T))
    ctx = _native.Context(N, M, T, K, 0)
    try:
        def nb_eval(r=rates):
            ctx.call("btf_nb_crit_eval", 1, S, dp(Ws), dp(Vs), dp(r), flags, 0, dp(curve), dp(tot), None)

        with pytest.raises(_native.BTFError, match="no statistics") as err:          # counts before statistics
            ctx.call("btf_crit_set_counts", 1, dp(Y4), nreps)
        assert err.value.code == _native.BTF_ESTATE
        ctx.call("btf_crit_set_data", 1, dp(S1), dp(cnt), dp(c0), dp(zero))
        with pytest.raises(_native.BTFError, match="btf_crit_set_counts") as err:    # statistics, no counts
            nb_eval()
        assert err.value.code == _native.BTF_ESTATE
        ctx.call("btf_crit_set_counts", 1, dp(Y4), nreps)
        nb_eval()
        assert np.all(np.isfinite(tot)) and np.any(tot != 0)
        bad = rates.copy()
        bad[1, 0] = 0.0
        with pytest.raises(_native.BTFError, match="rate") as err:
            nb_eval(bad)
        assert err.value.code == _native.BTF_EINVAL
        out = np.zeros((4, N, M))
        with pytest.raises(_native.BTFError, match="rate") as err:
            ctx.call("btf_nb_crit_loo", 1, S, dp(Ws), dp(Vs), dp(bad), flags, None, 0, dp(out), None, None)
        assert err.value.code == _native.BTF_EINVAL
        ctx.call("btf_crit_set_data", 1, dp(S1), dp(cnt), dp(c0), dp(zero))          # drops the counts
        with pytest.raises(_native.BTFError) as err:
            nb_eval()
        assert err.value.code == _native.BTF_ESTATE
        ctx.call("btf_crit_set_counts", 1, dp(Y4), nreps)
        ctx.call("btf_crit_set_counts", 1, None, 0)                                  # NULL frees them
        with pytest.raises(_native.BTFError) as err:
            nb_eval()
        assert err.value.code == _native.BTF_ESTATE
        with pytest.raises(_native.BTFError) as err:                                 # no seventh family of btf_crit_eval
            ctx.call("btf_crit_eval", 1, 6, 0.0, S, dp(Ws), dp(Vs), None, 0, dp(curve), dp(tot), None)
        assert err.value.code == _native.BTF_EINVAL
    finally:
        ctx.close()
    model = _model(N, M, T, K, (0, 0, 0), W, V, Rs[0])
    results = {"W": Ws, "V": Vs, "R": Rs}
    with pytest.raises(ValueError, match="leading dimension"):
        model.negbin_criteria(dict(results, R=Rs[:2]), data=Y)
    with pytest.raises(ValueError, match="rate"):
        model.negbin_criteria(dict(results, R=np.zeros_like(Rs)), data=Y)
    with pytest.raises(RuntimeError, match="no samples collected"):
        model.negbin_criteria(None, data=Y)
    Yb = Y.copy()
    Yb[0, 0, 0, 0] = -1.0
    with pytest.raises(ValueError, match=">= 0"):
        model.negbin_criteria(results, data=Yb)
    # the pinned refusals stay
    for call in (lambda: model.information_criteria(results, data=Y), lambda: model.loo(results, data=Y), lambda: model.logprob(Y)):
        with pytest.raises(NotImplementedError):
            call()
