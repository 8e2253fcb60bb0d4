"""Convergence diagnostics on the GPU (csrc/btf_diag.h via functionalmf_amd.diagnostics.convergence): per-cell outputs
against the numpy definition on explicitly formed Mu, nan cells, device-collected vs uploaded chains bit for bit,
determinism, an undisturbed chain, behaviour on sampled chains and the full C3 size."""
import time

import numpy as np
import pytest
from scipy.special import expit

from functionalmf_amd import diagnostics
from functionalmf_amd.factor import GaussianBayesianTensorFiltering

from test_host_diagnostics import spec

pytestmark = pytest.mark.gpu

FN = {None: lambda m: m, "identity": lambda m: m, "ilogit": expit, "square": np.square}


def _chains(C, S, N, M, T, K, seed, phi=0.4, dyadic=True):
    """C result dicts whose W and V follow AR(1) paths over the draws, chain c offset by a small amount.  Entries are
    multiples of 2^-8 below 8 in magnitude, so every w . v is exact in any summation order: the kernel's draws and the
    explicitly formed ones agree bit for bit (for even C*S the two middle draws are exactly equidistant from the median,
    and whether their folded values tie depends on the last bit)."""
    rs = np.random.RandomState(seed)
    out = []
    for c in range(C):
        W = np.zeros((S, N, K))
        V = np.zeros((S, M, T, K))
        W[0] = rs.normal(size=(N, K))
        V[0] = rs.normal(size=(M, T, K)) / np.sqrt(K)
        for s in range(1, S):
            W[s] = phi * W[s - 1] + np.sqrt(1 - phi * phi) * rs.normal(size=(N, K)) + 0.02 * c
            V[s] = phi * V[s - 1] + np.sqrt(1 - phi * phi) * rs.normal(size=(M, T, K)) / np.sqrt(K)
        if dyadic:
            W, V = np.clip(np.round(W * 256), -2047, 2047) / 256, np.clip(np.round(V * 256), -2047, 2047) / 256
        out.append({"W": W, "V": V})
    return out


def _nudged(x):
    """x and the copies of it with one of the two middle order statistics moved by one ulp (even size only): ilogit goes
    through exp, whose last bit may differ between numpy and the device, and that bit decides whether the two middle
    draws' distances to the median tie in the folded ranks."""
    out = [x]
    if x.size % 2 == 0:
        order = np.argsort(x, axis=None, kind="stable")
        for idx in order[x.size // 2 - 1:x.size // 2 + 1]:
            for to in (-np.inf, np.inf):
                y = x.copy()
                y.flat[idx] = np.nextafter(y.flat[idx], to)
                out.append(y)
    return out


def _close(got, want):
    return abs(got[0] / want[0] - 1) < 1e-10 and abs(got[1] / want[1] - 1) < 1e-8 and abs(got[2] / want[2] - 1) < 1e-8 \
        and abs(got[3] / want[3] - 1) < 1e-10


def _cells(chains, transform):
    """(N, M, T, C, S) draws of f(w . v), formed explicitly."""
    mu = np.stack([FN[transform](np.einsum("snk,smtk->snmt", ch["W"], ch["V"])) for ch in chains])   # (C,S,N,M,T)
    return np.moveaxis(mu, (0, 1), (3, 4))


@pytest.mark.parametrize("K", [1, 5, 10])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("S", [40, 41])
@pytest.mark.parametrize("transform", [None, "identity", "ilogit", "square"])
def test_cells_match_the_numpy_definition(K, C, S, transform):
    N, M, T = 3, 2, 4
    # (ilogit: continuous draws - on the coarse grid ilogit(u) + ilogit(-u) = 1 makes folded ties decided by exp's last bit)
    chains = _chains(C, S, N, M, T, K, seed=100 + 7 * K + C + S, dyadic=transform != "ilogit")
    res = diagnostics.convergence(chains, transform=transform)
    x = _cells(chains, transform)
    for i in range(N):
        for j in range(M):
            for t in range(T):
                got = [res[k][i, j, t] for k in ("rhat", "ess_bulk", "ess_tail", "mcse_mean")]
                cands = _nudged(x[i, j, t]) if transform == "ilogit" else [x[i, j, t]]
                wants = [spec(y) for y in cands]
                assert any(_close(got, w) for w in wants), (i, j, t, got, wants[0])
                assert abs(res["mean"][i, j, t] - x[i, j, t].mean()) <= 1e-12 * max(1.0, abs(x[i, j, t]).max()), (i, j, t)
    assert res["nchains"] == C and res["ndraws"] == S
    assert res["max_rhat"] == np.nanmax(res["rhat"])
    assert res["n_rhat_above"] == int(np.sum(res["rhat"] > 1.01))
    assert res["min_ess_bulk"] == np.nanmin(res["ess_bulk"]) and res["min_ess_tail"] == np.nanmin(res["ess_tail"])


def test_constant_and_non_finite_cells_give_nan():
    chains = _chains(2, 20, 3, 2, 4, 3, seed=5)
    for ch in chains:
        ch["V"][:, 1, 2, :] = 0.0                # column (1, 2): every draw is 0
    chains[1]["W"][7, 0, 1] = np.nan             # row 0: one non-finite draw
    chains[0]["W"][3, 2, 0] = np.inf             # row 2 (cells with v != 0 are inf or nan)
    for transform in (None, "ilogit"):
        res = diagnostics.convergence(chains, transform=transform)
        with np.errstate(invalid="ignore", over="ignore"):
            x = _cells(chains, transform)
        flat = x.reshape(3, 2, 4, -1)
        bad = ~np.all(np.isfinite(flat), axis=-1) | np.all(flat == flat[..., :1], axis=-1)
        assert bad[0].all() and bad[:, 1, 2].all() and not bad[1, 0].any()
        if transform is None:
            assert bad[2].all()                  # (ilogit(+-inf) is finite: only its nan cells are)
        for k in diagnostics.OUTPUTS:
            assert np.all(np.isnan(res[k][bad])), k
            assert not np.any(np.isnan(res[k][~bad])), k
        assert np.isfinite(res["max_rhat"]) and np.isfinite(res["min_ess_bulk"])


def _gauss_data(N=30, M=6, T=12, K=3, seed=0, noise=0.3):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    V = np.cumsum(rs.normal(0, 0.3, size=(M, T, K)), axis=1)
    return np.einsum("nk,mtk->nmt", W, V)[..., None] + rs.normal(0, noise, size=(N, M, T, 2))


def _model(seed, N=30, M=6, T=12, K=3):
    np.random.seed(seed)
    return GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_init=0.5, lam2_init=0.1, nu2_init=1,
                                           rng="device", device_seed=seed)


def _same(a, b):
    for k in diagnostics.OUTPUTS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["scalars"].keys() == b["scalars"].keys()
    for name, d in a["scalars"].items():
        assert all(np.array_equal(v, b["scalars"][name][k], equal_nan=True) for k, v in d.items()), name


def test_device_chains_equal_uploaded_bit_for_bit():
    Y = _gauss_data()
    models = [_model(3), _model(4)]
    results = [m.run_gibbs(Y, nburn=20, nsamples=30, verbose=False) for m in models]
    dev = diagnostics.convergence(models)
    up = diagnostics.convergence(results)
    _same(dev, up)
    _same(diagnostics.convergence([models[0], results[1]]), dev)
    _same(diagnostics.convergence([results[0], models[1]], transform=None), dev)
    _same(models[0].convergence_diagnostics(models[1]), dev)
    _same(diagnostics.convergence(models), dev)               # two calls, same bits
    for t in ("ilogit", "square"):
        _same(diagnostics.convergence(models, transform=t), diagnostics.convergence(results, transform=t))
    assert set(dev["scalars"]) == {"nu2", "sigma2", "lam2"}
    assert np.isfinite(dev["scalars"]["nu2"]["rhat"])
    single = diagnostics.convergence(models[0])               # one chain: its two halves
    assert single["nchains"] == 1 and single["rhat"].shape == (30, 6, 12)


def test_chain_is_undisturbed():
    Y = _gauss_data(seed=1)
    a, b = _model(11), _model(11)
    for m in (a, b):
        np.random.seed(12)
        m.run_gibbs(Y, nburn=4, nsamples=6, verbose=False)
    a.convergence_diagnostics()
    diagnostics.convergence([a, b], transform="square")
    outs = []
    for m in (a, b):
        np.random.seed(14)
        outs.append(m.run_gibbs(Y, nburn=3, nsamples=5, verbose=False))
    for k in ("W", "V", "nu2", "sigma2", "lam2"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(a.W, b.W) and np.array_equal(a.V, b.V)


def test_well_specified_chains_agree_and_a_far_start_is_flagged():
    Y = _gauss_data(seed=2)
    models = [_model(20 + c) for c in range(4)]
    for m in models:
        m.run_gibbs(Y, nburn=5000, nsamples=300, verbose=False)       # (500 sweeps are not enough here: R-hat 2.9)
    res = diagnostics.convergence(models)
    print("well specified: max_rhat %.4f, median %.4f, n_rhat_above %d, min_ess_bulk %.1f"
          % (res["max_rhat"], np.nanmedian(res["rhat"]), res["n_rhat_above"], res["min_ess_bulk"]))
    assert res["max_rhat"] < 1.2
    assert np.nanmedian(res["rhat"]) < 1.01
    assert res["min_ess_bulk"] > 50
    # three of them go on for 40 draws; a fourth starts far off with no burn-in
    for m in models[:3]:
        m.run_gibbs(Y, nburn=0, nsamples=40, verbose=False)
    far = _model(30)
    far.W = np.full_like(far.W, 30.0)
    far.V = np.full_like(far.V, 30.0)
    far.run_gibbs(Y, nburn=0, nsamples=40, verbose=False)
    good = diagnostics.convergence(models[:3])
    flagged = diagnostics.convergence(models[:3] + [far])
    print("far start: max_rhat %.4f, n_rhat_above %d (without it: %.4f, %d)"
          % (flagged["max_rhat"], flagged["n_rhat_above"], good["max_rhat"], good["n_rhat_above"]))
    assert flagged["max_rhat"] > 1.1 and flagged["n_rhat_above"] > good["n_rhat_above"]


def test_full_size_c3_four_chains_of_1000():
    """(512, 256, 64), K = 5, 4 device-collected chains of 1000 draws: 8.4 M cells of 4000 draws in well under 60 s."""
    N, M, T, K = 512, 256, 64, 5
    rs = np.random.RandomState(0)
    W = rs.normal(size=(N, K))
    V = 0.3 * np.cumsum(rs.normal(size=(M, T, K)), axis=1) / np.sqrt(T)
    Y = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.3, size=(N, M, T))
    models = []
    for c in range(4):
        m = _model(40 + c, N, M, T, K)
        m.run_gibbs(Y, nburn=50, nsamples=1000, verbose=False)
        models.append(m)
    diagnostics.convergence(models, scalars=())            # warm-up: code object load, first allocations
    t0 = time.perf_counter()
    res = diagnostics.convergence(models, scalars=())
    dt = time.perf_counter() - t0
    print("C3 4 x 1000 convergence: %.3f s, max_rhat %.4f, min_ess_bulk %.1f" % (dt, res["max_rhat"], res["min_ess_bulk"]))
    assert dt < 60.0
    assert res["rhat"].shape == (N, M, T) and np.isfinite(res["max_rhat"])
