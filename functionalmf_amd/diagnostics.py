"""Convergence diagnostics: split R-hat, bulk and tail ESS and the MCSE of the mean (Vehtari, Gelman, Simpson, Carpenter
and Buerkner 2021, "Rank-normalization, folding, and localization"; the algorithm ArviZ uses).

convergence() checks the cells of Mu = W V', one series per (i, j, t): W and V are identified only up to rotation and sign
between draws, so R-hat of a single factor entry means nothing.  The per-cell work is the HIP kernel of csrc/btf_diag.h
(btf_diag_eval); the (C, S, N, M, T) tensor of draws is never formed.  chain_diagnostics() is the same definition in
numpy for one (C, S) array: it gives the diagnostics of the scalar parameters and states what the kernel computes.

Definition, for x of C chains by S draws (one chain is allowed: its R-hat comes from its two halves):
  split(x)   the 2C half-chains of S // 2 draws; for odd S the middle draw of each chain is dropped
  zscale(x)  average ranks over all entries, then Phi^-1((r - 3/8) / (size + 1/4))
  rhat       max of the split R-hat of zscale(split(x)) and of zscale(split(|x - median(x)|)), median over all C*S draws
  ess_bulk   the ESS of zscale(split(x)), by Geyer's initial monotone positive sequence over direct autocovariances
  ess_tail   min of the ESS of split(x <= q05) and split(x <= q95), numpy 'linear' quantiles of all C*S draws
  mcse_mean  std(x, ddof=1) / sqrt(ESS of split(x))
Edge rules: at least 4 draws per chain; if all of a series' draws are equal, or one of them is not finite, every output of
that series is nan.
"""
import ctypes as C

import numpy as np

from ._analysis import check_states, transform_code

MIN_DRAWS = 4                 # draws per chain
MAX_CHAINS = 64               # DIAG_MAX_CHAINS of csrc/btf_diag.h
MAX_POOLED_DRAWS = 4096       # DIAG_MAX_DRAWS: chains x draws per cell (the kernel keeps a cell's draws in LDS)
RHAT_THRESHOLD = 1.01
OUTPUTS = ("rhat", "ess_bulk", "ess_tail", "mcse_mean", "mean")
_SCALAR_COLUMNS = {"nu2": 0, "sigma2": 1, "lam2": 2}     # of the collected scalars (btf_collect_end)


# ---------------------------------------------------------------------------- the definition in numpy
def _split(x):
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, x.shape[1] - h:]], axis=0)


def _zscale(x):
    from scipy.special import ndtri
    from scipy.stats import rankdata
    r = rankdata(x, method="average").reshape(x.shape)
    return ndtri((r - 0.375) / (x.size + 0.25))


def _rhat(x):
    n = x.shape[1]
    B = n * np.var(x.mean(axis=1), ddof=1)
    W = np.mean(np.var(x, axis=1, ddof=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt((B / W + n - 1) / n))


def _autocov(x):
    """(C, n) -> (C, n): acov[c, t] = sum_k xc[c, k] xc[c, k + t] / n, direct sums (np.correlate)."""
    n = x.shape[1]
    xc = x - x.mean(axis=1, keepdims=True)
    return np.stack([np.correlate(row, row, mode="full")[n - 1:] for row in xc]) / n


def _ess(x):
    Cc, n = x.shape
    acov = _autocov(x).mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_var = acov[0] * n / (n - 1)
        var_plus = mean_var * (n - 1) / n + (np.var(x.mean(axis=1), ddof=1) if Cc > 1 else 0.0)
        rho_all = 1.0 - (mean_var - acov) / var_plus          # every lag at once; Geyer reads what it needs
    rho = np.zeros(n)
    rho[0] = even = 1.0
    rho[1] = odd = rho_all[1]
    t = 1
    while t < n - 3 and even + odd > 0:
        even, odd = rho_all[t + 1], rho_all[t + 2]
        if even + odd >= 0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2
        t += 2
    tau = -1 + 2 * rho[:max_t + 1].sum() + rho[max_t + 1:max_t + 2].sum()
    tau = max(tau, 1 / np.log10(Cc * n))
    return Cc * n / tau


def chain_diagnostics(x):
    """Split R-hat, bulk ESS, tail ESS and MCSE of the mean of one (C, S) array of draws (C chains, S >= 4 draws each).
    Returns a dict {rhat, ess_bulk, ess_tail, mcse_mean} of floats; all nan if the draws are all equal or one is not
    finite.  A 1-d array is one chain."""
    x = np.asarray(x, dtype=float)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2:
        raise ValueError("chain_diagnostics: x must be (chains, draws)")
    if x.shape[1] < MIN_DRAWS:
        raise ValueError("chain_diagnostics: at least %d draws per chain" % MIN_DRAWS)
    if not np.all(np.isfinite(x)) or np.all(x == x.flat[0]):
        return {k: float("nan") for k in OUTPUTS[:4]}
    s = _split(x)
    folded = np.abs(x - np.median(x))
    rhat = max(_rhat(_zscale(s)), _rhat(_zscale(_split(folded))))
    ess_bulk = _ess(_zscale(s))
    q05, q95 = np.quantile(x, [0.05, 0.95])
    ess_tail = min(_ess(_split((x <= q05).astype(float))), _ess(_split((x <= q95).astype(float))))
    mcse = np.std(x, ddof=1) / np.sqrt(_ess(s))
    return {"rhat": float(rhat), "ess_bulk": float(ess_bulk), "ess_tail": float(ess_tail), "mcse_mean": float(mcse)}


# ---------------------------------------------------------------------------- per-cell diagnostics on the GPU
def _is_model(obj):
    from .factor import BayesianTensorFiltering
    return isinstance(obj, BayesianTensorFiltering)


def _describe(chain):
    """(kind, S, (N, M, T, K), device, payload) of one chain; model refusals here, before any device call."""
    if isinstance(chain, dict):
        if "W" not in chain or "V" not in chain:
            raise ValueError("a result dict needs W (S,N,K) and V (S,M,T,K)")
        W, V = check_states(chain["W"], chain["V"], what="a result dict: ")
        return "dict", W.shape[0], (W.shape[1], V.shape[1], V.shape[2], W.shape[2]), None, (W, V)
    if _is_model(chain):
        chain._unsharded("convergence diagnostics")
        n = chain._samples(None)[0]
        return "model", n, (chain.nrows, chain.ncols, chain.ndepth, chain.nembeds), chain.device, chain
    raise ValueError("a chain is a run_gibbs result dict or a model whose last run_gibbs collected on the device")


def _scalar_table(chain, S):
    """{name: one value per draw} of a chain: a result dict is its own table; a model's collected scalars come in one
    download."""
    if isinstance(chain, dict):
        return chain
    from . import _native
    sc = np.zeros((S, 8))
    chain._ctx.call("btf_collect_end", int(S), None, None, None, _native.dptr(sc))
    return {name: sc[:, col].copy() for name, col in _SCALAR_COLUMNS.items()}


def _scalar_series(table, S, name):
    if name not in table:
        return None
    v = np.asarray(table[name], dtype=float)
    return v.reshape(S) if v.size == S else None


def convergence(chains, transform=None, scalars=("nu2", "sigma2", "lam2")):
    """Convergence diagnostics of every cell of f(W V') over one or more chains (csrc/btf_diag.h).

    chains: one chain or a list of them.  A chain is a run_gibbs result dict (its W (S,N,K) and V (S,M,T,K) are uploaded)
        or a model whose last run_gibbs collected its samples on the device (rng="device"): those are read where they lie,
        no copy through the host.  Dicts and models may be mixed; all need the same S and shapes.
    transform: None / "identity", "ilogit" or "square" (as posterior_summary): the draws are f(w_i . v_jt).
    scalars: the scalar keys to diagnose as well, for each one every chain provides (a dict's key with S values; a
        model's collected nu2, sigma2 and lam2); on the host by chain_diagnostics.

    Per cell (i, j, t), over the pooled chains (definition: functionalmf_amd.diagnostics; one chain: its two halves):
    split R-hat (rank-normalised, the max of bulk and folded), bulk ESS, tail ESS (the min over the 5 % and 95 % quantile
    indicators), the MCSE of the mean, and the mean.  At least 4 draws per chain, at most 64 chains and at most 4096 pooled
    draws (chains x draws); 1 <= nembeds <= 10.  A cell whose draws are all equal, or hold a non-finite value, gets nan in
    every output.  Every sum of the kernel has a fixed order: two calls agree bit for bit.

    Returns {rhat, ess_bulk, ess_tail, mcse_mean, mean: (N,M,T) arrays; max_rhat; n_rhat_above: cells with R-hat > 1.01;
    min_ess_bulk, min_ess_tail (nan-aware); nchains; ndraws: S per chain; scalars: {name: {rhat, ess_bulk, ess_tail,
    mcse_mean}}}.  Raises ValueError (bad transform, shapes or sizes, chains on different devices) before any device call,
    RuntimeError for a model without device-collected samples, NotImplementedError for a sharded model."""
    tcode = transform_code(transform)
    if isinstance(chains, dict) or _is_model(chains):
        chains = [chains]
    chains = list(chains)
    if not chains:
        raise ValueError("no chains")
    desc = [_describe(c) for c in chains]
    S, shape = desc[0][1], desc[0][2]
    for d in desc[1:]:
        if d[1] != S:
            raise ValueError("chains of different lengths: %d and %d draws" % (S, d[1]))
        if d[2] != shape:
            raise ValueError("chains of different shapes: %r and %r" % (shape, d[2]))
    N, M, T, K = shape
    nch = len(desc)
    if S < MIN_DRAWS:
        raise ValueError("at least %d draws per chain (got %d)" % (MIN_DRAWS, S))
    if not 1 <= K <= 10:
        raise ValueError("nembeds must lie in 1..10 (got %d)" % K)
    if nch > MAX_CHAINS:
        raise ValueError("at most %d chains (got %d)" % (MAX_CHAINS, nch))
    if nch * S > MAX_POOLED_DRAWS:
        raise ValueError("at most %d pooled draws per cell (chains x draws; got %d x %d)" % (MAX_POOLED_DRAWS, nch, S))
    devices = {d[3] for d in desc if d[3] is not None}
    if len(devices) > 1:
        raise ValueError("models on different devices: %r" % sorted(devices))
    device = devices.pop() if devices else 0

    from . import _native
    lib = _native.load()
    wp, vp = (_native._c_dp * nch)(), (_native._c_dp * nch)()             # (desc keeps the uploaded arrays alive)
    ctxs = (C.c_void_p * nch)()
    for c, (kind, _, _, _, payload) in enumerate(desc):
        if kind == "model":
            ctxs[c] = payload._ctx.h
        else:
            W, V = payload
            wp[c], vp[c] = _native.dptr(W), _native.dptr(V)
    out = np.zeros((len(OUTPUTS), N, M, T))
    _native.check(lib.btf_diag_eval(int(device), nch, int(S), N, M, T, K, wp, vp, ctxs, tcode, _native.dptr(out)), lib)
    res = dict(zip(OUTPUTS, out))
    rhat = res["rhat"]
    with np.errstate(invalid="ignore"):
        res["max_rhat"] = float(np.nanmax(rhat)) if np.any(~np.isnan(rhat)) else float("nan")
        res["n_rhat_above"] = int(np.sum(rhat > RHAT_THRESHOLD))
    for k in ("ess_bulk", "ess_tail"):
        a = res[k]
        res["min_" + k] = float(np.nanmin(a)) if np.any(~np.isnan(a)) else float("nan")
    res["nchains"], res["ndraws"] = nch, int(S)
    res["scalars"] = {}
    tables = [_scalar_table(c, S) for c in chains] if scalars else []
    for name in scalars or ():
        series = [_scalar_series(t, S, name) for t in tables]
        if all(s is not None for s in series):
            res["scalars"][name] = chain_diagnostics(np.stack(series))
    return res
