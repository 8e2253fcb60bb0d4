"""Posterior predictive of the observations: replicated draws, bands, coverage and scores.

The data-sized work - y_rep ~ p(y | theta_s) for every cell (i,j,t), kept sample s and replicate r, and its reduction to
moments, percentiles, PIT values and interval membership - is the HIP kernel of csrc/btf_predict.h (btf_predict_eval):
the (S,N,M,T) draws never leave the device.  This module holds the host halves around it, in plain numpy (importable
without a GPU): the family table, the mean function E[y | eta], the argument checks, and `evaluate`, the one caller of
the C entry point that BayesianTensorFiltering.posterior_predictive and utils.posterior_predictive share.

The gamma-grid likelihood (loglikelihood="gamma_grid") has entry points of its own, as its criteria have: gamma_grid_evaluate
(btf_predict_gg_eval, behind NonconjugateBayesianTensorFiltering.gamma_grid_predictive and utils.gamma_grid_predictive),
gamma_grid_batch (btf_predict_gg_batch) and gamma_grid_mean; family_code and FAMILIES keep to the five of btf_predict_eval.

What the reference's benchmark applications do on the host (flutrends/benchmark.py:60-75, :129-134: Gaussian draws per
kept sample, 2.5 / 97.5 percentiles per cell in a Python loop, coverage of the held-out years; politics/benchmark.py:
147-172: per-sample RMSE / MAE of E[y | theta_s] with Mu = R p / (1 - p) for the Negative-Binomial model).
"""
import numpy as np

from ._analysis import check_q, check_states  # noqa: F401  (the shared checks, under the names this module had for them)

FAMILY_POISSON_LOG, FAMILY_POISSON_IDENTITY, FAMILY_LOGIT, FAMILY_GAUSSIAN, FAMILY_NEGBIN = 0, 1, 2, 3, 4
FAMILIES = {"poisson": FAMILY_POISSON_LOG, "poisson_log": FAMILY_POISSON_LOG, "poisson_identity": FAMILY_POISSON_IDENTITY,
            "binomial": FAMILY_LOGIT, "bernoulli": FAMILY_LOGIT, "logit": FAMILY_LOGIT,
            "gaussian": FAMILY_GAUSSIAN, "normal": FAMILY_GAUSSIAN,
            "negative_binomial": FAMILY_NEGBIN, "negbin": FAMILY_NEGBIN}
MAX_DRAWS = 16384           # PRED_MAX_DRAWS of csrc/btf_predict.h: S * draws_per_sample per cell (sorted in LDS)
POISSON_SWITCH = 10.0       # PRED_POIS_SWITCH: inversion below, transformed rejection (PTRS) from here
BINOMIAL_SWITCH = 10.0      # PRED_BINOM_SWITCH: inversion while n min(p, 1-p) is below, BTRS from here
ARRAY_OUTPUTS = ("mean", "y_mean", "y_var", "quantiles", "pit_lo", "pit_hi", "inside", "nobs", "rmse", "mae", "draws")


def family_code(family):
    """The integer family of btf_predict_eval from a name or a code."""
    if isinstance(family, str):
        if family not in FAMILIES:
            raise ValueError("unknown predictive family %r (one of %s)" % (family, sorted(FAMILIES)))
        return FAMILIES[family]
    code = int(family)
    if not 0 <= code <= 4:
        raise ValueError("unknown predictive family %r" % (family,))
    return code


def mean_function(family, eta, aux=None):
    """E[y | eta, aux]: eta (Gaussian); exp(eta) (Poisson, log link); eta, nan where eta <= 0 (Poisson, identity link);
    trials * ilogit(eta) (aux = trials, default 1); r * p / (1 - p) = r * exp(eta) (Negative-Binomial, aux = the rate r)."""
    code = family_code(family)
    eta = np.asarray(eta, dtype=float)
    if code == FAMILY_GAUSSIAN:
        return eta.copy()
    if code == FAMILY_POISSON_LOG:
        return np.exp(eta)
    if code == FAMILY_POISSON_IDENTITY:
        return np.where(eta > 0, eta, np.nan)
    if code == FAMILY_LOGIT:
        return (1.0 if aux is None else np.asarray(aux, dtype=float)) / (1.0 + np.exp(-eta))
    if aux is None:
        raise ValueError("the Negative-Binomial mean needs the rate r as aux")
    return np.asarray(aux, dtype=float) * np.exp(eta)


def check_draws(nsamples, draws_per_sample):
    nsamples, R = int(nsamples), int(draws_per_sample)
    if nsamples < 1:
        raise ValueError("posterior predictive: at least one sample")
    if R < 1:
        raise ValueError("draws_per_sample must be >= 1")
    if nsamples * R > MAX_DRAWS:
        raise ValueError("posterior predictive: nsamples * draws_per_sample = %d exceeds %d (the draws of a cell are sorted "
                         "in LDS); thin the samples or lower draws_per_sample" % (nsamples * R, MAX_DRAWS))
    return nsamples, R


def check_cells(cells, shape):
    """Flat int32 cell indices from flat indices or (i,j,t) triples."""
    if cells is None:
        return None
    c = np.asarray(cells)
    if c.size == 0:
        return None
    if c.ndim == 2 and c.shape[1] == 3:
        if np.any(c < 0) or np.any(c >= np.asarray(shape)):
            raise ValueError("cells: (i,j,t) out of range")
        c = np.ravel_multi_index(c.T, shape)
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("cells must be flat integer cell indices or (i,j,t) triples")
    if np.any(c < 0) or np.any(c >= int(np.prod(shape))):
        raise ValueError("cells: index out of range")
    return np.ascontiguousarray(c, dtype=np.int32)


def check_observations(Y, shape):
    """Observations as a contiguous (N,M,T,R) array (nan = missing), or None."""
    if Y is None:
        return None
    Y = np.asarray(Y, dtype=float)
    if Y.ndim not in (3, 4) or Y.shape[:3] != tuple(shape):
        raise ValueError("data shape %r does not match the model's %r" % (Y.shape, tuple(shape)))
    return np.ascontiguousarray(Y[..., None] if Y.ndim == 3 else Y, dtype=np.float64)


def check_trials(trials, shape):
    if trials is None:
        return None
    t = np.asarray(trials, dtype=float)
    if t.shape != tuple(shape):
        raise ValueError("trials shape %r does not match the model's %r" % (t.shape, tuple(shape)))
    return np.ascontiguousarray(t, dtype=np.float64)


def rate_layout(R, nsamples, shape):
    """Per-sample Negative-Binomial rates as (array (S, prod(extent)), flags): R is (S,) + a shape that broadcasts against
    (N,M,T) with every axis either full or 1 (the model's `rdims`), or (S,) / (S,1) for one shared rate."""
    from . import _native
    R = np.asarray(R, dtype=float)
    if R.ndim == 0 or R.shape[0] != nsamples:
        raise ValueError("R must hold one rate (tensor) per sample: leading dimension %d" % nsamples)
    tail = R.shape[1:]
    if int(np.prod(tail, dtype=np.int64)) == 1:
        tail = (1, 1, 1)
    if len(tail) != 3 or any(e not in (1, full) for e, full in zip(tail, shape)):
        raise ValueError("R %r: every axis after the first must be 1 or the model's %r" % (R.shape, tuple(shape)))
    flags = _native.PRED_AUX_PER_SAMPLE
    for e, bit in zip(tail, (_native.PRED_AUX_ROWS, _native.PRED_AUX_COLS, _native.PRED_AUX_DEPTH)):
        if e > 1:
            flags |= bit
    return np.ascontiguousarray(R.reshape(nsamples, -1), dtype=np.float64), flags


def _evaluate(ctx, entry, head, shape, nembeds, nsamples, Ws, Vs, tail, Y, q, draws_per_sample, seed, cells, check_Y=None):
    """The checks, the output arrays and the result dict that btf_predict_eval and btf_predict_gg_eval share: `entry` is
    called with head + (S, Ws, Vs) + tail(S) + (Y, nreps, R, seed, q, nq, cells, ncells) + the eleven outputs.
    tail: the family's own arguments, checked against the sample count (arrays go over as pointers, None as NULL);
    check_Y: the family's demands on the data."""
    from . import _native
    N, M, T = shape
    S, R = check_draws(nsamples, draws_per_sample)
    qs = check_q(q)
    if (Ws is None) != (Vs is None):
        raise ValueError("pass both Ws and Vs, or neither")
    if Ws is not None:
        Ws, Vs = check_states(Ws, Vs, shape, nembeds)
        if Ws.shape[0] != S:
            raise ValueError("nsamples does not match Ws")
    Y4 = check_observations(Y, shape)
    if check_Y is not None:
        check_Y(Y4)
    tail = tail(S)
    cl = check_cells(cells, shape)
    n = S * R
    out = {"mean": np.zeros((N, M, T)), "y_mean": np.zeros((N, M, T)), "y_var": np.zeros((N, M, T)),
           "quantiles": np.zeros((len(qs), N, M, T))}
    have_y = Y4 is not None
    for k in ("pit_lo", "pit_hi", "inside", "nobs"):
        out[k] = np.zeros((N, M, T)) if have_y else None
    for k in ("rmse", "mae"):
        out[k] = np.zeros(S) if have_y else None
    out["draws"] = np.zeros((len(cl), n)) if cl is not None else None
    dp = _native.dptr
    ctx.call(entry, *head, S, dp(Ws), dp(Vs), *(v if isinstance(v, int) else dp(v) for v in tail), dp(Y4),
             Y4.shape[3] if have_y else 0, R, int(seed) & 0xFFFFFFFFFFFFFFFF, dp(qs), len(qs),
             cl.ctypes.data_as(_native._c_ip) if cl is not None else None, len(cl) if cl is not None else 0,
             dp(out["mean"]), dp(out["y_mean"]), dp(out["y_var"]), dp(out["quantiles"]) if len(qs) else None, dp(out["pit_lo"]),
             dp(out["pit_hi"]), dp(out["inside"]), dp(out["nobs"]), dp(out["rmse"]), dp(out["mae"]), dp(out["draws"]))
    out = {k: v for k, v in out.items() if v is not None}
    if cl is not None:
        out["cells"] = cl
    out.update(summarise(out.get("inside"), out.get("nobs"), qs))
    out["nsamples"], out["ndraws"] = S, n
    return out


def evaluate(ctx, shape, nembeds, family, nsamples, Ws=None, Vs=None, param=None, aux=None, aux_flags=0, trials=None, Y=None,
             q=(2.5, 97.5), draws_per_sample=1, seed=0, cells=None):
    """btf_predict_eval on `ctx` (a _native.Context).  Ws / Vs None: the first `nsamples` device-collected samples.
    aux / aux_flags: per-sample parameters (Gaussian variances (S,); rates from rate_layout).  Returns the result dict."""
    code = family_code(family)

    def tail(S):
        tr, ax = check_trials(trials, shape), aux
        if ax is not None:
            ax = np.ascontiguousarray(ax, dtype=np.float64)
            if ax.shape[0] != S:
                raise ValueError("per-sample parameters: one per sample")
        return ax, int(aux_flags), tr
    return _evaluate(ctx, "btf_predict_eval", (code, float(param if param is not None else 0.0)), shape, nembeds, nsamples, Ws, Vs, tail,
                     Y, q, draws_per_sample, seed, cells)


def summarise(inside, nobs, qs):
    """coverage = observed replicates inside [q[0], q[-1]] over observed replicates (cells with nan draws left out);
    nominal = (q[-1] - q[0]) / 100."""
    res = {"nominal": float(qs[-1] - qs[0]) / 100.0 if len(qs) >= 2 else float("nan"), "coverage": float("nan")}
    if inside is not None and nobs is not None and len(qs) >= 2:
        ok = np.isfinite(inside)
        den = float(nobs[ok].sum())
        if den > 0:
            res["coverage"] = float(inside[ok].sum()) / den
    return res


def batch(family, eta, aux, seed=0, device=0):
    """out[i] ~ family(eta[i], aux[i]) from the device samplers (btf_predict_batch); draw i uses global draw index i.
    aux: trials (logit), variance (Gaussian), rate r (Negative-Binomial); ignored by the Poisson families."""
    from . import _native
    code = family_code(family)
    eta = np.ascontiguousarray(np.atleast_1d(eta), dtype=np.float64).ravel()
    aux = np.ascontiguousarray(np.broadcast_to(np.asarray(aux, dtype=np.float64), eta.shape)).ravel()
    out = np.zeros(eta.size)
    lib = _native.load()
    _native.check(lib.btf_predict_batch(int(device), code, eta.size, _native.dptr(eta), _native.dptr(aux),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, _native.dptr(out)), lib)
    return out


# ---- the gamma-grid likelihood (loglikelihood="gamma_grid"; csrc/btf_gg_predict.h).  The draw, as the kernel makes it:
# y | eta = eta s_g Gamma(a_g, 1), the component g chosen by the weights w_g = p_g / sum_h p_h of the table - NOT uniformly,
# as the reference's GammaGridLikelihood.sample does (np.random.choice(G) ignores mean_probs); a table with equal weights
# gives the reference's behaviour.  One component per replicated observation: the marginal predictive of one new
# observation (the likelihood shares one component among the replicates of a cell). ----
GAMMA_GRID_STREAM = 5       # PRED_FAM_GAMMA_GRID: the generator family of the draws


def gamma_grid_weights(likelihood):
    """(shape, scale, w, c, mbar) of anything likelihoods.gamma_grid_table accepts: the normalised weights w_g = p_g / sum p,
    their cumulative sums c_g and mbar = sum_g w_g a_g s_g, every sum accumulated in ascending g in float64 - what
    gg_pred_table of csrc/btf_gamma_grid.h computes (there c is 2 from the last positive weight on)."""
    from . import likelihoods
    a, s, p = likelihoods.gamma_grid_table(likelihood)
    psum = 0.0
    for v in p:
        psum += float(v)
    w = p / psum
    c, acc, mbar = np.zeros(len(p)), 0.0, 0.0
    for g in range(len(p)):
        acc += float(w[g])
        mbar += float(w[g]) * float(a[g]) * float(s[g])
        c[g] = acc
    return a, s, w, c, mbar


def gamma_grid_mean(likelihood, eta):
    """E[y | eta] = eta * sum_g w_g a_g s_g under the gamma-grid likelihood; nan where eta <= 0 (no such gamma)."""
    mbar = gamma_grid_weights(likelihood)[4]
    eta = np.asarray(eta, dtype=float)
    with np.errstate(invalid="ignore"):
        return np.where(eta > 0, eta * mbar, np.nan)


def check_gamma_grid_data(Y, shape):
    """Observations of a gamma-grid model as check_observations gives them; every observed y > 0, as gamma_grid_statistics
    of criteria.py demands."""
    if isinstance(Y, (tuple, list)):
        raise ValueError("the gamma_grid likelihood takes one tensor, not a (Y, N) pair")
    Y4 = check_observations(Y, shape)
    if Y4 is not None and np.any(Y4 <= 0):                 # (nan = missing compares false)
        raise ValueError("the gamma_grid likelihood needs every observed y > 0")
    return Y4


def gamma_grid_evaluate(ctx, shape, nembeds, nsamples, Ws=None, Vs=None, Y=None, q=(2.5, 97.5), draws_per_sample=1, seed=0, cells=None):
    """btf_predict_gg_eval on `ctx` (a _native.Context whose table is set: btf_set_likelihood_table).  Ws / Vs None: the
    first `nsamples` device-collected samples.  Returns the dictionary of `evaluate`."""
    if isinstance(Y, (tuple, list)):
        check_gamma_grid_data(Y, shape)
    return _evaluate(ctx, "btf_predict_gg_eval", (), shape, nembeds, nsamples, Ws, Vs, lambda S: (), Y, q, draws_per_sample, seed, cells,
                     check_Y=lambda Y4: check_gamma_grid_data(Y4, shape))


def gamma_grid_batch(eta, likelihood, seed=0, device=0, components=False):
    """out[i] = draw number i of y | eta[i] from the device sampler (btf_predict_gg_batch); likelihood: anything
    likelihoods.gamma_grid_table accepts (a bad table raises before any device call).  components=True: (out, comp), comp
    the int32 component of every draw (-1 where eta <= 0 or nan gave nan)."""
    from . import _native, likelihoods
    a, s, p = likelihoods.gamma_grid_table(likelihood)
    eta = np.ascontiguousarray(np.atleast_1d(eta), dtype=np.float64).ravel()
    out = np.zeros(eta.size)
    comp = np.zeros(eta.size, dtype=np.int32) if components else None
    lib = _native.load()
    _native.check(lib.btf_predict_gg_batch(int(device), eta.size, _native.dptr(eta), int(a.size), _native.dptr(a), _native.dptr(s),
                                           _native.dptr(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _native.dptr(out),
                                           comp.ctypes.data_as(_native._c_ip) if components else None), lib)
    return (out, comp) if components else out
