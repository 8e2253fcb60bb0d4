"""Posterior predictive checks: is a statistic of a whole observed curve plausible among the same statistic of curves
replicated from the fitted model?

The data-sized work - for every curve (i,j), kept sample s and rho < reps a replicated curve y_rep ~ p(y | theta_s) at the
curve's observed slots, five discrepancies of y_rep and of the data y under theta_s, and their comparison - is the HIP
kernel of csrc/btf_checks.h (btf_predict_check): no draw leaves the device.  This module is the written definition, in
plain numpy (importable without a GPU): the discrepancies, the variance function, `reference` (the whole result from a
given array of draws), the argument checks, and `evaluate`, the one caller of the C entry point that
BayesianTensorFiltering.posterior_checks and utils.posterior_checks share.

Replicates.  Data is Y (N,M,T,nreps), nan = missing.  With Rr = reps * nreps and n = S * Rr draws a cell, slot
(i,j,t,rep) of the replicated set e = s * reps + rho is draw number g = cell * n + s * Rr + rho * nreps + rep of the
family's device sampler, cell = (i M + j) T + t - exactly posterior_predictive(draws_per_sample=Rr, seed=seed,
cells=[cell])["draws"][0, s * Rr + rho * nreps + rep].  Only observed slots are drawn: a replicated curve has the
data's missingness.  There are nsets = S * reps replicated sets; per-set arrays are in the order of e.

Discrepancies T(y, theta_s) of a curve, with mu_t = E[y | theta_s], v_t = Var[y | theta_s]; sums run over the observed
slots with t ascending, then rep ascending, as plain adds in that order; slots with v_t == 0 are left out of 0-2:
    0 chisq   sum (y - mu_t)^2 / v_t
    1 max     max |y - mu_t| / sqrt(v_t)                                   (0 when no slot is left)
    2 lag1    sum_{t, t+1 both defined} e_t e_{t+1} / sum_{t defined} e_t^2,  e_t = sum_rep (y - mu_t) / sqrt(v_t m_t),
              m_t the observed replicates at t; t is defined when m_t > 0 and v_t != 0; nan when no adjacent pair
              exists or the denominator is 0.  The trend filter's own check: over- or under-smoothing leaves residuals
              that are correlated along depth.
    3 total   sum y
    4 zeros   the observed slots with y == 0

Per curve and discrepancy: p_ge / p_gt = the share of the sets e with T(y_rep_e, theta_s) >= / > T(y, theta_s), counted as
integers over the sets where both sides are defined (`defined` of them); t_obs / t_rep = the means of T(y, theta_s) and
T(y_rep_e, theta_s) over those same sets (t_obs is the mean over s when every set is defined); nobs = the observed slots.
All of them are nan for a curve without observations and for a bad curve - one with an observed slot nothing can be
drawn at in some sample (eta <= 0 under the identity link, a missing trial count), the nan cells of posterior_predictive.

Pooled (`overall`): per set, every discrepancy pooled over all curves that are neither empty nor bad - chisq, total and
zeros add, max is the maximum, lag1 pools numerator and denominator (and is nan when no curve has an adjacent pair).  The
order of the cross-curve sum is part of the definition: curves in row-major order, in tiles of POOL_TILE = 8 columns
(CHK_TILE of csrc/btf_checks.h) summed from zero, the tiles added in index order.
"""
import numpy as np

from . import predictive as _pred

DISCREPANCIES = ("chisq", "max", "lag1", "total", "zeros")
POOL_TILE = 8               # CHK_TILE of csrc/btf_checks.h: the columns of a tile of the pooled sums
# what is accumulated per (curve, set): lag1 as numerator, denominator and "has an adjacent pair"
_CHISQ, _MAX, _NUM, _DEN, _PAIR, _TOTAL, _ZEROS = range(7)


def variance_function(family, eta, aux=None):
    """Var[y | eta, aux]: aux (the variance nu2; Gaussian); the mean (both Poisson links; nan where eta <= 0 under the
    identity link); trials * p (1 - p), p = ilogit(eta) (aux = trials, default 1); r e^eta (1 + e^eta) (Negative-Binomial,
    aux = the rate r)."""
    code = _pred.family_code(family)
    eta = np.asarray(eta, dtype=float)
    if code == _pred.FAMILY_GAUSSIAN:
        if aux is None:
            raise ValueError("the Gaussian variance is the parameter nu2: pass it as aux")
        return np.broadcast_to(np.asarray(aux, dtype=float), eta.shape).copy()
    if code in (_pred.FAMILY_POISSON_LOG, _pred.FAMILY_POISSON_IDENTITY):
        return _pred.mean_function(code, eta)
    if code == _pred.FAMILY_LOGIT:
        e = np.exp(-np.abs(eta))                        # p (1 - p) = e / (1 + e)^2, either tail exact
        return (1.0 if aux is None else np.asarray(aux, dtype=float)) * (e / ((1.0 + e) * (1.0 + e)))
    if aux is None:
        raise ValueError("the Negative-Binomial variance needs the rate r as aux")
    e = np.exp(eta)
    return np.asarray(aux, dtype=float) * e * (1.0 + e)


def _terms(y, mu, v):
    """The seven running sums (..., 7) of curves y (..., T, nreps) (nan = missing) under mu, v (..., T), leading axes
    broadcast: slot by slot in the order of the definition."""
    y = np.asarray(y, dtype=float)
    mu, v = np.asarray(mu, dtype=float), np.asarray(v, dtype=float)
    T, nreps = y.shape[-2:]
    lead = np.broadcast_shapes(y.shape[:-2], mu.shape[:-1], v.shape[:-1])
    acc = np.zeros(lead + (7,))
    eprev, prevdef = np.zeros(lead), np.zeros(lead, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            mt, vt = np.broadcast_to(mu[..., t], lead), np.broadcast_to(v[..., t], lead)
            keep = vt != 0
            rsum, m = np.zeros(lead), np.zeros(lead)
            for r in range(nreps):
                yr = np.broadcast_to(y[..., t, r], lead)
                obs = ~np.isnan(yr)
                res = yr - mt
                use = obs & keep
                acc[..., _CHISQ] += np.where(use, res * res / vt, 0.0)
                acc[..., _MAX] = np.where(use, np.fmax(acc[..., _MAX], np.abs(res) / np.sqrt(vt)), acc[..., _MAX])
                rsum += np.where(use, res, 0.0)
                acc[..., _TOTAL] += np.where(obs, yr, 0.0)
                acc[..., _ZEROS] += np.where(obs & (yr == 0), 1.0, 0.0)
                m += obs
            defined = (m > 0) & keep
            e = rsum / np.sqrt(vt * m)
            acc[..., _DEN] += np.where(defined, e * e, 0.0)
            pair = defined & prevdef
            acc[..., _NUM] += np.where(pair, eprev * e, 0.0)
            acc[..., _PAIR] = np.where(pair, 1.0, acc[..., _PAIR])
            eprev, prevdef = np.where(defined, e, eprev), defined
    return acc


def _values(acc):
    """The five discrepancies (..., 5) from the running sums (..., 7)."""
    out = np.empty(acc.shape[:-1] + (5,))
    out[..., 0], out[..., 1], out[..., 3], out[..., 4] = acc[..., _CHISQ], acc[..., _MAX], acc[..., _TOTAL], acc[..., _ZEROS]
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., 2] = np.where((acc[..., _PAIR] != 0) & (acc[..., _DEN] != 0), acc[..., _NUM] / acc[..., _DEN], np.nan)
    return out


def discrepancies(y, mu, v):
    """The five discrepancies, in the order of DISCREPANCIES, of a curve y under the mean mu and variance v of one state.
    y: (T,) or (T, nreps), nan = missing; mu, v: (T,).  Leading batch axes broadcast: y (..., T, nreps), mu and v (..., T)
    give (..., 5)."""
    y = np.asarray(y, dtype=float)
    if y.ndim == 1:
        y = y[:, None]
    return _values(_terms(y, mu, v))


def two_sided(p_ge, p_gt):
    """min(1, 2 min(p_ge, 1 - p_gt)): the two-sided p-value from the upper tail P(T_rep >= T) and the lower 1 - P(T_rep > T)."""
    p_ge, p_gt = np.asarray(p_ge, dtype=float), np.asarray(p_gt, dtype=float)
    return np.minimum(1.0, 2.0 * np.minimum(p_ge, 1.0 - p_gt))


# ---- the argument checks
def check_which(which, family):
    """int32 discrepancy codes from names or codes; None: all five for the count families, the first four for Gaussian."""
    if which is None:
        which = DISCREPANCIES[:4] if _pred.family_code(family) == _pred.FAMILY_GAUSSIAN else DISCREPANCIES
    if isinstance(which, (str, int, np.integer)):
        which = (which,)
    codes = []
    for w in which:
        if isinstance(w, str):
            if w not in DISCREPANCIES:
                raise ValueError("unknown discrepancy %r (one of %s)" % (w, ", ".join(DISCREPANCIES)))
            w = DISCREPANCIES.index(w)
        elif not (isinstance(w, (int, np.integer)) and 0 <= int(w) < len(DISCREPANCIES)):
            raise ValueError("unknown discrepancy %r (a name of %s or a code 0..4)" % (w, ", ".join(DISCREPANCIES)))
        if int(w) in codes:
            raise ValueError("discrepancy %r is repeated: each of %s at most once" % (DISCREPANCIES[int(w)], ", ".join(DISCREPANCIES)))
        codes.append(int(w))
    if not codes:
        raise ValueError("which: at least one discrepancy of %s" % ", ".join(DISCREPANCIES))
    return np.asarray(codes, dtype=np.int32)


def check_reps(nsamples, reps, nreps=1):
    """(S, reps): reps >= 1, and the draws of a cell, S * reps * nreps, below 2^31."""
    S = int(nsamples)
    if S < 1:
        raise ValueError("posterior checks: at least one sample")
    if not (isinstance(reps, (int, np.integer)) and int(reps) >= 1):
        raise ValueError("reps must be an integer >= 1, got %r" % (reps,))
    if S * int(reps) * int(nreps) > 2 ** 31 - 1:
        raise ValueError("posterior checks: nsamples * reps * nreps = %d exceeds 2^31 - 1" % (S * int(reps) * int(nreps)))
    return S, int(reps)


def check_data(Y, shape):
    """The observations as a contiguous (N,M,T,nreps) array; they are required."""
    if Y is None:
        raise ValueError("posterior checks compare replicated curves with observations: no data bound, pass data=")
    return _pred.check_observations(Y, shape)


def check_curves(curves, shape):
    """Flat int32 curve indices i M + j from flat indices or (i,j) pairs; None: none."""
    if curves is None:
        return None
    c = np.asarray(curves)
    if c.size == 0:
        return None
    N, M = shape[:2]
    if c.ndim == 2 and c.shape[1] == 2 and np.issubdtype(c.dtype, np.integer):
        if np.any(c < 0) or np.any(c >= np.asarray((N, M))):
            raise ValueError("curves: (i,j) out of range for %d rows and %d columns" % (N, M))
        c = c[:, 0] * M + c[:, 1]
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("curves must be flat integer curve indices i * ncols + j or (i,j) pairs")
    if np.any(c < 0) or np.any(c >= N * M):
        raise ValueError("curves: index out of range for %d curves" % (N * M))
    return np.ascontiguousarray(c, dtype=np.int32)


# ---- the result, from what the device (or `reference`) hands over
def _share(num, den):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, np.nan)


def overall_counts(T_obs, T_rep, reps):
    """(count_ge, count_gt, defined) of pooled or listed values: T_obs (..., S) against T_rep (..., S * reps)."""
    to = np.repeat(np.asarray(T_obs, dtype=float), reps, axis=-1)
    tr = np.asarray(T_rep, dtype=float)
    ok = ~(np.isnan(to) | np.isnan(tr))
    with np.errstate(invalid="ignore"):
        return (ok & (tr >= to)).sum(-1), (ok & (tr > to)).sum(-1), ok.sum(-1)


def combine(codes, S, reps, nreps, seed, counts, nobs, pool_obs, pool_rep, curves=None, T_obs=None, T_rep=None, shape=None):
    """The result dict from the raw arrays of btf_predict_check: counts (5, nwhich, N, M) = the sets with >=, with >, with
    both sides defined, the sums of T(y) and of T(y_rep) over those; nobs (N,M); pool_obs (nwhich, S); pool_rep (nwhich, nsets)."""
    names = tuple(DISCREPANCIES[int(c)] for c in codes)
    out = {"which": names, "nobs": nobs, "overall": {}, "nsamples": int(S), "reps": int(reps), "nsets": int(S) * int(reps),
           "ndraws": int(S) * int(reps) * int(nreps), "seed": int(seed)}
    for k, name in enumerate(names):
        ge, gt, den = counts[0, k], counts[1, k], counts[2, k]
        out[name] = {"p_ge": _share(ge, den), "p_gt": _share(gt, den), "defined": den, "t_obs": _share(counts[3, k], den),
                     "t_rep": _share(counts[4, k], den)}
        cge, cgt, cdef = overall_counts(pool_obs[k], pool_rep[k], reps)
        out["overall"][name] = {"p_ge": float(cge) / cdef if cdef else float("nan"), "p_gt": float(cgt) / cdef if cdef else float("nan"),
                                "defined": int(cdef), "T_obs": pool_obs[k], "T_rep": pool_rep[k]}
    if curves is not None:
        M = shape[1]
        out["curves"] = {"index": np.stack([curves // M, curves % M], axis=1), "T_obs": T_obs, "T_rep": T_rep}
    return out


def reference(Y, Mu, Var, draws, reps=1, which=None, curves=None, seed=0):
    """The definition of the whole result in numpy, from given draws: Y (N,M,T) or (N,M,T,nreps); Mu, Var (S,N,M,T) the
    mean and variance of every cell under every state; draws (N,M,T,n) or (N M T, n), n = S * reps * nreps, in draw order
    (posterior_predictive(draws_per_sample=reps * nreps, cells=all)["draws"]).  Returns the dict of `evaluate`."""
    Mu, Var = np.asarray(Mu, dtype=float), np.asarray(Var, dtype=float)
    S, N, M, T = Mu.shape
    Y4 = check_data(Y, (N, M, T))
    nreps = Y4.shape[3]
    S, reps = check_reps(S, reps, nreps)
    codes = check_which(which, _pred.FAMILY_POISSON_LOG)
    cl = check_curves(curves, (N, M, T))
    nsets = S * reps
    d = np.asarray(draws, dtype=float).reshape(N, M, T, S, reps, nreps).transpose(3, 4, 0, 1, 2, 5)       # (S,reps,N,M,T,nreps)
    obs = ~np.isnan(Y4)
    yrep = np.where(obs, d, np.nan)
    nobs = obs.sum(axis=(2, 3)).astype(float)
    skip = (nobs == 0) | (np.isnan(d) & obs).any(axis=(0, 1, 4, 5))
    acc_rep = _terms(yrep, Mu[:, None], Var[:, None]).reshape(nsets, N, M, 7)
    acc_obs = np.repeat(_terms(Y4[None], Mu, Var), reps, axis=0)                                           # (nsets,N,M,7)
    t_rep, t_obs = _values(acc_rep)[..., codes], _values(acc_obs)[..., codes]                             # (nsets,N,M,nwhich)
    ok = ~(np.isnan(t_rep) | np.isnan(t_obs))
    with np.errstate(invalid="ignore"):
        counts = np.stack([(ok & (t_rep >= t_obs)).sum(0), (ok & (t_rep > t_obs)).sum(0), ok.sum(0),
                           np.where(ok, t_obs, 0.0).sum(0), np.where(ok, t_rep, 0.0).sum(0)]).astype(float)   # (5,N,M,nwhich)
    counts = np.ascontiguousarray(counts.transpose(0, 3, 1, 2))
    counts[:, :, skip] = np.nan
    nobs[skip] = np.nan
    # the pool: curves in row-major order, tiles of POOL_TILE columns from zero, tiles added in index order
    pool = np.zeros((2, nsets, 7))
    for i in range(N):
        for j0 in range(0, M, POOL_TILE):
            tile = np.zeros((2, nsets, 7))
            for j in range(j0, min(j0 + POOL_TILE, M)):
                if skip[i, j]:
                    continue
                for side, acc in enumerate((acc_rep, acc_obs)):
                    mx = np.fmax(tile[side, :, _MAX], acc[:, i, j, _MAX])
                    tile[side] += acc[:, i, j]
                    tile[side, :, _MAX] = mx
            mx = np.fmax(pool[..., _MAX], tile[..., _MAX])
            pool += tile
            pool[..., _MAX] = mx
    pooled = _values(pool)[..., codes]                                                                      # (2,nsets,nwhich)
    pool_rep, pool_obs = np.ascontiguousarray(pooled[0].T), np.ascontiguousarray(pooled[1, ::reps].T)
    T_obs = T_rep = None
    if cl is not None:
        ii, jj = cl // M, cl % M
        T_rep = np.ascontiguousarray(np.where(skip[ii, jj][None, :, None], np.nan, t_rep[:, ii, jj]).transpose(1, 2, 0))
        T_obs = np.ascontiguousarray(np.where(skip[ii, jj][None, :, None], np.nan, t_obs[::reps, ii, jj]).transpose(1, 2, 0))
    return combine(codes, S, reps, nreps, seed, counts, nobs, pool_obs, pool_rep, cl, T_obs, T_rep, (N, M, T))


def evaluate(ctx, shape, nembeds, family, nsamples, Ws=None, Vs=None, param=None, aux=None, aux_flags=0, trials=None, Y=None,
             which=None, reps=1, seed=0, curves=None, _chunk_rows=0):
    """btf_predict_check on `ctx` (a _native.Context).  Ws / Vs None: the first `nsamples` device-collected samples.
    aux / aux_flags, trials: as predictive.evaluate.  _chunk_rows: rows per launch (0: what 192 MiB of pooled partials
    hold) - no bit of the result depends on it.  Returns the result dict (see BayesianTensorFiltering.posterior_checks)."""
    from . import _native
    from ._analysis import check_states
    N, M, T = shape
    code = _pred.family_code(family)
    codes = check_which(which, code)
    Y4 = check_data(Y, shape)
    nreps = Y4.shape[3]
    S, reps = check_reps(nsamples, reps, nreps)
    if (Ws is None) != (Vs is None):
        raise ValueError("pass both Ws and Vs, or neither")
    if Ws is not None:
        Ws, Vs = check_states(Ws, Vs, shape, nembeds)
        if Ws.shape[0] != S:
            raise ValueError("nsamples does not match Ws")
    tr = _pred.check_trials(trials, shape)
    if aux is not None:
        aux = np.ascontiguousarray(aux, dtype=np.float64)
        if aux.shape[0] != S:
            raise ValueError("per-sample parameters: one per sample")
    cl = check_curves(curves, shape)
    if not (isinstance(_chunk_rows, (int, np.integer)) and _chunk_rows >= 0):
        raise ValueError("_chunk_rows must be an integer >= 0")
    nsets, nw, L = S * reps, len(codes), 0 if cl is None else len(cl)
    counts, nobs = np.zeros((5, nw, N, M)), np.zeros((N, M))
    pool_obs, pool_rep = np.zeros((nw, S)), np.zeros((nw, nsets))
    T_obs, T_rep = (np.zeros((L, nw, S)), np.zeros((L, nw, nsets))) if L else (None, None)
    dp, ip = _native.dptr, lambda a: a.ctypes.data_as(_native._c_ip) if a is not None else None
    ctx.call("btf_predict_check", code, float(param if param is not None else 0.0), S, dp(Ws), dp(Vs), dp(aux), int(aux_flags), dp(tr),
             dp(Y4), nreps, reps, int(seed) & 0xFFFFFFFFFFFFFFFF, ip(codes), nw, ip(cl), L, int(_chunk_rows), dp(counts), dp(nobs),
             dp(pool_obs), dp(pool_rep), dp(T_obs), dp(T_rep))
    return combine(codes, S, reps, nreps, seed, counts, nobs, pool_obs, pool_rep, cl, T_obs, T_rep, shape)
