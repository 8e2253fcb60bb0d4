"""Model selection: per-curve log-likelihood over the kept samples, WAIC and DIC.

The data-sized work - ll_s(i,j) for every curve (i,j) and kept sample s - is the HIP kernel of
csrc/btf_criteria.h (btf_crit_eval).  This module holds the two host halves around it:

  statistics()  the kernel's own compact statistics of one data tensor, built once with numpy / scipy:
                per cell S1 = sum_r y and cnt (observed replicates; Binomial: trials), laid out [M][T][N] so that
                the kernel's loads coalesce, and per curve the normalising constant (Gaussian: Q = sum y^2 and the
                observation count n; Binomial: sum log C(n,y); Poisson: - sum lgamma(y+1); Negative-Binomial with a
                known rate r: sum lgamma(y+r) - lgamma(r) - lgamma(y+1)).  Device memory: 16 B per cell plus 16 B per
                curve (134 MB at (512,256,64), 4.3 GB at (2048,2048,64)); a criteria call adds 8 B per cell of
                scratch (the plug-in sums) for its duration.
  combine()     the kernel's per-curve accumulators and per-sample totals -> the dictionary of
                BayesianTensorFiltering.information_criteria (plain numpy over (N,M)).

  psis_loo_host()  the written definition of the PSIS-LOO kernel (csrc/btf_loo.h, btf_crit_loo): plain numpy / scipy over a
                (S,N,M) log-likelihood matrix; loo_combine() builds the dictionary of BayesianTensorFiltering.loo()
                and compare() the paired elpd difference of two models scored on the same data.

  gamma_grid_statistics() / gamma_grid_loglik()  the same two halves for the gamma-grid likelihood (family 5,
                csrc/btf_gg_criteria.h): its three per-cell statistics, and the written definition of what the kernel
                computes - the host class, one sample at a time.

  negbin_statistics() / negbin_rates() / negbin_loglik()  the same for the conjugate Negative-Binomial model, whose rate is
                sampled (csrc/btf_nb_criteria.h): the statistics and raw counts of a slot, the (S + 1, extent) rate array
                with R-bar appended, and the written definition by numpy / scipy.

It deliberately does not read the sampler's accumulation layouts: those differ by model and data form.
"""
import numpy as np

FAMILY_POISSON_LOG, FAMILY_POISSON_IDENTITY, FAMILY_LOGIT, FAMILY_GAUSSIAN, FAMILY_NEGBIN = 0, 1, 2, 3, 4
FAMILY_GAMMA_GRID = 5     # CRIT_FAM_GAMMA_GRID of csrc/btf_gg_criteria.h: statistics from gamma_grid_statistics, not statistics
CURVE_OUTPUTS = 5         # CRIT_OUT of csrc/btf_criteria.h: sumexp, max, mean, M2, ll at the plug-in
GRID_KEYS = ("lam2", "min_lam2", "max_lam2", "num_lam2")


def _cells(data, shape):
    """(S1, cnt, y4, obs4) of a (N,M,T) / (N,M,T,R) tensor with NaN = missing, or of a Binomial (Y, N) pair."""
    if isinstance(data, (tuple, list)):
        Y, Nt = (np.asarray(a, dtype=float) for a in data)
        if Y.shape != tuple(shape) or Nt.shape != Y.shape:
            raise ValueError("binomial data must be a (Y, N) pair of %r arrays" % (tuple(shape),))
        obs = ~(np.isnan(Y) | np.isnan(Nt))
        y, n = np.where(obs, Y, 0.0), np.where(obs, Nt, 0.0)
        return y, n, (y, n), obs
    Y = np.asarray(data, dtype=float)
    if Y.ndim not in (3, 4):
        raise AssertionError('Observations must be 3- or 4-tensor.')
    Y4 = Y[..., None] if Y.ndim == 3 else Y
    if Y4.shape[:3] != tuple(shape):
        raise ValueError("data shape %r does not match the model" % (Y.shape,))
    obs4 = ~np.isnan(Y4)
    y4 = np.where(obs4, Y4, 0.0)
    return y4.sum(axis=3), obs4.sum(axis=3).astype(float), y4, obs4


def statistics(family, data, shape, param=None):
    """Compact statistics of `data` for the criteria kernel.  Returns (S1, cnt) as contiguous [M][T][N] arrays,
    (c0, c1) as [N][M] arrays and the bool (N,M) mask of curves with at least one observation."""
    from scipy.special import gammaln
    S1, cnt, y, obs = _cells(data, shape)
    c1 = np.zeros(S1.shape[:2])
    if isinstance(y, tuple):                              # Binomial (Y, N): y successes of n trials
        if family != FAMILY_LOGIT:
            raise ValueError("a (Y, N) pair is Binomial data")
        yy, nn = y
        c0 = np.where(obs, gammaln(nn + 1.0) - gammaln(yy + 1.0) - gammaln(nn - yy + 1.0), 0.0).sum(axis=2)
        observed = obs.any(axis=2)
    else:
        ax = (2, 3)
        if family in (FAMILY_POISSON_LOG, FAMILY_POISSON_IDENTITY):
            c0 = -np.where(obs, gammaln(y + 1.0), 0.0).sum(axis=ax)
        elif family == FAMILY_LOGIT:
            c0 = np.zeros(S1.shape[:2])
        elif family == FAMILY_GAUSSIAN:
            c0 = (y * y).sum(axis=ax)
            c1 = obs.sum(axis=ax).astype(float)
        elif family == FAMILY_NEGBIN:
            r = float(param)
            c0 = np.where(obs, gammaln(y + r) - gammaln(r) - gammaln(y + 1.0), 0.0).sum(axis=ax)
        else:
            raise ValueError("unknown likelihood family %r" % (family,))
        observed = obs.any(axis=ax)
    layout = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0), dtype=np.float64)      # (N,M,T) -> [M][T][N]
    return layout(S1), layout(cnt), np.ascontiguousarray(c0, dtype=np.float64), np.ascontiguousarray(c1, dtype=np.float64), observed


def combine(curve, totals, observed, loglik=None):
    """The criteria dictionary from the kernel's outputs.

    curve: (5, N, M) = per curve, over the S samples: max-shifted sum of exp(ll_s), max, mean, Welford M2, ll at the
    plug-in; totals: (S,) = sum_ij ll_s; observed: (N, M) bool.  Curves without observations count 0 and are not
    counted in n_curves.  Follows numpy / scipy on -inf: a curve with a -inf sample has lppd from
    scipy.special.logsumexp and p_waic = nan (np.var)."""
    curve = np.asarray(curve, dtype=float)
    totals = np.asarray(totals, dtype=float)
    S = totals.shape[0]
    sumexp, mx, mean, m2, plug = curve
    obs = np.asarray(observed, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd = np.where(obs, mx + np.log(sumexp) - np.log(S), 0.0)
        p_waic = np.where(obs, m2 / (S - 1), 0.0) if S > 1 else np.zeros_like(mx)
        elpd_i = (lppd - p_waic)[obs]
        n = int(obs.sum())
        elpd_waic = float(elpd_i.sum())
        waic_se = float(2.0 * np.sqrt(n * np.var(elpd_i))) if n > 0 else 0.0
    mean_ll = np.where(obs, mean, 0.0)
    ll_at_mean = np.where(obs, plug, 0.0)
    mean_deviance = float(-2.0 * totals.mean())
    deviance_at_mean = float(-2.0 * ll_at_mean.sum())
    p_dic = mean_deviance - deviance_at_mean
    out = {"waic": -2.0 * elpd_waic, "elpd_waic": elpd_waic, "p_waic": float(p_waic.sum()), "lppd": float(lppd.sum()),
           "waic_se": waic_se, "dic": mean_deviance + p_dic, "p_dic": p_dic, "mean_deviance": mean_deviance,
           "deviance_at_mean": deviance_at_mean, "n_curves": n, "nsamples": int(S), "loglik_per_sample": totals.copy(),
           "curves": {"lppd": lppd, "p_waic": p_waic, "mean_ll": mean_ll, "ll_at_mean": ll_at_mean}}
    if loglik is not None:
        out["loglik"] = loglik
    return out


def evaluate(ctx, head, shape, pointwise=False):
    """btf_crit_eval on `ctx` (a _native.Context).  head: the arguments it shares with btf_crit_loo - slot, family, parameter,
    nsamples, Ws, Vs, noise, flags (PosteriorAnalysis._crit_head); shape (N,M).  Returns (curve (5,N,M), totals (S,),
    pointwise (S,N,M) or None): what combine() takes."""
    from . import _native
    S = head[3]
    curve = np.zeros((CURVE_OUTPUTS,) + tuple(shape))
    totals = np.zeros(S)
    pw = np.zeros((S,) + tuple(shape)) if pointwise else None
    ctx.call("btf_crit_eval", *head, _native.dptr(curve), _native.dptr(totals), _native.dptr(pw))
    return curve, totals, pw


def from_loglik(L, observed, L_at_mean):
    """The criteria dictionary straight from a (S, N, M) log-likelihood matrix and the (N, M) plug-in log-likelihood,
    by scipy / numpy (the definition combine() implements; used to check it)."""
    from scipy.special import logsumexp
    L = np.asarray(L, dtype=float)
    S = L.shape[0]
    obs = np.asarray(observed, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd = np.where(obs, logsumexp(L, axis=0) - np.log(S), 0.0)
        p_waic = np.where(obs, np.var(L, axis=0, ddof=1), 0.0) if S > 1 else np.zeros(obs.shape)
    elpd_i = (lppd - p_waic)[obs]
    tot = np.where(obs[None], L, 0.0).sum(axis=(1, 2))
    mean_dev = -2.0 * tot.mean()
    dev_mean = -2.0 * np.where(obs, L_at_mean, 0.0).sum()
    return {"waic": -2.0 * elpd_i.sum(), "elpd_waic": elpd_i.sum(), "p_waic": p_waic.sum(), "lppd": lppd.sum(),
            "waic_se": 2.0 * np.sqrt(obs.sum() * np.var(elpd_i)), "dic": 2 * mean_dev - dev_mean, "p_dic": mean_dev - dev_mean,
            "mean_deviance": mean_dev, "deviance_at_mean": dev_mean, "n_curves": int(obs.sum()), "nsamples": S,
            "loglik_per_sample": tot, "curves": {"lppd": lppd, "p_waic": p_waic}}


# ---- the gamma-grid likelihood (loglikelihood="gamma_grid"; csrc/btf_gg_criteria.h).  Conventions:
#   cell values     exactly gg_term's (csrc/btf_gamma_grid.h) = likelihoods.GammaGridLikelihood.logpdf: an unobserved cell
#                   inside an observed curve contributes lsp = log sum_g p_g, an observed cell with w.v <= 0 gives -inf, so
#                   L[s] equals model.logprob(Y, reduce="curve", W=Ws[s], V=Vs[s]);
#   unobserved curves  count 0 and are left out of n_curves, as for every other family;
#   the reference's DIC (doseresponse/select_btf.py:9-23: a nansum of logpdf over EVERY cell) therefore equals ours minus
#                   2 lsp T (number of unobserved curves): each such curve adds T lsp to every log-likelihood there, so
#                   -2 T lsp to 2 mean_D - D_mean.  lsp is 0 for the normalised weights estimate_likelihood always produces:
#                   the two agree on real tables (tests/golden/g18_gamma_grid_dic.npz checks both kinds). ----
def gamma_grid_statistics(Y, shape):
    """The three per-cell statistics of the gamma-grid criteria kernel.  Y: (N,M,T) or (N,M,T,R) with NaN = missing.
    Returns (S1, cnt, L) - sum_r y, the observed replicates, sum_r log y - as contiguous [M][T][N] float64 arrays, and the
    bool (N,M) mask of curves with at least one observation.  ValueError if an observed y <= 0."""
    S1, cnt, y4, obs4 = _cells(Y, shape)
    if isinstance(y4, tuple):
        raise ValueError("the gamma_grid likelihood takes one tensor, not a (Y, N) pair")
    if np.any(obs4 & (y4 <= 0)):
        raise ValueError("the gamma_grid likelihood needs every observed y > 0")
    L = np.where(obs4, np.log(np.where(obs4, y4, 1.0)), 0.0).sum(axis=3)
    layout = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0), dtype=np.float64)      # (N,M,T) -> [M][T][N]
    return layout(S1), layout(cnt), layout(L), obs4.any(axis=(2, 3))


def gamma_grid_loglik(Y, Ws, Vs, likelihood):
    """The written definition of the gamma-grid criteria kernel, by the host class one sample at a time.

    Y: (N,M,T) / (N,M,T,R), NaN = missing; Ws (S,N,K), Vs (S,M,T,K); likelihood: anything likelihoods.gamma_grid_table
    accepts.  Returns (L (S,N,M), L_at_mean (N,M), observed (N,M)): L[s,i,j] = sum_t logpdf(Y[i,j,t,:], w_i^s . v_jt^s),
    L_at_mean the same at Mu-bar = mean_s W_s V_s' (what select_btf.py plugs in); both 0 on curves without observations.
    from_loglik(L, observed, L_at_mean) gives the criteria dictionary."""
    from . import likelihoods
    lik = likelihoods.GammaGridLikelihood.from_table(*likelihoods.gamma_grid_table(likelihood))
    Y = np.asarray(Y, dtype=float)
    if Y.ndim not in (3, 4):
        raise AssertionError('Observations must be 3- or 4-tensor.')
    Y4 = Y[..., None] if Y.ndim == 3 else Y
    Ws, Vs = np.asarray(Ws, dtype=float), np.asarray(Vs, dtype=float)
    if Ws.ndim != 3 or Vs.ndim != 4 or Ws.shape[::2] != Vs.shape[::3] or Y4.shape[:3] != (Ws.shape[1],) + Vs.shape[1:3]:
        raise ValueError("Ws must be (S,N,K), Vs (S,M,T,K) and Y (N,M,T[,R]), got %r / %r / %r" % (Ws.shape, Vs.shape, Y.shape))
    observed = np.any(~np.isnan(Y4), axis=(2, 3))
    S = Ws.shape[0]
    L = np.zeros((S,) + observed.shape)
    mu = np.zeros(Y4.shape[:3])
    for s in range(S):
        eta = np.einsum("nk,mtk->nmt", Ws[s], Vs[s])
        mu += eta
        L[s] = np.where(observed, lik.logpdf(Y4, eta[..., None]).sum(axis=-1), 0.0)
    L_at_mean = np.where(observed, lik.logpdf(Y4, (mu / S)[..., None]).sum(axis=-1), 0.0)
    return L, L_at_mean, observed


def gamma_grid_upload(ctx, slot, Y, shape):
    """The gamma-grid statistics of Y into criteria slot `slot` of `ctx` (a _native.Context whose table is set:
    btf_set_likelihood_table); returns the observed-curve mask."""
    from . import _native
    S1, cnt, L, obs = gamma_grid_statistics(Y, shape)
    zero = np.zeros(tuple(shape)[:2])
    ctx.call("btf_crit_set_data", int(slot), _native.dptr(S1), _native.dptr(cnt), _native.dptr(zero), _native.dptr(zero))
    ctx.call("btf_crit_set_logsum", int(slot), _native.dptr(L))
    return obs


def gamma_grid_head(slot, nsamples, Ws=None, Vs=None):
    """The arguments btf_crit_eval and btf_crit_loo share (evaluate / loo_evaluate's `head`) for the gamma-grid family.
    Ws = Vs = None: the device-collected samples."""
    from . import _native
    Ws = None if Ws is None else _native.as_f64(Ws)
    Vs = None if Vs is None else _native.as_f64(Vs)
    return (int(slot), FAMILY_GAMMA_GRID, 0.0, int(nsamples), _native.dptr(Ws), _native.dptr(Vs), None, 0)


# ---- the conjugate Negative-Binomial model, whose rate R is sampled (csrc/btf_nb_criteria.h; btf_nb_crit_eval /
# btf_nb_crit_loo).  Family 4 above has one known rate and folds lgamma(y+r) - lgamma(r) into the curve constant; here
# that part depends on the sample and is the device's (nb_crit_const_kernel), c0 keeps - sum lgamma(y+1) only. ----
FAMILY_NEGBIN_RATES = "negbin_rates"      # the slot-cache key of PosteriorAnalysis._crit_slot; not a family of btf_crit_eval


def _rate_tensor(Rs, nsamples, shape):
    """Rs as (S, n0, n1, n2) with every n full or 1, and the BTF_PRED_AUX_* flags (predictive.rate_layout's checks), every
    rate finite and > 0."""
    from . import predictive
    flat, flags = predictive.rate_layout(Rs, nsamples, shape)
    if not (np.isfinite(flat).all() and (flat > 0).all()):
        raise ValueError("every Negative-Binomial rate must be finite and > 0")
    from . import _native
    tail = tuple(full if flags & bit else 1
                 for full, bit in zip(shape, (_native.PRED_AUX_ROWS, _native.PRED_AUX_COLS, _native.PRED_AUX_DEPTH)))
    return flat.reshape((nsamples,) + tail), flags


def negbin_rates(Rs, nsamples, shape):
    """The rate array of btf_nb_crit_eval / btf_nb_crit_loo: (S + 1, extent) float64 - the S rate tensors and, as tensor S,
    R-bar = np.mean(Rs, axis=0), the plug-in's rate - and its BTF_PRED_AUX_* axis flags.  Rs: what predictive.rate_layout
    accepts, every rate finite and > 0 (ValueError)."""
    R4, flags = _rate_tensor(Rs, nsamples, shape)
    out = np.concatenate([R4, np.mean(R4, axis=0)[None]], axis=0)
    return np.ascontiguousarray(out.reshape(nsamples + 1, -1), dtype=np.float64), flags


def negbin_statistics(Y, shape):
    """The statistics of a count tensor for the Negative-Binomial criteria kernels.  Y: (N,M,T) or (N,M,T,R), NaN = missing.
    Returns (S1, cnt) as contiguous [M][T][N] arrays, c0 [N][M] = - sum lgamma(y+1) over the curve's observed counts, the
    raw counts as a contiguous (N,M,T,R) array and the bool (N,M) mask of curves with an observation.  ValueError for an
    observed y < 0 (or infinite)."""
    if isinstance(Y, (tuple, list)):
        raise ValueError("negative-binomial data is the count tensor itself, not a (Y, N) pair")
    S1, cnt, c0, _, observed = statistics(FAMILY_POISSON_LOG, Y, shape)
    Y = np.asarray(Y, dtype=float)
    Y4 = np.ascontiguousarray(Y[..., None] if Y.ndim == 3 else Y, dtype=np.float64)
    if np.any(Y4 < 0) or np.any(np.isinf(Y4)):            # (NaN compares False: missing replicates pass)
        raise ValueError("the Negative-Binomial likelihood needs every observed y finite and >= 0")
    return S1, cnt, c0, Y4, observed


def negbin_loglik(Y, Ws, Vs, Rs):
    """The written definition of the Negative-Binomial criteria kernels (csrc/btf_nb_criteria.h), by numpy / scipy.

    Y: (N,M,T) / (N,M,T,R) counts, NaN = missing; Ws (S,N,K), Vs (S,M,T,K); Rs: (S,) + a shape that broadcasts against
    (N,M,T) with every axis full or 1, or (S,) / (S,1) - what predictive.rate_layout accepts.
    Returns (L (S,N,M), L_at_mean (N,M), observed (N,M)):
        L[s,i,j] = sum over observed (t,r) of scipy.stats.nbinom.logpmf(y_ijtr, R_s[i,j,t], 1 - ilogit(w_i^s . v_jt^s))
                 = sum lgamma(y+R) - lgamma(R) - lgamma(y+1) + y eta - (y+R) softplus(eta),
    the linear predictor eta not clipped (as family 4 and the predictive sampler); L_at_mean the same at
    Mu-bar = mean_s W_s V_s' and R-bar = mean_s R_s elementwise (the analogue of the Gaussian plug-in's mean nu2); both 0
    on curves without observations.  from_loglik(L, observed, L_at_mean) gives the criteria dictionary, psis_loo_host the
    PSIS-LOO one.  ValueError for an observed y < 0, a rate <= 0 or not finite, a rate array whose leading dimension is
    not S."""
    from scipy.special import gammaln
    Ws, Vs = np.asarray(Ws, dtype=float), np.asarray(Vs, dtype=float)
    Y = np.asarray(Y, dtype=float)
    if Y.ndim not in (3, 4):
        raise AssertionError('Observations must be 3- or 4-tensor.')
    Y4 = Y[..., None] if Y.ndim == 3 else Y
    if Ws.ndim != 3 or Vs.ndim != 4 or Ws.shape[::2] != Vs.shape[::3] or Y4.shape[:3] != (Ws.shape[1],) + Vs.shape[1:3]:
        raise ValueError("Ws must be (S,N,K), Vs (S,M,T,K) and Y (N,M,T[,R]), got %r / %r / %r" % (Ws.shape, Vs.shape, Y.shape))
    S = Ws.shape[0]
    R4, _ = _rate_tensor(Rs, S, Y4.shape[:3])
    obs4 = ~np.isnan(Y4)
    y = np.where(obs4, Y4, 0.0)
    if np.any(y < 0) or np.any(np.isinf(y)):
        raise ValueError("the Negative-Binomial likelihood needs every observed y finite and >= 0")
    observed = obs4.any(axis=(2, 3))

    def curves(eta, R):
        r, e = R[..., None], eta[..., None]
        ll = gammaln(y + r) - gammaln(r) - gammaln(y + 1.0) + y * e - (y + r) * np.logaddexp(0.0, e)
        return np.where(obs4, ll, 0.0).sum(axis=(2, 3))

    L = np.zeros((S,) + observed.shape)
    mu = np.zeros(Y4.shape[:3])
    for s in range(S):
        eta = np.einsum("nk,mtk->nmt", Ws[s], Vs[s])
        mu += eta
        L[s] = curves(eta, R4[s])
    L_at_mean = curves(mu / S, np.mean(R4, axis=0))
    return L, L_at_mean, observed


def negbin_upload(ctx, slot, Y, shape):
    """The Negative-Binomial statistics and raw counts of Y into criteria slot `slot` of `ctx` (a _native.Context); returns
    the observed-curve mask."""
    from . import _native
    S1, cnt, c0, Y4, obs = negbin_statistics(Y, shape)
    zero = np.zeros(tuple(shape)[:2])
    ctx.call("btf_crit_set_data", int(slot), _native.dptr(S1), _native.dptr(cnt), _native.dptr(c0), _native.dptr(zero))
    ctx.call("btf_crit_set_counts", int(slot), _native.dptr(Y4), int(Y4.shape[3]))
    return obs


def negbin_head(slot, nsamples, Ws, Vs, rates, flags):
    """The arguments btf_nb_crit_eval and btf_nb_crit_loo share: slot, nsamples, Ws, Vs (None: the context's current
    state), the (S + 1, extent) rates of negbin_rates and their axis flags."""
    from . import _native
    Ws = None if Ws is None else _native.as_f64(Ws)
    Vs = None if Vs is None else _native.as_f64(Vs)
    return (int(slot), int(nsamples), _native.dptr(Ws), _native.dptr(Vs), _native.dptr(rates), int(flags))


def negbin_evaluate(ctx, head, shape, pointwise=False, current=False):
    """btf_nb_crit_eval on `ctx`; head: negbin_head's; shape (N,M).  Returns what evaluate() does."""
    from . import _native
    S = head[1]
    curve = np.zeros((CURVE_OUTPUTS,) + tuple(shape))
    totals = np.zeros(S)
    pw = np.zeros((S,) + tuple(shape)) if pointwise else None
    ctx.call("btf_nb_crit_eval", *head, _native.CRIT_CURRENT if current else 0, _native.dptr(curve), _native.dptr(totals), _native.dptr(pw))
    return curve, totals, pw


# ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-curve-out (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson,
# Gelman, Yao, Gabry 2024).  psis_loo_host is the definition; the kernel of csrc/btf_loo.h implements the same steps. ----
LOO_MAX_SAMPLES = 4096    # LOO_MAX_S of csrc/btf_loo.h (the bound of btf_diag_eval)
LOO_MIN_TAIL = 5          # fewer tail samples: no Pareto fit, k = inf and the unsmoothed estimate


def tail_length(S, r_eff=1.0):
    """Mt = min(floor(0.2 S), ceil(3 sqrt(S / r_eff))): the number of largest importance ratios the Pareto fit uses."""
    return int(min(S // 5, np.ceil(3.0 * np.sqrt(S / float(r_eff)))))


def gpd_fit(x):
    """Zhang and Stephens (2009) estimate of the generalised Pareto distribution of the ascending excesses x > 0, with
    the weak prior of the PSIS paper on the shape.  Returns (k, sigma); (nan, nan) when no grid weight survives."""
    x = np.asarray(x, dtype=float)
    n = x.shape[0]
    m = 30 + int(np.floor(np.sqrt(n)))
    i = np.arange(1, m + 1, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b = 1.0 / x[n - 1] + (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * x[int(np.floor(n / 4.0 + 0.5)) - 1])
        k = np.log1p(-b[:, None] * x[None, :]).mean(axis=1)
        l = n * (np.log(-b / k) - k - 1.0)
        w = 1.0 / np.exp(l[None, :] - l[:, None]).sum(axis=1)
        keep = w >= 10.0 * np.finfo(float).eps
        if not keep.any():                                # no grid point survives (a nan in every l_i): no fit
            return np.nan, np.nan
        w, b = w[keep], b[keep]
        w = w / w.sum()
        bp = (w * b).sum()
        kp = np.log1p(-bp * x).mean()
        sigma = -kp / bp
    return (n * kp + 5.0) / (n + 10.0), sigma


def psis_curve(ll, r_eff=1.0):
    """PSIS-LOO of one curve from its S log-likelihoods: (elpd_loo, pareto_k, normalised log weights (S,)).
    A nan (or +inf) sample: all nan.  A -inf sample, an infinite importance ratio: elpd_loo = -inf, k = inf, weights nan."""
    from scipy.special import logsumexp
    ll = np.asarray(ll, dtype=float)
    S = ll.shape[0]
    if np.isnan(ll).any() or (ll == np.inf).any():
        return np.nan, np.nan, np.full(S, np.nan)
    if (ll == -np.inf).any():
        return -np.inf, np.inf, np.full(S, np.nan)
    lr = -ll
    lr = lr - lr.max()
    lw = lr.copy()
    k = np.inf
    Mt = tail_length(S, r_eff)
    if Mt >= LOO_MIN_TAIL:
        order = np.argsort(lr, kind="stable")             # ascending; ties in lr by ascending sample index
        cut = max(lr[order[S - Mt - 1]], np.log(np.finfo(float).tiny))
        tail = order[lr[order] > cut]                     # strictly above: ties with the cut-off stay outside
        n = tail.shape[0]
        if n >= LOO_MIN_TAIL:
            ecut = np.exp(cut)
            x = np.exp(lr[tail]) - ecut
            if x[0] > 0.0:
                kf, sigma = gpd_fit(x)
                if np.isfinite(kf) and np.isfinite(sigma):
                    k = kf
                    p = (np.arange(1, n + 1) - 0.5) / n
                    with np.errstate(divide="ignore", invalid="ignore"):
                        q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
                        lw[tail] = np.log(q + ecut)
    lw = np.minimum(lw, 0.0)                              # truncate at the raw maximum
    lw = lw - logsumexp(lw)
    return float(logsumexp(lw + ll)), float(k), lw


def psis_loo_host(L, observed, r_eff=1.0, log_weights=False):
    """PSIS-LOO of every curve of a (S,N,M) log-likelihood matrix, curve by curve on the host (psis_curve).

    observed: (N,M) bool; r_eff: a scalar or (N,M), the relative efficiency of the draws (1: independent).
    Returns the dictionary of loo_combine (without `mean`)."""
    from scipy.special import logsumexp
    L = np.asarray(L, dtype=float)
    S, N, M = L.shape
    r = np.broadcast_to(np.asarray(r_eff, dtype=float), (N, M))
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError("r_eff must be finite and > 0")
    elpd, kk = np.zeros((N, M)), np.zeros((N, M))
    lw = np.zeros((S, N, M)) if log_weights else None
    for i in range(N):
        for j in range(M):
            elpd[i, j], kk[i, j], w = psis_curve(L[:, i, j], r[i, j])
            if log_weights:
                lw[:, i, j] = w
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd = logsumexp(L, axis=0) - np.log(S)
    return loo_combine(elpd, kk, lppd, observed, S, log_weights=lw)


def loo_combine(elpd_loo, pareto_k, lppd, observed, nsamples, mean=None, log_weights=None):
    """The dictionary of BayesianTensorFiltering.loo() from the per-curve (N,M) arrays.  Curves without observations
    count 0 (pareto_k: nan there) and are left out of n_curves; the totals follow numpy on -inf / nan curves."""
    obs = np.asarray(observed, dtype=bool)
    S = int(nsamples)
    elpd = np.where(obs, np.asarray(elpd_loo, dtype=float), 0.0)
    lppd = np.where(obs, np.asarray(lppd, dtype=float), 0.0)
    k = np.where(obs, np.asarray(pareto_k, dtype=float), np.nan)
    with np.errstate(invalid="ignore"):
        p_loo = np.where(obs, lppd - elpd, 0.0)
        n = int(obs.sum())
        e = elpd[obs]
        total = float(e.sum())
        se = float(np.sqrt(n * np.var(e))) if n > 0 else 0.0
        good_k = min(1.0 - 1.0 / np.log10(S), 0.7) if S > 1 else 0.0
        n_bad = int((k[obs] > good_k).sum())
    out = {"elpd_loo": total, "p_loo": float(p_loo[obs].sum()), "looic": -2.0 * total, "se": se, "n_curves": n, "nsamples": S,
           "good_k": float(good_k), "n_bad": n_bad, "observed": obs.copy(),
           "curves": {"elpd_loo": elpd, "p_loo": p_loo, "pareto_k": k, "lppd": lppd}}
    if mean is not None:
        out["mean"] = mean
    if log_weights is not None:
        out["log_weights"] = log_weights
    return out


def loo_evaluate(ctx, head, shape, observed, r_eff=None, transform=0, mean=False, log_weights=False, negbin=False):
    """btf_crit_loo on `ctx` (a _native.Context) and the dictionary of BayesianTensorFiltering.loo().  head: as evaluate();
    shape (N,M,T); r_eff: None or a contiguous (N,M) array; transform: the code of the leave-curve-out mean.
    negbin: btf_nb_crit_loo, with negbin_head's head."""
    from . import _native
    N, M, T = shape
    S = head[1] if negbin else head[3]
    out = np.zeros((4, N, M))
    mean_out = np.zeros((N, M, T)) if mean else None
    lw = np.zeros((S, N, M)) if log_weights else None
    ctx.call("btf_nb_crit_loo" if negbin else "btf_crit_loo", *head, _native.dptr(r_eff), int(transform), _native.dptr(out),
             _native.dptr(mean_out), _native.dptr(lw))
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd = out[3] + np.log(out[2]) - np.log(S)            # (as combine forms it: the same bits)
    return loo_combine(out[0], out[1], lppd, observed, S, mean=mean_out, log_weights=lw)


def _curve_elpd(res):
    c = res["curves"]
    return np.asarray(c["elpd_loo"] if "elpd_loo" in c else c["lppd"] - c["p_waic"], dtype=float)


def compare(a, b, observed=None):
    """Paired comparison of two models scored on the same data: a, b are result dictionaries of loo() or
    information_criteria() (per-curve elpd: curves["elpd_loo"], or curves["lppd"] - curves["p_waic"]).
    elpd_diff = sum_ij (a_ij - b_ij) over the curves observed in both (positive: a predicts better) and
    se_diff = sqrt(n var_ij(a_ij - b_ij)), the standard error of that sum.  observed: the (N,M) mask of the curves to
    compare; None: the curves both results mark as observed."""
    ea, eb = _curve_elpd(a), _curve_elpd(b)
    if ea.shape != eb.shape:
        raise ValueError("compare: the two results score different shapes, %r and %r" % (ea.shape, eb.shape))
    both = (_curve_observed(a) & _curve_observed(b)) if observed is None else np.asarray(observed, dtype=bool)
    d = (ea - eb)[both]
    n = int(both.sum())
    with np.errstate(invalid="ignore"):
        return {"elpd_diff": float(d.sum()), "se_diff": float(np.sqrt(n * np.var(d))) if n > 0 else 0.0, "n_curves": n}


def _curve_observed(res):
    """The observed-curve mask of a result dictionary: loo() carries it as `observed`; information_criteria() carries none
    and sets every per-curve array of an unobserved curve to exactly 0."""
    if "observed" in res:
        return np.asarray(res["observed"], dtype=bool)
    c = res["curves"]
    return ~np.logical_and.reduce([np.asarray(c[key], dtype=float) == 0.0 for key in ("lppd", "p_waic", "mean_ll", "ll_at_mean") if key in c])
