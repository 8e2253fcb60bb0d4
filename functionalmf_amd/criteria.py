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

It deliberately does not read the sampler's accumulation layouts: those differ by model and data form.
"""
import numpy as np

FAMILY_POISSON_LOG, FAMILY_POISSON_IDENTITY, FAMILY_LOGIT, FAMILY_GAUSSIAN, FAMILY_NEGBIN = 0, 1, 2, 3, 4
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
