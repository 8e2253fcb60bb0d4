"""The Python front end of the posterior analysis features: summary, diagnostics, criteria / PSIS-LOO, predictive,
predictive checks, functionals, simultaneous bands, ranking, feature association, monotone projection and fold-in.

Two halves.  The argument checks every feature shares, as plain functions (importable without a GPU): the transform table,
the percentile check, the (S,N,K) / (S,M,T,K) shape check and the per-sample scalar check - the stateless forms in utils.py
and the feature modules (predictive.py, functionals.py, fold_in.py, diagnostics.py) use them too.  And `PosteriorAnalysis`,
the mixin BayesianTensorFiltering inherits its analysis methods from: each method refuses what it cannot do in a fixed order
(`_unsharded`, the family hook of the model, its own arguments), resolves its samples in one place (`_samples`: the
device-collected ones, or an uploaded run_gibbs result dict) and hands over to the `evaluate` of its feature module, the one
caller of the C entry point.  The hooks that differ by likelihood (_crit_family, _pred_family, _pred_aux, _fold_family,
_fold_cols_family, _fold_depth_family) stay with the models in factor.py.
"""
import numpy as np

from . import _native
from . import criteria as _criteria

TRANSFORMS = {None: 0, "identity": 0, "ilogit": 1, "square": 2}      # f of f(w_i . v_jt): the code of the kernels


class TransformError(ValueError, KeyError):
    """An unknown transform.  Also a KeyError, what posterior_summary's table lookup raised before the check was shared."""
    __str__ = ValueError.__str__            # (KeyError prints the repr of its argument)


def transform_code(transform):
    if not isinstance(transform, (str, type(None))) or transform not in TRANSFORMS:
        raise TransformError("transform must be None, 'identity', 'ilogit' or 'square', not %r" % (transform,))
    return TRANSFORMS[transform]


def check_q(q, allow_none=False):
    """Percentiles as a contiguous float64 1-D array; None (where allowed): none."""
    if q is None and allow_none:
        return np.zeros(0)
    qs = _native.as_f64(np.atleast_1d(q))
    if qs.ndim != 1 or not np.all((qs >= 0) & (qs <= 100)):
        raise ValueError("percentiles q must lie in [0, 100]")
    return qs


def check_states(Ws, Vs, shape=None, nembeds=None, what=""):
    """(Ws, Vs) as contiguous float64 (S,N,K) / (S,M,T,K) arrays.  shape=None: they only have to agree with each other
    (the stateless forms); shape (N,M,T) and nembeds: they match the model and hold at least one sample.  Ws=None: Vs alone
    (fold_in_rows: at least one sample either way)."""
    Vs = _native.as_f64(Vs)
    S = Vs.shape[0] if Vs.ndim == 4 else -1
    if Ws is not None:
        Ws = _native.as_f64(Ws)
    if shape is None:
        N, M, T, K = ("N", "M", "T", "K")
        ok = Vs.ndim == 4 and (S >= 1 if Ws is None else Ws.ndim == 3 and Ws.shape[::2] == Vs.shape[::3])
    else:
        (N, M, T), K = shape, nembeds
        ok = S >= 1 and Vs.shape == (S, M, T, K) and (Ws is None or Ws.shape == (S, N, K))
    if not ok:
        want_V = "(S,%s,%s,%s)" % (M, T, K)
        if Ws is None:
            raise ValueError("%sVs must be %s, got %r" % (what, want_V, Vs.shape))
        raise ValueError("%sWs must be (S,%s,%s) and Vs %s, got %r / %r" % (what, N, K, want_V, Ws.shape, Vs.shape))
    return Ws, Vs


def check_scalars(name, v, S, positive=True):
    """One value per sample (nu2, sigma2) as a contiguous (S,) array; positive: each finite and > 0."""
    if v is None:
        raise ValueError("%s: one value per sample is needed" % name)
    a = np.asarray(v, dtype=float)
    if a.size != S:
        raise ValueError("%s must hold one value per sample (%d), got shape %r" % (name, S, a.shape))
    a = np.ascontiguousarray(a.reshape(S))
    if positive and not (np.all(np.isfinite(a)) and np.all(a > 0)):
        raise ValueError("%s must be finite and positive" % name)
    return a


def check_r_eff(r_eff, shape):
    """The r_eff of loo(): None, or a scalar / (N,M) array, finite and > 0, as a contiguous (N,M) float64 array."""
    if r_eff is None:
        return None
    r_eff = np.asarray(r_eff, dtype=float)
    if r_eff.shape not in ((), tuple(shape)):
        raise ValueError("r_eff must be a scalar or a (%d,%d) array" % tuple(shape))
    if not (np.all(np.isfinite(r_eff)) and np.all(r_eff > 0)):
        raise ValueError("r_eff must be finite and > 0")
    return _native.as_f64(np.broadcast_to(r_eff, tuple(shape)))


def check_loo_samples(S, what="loo"):
    if S > _criteria.LOO_MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d" % (what, S, _criteria.LOO_MAX_SAMPLES))


def summary(call, shape, q, transform):
    """(mean (N,M,T), quantiles (len(q),N,M,T)) of f(W V') from a summary entry point: call(code, q, nq, mean, quantiles)
    runs it with whatever precedes those five arguments (btf_collect_summary, btf_posterior_summary)."""
    code = transform_code(transform)
    qs = _native.as_f64(np.atleast_1d(q))
    mean = np.zeros(tuple(shape))
    quant = np.zeros((len(qs),) + mean.shape)
    call(code, _native.dptr(qs), len(qs), _native.dptr(mean), _native.dptr(quant))
    return mean, quant


class PosteriorAnalysis:
    """The analysis methods of BayesianTensorFiltering (functionalmf_amd/factor.py), over the samples a device-collecting
    run_gibbs kept (`_collected` of them) or a run_gibbs result dict."""

    def _unsharded(self, what):
        if self._plan.world > 1 or self._exchange.active:
            raise NotImplementedError("%s: unsharded models only" % what)

    def _samples(self, results, need=("W", "V")):
        """(S, Ws, Vs) of an analysis call.  results None: the S samples the last device-collecting run_gibbs kept, and
        Ws = Vs = None (they are read where they lie); otherwise the dict's states, checked against the model, as contiguous
        float64 arrays to upload (Ws None unless "W" is needed)."""
        if results is None:
            S = getattr(self, "_collected", 0)
            if S < 1:
                raise RuntimeError("no samples collected on the device (run_gibbs with rng='device' first), and no results given")
            return S, None, None
        try:
            Ws, Vs = results["W"] if "W" in need else None, results["V"]
        except (KeyError, TypeError):
            raise ValueError("results must be a run_gibbs result dict with %sV (S,M,T,K)" % ("W (S,N,K) and " if "W" in need else ""))
        Ws, Vs = check_states(Ws, Vs, (self.nrows, self.ncols, self.ndepth), self.nembeds, what="results: ")
        return Vs.shape[0], Ws, Vs

    def posterior_summary(self, q=(5, 95), transform=None):
        """Mean and percentiles of f(W V') over the samples the last device-collecting run_gibbs kept,
        computed where they lie (btf_collect_summary); see functionalmf_amd.utils.posterior_summary."""
        self._unsharded("posterior_summary")
        S = self._samples(None)[0]
        return summary(lambda *tail: self._ctx.call("btf_collect_summary", int(S), *tail), (self.nrows, self.ncols, self.ndepth),
                       q, transform)

    def convergence_diagnostics(self, *others, transform=None):
        """Split R-hat, bulk / tail ESS and MCSE per cell of f(W V') over this model's device-collected samples and
        those of `others` (models or run_gibbs result dicts): functionalmf_amd.diagnostics.convergence([self, *others])."""
        from . import diagnostics
        return diagnostics.convergence([self] + list(others), transform=transform)

    # ---- model selection: per-curve log-likelihood, WAIC, DIC, PSIS-LOO (functionalmf_amd/criteria.py, csrc/btf_criteria.h) ----
    def _crit_drop(self, slot):
        keys = getattr(self, "_crit_keys", None)
        if keys is not None and keys[slot] is not None:
            self._ctx.call("btf_crit_set_data", slot, None, None, None, None)
            keys[slot] = None

    def _crit_slot(self, data, family, param):
        """Upload the criteria statistics of `data` once (cached by identity, shape and fingerprint, as set_data
        recognises the bound data); returns (slot, observed-curve mask).  Slot 0 holds the bound data, 1 held-out data."""
        from .factor import _fingerprint
        if data is None:
            data = getattr(self, "_data_ref", None)
            if data is None:
                raise ValueError("no data bound to the model: pass data=")
        arrays = data if isinstance(data, (tuple, list)) else (data,)
        key = (family, param) + tuple((id(a), np.shape(a), _fingerprint(a)) for a in arrays)
        if getattr(self, "_crit_keys", None) is None:
            self._crit_keys, self._crit_obs, self._crit_refs = [None, None], [None, None], [None, None]
        for slot in (0, 1):
            if self._crit_keys[slot] == key:
                return slot, self._crit_obs[slot]
        bound = getattr(self, "_data_ref", None)
        bound = bound if isinstance(bound, (tuple, list)) else (bound,)
        slot = 0 if len(bound) == len(arrays) and all(a is b for a, b in zip(arrays, bound)) else 1
        obs = self._crit_upload(slot, family, data, param)
        self._crit_keys[slot], self._crit_obs[slot], self._crit_refs[slot] = key, obs, data     # (refs: ids stay unique)
        return slot, obs

    def _crit_upload(self, slot, family, data, param):
        """The statistics of `data` into the slot; returns the observed-curve mask."""
        S1, cnt, c0, c1, obs = _criteria.statistics(family, data, (self.nrows, self.ncols, self.ndepth), param)
        self._ctx.call("btf_crit_set_data", slot, _native.dptr(S1), _native.dptr(cnt), _native.dptr(c0), _native.dptr(c1))
        return obs

    def _crit_check(self):
        """Refusals before any work: sharded contexts, likelihoods without a device form."""
        self._unsharded("model-selection criteria")
        return self._crit_family()

    def _crit_noise(self, results, S):
        """The per-sample noise variances of a result dict (None: the collected ones, or a likelihood without)."""
        if results is None or not self._crit_family()[2]:
            return None
        return check_scalars("results: nu2", results.get("nu2"), S, positive=False)

    def _crit_head(self, data, nsamples, Ws=None, Vs=None, noise=None, current=False):
        """The arguments btf_crit_eval and btf_crit_loo share - slot, family, parameter, samples, noise, flags - and the
        observed-curve mask of the slot."""
        family, param, per_sample = self._crit_check()
        slot, obs = self._crit_slot(data, family, param)
        flags = (_native.CRIT_NOISE_PER_SAMPLE if per_sample else 0) | (_native.CRIT_CURRENT if current else 0)
        noise = _native.as_f64(np.reshape(noise, -1)) if (per_sample and noise is not None) else None
        Ws = None if Ws is None else _native.as_f64(Ws)
        Vs = None if Vs is None else _native.as_f64(Vs)
        return (slot, int(family), float(param if param is not None else 0.0), int(nsamples), _native.dptr(Ws), _native.dptr(Vs),
                _native.dptr(noise), flags), obs

    def _crit_eval(self, data, nsamples, Ws=None, Vs=None, noise=None, current=False, pointwise=False):
        head, obs = self._crit_head(data, nsamples, Ws, Vs, noise, current)
        curve, totals, pw = _criteria.evaluate(self._ctx, head, (self.nrows, self.ncols), pointwise)
        return curve, totals, obs, pw

    def information_criteria(self, results=None, data=None, pointwise=False):
        """WAIC and DIC of the posterior samples, from the per-curve log-likelihood (csrc/btf_criteria.h; replaces the
        scoring of _BayesianModel.select_hyperparams_DIC, genlasso.py:69-136, and doseresponse/select_btf.py:9-23).

        results: a run_gibbs result dict (W (S,N,K), V (S,M,T,K); Gaussian: nu2 (S,1)), uploaded; None: the samples the
            last device-collecting run_gibbs left on the device (no upload).
        data: the observations to score; None: the data the model is bound to.  Another tensor of the same shape scores
            held-out observations (NaN everywhere else): `lppd` is then their log pointwise predictive density.

        The pointwise unit is the curve (i,j): ll_s(i,j) = the normalised log-likelihood of all observed y_ijtr of the
        curve under sample s.  Curves without observations count 0 and are left out of n_curves.
            lppd_ij = logsumexp_s ll_s(i,j) - log S        p_waic_ij = var_s ll_s(i,j) (ddof 1; 0 when S = 1)
            elpd_waic = sum (lppd_ij - p_waic_ij),  waic = -2 elpd_waic,  waic_se = 2 sqrt(n_curves var_ij(lppd - p_waic))
            mean_deviance = -2 mean_s sum_ij ll_s,   deviance_at_mean = -2 sum_ij ll(Mu-bar, theta-bar)
            p_dic = mean_deviance - deviance_at_mean,   dic = mean_deviance + p_dic
        Mu-bar_ijt = mean_s w_i^s . v_jt^s is the posterior mean of the product, NOT W-bar V-bar': W and V are identified
        only up to rotation and sign between samples, so their means are meaningless (doseresponse/select_btf.py plugs in
        the mean of W V' too).  theta-bar: the mean sampled nu2 (Gaussian), the fixed likelihood_param otherwise.
        A -inf sample (poisson_identity where w.v <= 0) follows scipy.special.logsumexp / np.var: that curve's p_waic is nan.

        Returns a dict with waic, elpd_waic, p_waic, lppd, waic_se, dic, p_dic, mean_deviance, deviance_at_mean,
        n_curves, nsamples, loglik_per_sample (S,) and curves = {lppd, p_waic, mean_ll, ll_at_mean} of (N,M) arrays;
        pointwise=True adds loglik (S,N,M), the full matrix (S*N*M doubles of host memory; PSIS-LOO from it stays on the
        device: loo()).
        A gamma_grid model is refused here (NotImplementedError): gamma_grid_criteria / gamma_grid_loo score it; so is the
        Negative-Binomial model with its sampled rate: negbin_criteria / negbin_loo.
        Device memory: the criteria statistics, 16 B per cell (functionalmf_amd/criteria.py), and 8 B per cell of scratch."""
        self._crit_check()
        S, Ws, Vs = self._samples(results)
        curve, totals, obs, pw = self._crit_eval(data, S, Ws, Vs, self._crit_noise(results, S), pointwise=pointwise)
        return _criteria.combine(curve, totals, obs, pw)

    def loo(self, results=None, data=None, r_eff=None, mean=False, transform=None, log_weights=False):
        """PSIS-LOO: Pareto-smoothed importance-sampling leave-one-curve-out (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson,
        Gelman, Yao, Gabry 2024) on the GPU (csrc/btf_loo.h); functionalmf_amd.criteria.psis_curve is its written definition.

        results, data: as information_criteria, with the same pointwise unit: the curve (i,j) = all observed y_ijtr over
            depth and replicates; curves without observations count 0 and are left out.
        r_eff: the relative efficiency of the draws, None (1), a scalar or (N,M); finite and > 0.  It sets the number of
            largest importance ratios the Pareto fit uses, min(floor(0.2 S), ceil(3 sqrt(S / r_eff))).
        mean: also return the leave-curve-out fitted curve, mean (N,M,T) = sum_s w_s(i,j) f(w_i^s . v_jt^s) with the smoothed
            normalised weights - what the model predicts for (i,j) had it not seen that curve; transform: f, as
            posterior_summary (None / "identity", "ilogit", "square").
        log_weights: also return the normalised log weights (S,N,M) (S*N*M doubles of host memory).

        Returns a dict: elpd_loo = sum_ij elpd_loo_ij, p_loo = sum (lppd_ij - elpd_loo_ij), looic = -2 elpd_loo,
        se = sqrt(n_curves var_ij elpd_loo_ij), n_curves, nsamples, good_k = min(1 - 1 / log10(S), 0.7), n_bad = the curves
        with pareto_k > good_k (their elpd_loo_ij is not to be trusted), observed (N,M) bool, curves = {elpd_loo, p_loo, pareto_k, lppd} of (N,M)
        arrays (0 for unobserved curves; pareto_k: nan there).  pareto_k = inf: no Pareto fit (S < 25, or every ratio of
        the curve equal) and the unsmoothed estimate.  A curve with a -inf sample (poisson_identity where w.v <= 0) has
        elpd_loo = -inf and pareto_k = inf, one with a nan sample nan; both have nan log weights and mean.
        S <= 4096.  Device memory for the call's duration: 8 S N M bytes (1.05 GB at (512,256,64), S = 1000) beside the
        criteria statistics.  criteria.compare(a, b) gives the paired elpd difference of two models' results."""
        self._crit_check()
        code = transform_code(transform)
        shape = (self.nrows, self.ncols, self.ndepth)
        r_eff = check_r_eff(r_eff, shape[:2])
        S, Ws, Vs = self._samples(results)
        noise = self._crit_noise(results, S)
        check_loo_samples(S)
        head, obs = self._crit_head(data, S, Ws, Vs, noise)
        return _criteria.loo_evaluate(self._ctx, head, shape, obs, r_eff=r_eff, transform=code, mean=mean, log_weights=log_weights)

    # ---- posterior predictive: replicated observations, bands, coverage, scores (functionalmf_amd/predictive.py) ----
    def posterior_predictive(self, results=None, data=None, q=(2.5, 97.5), draws_per_sample=1, seed=None, trials=None,
                             cells=None):
        """Posterior predictive of the observations on the GPU (csrc/btf_predict.h): for every cell (i,j,t), kept sample s
        and r < draws_per_sample a replicated observation y_rep ~ p(y | w_i^s . v_jt^s, theta_s), reduced on the device.
        What flutrends/benchmark.py:60-75, :129-134 and politics/benchmark.py:147-172 compute on the host.

        results: a run_gibbs result dict (W, V; Gaussian: nu2; Negative-Binomial: R, else the current rate), uploaded;
            None: the samples the last device-collecting run_gibbs left on the device (no upload).
        data: the observations to compare with; None: the data the model is bound to (nothing, if none is bound).  Another
            tensor of the same shape (NaN elsewhere) scores held-out observations, as information_criteria(data=).
        q: percentiles of the draws; coverage is that of the interval [q[0], q[-1]].
        seed: None takes the model's next device seed (the model's draw counter moves on by one, as for any device draw);
            an integer leaves the model untouched, and two calls with it return identical bits.
        trials: (N,M,T) Binomial trial counts for the draws; None: the N of the (Y, N) data pair (1 for Bernoulli tensors).
        cells: flat indices or (i,j,t) triples of cells whose raw draws come back as `draws` (ncells, S * draws_per_sample).

        Returns a dict: mean = mean_s E[y | theta_s]; y_mean, y_var (ddof 1) of the draws; quantiles (len(q),N,M,T); with
        data: pit_lo / pit_hi (fraction of draws < y / <= y, averaged over the cell's observed replicates), inside and nobs
        (observed replicates inside the interval / observed), rmse and mae (S,) of y - E[y | theta_s] over all observed y,
        coverage = inside.sum() / nobs.sum(); nominal = (q[-1] - q[0]) / 100, nsamples, ndraws.
        S * draws_per_sample <= 16384; unsharded models; gamma_grid and Python-callable likelihoods are not supported."""
        from . import predictive as _pred
        family, param, per_sample = self._pred_family()
        self._unsharded("posterior predictive")
        S, Ws, Vs = self._samples(results)
        S, R = _pred.check_draws(S, draws_per_sample)
        aux, flags = self._pred_aux(results, S) if per_sample else (None, 0)
        if data is None:
            data = getattr(self, "_data_ref", None)
        Y = data
        if isinstance(data, (tuple, list)):               # Binomial (Y, N): successes of N trials
            Y = data[0]
            if trials is None:
                trials = data[1]
        if seed is None:
            seed = self._next_seed()
        return _pred.evaluate(self._ctx, (self.nrows, self.ncols, self.ndepth), self.nembeds, family, S, Ws, Vs, param=param,
                              aux=aux, aux_flags=flags, trials=trials, Y=Y, q=q, draws_per_sample=R, seed=seed, cells=cells)

    # ---- posterior predictive checks: predictive p-values of whole-curve discrepancies (functionalmf_amd/checks.py) ----
    def posterior_checks(self, results=None, data=None, which=None, reps=1, seed=None, trials=None, curves=None):
        """Posterior predictive checks on the GPU (csrc/btf_checks.h): is a statistic of a whole observed curve plausible
        among the same statistic of curves replicated from the fitted model?  For every curve (i,j), kept sample s and
        rho < reps a replicated curve y_rep ~ p(y | theta_s) is drawn at the curve's observed slots and compared with the
        data through T(y_rep, theta_s) >= T(y, theta_s); functionalmf_amd.checks is the written definition.

        results, data, seed, trials: as posterior_predictive (data is required: the bound data, another tensor, a (Y, N) pair).
        which: names of checks.DISCREPANCIES - "chisq" (dispersion), "max", "lag1" (residual correlation along depth: over-
            or under-smoothing), "total", "zeros"; None: all five for the count families, the first four for Gaussian.
        reps: replicated data sets per kept sample; there are nsets = S * reps of them, and no limit on their number.
        curves: flat indices i * ncols + j or (i,j) pairs of curves whose raw T values come back.

        Returns a dict: for each requested name a dict of (N,M) arrays p_ge, p_gt (the share of the sets with T_rep >= / >
        T_obs among the `defined` ones), defined, t_obs, t_rep (the means of both sides); nobs (N,M); overall[name] = p_ge,
        p_gt, defined, T_obs (S,), T_rep (nsets,) of the discrepancy pooled over all curves; with curves: curves = {index
        (L,2), T_obs (L,nwhich,S), T_rep (L,nwhich,nsets)}; which, nsamples, reps, nsets, ndraws, seed.  Curves without
        observations and curves with a slot nothing can be drawn at are nan and left out of the pool.
        checks.two_sided(p_ge, p_gt) gives a two-sided p-value.  The sampler's state is not touched.  Unsharded models;
        gamma_grid and Python-callable likelihoods are not supported."""
        from . import checks as _checks
        family, param, per_sample = self._pred_family()
        self._unsharded("posterior checks")
        shape = (self.nrows, self.ncols, self.ndepth)
        codes = _checks.check_which(which, family)
        if data is None:
            data = getattr(self, "_data_ref", None)
        Y = data
        if isinstance(data, (tuple, list)):               # Binomial (Y, N): successes of N trials
            Y = data[0]
            if trials is None:
                trials = data[1]
        Y4 = _checks.check_data(Y, shape)
        _checks.check_curves(curves, shape)
        S, Ws, Vs = self._samples(results)
        S, reps = _checks.check_reps(S, reps, Y4.shape[3])
        aux, flags = self._pred_aux(results, S) if per_sample else (None, 0)
        if seed is None:
            seed = self._next_seed()
        return _checks.evaluate(self._ctx, shape, self.nembeds, family, S, Ws, Vs, param=param, aux=aux, aux_flags=flags,
                                trials=trials, Y=Y4, which=codes, reps=reps, seed=seed, curves=curves)

    # ---- posterior curve functionals: AUC, peak, level crossing (functionalmf_amd/functionals.py) ----
    def posterior_functionals(self, results=None, which=("auc",), q=(5, 95), transform=None, x=None, level=None, exceed=None,
                              curves=None, pointwise=False):
        """Per-curve functionals of f(w_i . v_j,:) over depth - area under the curve, maximum / minimum and where they lie,
        total rise, the first crossing of a level - summarised over the kept samples on the GPU (csrc/btf_functionals.h).
        What doseresponse/feature_importance.py:40 computes from the (S,N,M,T) tensor on the host.

        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        The other arguments and the returned dict: functionalmf_amd.utils.posterior_functionals.  The sampler's state is not
        touched: a chain continued after the call walks the same path.  Unsharded models."""
        from . import functionals as _func
        self._unsharded("posterior functionals")
        shape = (self.nrows, self.ncols, self.ndepth)
        if results is not None:                            # a bad argument is reported before a malformed results
            _func.check_args(which, q, transform, x, level, exceed, curves, 1, *shape)
        S, Ws, Vs = self._samples(results)
        return _func.evaluate(shape, self.nembeds, S, which=which, q=q, transform=transform, x=x, level=level, exceed=exceed,
                              curves=curves, pointwise=pointwise, ctx=self._ctx, Ws=Ws, Vs=Vs, device=self._ctx.device)

    # ---- simultaneous credible bands: the band that holds the whole curve (functionalmf_amd/bands.py) ----
    def posterior_bands(self, results=None, method="supt", level=95, depths=None, transform=None, curves=None, truth=None,
                        _scratch_bytes=0):
        """A band around every fitted curve f(w_i . v_j,:) that holds the WHOLE curve over depth with probability level / 100
        among the kept samples, on the GPU (csrc/btf_bands.h) - where the percentiles of posterior_summary hold each cell
        alone, and the curve as a whole far less often.

        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        The other arguments and the returned dict: functionalmf_amd.utils.posterior_bands.  The sampler's state is not
        touched: a chain continued after the call walks the same path.  Unsharded models."""
        from . import bands as _bands
        self._unsharded("posterior bands")
        shape = (self.nrows, self.ncols, self.ndepth)
        _bands.check_args(method, level, depths, transform, curves, truth, 2, *shape)
        S, Ws, Vs = self._samples(results)
        return _bands.evaluate(shape, self.nembeds, S, method=method, level=level, depths=depths, transform=transform, curves=curves,
                               truth=truth, ctx=self._ctx, Ws=Ws, Vs=Vs, device=self._ctx.device, _scratch_bytes=_scratch_bytes)

    # ---- posterior ranking: which column is best for a row, with what probability (functionalmf_amd/ranking.py) ----
    def posterior_ranking(self, which="auc", along="cols", order="ascending", top=(1, 5), transform=None, x=None, level=None,
                          pairs=None, pointwise=False, results=None):
        """The rank of every curve within its row (along="cols": the columns of a row are ranked) or its column
        (along="rows") by one functional of posterior_functionals, per kept sample, summarised over the samples on the GPU
        (csrc/btf_ranking.h): expected rank, its variance and the probability of being among the best k.  A property of the
        joint posterior across curves, which the per-curve summaries of posterior_functionals cannot give.

        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        The other arguments and the returned dict: functionalmf_amd.utils.posterior_ranking.  The sampler's state is not
        touched: a chain continued after the call walks the same path.  Unsharded models."""
        from . import ranking as _rank
        self._unsharded("posterior ranking")
        shape = (self.nrows, self.ncols, self.ndepth)
        _rank.check_args(which, along, order, top, transform, x, level, pairs, 1, *shape)
        S, Ws, Vs = self._samples(results)
        return _rank.evaluate(shape, self.nembeds, S, which=which, along=along, order=order, top=top, transform=transform, x=x,
                              level=level, pairs=pairs, pointwise=pointwise, ctx=self._ctx, Ws=Ws, Vs=Vs, device=self._ctx.device)

    # ---- posterior similarity: which rows or columns are alike (functionalmf_amd/similarity.py) ----
    def posterior_similarity(self, results=None, along="rows", metric="rms", over=None, q=(5, 95), nearest=(1, 5), pairs=None,
                             pointwise=False, _scratch_bytes=0):
        """The distance between the fitted surfaces of every two rows (along="rows") or columns (along="cols") per kept
        sample, summarised over the samples, and every entity's neighbours with their probabilities, on the GPU
        (csrc/btf_similarity.h).  The posterior form of the embedding scatter of doseresponse/plot_embeddings.py: invariant
        under the K x K map the embeddings are identified up to.

        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        The other arguments and the returned dict: functionalmf_amd.utils.posterior_similarity.  The sampler's state is not
        touched: a chain continued after the call walks the same path.  Unsharded models."""
        from . import similarity as _sim
        self._unsharded("posterior similarity")
        shape = (self.nrows, self.ncols, self.ndepth)
        _sim.check_args(along, metric, over, q, nearest, pairs, False, 1, *shape, self.nembeds)
        S, Ws, Vs = self._samples(results)
        return _sim.evaluate(shape, self.nembeds, S, along=along, metric=metric, over=over, q=q, nearest=nearest, pairs=pairs,
                             pointwise=pointwise, ctx=self._ctx, Ws=Ws, Vs=Vs, device=self._ctx.device,
                             _scratch_bytes=_scratch_bytes)

    # ---- posterior feature association: which biomarker goes with which drug (functionalmf_amd/association.py) ----
    def posterior_feature_association(self, U=None, results=None, which="auc", stats=("r",), q=(5, 95), transform=None, x=None,
                                      level=None, pairs=None, of_means=True):
        """The association across the rows between every row feature's probability w_i . u_f and one functional of
        posterior_functionals of every column's curves - correlation and regression slope per kept sample, summarised over
        the samples on the GPU (csrc/btf_assoc.h) - and the plug-in table doseresponse/feature_importance.py:39-54 computes
        from posterior means.

        U: the sampled feature embeddings (S,F,nembeds), one per kept sample; None: results["U"] (run_gibbs returns it for a
            model with row_features= and sample_features=True; it stays on the host, so it is uploaded either way).
        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        The other arguments and the returned dict: functionalmf_amd.utils.posterior_feature_association.  The sampler's
        state is not touched: a chain continued after the call walks the same path.  Unsharded models."""
        from . import association as _assoc
        self._unsharded("posterior feature association")
        shape = (self.nrows, self.ncols, self.ndepth)
        if U is None and results is not None:
            try:
                U = results["U"] if "U" in results else None
            except TypeError:
                raise ValueError("results must be a run_gibbs result dict")
        U = _assoc.check_features(U, K=self.nembeds)
        _assoc.check_args(which, stats, q, transform, x, level, pairs, 1, shape[1], shape[2], U.shape[1])
        S, Ws, Vs = self._samples(results)
        U = _assoc.check_features(U, S, self.nembeds)        # one embedding per kept sample
        return _assoc.evaluate(shape, self.nembeds, S, U, which=which, stats=stats, q=q, transform=transform, x=x, level=level,
                               pairs=pairs, of_means=of_means, ctx=self._ctx, Ws=Ws, Vs=Vs, device=self._ctx.device)

    # ---- monotone projection of the posterior: factor_pav of every kept sample (functionalmf_amd/monotone.py) ----
    def posterior_monotone(self, results=None, q=(5, 95), transform=None, increasing=False, return_V=False, in_place=False):
        """Project every kept sample to monotone curves on the GPU (csrc/btf_monotone.h): V'_s[j] = factor_pav(W_s, V_s[j])
        for every sample and column in one launch, and the mean and percentiles of f(W_s V'_s) from the summary kernel on the
        projected states where they lie.  What doseresponse/fit.py:365-374 does on the host, sample by sample.

        results: a run_gibbs result dict (W, V), uploaded; None: the samples the last device-collecting run_gibbs left on
            the device (no upload).
        q, transform: as posterior_summary; q=None: no summary.  increasing: no curve may decrease (-factor_pav(W, -V)).
        return_V: also return the projected samples V (S,M,T,K); dict(W=res["W"], V=out["V"]) is a results= for every
            other analysis call.
        in_place: (results=None only; ValueError otherwise) overwrite the device-collected V samples with their
            projection, without a second copy of them.  Every later analysis call on the collected samples -
            posterior_summary, posterior_functionals, posterior_ranking, posterior_feature_association,
            information_criteria, loo - then sees the projected posterior: the btf_mono route of select_btf.py.  THIS
            CANNOT BE UNDONE: the unprojected samples on the device are gone (the host dict run_gibbs returned is not
            touched, and the next collecting run_gibbs starts a fresh, unprojected set).

        The returned dict: functionalmf_amd.utils.posterior_monotone.  The sampler's state is not touched: a chain continued
        after the call walks the same path.  Works for every model class (it needs only W and V).  Unsharded models."""
        from . import monotone as _mono
        self._unsharded("posterior monotone")
        _mono.check_args(q, transform, increasing, return_V, in_place, self.ndepth, self.nembeds, uploaded=results is not None)
        S, Ws, Vs = self._samples(results)
        return _mono.evaluate((self.nrows, self.ncols, self.ndepth), self.nembeds, S, q=q, transform=transform,
                              increasing=increasing, return_V=return_V, in_place=in_place, ctx=self._ctx, Ws=Ws, Vs=Vs)

    # ---- folding new rows in (functionalmf_amd/fold_in.py, csrc/btf_fold_in.h) ----
    def fold_in_rows(self, Y_new, results=None, seed=None, z=None, summary=True, q=(5, 95), transform=None, inner_sweeps=None,
                     trials=None):
        """Embeddings and curves of rows the chain never saw (a new cell line with a handful of drugs tested, a new
        season), with uncertainty, on the GPU (csrc/btf_fold_in.h).  Given V the rows of W are conditionally independent
        with prior N(0, sigma2 I) (factor.py:333), so under kept sample s the new row has the conditional _resample_W
        draws from (factor.py:333-362), and one draw per kept sample is a draw from p(w_new | y_new, training data).
        Exact for the Gaussian model; the Binomial model runs `inner_sweeps` Polya-Gamma rounds per (sample, row) from
        w = 0 (factor.py:437-460; default: functionalmf_amd.fold_in.DEFAULT_INNER_SWEEPS).

        Y_new: (R,M,T) or (R,M,T,nreps), NaN = missing; Binomial: the (Y, N) pair, or Y with trials= (default 1), counts
            up to 32.  A row with no observation at all is allowed: its draw is the prior's.
        results: a run_gibbs result dict (V (S,M,T,K), sigma2 one value per sample, Gaussian nu2 likewise), uploaded; None:
            the samples the last device-collecting run_gibbs left on the device - no upload of V, and nu2_s, sigma2_s are read
            from the collected scalars.
        seed: None takes the model's next device seed (the model's draw counter moves on by one, as for any device draw);
            an integer leaves the model untouched, and two calls with it return identical bits.
        z: optional (S,R,K) standard normals replacing the device generator (Gaussian only): w = Q^-1 b + L^-T z, Q = L L'.

        Returns a dict: W (S,R,K) one draw per kept sample; W_mean (S,R,K) the conditional means Q_s^-1 b_s (Gaussian
        only); with summary=True, mean (R,M,T) and quantiles (len(q),R,M,T) of f(w_new^s . v_jt^s) from the summary kernel
        on the device-resident W and V (transform as posterior_summary; at most 16384 samples); nsamples.  out["W"] together
        with results["V"] goes straight into utils.posterior_summary, utils.posterior_predictive and
        utils.posterior_functionals.  The sampler's state is not touched: a chain continued after the call walks the same
        path.  Unsharded models.  New COLUMNS are folded in by fold_in_cols, which samples the horseshoe local scales of
        the new column in a short chain of its own."""
        from . import fold_in as _fold
        family = self._fold_family()
        self._unsharded("fold_in_rows")
        M, T, K = self.ncols, self.ndepth, self.nembeds
        R, weights, sums = _fold.row_statistics(Y_new, family, M, T, trials=trials)
        S, _, Vs = self._samples(results, need=("V",))
        _fold.check_args(family, S, R, K, z, summary, q, transform, inner_sweeps)
        nu2 = sigma2 = None
        if results is not None:
            sigma2 = check_scalars("results: sigma2", results.get("sigma2"), S)
            if _fold.FAMILIES[family] == _fold.FAMILIES["gaussian"]:
                nu2 = check_scalars("results: nu2", results.get("nu2"), S)
        if seed is None:
            seed = self._next_seed() if z is None else 0
        return _fold.evaluate(family, S, R, M, T, K, weights, sums, z=z, seed=seed, summary=summary, q=q, transform=transform,
                              inner_sweeps=inner_sweeps, ctx=self._ctx, Vs=Vs, nu2=nu2, sigma2=sigma2, device=self._ctx.device)

    # ---- folding new columns in (functionalmf_amd/fold_in_cols.py, csrc/btf_fold_in_cols.h) ----
    def fold_in_cols(self, Y_new, results=None, seed=None, draws=None, sweeps=None, summary=True, q=(5, 95), transform=None,
                     trials=None, first_sample=0):
        """Curves of columns the chain never saw (a new drug tested on a handful of the fitted cell lines) for every row,
        with uncertainty, on the GPU (csrc/btf_fold_in_cols.h).  Given W the columns of V are conditionally independent
        (factor.py:378), and given a kept sample's W_s, nu2_s and lam2_s the new column's curve and its horseshoe+ levels
        form a small Gibbs chain: `sweeps` rounds (default: functionalmf_amd.fold_in_cols.DEFAULT_SWEEPS) of the
        conditionals of _resample_V (factor.py:378-409) and _resample_Tau2 (factor.py:136-141) for that one column, from
        the prior draw of the levels.  One chain per (kept sample, new column); its last state is a draw from
        p(V_c | y_c, W_s, nu2_s, lam2_s) up to the chain's finite length.  As in fold_in_rows the new data does not inform
        W or the hyper-parameters.  The Binomial model opens every round with Polya-Gamma draws from the current curve,
        starting at v = 0 (factor.py:437-460).  functionalmf_amd.fold_in_cols.chain is the definition in numpy.

        Y_new: (C,N,T) or (C,N,T,nreps), NaN = missing; Binomial: the (Y, N) pair, or Y with trials= (default 1), counts
            up to 32.  A column with no observation at all is allowed: its chain is the prior's.
        results: a run_gibbs result dict (W (S,N,K), lam2 one value per sample, Gaussian nu2 likewise), uploaded; None: the
            samples the last device-collecting run_gibbs left on the device - no upload of W, and nu2_s, lam2_s are read
            from the collected scalars.
        seed: None takes the model's next device seed (the model's draw counter moves on by one, as for any device draw);
            an integer leaves the model untouched, and two calls with it return identical bits.
        draws: optional (S,C,4 nD + sweeps (T K + 4 nD)) variates replacing the device generator (Gaussian only), per chain
            in the layout of fold_in_cols.chain (fold_in_cols.random_draws builds one).
        first_sample: the index of the first sample among the kept ones - with it a call over a slice of the samples
            returns the bits of the whole call.

        Returns a dict: V (S,C,T,K) one draw per kept sample; V_mean (S,C,T,K) the last conditional means (Gaussian only);
        Tau2 (S,C,nD) the last local scales; with summary=True, mean (N,C,T) and quantiles (len(q),N,C,T) of
        f(w_i^s . v_ct^s) from the summary kernel on the device-resident W and new V (transform as posterior_summary; at
        most 16384 samples); nsamples.  results["W"] together with out["V"] goes straight into utils.posterior_summary,
        utils.posterior_predictive and utils.posterior_functionals.  The sampler's state is not touched: a chain continued
        after the call walks the same path.  Unsharded models.  A band of Q beyond one workgroup's LDS
        (fold_in_cols.lds_bytes > LDS_LIMIT) is refused with ValueError."""
        from . import fold_in_cols as _fc
        family = self._fold_cols_family()
        self._unsharded("fold_in_cols")
        N, T, K = self.nrows, self.ndepth, self.nembeds
        C, weights, sums = _fc.column_statistics(Y_new, family, N, T, trials=trials)
        S, Ws, _ = self._samples(results, need=("W", "V")) if results is None else self._fold_cols_W(results)
        _fc.check_args(family, S, C, T, K, self.tf_order, draws, sweeps, summary, q, transform, first_sample)
        nu2 = lam2 = None
        if results is not None:
            lam2 = check_scalars("results: lam2", results.get("lam2"), S)
            if _fc.FAMILIES[family] == _fc.FAMILIES["gaussian"]:
                nu2 = check_scalars("results: nu2", results.get("nu2"), S)
        if seed is None:
            seed = self._next_seed() if draws is None else 0
        return _fc.evaluate(family, S, C, N, T, K, self.tf_order, weights, sums, draws=draws, seed=seed, sweeps=sweeps,
                            summary=summary, q=q, transform=transform, first_sample=first_sample, stability=float(self.stability),
                            ctx=self._ctx, Ws=Ws, nu2=nu2, lam2=lam2, device=self._ctx.device)

    def _fold_cols_W(self, results):
        """(S, Ws, None) of a result dict for fold_in_cols: W alone is needed, checked against the model."""
        try:
            Ws = _native.as_f64(results["W"])
        except (KeyError, TypeError):
            raise ValueError("results must be a run_gibbs result dict with W (S,N,K)")
        if Ws.ndim != 3 or Ws.shape[0] < 1 or Ws.shape[1:] != (self.nrows, self.nembeds):
            raise ValueError("results: Ws must be (S,%d,%d), got %r" % (self.nrows, self.nembeds, Ws.shape))
        return Ws.shape[0], Ws, None

    # ---- folding new depth slices in (functionalmf_amd/fold_in_depth.py, csrc/btf_fold_in_depth.h) ----
    def fold_in_depth(self, Y_new, horizon=None, results=None, seed=None, draws=None, sweeps=None, summary=True, q=(5, 95),
                      transform=None, trials=None, first_sample=0):
        """Curves of every fitted column at depths the chain never saw (new weeks of a series, a new dose), for every row,
        with uncertainty, on the GPU (csrc/btf_fold_in_depth.h) and without another burn-in.  The trend-filtering prior
        couples a new depth with the last tf_order + 1 kept depths of its column through penalty rows whose horseshoe+
        local scales nobody has sampled; given a kept sample's W_s, V_s[j], nu2_s and lam2_s the H new depths of column j
        and the scales of those rows form a small Gibbs chain: `sweeps` rounds (default:
        functionalmf_amd.fold_in_depth.DEFAULT_SWEEPS) from the prior draw of the levels, one chain per (kept sample,
        fitted column).  functionalmf_amd.fold_in_depth.chain is the definition in numpy.  The new data does not inform W,
        the kept depths (the past is not smoothed) or the hyper-parameters; the new depths continue the fitted grid at
        its spacing.  The Binomial model opens every round with Polya-Gamma draws from the current curve, starting at the
        last kept depth.

        Y_new: (N,M,H) or (N,M,H,nreps), NaN = missing; Binomial: the (Y, N) pair, or Y with trials= (default 1), counts
            up to 32.  A column slice with no observation at all is allowed.  Y_new=None with horizon=H is the model's
            FORECAST: no data at all, every chain runs on the prior given the kept curve (sweeps=1 is then an exact draw).
            The forecast is honest but weak - fresh local scales on the low-order rows shrink the continuation towards
            flat, and its curves are heavy-tailed: folding in even a few observed rows is what the call is for.
        results: a run_gibbs result dict (W (S,N,K), V (S,M,T,K), lam2 one value per sample, Gaussian nu2 likewise),
            uploaded (of V only the last min(T, tf_order + 1) depths); None: the samples the last device-collecting
            run_gibbs left on the device - nothing but the new data is uploaded.
        seed: None takes the model's next device seed (the model's draw counter moves on by one, as for any device draw);
            an integer leaves the model untouched, and two calls with it return identical bits.
        draws: optional (S,M,4 nR + sweeps (H K + 4 nR)) variates replacing the device generator (Gaussian only), per chain
            in the layout of fold_in_depth.chain (fold_in_depth.random_draws builds one).
        first_sample: the index of the first sample among the kept ones - with it a call over a slice of the samples
            returns the bits of the whole call.

        Returns a dict: V (S,M,H,K) one draw per kept sample; V_mean (S,M,H,K) the last conditional means (Gaussian only);
        Tau2 (S,M,nR) the last local scales of the new penalty rows; with summary=True, mean (N,M,H) and quantiles
        (len(q),N,M,H) of f(w_i^s . v_jt^s) from the summary kernel on the device-resident W and new V (transform as
        posterior_summary; at most 16384 samples); nsamples.  np.concatenate([results["V"], out["V"]], axis=2) with
        results["W"] goes straight into utils.posterior_summary, utils.posterior_predictive and
        utils.posterior_functionals.  The sampler's state is not touched: a chain continued after the call walks the same
        path.  Unsharded models.  A band beyond one workgroup's LDS (fold_in_depth.lds_bytes > LDS_LIMIT) is refused with
        ValueError."""
        from . import fold_in_depth as _fd
        family = self._fold_depth_family()
        self._unsharded("fold_in_depth")
        N, M, T, K = self.nrows, self.ncols, self.ndepth, self.nembeds
        H, weights, sums = _fd.slice_statistics(Y_new, family, N, M, trials=trials, horizon=horizon)
        S, Ws, Vs = self._samples(results)
        _fd.check_args(family, S, M, T, H, K, self.tf_order, draws, sweeps, summary, q, transform, first_sample)
        nu2 = lam2 = None
        if results is not None:
            lam2 = check_scalars("results: lam2", results.get("lam2"), S)
            if _fd.FAMILIES[family] == _fd.FAMILIES["gaussian"]:
                nu2 = check_scalars("results: nu2", results.get("nu2"), S)
        if seed is None:
            seed = self._next_seed() if draws is None else 0
        return _fd.evaluate(family, S, N, M, T, H, K, self.tf_order, weights, sums, draws=draws, seed=seed, sweeps=sweeps,
                            summary=summary, q=q, transform=transform, first_sample=first_sample, stability=float(self.stability),
                            ctx=self._ctx, Ws=Ws, Vs=Vs, nu2=nu2, lam2=lam2, device=self._ctx.device)

    def logprob(self, data, reduce="sum", **state):
        """Normalised log-likelihood of `data` under the current state, or under the state in W=, V= (and, Gaussian,
        nu2=); further keys (Tau2, lam2, sigma2, ...: what the reference's DIC passes) are ignored.  reduce="sum": a
        float; "curve": the (N,M) per-curve values (0 for curves without observations).  The criteria kernel with one sample.
        Deviation: the reference (factor.py:262-264, :610-612, :1002-1005) returns an elementwise array built from an
        undefined name, with sigma2 where the noise variance nu2 belongs."""
        from .factor import _scalar
        if reduce not in ("sum", "curve"):
            raise ValueError("reduce must be 'sum' or 'curve'")
        per_sample = self._crit_check()[2]
        W, V = state.get("W"), state.get("V")
        noise = None
        if per_sample:
            noise = np.array([_scalar(state["nu2"] if state.get("nu2") is not None else self.nu2)])
        if W is None and V is None and not (self._W_host_new or self._V_host_new):
            curve, totals, obs, _ = self._crit_eval(data, 1, noise=noise, current=True)       # the device's own W, V
        else:
            if W is None:
                self._pull_W()
                W = self._W
            if V is None:
                self._pull_V()
                V = self._V
            W, V = np.asarray(W, dtype=float), np.asarray(V, dtype=float)
            if W.shape != (self.nrows, self.nembeds) or V.shape != (self.ncols, self.ndepth, self.nembeds):
                raise ValueError("W %r / V %r do not match the model" % (W.shape, V.shape))
            curve, totals, obs, _ = self._crit_eval(data, 1, W[None], V[None], noise)
        if reduce == "sum":
            return float(totals[0])
        return np.where(obs, curve[2], 0.0)
