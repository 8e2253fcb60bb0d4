"""MCMC driver and the conjugate inverse-gamma update: counterpart of
functionalmf/genlasso.py:1-66 and :139-171 (same class and method names)."""
import numpy as np


class _BayesianModel(object):
    def __init__(self, **kwargs):
        # the reference swallows unknown kwargs here (genlasso.py:8), e.g. nthreads=1
        pass

    def resample(self, data, **kwargs):
        raise NotImplementedError

    def _inferred_variables(self, var_map):
        raise NotImplementedError

    def inferred_variables(self):
        """All non-nuisance parameters inferred by calling resample."""
        out = {}
        self._inferred_variables(out)
        return out

    def run_gibbs(self, data, nburn=1000, nthin=1, nsamples=1000, verbose=True, print_freq=100,
                  callback=None, **kwargs):
        """Burn in, then keep every `nthin`-th state.  Result layout as the reference
        (genlasso.py:51-65): dict of arrays [nsamples]+shape; scalars stored as [nsamples,1]."""
        results = None
        for step in range(nburn + nthin * nsamples):
            if verbose and step % print_freq == 0:
                print('\tStep {}'.format(step))
            self.resample(data, **kwargs)
            if callback is not None:
                callback(self, data, step, **kwargs)
            kept, rem = divmod(step - nburn, nthin)
            if step >= nburn and rem == 0:
                state = self.inferred_variables()
                if kept == 0:
                    results = {k: np.zeros([nsamples] + ([1] if np.isscalar(v) else list(v.shape)))
                               for k, v in state.items()}
                for k, v in state.items():
                    results[k][kept] = v
        return results

    def _default_hyperparam_options(self, hyperparams, lam2=None, min_lam2=1e-6, max_lam2=1e3, num_lam2=10, **kwargs):
        """The lam2 grid of the DIC search (factor.py:267-275, with the reference's undefined `lam` read as lam2):
        the caller's lam2 values, or num_lam2 log-spaced values from max_lam2 down to min_lam2."""
        if lam2 is None:
            hyperparams['lam2'] = np.exp(np.linspace(np.log(min_lam2), np.log(max_lam2), num_lam2))[::-1]
        else:
            hyperparams['lam2'] = np.atleast_1d(np.asarray(lam2, dtype=float))

    def _dic_score(self, results):
        """The score select_hyperparams_DIC gives a grid point's samples; a gamma_grid model scores through
        gamma_grid_criteria (factor.py)."""
        return self.information_criteria(results)["dic"]

    def select_hyperparams_DIC(self, data, verbose=True, **kwargs):
        """Grid search of the hyper-parameters by the deviance information criterion (genlasso.py:69-136, made to run):
        for every grid point the hyper-parameters are set, run_gibbs(data, verbose=False, **kwargs) continues the chain
        from where the previous point left it, and the point is scored by _dic_score(results): information_criteria(results)["dic"],
        for a gamma_grid model gamma_grid_criteria(results)["dic"]
        (DIC = 2 mean_s D(theta_s) - D(plug-in), D = -2 log-likelihood; see information_criteria).  The grid keywords
        (lam2, min_lam2, max_lam2, num_lam2) are taken off before run_gibbs.  The best point's values are left set.
        Returns {'scores', 'options', 'best', 'fit'}: the DIC per grid point, the grid, the best values and the best
        point's samples."""
        hyperparam_options = {}
        self._default_hyperparam_options(hyperparam_options, **kwargs)
        rest = {k: v for k, v in kwargs.items() if k not in ("lam2", "min_lam2", "max_lam2", "num_lam2")}
        if verbose:
            print('Grid search for hyperparameters:')
            for key, val in hyperparam_options.items():
                print('{}: {} values from {} to {}'.format(key, len(val), min(val), max(val)))
        param_names = list(hyperparam_options.keys())
        param_options = [hyperparam_options[name] for name in param_names]
        all_indices = list(np.ndindex(*[len(p) for p in param_options]))
        dic_scores = np.zeros(len(all_indices))
        best_results, best_idx = None, None
        for score_idx, indices in enumerate(all_indices):
            cur = {param_names[p]: param_options[p][v] for p, v in enumerate(indices)}
            if verbose:
                print(' '.join('{}={}'.format(k, v) for k, v in cur.items()))
            self._set_hyperparameters(cur)
            results = self.run_gibbs(data, verbose=False, **rest)
            dic_scores[score_idx] = self._dic_score(results)
            if best_idx is None or dic_scores[score_idx] < dic_scores[best_idx]:
                best_results, best_idx = results, score_idx
        best_options = {param_names[p]: param_options[p][v] for p, v in enumerate(all_indices[best_idx])}
        self._set_hyperparameters(best_options)
        return {'scores': dic_scores, 'options': hyperparam_options, 'best': best_options, 'fit': best_results}


class ConjugateInverseGammaPrior(object):
    """Gamma(shape, rate) prior on a shared precision of Gaussian observations."""

    def __init__(self, N, shape=0.1, rate=0.1):
        self.N = N
        self.shape = shape
        self.rate = rate

    def resample_from_stats(self, sqerr, nobs):
        """Posterior precision draw given the two sufficient statistics
        (genlasso.py:157-164): one legacy-RNG gamma, scale parameterisation."""
        prec = np.random.gamma(self.shape + nobs / 2, 1 / (self.rate + sqerr / 2))
        return prec if self.N == 1 else np.full(self.N, prec)

    def resample(self, data, **kwargs):
        means, obs = data
        means = np.atleast_1d(means)
        obs = np.atleast_1d(obs)
        seen = ~np.isnan(obs)
        return self.resample_from_stats(np.nansum((means - obs) ** 2), np.sum(seen))

    def draw_from_prior(self, size=1):
        return np.random.gamma(self.shape, 1 / self.rate, size=size)
