"""Host forms of the device likelihood families that carry a table.

GammaGridLikelihood is the dose-response likelihood of the reference (doseresponse/empirical_bayes.py:9-33): an
empirical-Bayes mixture of gammas over a grid of initial cell-population means.  The model classes evaluate it on the
device (loglikelihood="gamma_grid", csrc/btf_gamma_grid.h); this class holds the same table and a numpy `logpdf` for
tests, examples and checks, never on the sampling path.
"""
import numpy as np
from scipy.special import gammaln, logsumexp

GAMMA_GRID_MAX_COMPONENTS = 128


class GammaGridLikelihood:
    """Components g: shape = mean_g^2 / variance, scale = variance / mean_g, weight mean_probs[g] (used as given)."""

    def __init__(self, mean_grid, mean_probs, variance):
        mean_grid = np.asarray(mean_grid, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):        # (a zero mean: gamma_grid_table rejects the table)
            self.shape_grid = mean_grid ** 2 / variance
            self.scale_grid = variance / mean_grid
        self.probs_grid = np.asarray(mean_probs, dtype=np.float64)

    @classmethod
    def from_table(cls, shape, scale, prob):
        """The same class from its components directly (gamma_grid_table's output)."""
        self = cls.__new__(cls)
        self.shape_grid, self.scale_grid, self.probs_grid = (np.asarray(v, dtype=np.float64) for v in (shape, scale, prob))
        return self

    def logpdf(self, y, effect):
        """log sum_g p_g prod_r Gamma(y_r; shape_g, scale_g * effect) over the last axis of `y` (the replicates; NaN =
        missing), `effect` broadcasting against y with that axis of length 1 - the reference's signature
        (fit.py:37 passes WV[..., None]).  A cell without observations gives log sum_g p_g (the reference's nansum); an
        observed cell with effect <= 0 gives -inf (where the reference's nansum counts the NaN as unobserved)."""
        y = np.asarray(y, dtype=np.float64)
        if y.ndim < 2:
            raise ValueError("y needs a replicate axis (last)")
        eta = np.broadcast_to(np.asarray(effect, dtype=np.float64), y.shape[:-1] + (1,))[..., 0]
        obs = ~np.isnan(y)
        yo = np.where(obs, y, 1.0)
        S1 = np.where(obs, yo, 0.0).sum(axis=-1)
        L = np.where(obs, np.log(yo), 0.0).sum(axis=-1)
        cnt = obs.sum(axis=-1).astype(np.float64)
        a, s, p = self.shape_grid, self.scale_grid, self.probs_grid
        with np.errstate(divide="ignore", invalid="ignore"):
            le = np.log(np.where(eta > 0, eta, 1.0))[..., None]
            x = (S1 / np.where(eta > 0, eta, 1.0))[..., None]
            comp = (a - 1.0) * L[..., None] - x / s - cnt[..., None] * (a * (np.log(s) + le) + gammaln(a))
            out = logsumexp(comp, b=p, axis=-1)
        lsp = np.log(p.sum())
        out = np.where(cnt > 0, out, lsp)
        return np.where((cnt > 0) & ~(eta > 0), -np.inf, out)

    def sample(self, effect, size=1, rng=None):
        """Draws y = effect * scale_g * Gamma(shape_g, 1), the component g chosen with the weights probs_grid / sum - the
        numpy statement of the device draw (csrc/btf_gg_predict.h), for tests and examples, never on a device path.  The
        reference's sample (empirical_bayes.py:21-27) picks g by np.random.choice(G): uniformly, whatever mean_probs says;
        equal weights give that.  `size` as numpy's; `effect` broadcasts against it; one component per drawn value.
        effect <= 0 or nan gives nan.  rng: a np.random.RandomState / Generator (default: numpy's global state)."""
        rng = np.random if rng is None else rng
        a, s, p = gamma_grid_table(self)
        size = tuple(np.atleast_1d(size))
        effect = np.broadcast_to(np.asarray(effect, dtype=np.float64), size)
        g = rng.choice(a.size, size=size, p=p / p.sum())
        x = rng.gamma(a[g], 1.0, size=size)
        with np.errstate(invalid="ignore"):
            return np.where(effect > 0, effect * s[g] * x, np.nan)


def gamma_grid_table(param):
    """(shape, scale, prob) float64 arrays of `param`: a (mean_grid, mean_probs, variance) triple - the arguments of
    the reference's class - or any object with shape_grid, scale_grid, probs_grid attributes (the reference's own
    GammaGridLikelihood instance works unchanged).  ValueError for a table the device family rejects."""
    if all(hasattr(param, k) for k in ("shape_grid", "scale_grid", "probs_grid")):
        shape, scale, prob = param.shape_grid, param.scale_grid, param.probs_grid
    elif isinstance(param, (tuple, list)) and len(param) == 3:
        g = GammaGridLikelihood(*param)
        shape, scale, prob = g.shape_grid, g.scale_grid, g.probs_grid
    else:
        raise ValueError("likelihood_param for 'gamma_grid': (mean_grid, mean_probs, variance) or an object with "
                         "shape_grid, scale_grid and probs_grid")
    try:
        shape, scale, prob = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (shape, scale, prob))
    except (TypeError, ValueError) as e:
        raise ValueError("gamma grid: numeric arrays expected (%s)" % e)
    G = shape.size
    if scale.size != G or prob.size != G:
        raise ValueError("gamma grid: shape, scale and weights of different lengths")
    if not 1 <= G <= GAMMA_GRID_MAX_COMPONENTS:
        raise ValueError("gamma grid: 1..%d components, got %d" % (GAMMA_GRID_MAX_COMPONENTS, G))
    if not (np.all(np.isfinite(shape)) and np.all(np.isfinite(scale)) and np.all(np.isfinite(prob))):
        raise ValueError("gamma grid: non-finite entries")
    if not (np.all(shape > 0) and np.all(scale > 0)):
        raise ValueError("gamma grid: shapes and scales must be positive")
    if np.any(prob < 0) or not np.any(prob > 0):
        raise ValueError("gamma grid: weights must be >= 0 and not all zero")
    return shape, scale, prob
