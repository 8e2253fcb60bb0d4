"""Host-side helpers of the hot path: trend-filtering penalty and horseshoe
initial scales.  Counterpart of the slice of functionalmf/utils.py the path uses
(utils.py:56-124); same function names and return types."""
import numpy as np
from scipy.sparse import csc_matrix, diags, vstack, issparse


def get_1d_penalty_matrix(N):
    """(N-1) x N first-difference operator, sparse csc (utils.py:93-98)."""
    return diags([-np.ones(N - 1), np.ones(N - 1)], [0, 1], shape=(N - 1, N), format="csc")


def get_delta(D, k):
    """k-th order trend-filtering operator from the oriented incidence matrix
    (utils.py:56-64): alternate left-multiplication by D' and D."""
    if k < 0:
        raise Exception("k must be at least 0th order.")
    out = D
    for i in range(k):
        out = (D.T if i % 2 == 0 else D).dot(out)
    return out


def bayes_delta(D, K, anchor=0):
    """Stack an anchor row e_anchor' on top of the operators of order 0..K
    (utils.py:66-81)."""
    top = np.zeros((1, D.shape[1]))
    top[0, anchor] = 1
    blocks = [csc_matrix(top) if issparse(D) else top]
    blocks += [get_delta(D, k) for k in range(K + 1)]
    if issparse(D):
        return vstack(blocks).tocsc()
    return np.concatenate(blocks, axis=0)


def bayes_grid_penalty(dims, k, anchor=0):
    """Bayesian trend-filtering penalty for a 1-D grid of `dims` points
    (utils.py:83-90).  Multi-dimensional grids are outside the hot path."""
    if hasattr(dims, "__len__"):
        if len(dims) != 1:
            raise NotImplementedError("only 1-D depth grids are on the accelerated path")
        dims = dims[0]
    return bayes_delta(get_1d_penalty_matrix(int(dims)), k, anchor=anchor)


def ilogit(x):
    return 1 / (1 + np.exp(-x))


def mse(x, y):
    return np.nanmean((x - y) ** 2)


def mae(x, y):
    return np.nanmean(np.abs(x - y))


def sample_horseshoe_plus(size=1):
    """Four-level half-Cauchy scale mixture drawn as nested inverse gammas
    (utils.py:115-120); returns (tau2, c, b, a)."""
    a = 1 / np.random.gamma(0.5, 1, size=size)
    b = 1 / np.random.gamma(0.5, a)
    c = 1 / np.random.gamma(0.5, b)
    d = 1 / np.random.gamma(0.5, c)
    return d, c, b, a


def sample_horseshoe(size=1):
    """(utils.py:122-124)"""
    a = 1 / np.random.gamma(0.5, 1, size=size)
    return 1 / np.random.gamma(0.5, a), a


def posterior_summary(Ws, Vs, q=(5, 95), transform=None, device=0):
    """Mean and percentiles over the kept samples of f(w_s[i] . v_s[j,t]) for every cell, on the GPU.

    The reference's example scripts do this on the host
    (examples/gaussian_tensor_filtering.py:82-85):

        Mu_hat = np.einsum('znk,zmtk->znmt', Ws, Vs)        # (S, N, M, T): 67 GB at S=1000, (512,256,64)
        mean, lo, hi = Mu_hat.mean(0), np.percentile(Mu_hat, 5, axis=0), np.percentile(Mu_hat, 95, axis=0)

    Here the (S, N, M, T) tensor is never materialised (btf_posterior_summary: per-cell bitonic sort in
    LDS).  `transform`: None, "ilogit" (the Binomial examples) or "square".  Returns (mean, quantiles)
    with shapes (N, M, T) and (len(q), N, M, T); percentiles use numpy's default linear interpolation.
    There is no CPU fallback."""
    from . import _analysis, _native
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    M, T = Vs.shape[1:3]

    def call(*tail):
        lib = _native.load()
        _native.check(lib.btf_posterior_summary(int(device), S, N, M, T, K, _native.dptr(Ws), _native.dptr(Vs), *tail), lib)
    return _analysis.summary(call, (N, M, T), q, transform)


def posterior_predictive(Ws, Vs, family, data=None, q=(2.5, 97.5), draws_per_sample=1, seed=0, param=None, nu2=None, R=None,
                         trials=None, cells=None, device=0):
    """Posterior predictive of the observations from samples on the host, without a model: the stateless form of
    BayesianTensorFiltering.posterior_predictive (see there for the outputs), next to posterior_summary.

    Ws (S,N,K), Vs (S,M,T,K); family: "gaussian", "poisson", "poisson_identity", "binomial" or "negative_binomial".
    Gaussian: nu2 (S,) per-sample variances, or param = one variance; Negative-Binomial: R (S,) + a shape broadcasting
    against (N,M,T), or param = one rate; Binomial: trials (N,M,T) (default 1).  data: (N,M,T) or (N,M,T,R) observations
    with NaN = missing, or a Binomial (Y, N) pair.  Needs ndepth >= 2 (a context is opened for the call).  No CPU fallback."""
    from . import _analysis, _native, predictive
    Ws, Vs = _analysis.check_states(Ws, Vs)
    code = predictive.family_code(family)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    predictive.check_draws(S, draws_per_sample)
    aux, flags = None, 0
    if code == predictive.FAMILY_GAUSSIAN and nu2 is not None:
        aux, flags = np.asarray(nu2, dtype=float).reshape(S), _native.PRED_AUX_PER_SAMPLE
    elif code == predictive.FAMILY_NEGBIN and R is not None:
        aux, flags = predictive.rate_layout(R, S, shape)
    elif code in (predictive.FAMILY_GAUSSIAN, predictive.FAMILY_NEGBIN) and param is None:
        raise ValueError("the Gaussian family needs nu2= or param= (variance), the Negative-Binomial R= or param= (rate)")
    Y = data
    if isinstance(data, (tuple, list)):
        Y = data[0]
        trials = data[1] if trials is None else trials
    ctx = _native.Context(N, shape[1], shape[2], K, 0, device=device)
    try:
        return predictive.evaluate(ctx, shape, K, code, S, Ws, Vs, param=param, aux=aux, aux_flags=flags, trials=trials, Y=Y, q=q,
                                   draws_per_sample=draws_per_sample, seed=seed, cells=cells)
    finally:
        ctx.close()


def posterior_checks(Ws, Vs, family, data, which=None, reps=1, seed=0, param=None, nu2=None, R=None, trials=None, curves=None,
                     device=0, _chunk_rows=0):
    """Posterior predictive checks from samples on the host, without a model: the stateless form of
    BayesianTensorFiltering.posterior_checks (see there for `which`, `reps`, `curves` and the outputs; functionalmf_amd.checks
    is the written definition), beside posterior_predictive.

    Ws, Vs, family, param / nu2 / R, trials and data as posterior_predictive; data is required.  Needs ndepth >= 2 (a
    context is opened for the call).  No CPU fallback."""
    from . import _analysis, _native, checks, predictive
    Ws, Vs = _analysis.check_states(Ws, Vs)
    code = predictive.family_code(family)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    codes = checks.check_which(which, code)
    Y = data
    if isinstance(data, (tuple, list)):
        Y = data[0]
        trials = data[1] if trials is None else trials
    Y4 = checks.check_data(Y, shape)
    checks.check_reps(S, reps, Y4.shape[3])
    checks.check_curves(curves, shape)
    aux, flags = None, 0
    if code == predictive.FAMILY_GAUSSIAN and nu2 is not None:
        aux, flags = np.asarray(nu2, dtype=float).reshape(S), _native.PRED_AUX_PER_SAMPLE
    elif code == predictive.FAMILY_NEGBIN and R is not None:
        aux, flags = predictive.rate_layout(R, S, shape)
    elif code in (predictive.FAMILY_GAUSSIAN, predictive.FAMILY_NEGBIN) and param is None:
        raise ValueError("the Gaussian family needs nu2= or param= (variance), the Negative-Binomial R= or param= (rate)")
    ctx = _native.Context(N, shape[1], shape[2], K, 0, device=device)
    try:
        return checks.evaluate(ctx, shape, K, code, S, Ws, Vs, param=param, aux=aux, aux_flags=flags, trials=trials, Y=Y4, which=codes,
                               reps=reps, seed=seed, curves=curves, _chunk_rows=_chunk_rows)
    finally:
        ctx.close()


def _gamma_grid_context(Ws, Vs, Y, likelihood, device):
    """A context for one model-free gamma-grid criteria call: the table set, the statistics of Y in slot 0.  Returns
    (ctx, head of btf_crit_eval / btf_crit_loo, (N,M,T), observed-curve mask); the caller closes ctx."""
    from . import _analysis, _native, criteria, likelihoods
    table = likelihoods.gamma_grid_table(likelihood)               # (a bad table raises before any device call)
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    ctx = _native.Context(N, shape[1], shape[2], K, 0, device=device)
    try:
        ctx.call("btf_set_likelihood_table", criteria.FAMILY_GAMMA_GRID, *(_native.dptr(v) for v in table), int(table[0].size))
        obs = criteria.gamma_grid_upload(ctx, 0, Y, shape)
    except Exception:
        ctx.close()
        raise
    return ctx, criteria.gamma_grid_head(0, S, Ws, Vs), shape, obs


def gamma_grid_criteria(Ws, Vs, Y, likelihood, pointwise=False, device=0):
    """WAIC and DIC of saved samples under the gamma-grid likelihood on the GPU, without a model: the stateless form of
    NonconjugateBayesianTensorFiltering.gamma_grid_criteria (see there), the shape doseresponse/select_btf.py has.

    Ws (S,N,K), Vs (S,M,T,K); Y (N,M,T) or (N,M,T,R), NaN = missing, every observed y > 0; likelihood: the reference's
    (mean_grid, mean_probs, variance) or an object with shape_grid / scale_grid / probs_grid (likelihoods.gamma_grid_table).
    Needs ndepth >= 2 (a context is opened for the call).  No CPU fallback."""
    from . import criteria
    ctx, head, shape, obs = _gamma_grid_context(Ws, Vs, Y, likelihood, device)
    try:
        curve, totals, pw = criteria.evaluate(ctx, head, shape[:2], pointwise)
    finally:
        ctx.close()
    return criteria.combine(curve, totals, obs, pw)


def gamma_grid_loo(Ws, Vs, Y, likelihood, r_eff=None, mean=False, transform=None, log_weights=False, device=0):
    """PSIS-LOO of saved samples under the gamma-grid likelihood on the GPU, without a model: the stateless form of
    NonconjugateBayesianTensorFiltering.gamma_grid_loo (see there and BayesianTensorFiltering.loo); arguments as
    gamma_grid_criteria.  S <= 4096."""
    from . import _analysis, criteria
    code = _analysis.transform_code(transform)
    S, N = np.shape(Ws)[:2] if np.ndim(Ws) == 3 else (0, 0)
    M = np.shape(Vs)[1] if np.ndim(Vs) == 4 else 0
    r_eff = _analysis.check_r_eff(r_eff, (N, M))
    _analysis.check_loo_samples(S, "gamma_grid_loo")
    ctx, head, shape, obs = _gamma_grid_context(Ws, Vs, Y, likelihood, device)
    try:
        return criteria.loo_evaluate(ctx, head, shape, obs, r_eff=r_eff, transform=code, mean=mean, log_weights=log_weights)
    finally:
        ctx.close()


def _negbin_context(Ws, Vs, Rs, Y, device):
    """A context for one model-free Negative-Binomial criteria call: the statistics and counts of Y in slot 0.  Returns
    (ctx, head of btf_nb_crit_eval / btf_nb_crit_loo, (N,M,T), observed-curve mask); the caller closes ctx."""
    from . import _analysis, _native, criteria
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    rates, flags = criteria.negbin_rates(Rs, S, shape)              # (bad rates raise before any device call)
    ctx = _native.Context(N, shape[1], shape[2], K, 0, device=device)
    try:
        obs = criteria.negbin_upload(ctx, 0, Y, shape)
    except Exception:
        ctx.close()
        raise
    return ctx, criteria.negbin_head(0, S, Ws, Vs, rates, flags), shape, obs


def negbin_criteria(Ws, Vs, Rs, Y, pointwise=False, device=0):
    """WAIC and DIC of saved samples under the Negative-Binomial likelihood with a sampled rate on the GPU, without a
    model: the stateless form of NegativeBinomialBayesianTensorFiltering.negbin_criteria (see there).

    Ws (S,N,K), Vs (S,M,T,K); Rs (S,) + a shape broadcasting against (N,M,T) with every axis full or 1, or (S,);
    Y (N,M,T) or (N,M,T,R) counts, NaN = missing.  Needs ndepth >= 2 (a context is opened for the call).  No CPU fallback."""
    from . import criteria
    ctx, head, shape, obs = _negbin_context(Ws, Vs, Rs, Y, device)
    try:
        curve, totals, pw = criteria.negbin_evaluate(ctx, head, shape[:2], pointwise)
    finally:
        ctx.close()
    return criteria.combine(curve, totals, obs, pw)


def negbin_loo(Ws, Vs, Rs, Y, r_eff=None, mean=False, transform=None, log_weights=False, device=0):
    """PSIS-LOO of saved samples under the Negative-Binomial likelihood with a sampled rate on the GPU, without a model: the
    stateless form of NegativeBinomialBayesianTensorFiltering.negbin_loo (see there and BayesianTensorFiltering.loo);
    arguments as negbin_criteria.  S <= 4096."""
    from . import _analysis, criteria
    code = _analysis.transform_code(transform)
    S, N = np.shape(Ws)[:2] if np.ndim(Ws) == 3 else (0, 0)
    M = np.shape(Vs)[1] if np.ndim(Vs) == 4 else 0
    r_eff = _analysis.check_r_eff(r_eff, (N, M))
    _analysis.check_loo_samples(S, "negbin_loo")
    ctx, head, shape, obs = _negbin_context(Ws, Vs, Rs, Y, device)
    try:
        return criteria.loo_evaluate(ctx, head, shape, obs, r_eff=r_eff, transform=code, mean=mean, log_weights=log_weights,
                                     negbin=True)
    finally:
        ctx.close()


def gamma_grid_predictive(Ws, Vs, likelihood, data=None, q=(2.5, 97.5), draws_per_sample=1, seed=0, cells=None, device=0):
    """Posterior predictive of the observations under the gamma-grid likelihood on the GPU, without a model: the stateless
    form of NonconjugateBayesianTensorFiltering.gamma_grid_predictive (see there, and posterior_predictive for the outputs),
    the shape doseresponse/fit.py:475-478, plot_example.py:86 and plot_results.py:90 have.

    Ws (S,N,K), Vs (S,M,T,K); likelihood: as gamma_grid_criteria.  The component of a draw follows the table's weights; the
    reference's sample picks it uniformly - pass a table with equal weights for that.  data: (N,M,T) or (N,M,T,R), NaN =
    missing, every observed y > 0.  Needs ndepth >= 2 (a context is opened for the call).  No CPU fallback."""
    from . import _analysis, _native, criteria, likelihoods, predictive
    table = likelihoods.gamma_grid_table(likelihood)               # (a bad table raises before any device call)
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    predictive.check_draws(S, draws_per_sample)
    predictive.check_q(q)
    predictive.check_cells(cells, shape)
    Y4 = predictive.check_gamma_grid_data(data, shape)
    ctx = _native.Context(N, shape[1], shape[2], K, 0, device=device)
    try:
        ctx.call("btf_set_likelihood_table", criteria.FAMILY_GAMMA_GRID, *(_native.dptr(v) for v in table), int(table[0].size))
        return predictive.gamma_grid_evaluate(ctx, shape, K, S, Ws, Vs, Y=Y4, q=q, draws_per_sample=draws_per_sample, seed=seed,
                                              cells=cells)
    finally:
        ctx.close()


def posterior_functionals(Ws, Vs, which=("auc",), q=(5, 95), transform=None, x=None, level=None, exceed=None, curves=None,
                          pointwise=False, device=0):
    """Per-curve functionals of f(w_s[i] . v_s[j,:]) over depth, summarised over the kept samples, on the GPU, without a
    model: the stateless form of BayesianTensorFiltering.posterior_functionals, next to posterior_summary.

    The reference application does this on the host (doseresponse/feature_importance.py:40):

        np.trapz(np.einsum('znk,zmtk->znmt', Ws, Vs), dx=1/(T-1), axis=-1).mean(axis=0)     # == out["auc"]["mean"]

    which: any of "auc", "max", "min", "argmax", "argmin", "rise", "crossing" (functionalmf_amd.functionals.curve_functionals
    is their definition in numpy); x: (T,) strictly increasing depth coordinates, default np.linspace(0, 1, T); level: the
    level of `crossing` (e.g. 0.5 with transform="ilogit": the IC50).  Returns {name: {"mean", "var" (N,M; ddof 1),
    "quantiles" (len(q),N,M)}}; crossing adds "defined" (N,M), the share of samples in which the level is crossed - its mean
    and var run over those, its percentiles count the others as +inf and are nan where they reach them; exceed=c adds
    "prob_above" (share of samples with value > c); curves=[(i,j), ...] adds "curves" (ncurves,S), the raw values in
    sample order; pointwise=True adds "pointwise" (S,N,M).  At most 8192 samples, ndepth >= 2.  There is no CPU fallback."""
    from . import _analysis, functionals
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    return functionals.evaluate(shape, K, S, which=which, q=q, transform=transform, x=x, level=level, exceed=exceed, curves=curves,
                                pointwise=pointwise, Ws=Ws, Vs=Vs, device=device)


def posterior_bands(Ws, Vs, method="supt", level=95, depths=None, transform=None, curves=None, truth=None, device=0,
                    _scratch_bytes=0):
    """Simultaneous credible bands per curve on the GPU, without a model: the stateless form of
    BayesianTensorFiltering.posterior_bands, next to posterior_summary.

    posterior_summary(q=(2.5, 97.5)) holds each cell with 95 %; the whole curve leaves that band somewhere far more often.
    The band returned here holds at least ceil(level / 100 * S) of the S kept curves at every used depth at once.  On the
    host this takes the (S,N,M,T) tensor (functionalmf_amd.bands.supt_band / rank_band are exactly that, in numpy).

    method="supt": center -+ crit * scale with the per-cell mean and sd and crit an order statistic of the samples' largest
    standardised deviation; "rank": distribution-free, the k-th smallest and k-th largest value of every cell with k from the
    samples' rank depth - for ilogit curves near 0 or 1.  level in (0, 100); depths: a boolean mask (T,) of the depths the
    band is simultaneous over (default all; the band is returned at every depth); transform as posterior_summary.

    Returns a dict: lower, upper (N,M,T); inside (N,M) = the share of kept curves wholly inside (>= need / S); method,
    level, need, nsamples; supt: center, scale (N,M,T), crit (N,M); rank: k (N,M) int, k_pointwise and pointwise_inside
    (N,M) = the share of kept curves wholly inside the pointwise band of the same level - the figure that says why the
    pointwise band is not the answer.  curves=[(i,j), ...] adds "stat" (ncurves,S), the samples' raw deviation or depth;
    truth (N,M,T; NaN = unknown) adds covered (N,M: 1, 0, nan where no used depth is known) and coverage, their mean.
    At least 2 and at most 8192 (supt) / 4096 (rank) samples.  There is no CPU fallback."""
    from . import _analysis, bands
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    return bands.evaluate(shape, K, S, method=method, level=level, depths=depths, transform=transform, curves=curves, truth=truth,
                          Ws=Ws, Vs=Vs, device=device, _scratch_bytes=_scratch_bytes)


def posterior_ranking(Ws, Vs, which="auc", along="cols", order="ascending", top=(1, 5), transform=None, x=None, level=None,
                      pairs=None, pointwise=False, device=0, _scratch_bytes=0):
    """Which column is best for a row (or which row for a column), and with what probability, on the GPU, without a model:
    the stateless form of BayesianTensorFiltering.posterior_ranking, next to posterior_functionals.

    On the host this takes the (S,N,M) array of posterior_functionals(pointwise=True) and an argsort per group:

        f = posterior_functionals(Ws, Vs, which=("auc",), pointwise=True)["auc"]["pointwise"]
        (f.argsort(-1, kind="stable").argsort(-1) == 0).mean(0)                             # == out["p_top"][0], top=(1,)

    which: ONE of "auc", "max", "min", "argmax", "argmin", "rise", "crossing"; transform, x, level: as posterior_functionals.
    along="cols" ranks the M columns within each row, along="rows" the N rows within each column; order="ascending" gives
    rank 1 to the smallest value, "descending" to the largest.  Ties go to the smaller index; an undefined value (a crossing
    that never happens) ranks after every defined one in both orders.  top: 1 to 8 distinct integers k >= 1.
    functionalmf_amd.ranking.ranks / summarize are the definition in numpy; the device agrees with them exactly.

    Returns a dict: expected_rank and rank_var (N,M; ddof 1, 0 for a single sample) of the rank over the samples,
    p_top (len(top),N,M) = the share of samples with rank <= k, and top, along, order, which, nsamples.  pointwise=True adds
    ranks (S,N,M) int32.  pairs: a (P,4) integer array of curve pairs (i, j, i2, j2) anywhere in the tensor adds prob_less (P,)
    = the share of samples with f(i,j) < f(i2,j2) and prob_defined, the share in which both values are defined (a sample
    with an undefined value counts for neither).  At most 8192 samples and 4096 members in a group, ndepth >= 2.  There is
    no CPU fallback."""
    from . import _analysis, ranking
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    return ranking.evaluate(shape, K, S, which=which, along=along, order=order, top=top, transform=transform, x=x, level=level,
                            pairs=pairs, pointwise=pointwise, Ws=Ws, Vs=Vs, device=device, _scratch_bytes=_scratch_bytes)


def posterior_similarity(Ws, Vs, along="rows", metric="rms", over=None, q=(5, 95), nearest=(1, 5), pairs=None, pointwise=False,
                         device=0, _scratch_bytes=0):
    """Which rows (or columns) are alike: the distance between their fitted surfaces W V' per kept sample, summarised over
    the samples, and every entity's neighbours with their probabilities, on the GPU, without a model: the stateless form of
    BayesianTensorFiltering.posterior_similarity, next to posterior_ranking.

    The embeddings themselves are identified only up to an invertible K x K map that differs from sample to sample; the
    distance between two surfaces does not depend on it.  On the host this takes the quadratic form per sample, an (S,E,E)
    array, np.percentile and an argsort per sample (functionalmf_amd.similarity.reference is exactly that, in numpy).

    along="rows": the E = N rows are compared, each by its surface over the columns `over` (default: all) and all depths;
    along="cols": the E = M columns, over the rows `over`.  metric="rms": the root-mean-square gap between the two surfaces
    of the linear predictor w_i . v_jt; "cosine": 1 - the cosine of the angle between them (a zero surface is at distance 1
    from everything but itself).  No transform= is offered: under a non-linear transform the distance is no quadratic form
    in the embeddings any more.  Identical embeddings are at exactly 0, the result is symmetric bit for bit, the diagonal 0.
    nearest: 1 to 8 distinct integers k >= 1.

    Returns a dict: mean, var (E,E; ddof 1, nan for a single sample) and quantiles (len(q),E,E) of the distance over the
    samples; expected_rank, rank_var (E,E) and p_nearest (len(nearest),E,E): out["p_nearest"][k, e, f] is the share of
    samples in which f is among the nearest[k] nearest neighbours of e (ties to the smaller index, e itself last); along,
    metric, nearest, nsamples, ncells.  pairs: a (P,2) integer array of (e, f) adds pair_values (S,P), the distances in
    sample order; pointwise=True adds distances (S,E,E), refused above 1 GiB (use pairs=).  At most 8192 samples, 4096
    entities and nembeds 10.  functionalmf_amd.similarity.embed(out) gives multidimensional-scaling coordinates.  There is
    no CPU fallback."""
    from . import _analysis, similarity
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    return similarity.evaluate(shape, K, S, along=along, metric=metric, over=over, q=q, nearest=nearest, pairs=pairs,
                               pointwise=pointwise, Ws=Ws, Vs=Vs, device=device, _scratch_bytes=_scratch_bytes)


def posterior_feature_association(Ws, Vs, Us, which="auc", stats=("r",), q=(5, 95), transform=None, x=None, level=None, pairs=None,
                                  of_means=True, device=0, _scratch_bytes=0):
    """Which row feature (biomarker) goes with which column's curve functional (drug sensitivity), with uncertainty, on the
    GPU, without a model: the stateless form of BayesianTensorFiltering.posterior_feature_association.  What
    doseresponse/feature_importance.py:39-54 computes on posterior means only.

    Ws (S,N,K), Vs (S,M,T,K) and Us (S,F,K), the sampled feature embeddings (run_gibbs returns "U" for a model with
    row_features= and sample_features=True).  For kept sample s, feature f and column j: y_i = the functional `which` of curve
    (i,j) - ONE of "auc", "max", "min", "argmax", "argmin", "rise", "crossing"; transform, x, level as posterior_functionals,
    whose pointwise values these are bit for bit - is regressed over the rows i on x_i = w_i^s . u_f^s:
        r = Sxy / sqrt(Sxx Syy),   slope = Sxy / Sxx     (centred sums over the rows with a defined y_i; n of them)
    A row whose `crossing` is undefined is left out of that column's regression in that sample; the triple is defined when
    n >= 3, Sxx > 0 and Syy > 0.  functionalmf_amd.association.statistics / summarize are the definition in numpy.

    Returns a dict: for every name of stats (a subset of ("r", "slope")) a dict of mean, var (ddof 1; 0 with one defined
    sample), quantiles (len(q),F,M) by np.nanpercentile's rule and prob_positive, each (F,M) over the DEFINED samples (nan
    when there is none); defined (F,M) = defined samples / S; n_mean (M,) = the mean of n over the samples; which, stats,
    nsamples.  pairs: a (P,2) integer array of (feature, column) adds values (P,S) to every statistic, the raw per-sample
    values with nan where undefined.  of_means=True adds the plug-in table of the reference: of_means = {r, slope, intercept,
    stderr, n (F,M); sd_x (F,), sd_y (M,)} of the regression of the posterior-mean functional on the posterior-mean feature
    probability mean_s W_s U_s' - scipy.stats.linregress's numbers and the two ddof-0 standard deviations
    feature_importance.py:50 filters on; the p-value follows from r and n.
    At most 8192 samples, ndepth >= 2.  There is no CPU fallback."""
    from . import _analysis, association
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    shape = (N,) + Vs.shape[1:3]
    return association.evaluate(shape, K, S, Us, which=which, stats=stats, q=q, transform=transform, x=x, level=level, pairs=pairs,
                                of_means=of_means, Ws=Ws, Vs=Vs, device=device, _scratch_bytes=_scratch_bytes)


def posterior_monotone(Ws, Vs, q=(5, 95), transform=None, increasing=False, return_V=True, device=0):
    """Project posterior samples to monotone curves on the GPU, without a model: the stateless form of
    BayesianTensorFiltering.posterior_monotone.  What doseresponse/fit.py:365-374 does on the host, sample by sample.

    Ws (S,N,K), Vs (S,M,T,K).  For sample s and column j, V'_s[j] = factor_pav(Ws[s], Vs[s, j]), bit for bit: the
    left-to-right pool-adjacent-violators sweep after which no row's curve w_i . v'_jt increases with depth
    (increasing=True: -factor_pav(Ws[s], -Vs[s, j]), no curve decreases).  All S x M blocks are projected in one launch;
    Ws is not changed.  functionalmf_amd.monotone.project_host is the definition in numpy.

    Returns a dict: mean (N,M,T) and quantiles (len(q),N,M,T) of f(W_s V'_s) over the samples - posterior_summary's
    numbers on the projected states, which never leave the device for it (q=None: neither); pools (S,M) int32 = T minus
    the merges made for that sample and column (T: it was monotone already); changed (M,) = the share of samples in
    which the column needed a merge; V (S,M,T,K), the projected samples, with return_V - dict(W=Ws, V=out["V"]) goes
    into every other posterior_* call; nsamples.
    At most 16384 samples with a summary; 8 T K + 4 T <= 65536 (a column block in LDS, as factor_pav).  There is no CPU
    fallback."""
    from . import _analysis, monotone
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, N, K = Ws.shape
    return monotone.evaluate((N,) + Vs.shape[1:3], K, S, q=q, transform=transform, increasing=increasing, return_V=return_V,
                             Ws=Ws, Vs=Vs, device=device)


def fold_in_rows(Y_new, Vs, family, nu2=None, sigma2=None, seed=0, z=None, summary=True, q=(5, 95), transform=None,
                 inner_sweeps=None, trials=None, first_sample=0, device=0):
    """Embeddings of rows the chain never saw, one draw per kept sample, on the GPU, without a model: the stateless form of
    BayesianTensorFiltering.fold_in_rows (see there for the outputs), next to posterior_summary.

    Vs (S,M,T,K); family "gaussian" (nu2 and sigma2: one value per sample) or "binomial" (sigma2).  Y_new: (R,M,T) or
    (R,M,T,nreps) with NaN = missing; Binomial: a (Y, N) pair of (R,M,T) arrays, or Y with trials= (default 1), counts up to
    32.  z: optional (S,R,K) standard normals in the place of the device generator (Gaussian only): w = Q^-1 b + L^-T z.
    first_sample: the index of Vs[0] among the kept samples - with it a call over a slice of the samples returns the bits
    of the whole call.  out["W"] and Vs go straight into posterior_summary, posterior_predictive and posterior_functionals.
    functionalmf_amd.fold_in.conditional is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, fold_in
    Vs = _analysis.check_states(None, Vs)[1]
    S, M, T, K = Vs.shape
    code = fold_in.family_code(family)
    R, weights, sums = fold_in.row_statistics(Y_new, family, M, T, trials=trials)
    fold_in.check_args(family, S, R, K, z, summary, q, transform, inner_sweeps, first_sample)
    sigma2 = _analysis.check_scalars("sigma2", sigma2, S)
    nu2 = _analysis.check_scalars("nu2", nu2, S) if code == fold_in.FAMILIES["gaussian"] else None
    return fold_in.evaluate(family, S, R, M, T, K, weights, sums, z=z, seed=seed, summary=summary, q=q, transform=transform,
                            inner_sweeps=inner_sweeps, first_sample=first_sample, Vs=Vs, nu2=nu2, sigma2=sigma2, device=device)


def fold_in_cols(Y_new, Ws, family, nu2=None, lam2=None, tf_order=2, seed=0, draws=None, sweeps=None, summary=True, q=(5, 95),
                 transform=None, trials=None, first_sample=0, stability=1e-6, device=0):
    """Curves of columns the chain never saw, one short Gibbs chain per (kept sample, new column), on the GPU, without a
    model: the stateless form of BayesianTensorFiltering.fold_in_cols (see there for the method and the outputs).

    Ws (S,N,K); family "gaussian" (nu2 and lam2: one value per sample) or "binomial" (lam2); tf_order and stability as the
    model was built with.  Y_new: (C,N,T) or (C,N,T,nreps) with NaN = missing; Binomial: a (Y, N) pair of (C,N,T) arrays,
    or Y with trials= (default 1), counts up to 32.  draws: optional (S,C,4 nD + sweeps (T K + 4 nD)) variates in the place
    of the device generator (Gaussian only).  first_sample: the index of Ws[0] among the kept samples - with it a call over
    a slice of the samples returns the bits of the whole call.  Ws and out["V"] go straight into posterior_summary,
    posterior_predictive and posterior_functionals.  functionalmf_amd.fold_in_cols.chain is the definition in numpy.
    There is no CPU fallback."""
    from . import _analysis, _native, fold_in_cols as _fc
    code = _fc.family_code(family)
    Ws = _native.as_f64(Ws)
    if Ws.ndim != 3 or Ws.shape[0] < 1:
        raise ValueError("Ws must be (S,N,K), got %r" % (Ws.shape,))
    S, N, K = Ws.shape
    Yshape = np.shape(Y_new[0] if isinstance(Y_new, (tuple, list)) and len(Y_new) else Y_new)
    T = Yshape[2] if len(Yshape) >= 3 else -1
    C, weights, sums = _fc.column_statistics(Y_new, family, N, T, trials=trials)
    _fc.check_args(family, S, C, T, K, tf_order, draws, sweeps, summary, q, transform, first_sample)
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    nu2 = _analysis.check_scalars("nu2", nu2, S) if code == _fc.FAMILIES["gaussian"] else None
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    return _fc.evaluate(family, S, C, N, T, K, tf_order, weights, sums, draws=draws, seed=seed, sweeps=sweeps, summary=summary,
                        q=q, transform=transform, first_sample=first_sample, stability=stability, Ws=Ws, nu2=nu2, lam2=lam2,
                        device=device)


def fold_in_depth(Y_new, Ws, Vs, family, horizon=None, nu2=None, lam2=None, tf_order=2, seed=0, draws=None, sweeps=None, summary=True,
                  q=(5, 95), transform=None, trials=None, first_sample=0, stability=1e-6, device=0):
    """Curves of every fitted column at depths the chain never saw, one short Gibbs chain per (kept sample, fitted column),
    on the GPU, without a model: the stateless form of BayesianTensorFiltering.fold_in_depth (see there for the method and
    the outputs).

    Ws (S,N,K) and Vs (S,M,T,K): the kept samples (of Vs only the last min(T, tf_order + 1) depths are uploaded); family
    "gaussian" (nu2 and lam2: one value per sample) or "binomial" (lam2); tf_order and stability as the model was built
    with.  Y_new: (N,M,H) or (N,M,H,nreps) with NaN = missing; Binomial: a (Y, N) pair of (N,M,H) arrays, or Y with trials=
    (default 1), counts up to 32; None with horizon=H: the forecast (no data).  draws: optional (S,M,4 nR + sweeps (H K +
    4 nR)) variates in the place of the device generator (Gaussian only).  first_sample: the index of Ws[0] among the kept
    samples - with it a call over a slice of the samples returns the bits of the whole call.  Ws with
    np.concatenate([Vs, out["V"]], axis=2) goes straight into posterior_summary, posterior_predictive and
    posterior_functionals.  functionalmf_amd.fold_in_depth.chain is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, fold_in_depth as _fd
    code = _fd.family_code(family)
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, M, T, K = Vs.shape
    N = Ws.shape[1]
    H, weights, sums = _fd.slice_statistics(Y_new, family, N, M, trials=trials, horizon=horizon)
    _fd.check_args(family, S, M, T, H, K, tf_order, draws, sweeps, summary, q, transform, first_sample)
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    nu2 = _analysis.check_scalars("nu2", nu2, S) if code == _fd.FAMILIES["gaussian"] else None
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    if not np.all(np.isfinite(Vs[:, :, T - _fd.tail_depths(T, tf_order):])):
        raise ValueError("Vs must be finite at the last kept depths")
    return _fd.evaluate(family, S, N, M, T, H, K, tf_order, weights, sums, draws=draws, seed=seed, sweeps=sweeps, summary=summary,
                        q=q, transform=transform, first_sample=first_sample, stability=stability, Ws=Ws, Vs=Vs, nu2=nu2, lam2=lam2,
                        device=device)


def negbin_fold_in_cols(Y_new, Ws, R, lam2=None, tf_order=2, seed=0, sweeps=None, summary=True, q=(5, 95), transform=None,
                        first_sample=0, stability=1e-6, draws=None, omega=None, device=0):
    """fold_in_cols for a Negative-Binomial fit, without a model: the stateless form of
    NegativeBinomialBayesianTensorFiltering.negbin_fold_in_cols (see there for the method and the outputs).

    Ws (S,N,K); lam2 one value per sample; tf_order and stability as the model was built with.  Y_new: counts (C,N,T) or
    (C,N,T,nreps) with nan = missing.  R: the rate of the new columns, (S,) plus a shape that broadcasts against (C,N,T) -
    what the model's call takes as rate=.  draws with omega (S,C,sweeps,N,T): every variate and Polya-Gamma weight of every
    chain in the place of the device generators.  functionalmf_amd.negbin_fold_in.chain_cols is the definition in numpy.
    There is no CPU fallback."""
    from . import _analysis, _native, negbin_fold_in as _nf
    Ws = _native.as_f64(Ws)
    if Ws.ndim != 3 or Ws.shape[0] < 1:
        raise ValueError("Ws must be (S,N,K), got %r" % (Ws.shape,))
    S, N, K = Ws.shape
    shape = np.shape(Y_new)
    if len(shape) not in (3, 4) or shape[0] < 1:
        raise ValueError("Y_new %r must be (C,%d,T) or (C,%d,T,nreps)" % (shape, N, N))
    C, T = int(shape[0]), int(shape[2])
    cnt, ysum = _nf.cell_statistics(Y_new, (C, N, T))
    if R is None:
        raise ValueError("R: the rate of the new columns is required")
    rate = _nf.resolve_rate("cols", None, R, S, C, N, T)
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    return _nf.evaluate("cols", S, C, N, T, K, tf_order, cnt, ysum, rate, Ws, lam2, draws=draws, omega=omega, seed=seed, sweeps=sweeps,
                        summary=summary, q=q, transform=transform, first_sample=first_sample, stability=stability, device=device)


def negbin_fold_in_depth(Y_new, Ws, Vs, R, horizon=None, lam2=None, tf_order=2, seed=0, sweeps=None, summary=True, q=(5, 95),
                         transform=None, first_sample=0, stability=1e-6, draws=None, omega=None, device=0):
    """fold_in_depth for a Negative-Binomial fit, without a model: the stateless form of
    NegativeBinomialBayesianTensorFiltering.negbin_fold_in_depth (see there for the method and the outputs).

    Ws (S,N,K) and Vs (S,M,T,K): the kept samples; lam2 one value per sample.  Y_new: counts (N,M,H) or (N,M,H,nreps) with
    nan = missing; None with horizon=H: the forecast (R may then be None).  R: the rate at the new depths, (S,) plus a shape
    that broadcasts against (N,M,H).  draws with omega (S,M,sweeps,N,H) as in negbin_fold_in_cols.
    functionalmf_amd.negbin_fold_in.chain_depth is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, negbin_fold_in as _nf, fold_in_depth as _fd
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, M, T, K = Vs.shape
    N = Ws.shape[1]
    H, cnt, ysum = _nf.slice_cells(Y_new, N, M, horizon)
    if R is None and cnt.any():
        raise ValueError("R: the rate at the new depths is required")
    rate = _nf.resolve_rate("depth", None, R, S, M, N, H, needed=bool(cnt.any()))
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    if not np.all(np.isfinite(Vs[:, :, T - _fd.tail_depths(T, tf_order):])):
        raise ValueError("Vs must be finite at the last kept depths")
    return _nf.evaluate("depth", S, M, N, T, K, tf_order, cnt, ysum, rate, Ws, lam2, Vs=Vs, horizon=H, draws=draws, omega=omega,
                        seed=seed, sweeps=sweeps, summary=summary, q=q, transform=transform, first_sample=first_sample,
                        stability=stability, device=device)


def negbin_fold_in_rows(Y_new, Vs, sigma2, R=None, rate=None, sample_rate=None, rate_init=None, nmetropolis=30, rpropstdev=0.1, rstdev=1,
                        seed=0, sweeps=None, summary=True, q=(5, 95), transform=None, first_sample=0, draws=None, omega=None, device=0):
    """Embeddings of rows a Negative-Binomial chain never saw, with a fixed or a SAMPLED rate, on the GPU, without a model:
    the stateless form of NegativeBinomialBayesianTensorFiltering.negbin_fold_in_rows (see there for the method and the
    outputs).

    Vs (S,M,T,K); sigma2 one value per sample.  Y_new: counts (R,M,T) or (R,M,T,nreps) with nan = missing.  R: the fit's
    results["R"], (S,) plus the model's rate shape; rate: (S,) plus a shape that broadcasts against (R,M,T).  Where the
    rate of a new row comes from: rate= when given; else the kept sample's where R does not vary along the rows
    (S,1,M|1,T|1); else, with one rate per row (S,N,1,1), one scalar per (sample, new row) SAMPLED by the model's
    Metropolis step (nmetropolis, rpropstdev, rstdev as the model was built with) from rate_init, (S,) or (S,R), default
    the geometric mean of the kept sample's rates; any other layout is a ValueError asking for rate=.  sample_rate=True
    forces sampling, False refuses it.  draws (S,R,sweeps (2 nmetropolis + K)) with omega (S,R,sweeps,M,T): every variate
    and Polya-Gamma weight of every chain in the place of the device generators.
    functionalmf_amd.negbin_fold_in.chain_rows is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, negbin_fold_in as _nf
    Vs = _analysis.check_states(None, Vs)[1]
    S, M, T, K = Vs.shape
    shape = np.shape(Y_new)
    if len(shape) not in (3, 4) or shape[0] < 1:
        raise ValueError("Y_new %r must be (R,%d,%d) or (R,%d,%d,nreps)" % (shape, M, T, M, T))
    nrows = int(shape[0])
    mode, fixed = _nf.resolve_row_rate(R, rate, sample_rate, S, nrows, M, T)
    r0 = _nf.resolve_rate_init(rate_init, R, S, nrows) if mode == "sampled" else None
    sigma2 = _analysis.check_scalars("sigma2", sigma2, S, positive=False)
    if np.any(sigma2 <= 0):
        raise ValueError("sigma2 must be positive")
    return _nf.evaluate_rows(S, nrows, M, T, K, Y_new, Vs, sigma2, rate=fixed, rate_init=r0, nmetropolis=nmetropolis,
                             rpropstdev=rpropstdev, rstdev=rstdev, draws=draws, omega=omega, seed=seed, sweeps=sweeps, summary=summary,
                             q=q, transform=transform, first_sample=first_sample, device=device)


def slice_fold_in_rows(Y_new, Vs, family, sigma2=None, Ws=None, likelihood_param=None, Constraints=None, Row_constraints=None,
                       row_features=None, Us=None, start=None, seed=0, draws=None, sweeps=None, max_rounds=40, summary=True,
                       q=(5, 95), transform=None, first_sample=0, device=0):
    """Embeddings of rows the chain never saw for a slice-sampled fit, one draw per kept sample, on the GPU, without a
    model: the stateless form of NonconjugateBayesianTensorFiltering.slice_fold_in_rows (see there for the method, the
    arguments and the outputs).

    Vs (S,M,T,K); sigma2 one value per sample; family: a device likelihood name ("poisson", "poisson_identity",
    "bernoulli_logit", "gaussian", "negbin_logit", "gamma_grid") with likelihood_param as the model class takes it.
    Ws (S,N,K): the fitted rows, read for the default start (their mean per sample) only; start= replaces it.
    Constraints (J,T+1) / Row_constraints (n,K+1) as ConstrainedNonconjugateBayesianTensorFiltering takes them;
    row_features (R,F) of 0 / 1 / nan with Us (S,F,K).  Y_new=None with row_features: rows known by their features alone.
    first_sample: the index of Vs[0] among the kept samples - with it a call over a slice of the samples returns the bits
    of the whole call.  functionalmf_amd.slice_fold_in.chain is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, slice_fold_in as _sf
    _sf.family_code(family)
    Ws, Vs = _analysis.check_states(Ws if start is None else None, Vs)
    S, M, T, K = Vs.shape
    param = _sf.check_param(family, likelihood_param)
    codes = None if row_features is None else _sf.feature_codes(row_features)
    R, S1, cnt, L = _sf.row_statistics(Y_new, family, M, T, R=None if codes is None else codes.shape[0])
    _sf.check_args(family, param, S, R, K, start, draws, sweeps, max_rounds, summary, q, transform, first_sample, Us, codes,
                   have_W=Ws is not None)
    _sf.check_constraints(Constraints, Row_constraints, T, K)
    sigma2 = _analysis.check_scalars("sigma2", sigma2, S)
    return _sf.evaluate(family, param, S, R, M, T, K, S1, cnt, L, start=start, Constraints=Constraints,
                        Row_constraints=Row_constraints, Us=Us, codes=codes, draws=draws, seed=seed, sweeps=sweeps,
                        max_rounds=max_rounds, summary=summary, q=q, transform=transform, first_sample=first_sample, Vs=Vs, Ws=Ws,
                        sigma2=sigma2, device=device)


def slice_fold_in_cols(Y_new, Ws, family, lam2=None, Vs=None, likelihood_param=None, Constraints=None, tf_order=2, fit=None,
                       start=None, tau2=None, seed=0, draws=None, sweeps=None, max_rounds=40, summary=True, q=(5, 95),
                       transform=None, first_sample=0, stability=1e-6, device=0):
    """Curves of columns the chain never saw for a slice-sampled fit, one draw per kept sample, on the GPU, without a
    model: the stateless form of NonconjugateBayesianTensorFiltering.slice_fold_in_cols (see there for the method, the
    arguments and the outputs).

    Ws (S,N,K); lam2 one value per sample; family: a device likelihood name ("poisson", "poisson_identity",
    "bernoulli_logit", "gaussian", "negbin_logit", "gamma_grid") with likelihood_param as the model class takes it;
    tf_order and stability as the model was built with.  Vs (S,M,T,K): the fitted columns, read for the default start
    (their mean per sample) only; start= replaces it.  Constraints (J,T+1) as
    ConstrainedNonconjugateBayesianTensorFiltering takes them: they hold for every fitted row.  first_sample: the index
    of Ws[0] among the kept samples - with it a call over a slice of the samples returns the bits of the whole call.
    functionalmf_amd.slice_fold_in_cols.chain is the definition in numpy.  There is no CPU fallback."""
    from . import _analysis, _native, slice_fold_in as _sf, slice_fold_in_cols as _sc
    _sf.family_code(family)
    Ws = _native.as_f64(Ws)
    if Ws.ndim != 3 or Ws.shape[0] < 1:
        raise ValueError("Ws must be (S,N,K), got %r" % (Ws.shape,))
    S, N, K = Ws.shape
    Yshape = np.shape(Y_new)
    T = Yshape[2] if len(Yshape) >= 3 else -1
    param = _sf.check_param(family, likelihood_param)
    C, S1, cnt, L = _sc.column_statistics(Y_new, family, N, T)
    if start is None and Vs is not None:
        Vs = _native.as_f64(Vs)
        if Vs.ndim != 4 or Vs.shape[0] != S or Vs.shape[1] < 1 or Vs.shape[2:] != (T, K):
            raise ValueError("Vs must be (S,M,T,K) = (%d,M,%d,%d), got %r" % (S, T, K, Vs.shape))
    else:
        Vs = None
    _sc.check_args(family, param, S, C, N, T, K, tf_order, start, tau2, draws, sweeps, max_rounds, summary, q, transform,
                   first_sample, have_V=Vs is not None)
    _sf.check_constraints(Constraints, None, T, K)
    if fit is None:
        fit = _sc.gaussian_fit(Y_new, family, param)
    weights, sums = _sc.fit_weights(fit, C, N, T)
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    return _sc.evaluate(family, param, S, C, N, T, K, tf_order, S1, cnt, L, weights, sums, start=start, Constraints=Constraints,
                        tau2=tau2, draws=draws, seed=seed, sweeps=sweeps, max_rounds=max_rounds, summary=summary, q=q,
                        transform=transform, first_sample=first_sample, stability=stability, Ws=Ws, Vs=Vs, lam2=lam2,
                        device=device)


def slice_fold_in_depth(Y_new, Ws, Vs, family, horizon=None, lam2=None, likelihood_param=None, Constraints=None, tf_order=2,
                        fit=None, start=None, tau2=None, seed=0, draws=None, sweeps=None, max_rounds=40, summary=True, q=(5, 95),
                        transform=None, first_sample=0, stability=1e-6, device=0):
    """Curves of every fitted column at depths the chain never saw for a slice-sampled fit, one draw per kept sample, on
    the GPU, without a model: the stateless form of NonconjugateBayesianTensorFiltering.slice_fold_in_depth (see there for
    the method, the arguments and the outputs).

    Ws (S,N,K) and Vs (S,M,T,K): the kept samples (of Vs only the last max(min(T, tf_order + 1), B) depths are uploaded, B
    the kept depths the constraints reach); lam2 one value per sample; family: a device likelihood name ("poisson",
    "poisson_identity", "bernoulli_logit", "gaussian", "negbin_logit", "gamma_grid") with likelihood_param as the model
    class takes it; tf_order and stability as the model was built with.  Y_new (N,M,H) or (N,M,H,nreps), NaN = missing;
    None with horizon=H: the (constrained) forecast.  Constraints (J, T + H + 1) on the extended grid: they hold for every
    fitted row.  first_sample: the index of Ws[0] among the kept samples - with it a call over a slice of the samples
    returns the bits of the whole call.  functionalmf_amd.slice_fold_in_depth.chain is the definition in numpy.  There is
    no CPU fallback."""
    from . import _analysis, slice_fold_in as _sf, slice_fold_in_cols as _sc, slice_fold_in_depth as _sd
    _sf.family_code(family)
    Ws, Vs = _analysis.check_states(Ws, Vs)
    S, M, T, K = Vs.shape
    N = Ws.shape[1]
    param = _sf.check_param(family, likelihood_param)
    H, S1, cnt, L = _sd.slice_statistics(Y_new, family, N, M, horizon=horizon)
    B = _sd.reduce_constraints(Constraints, T, H)[3]
    _sd.check_args(family, param, S, M, N, T, H, K, tf_order, start, tau2, draws, sweeps, max_rounds, summary, q, transform,
                   first_sample, B)
    if fit is None:
        fit = _sd.default_fit(Y_new, family, param, N, M)
    weights, sums = _sc.fit_weights(fit, M, N, H)
    lam2 = _analysis.check_scalars("lam2", lam2, S)
    if not 0 < float(stability) <= 1:
        raise ValueError("stability must lie in (0, 1]")
    if not np.all(np.isfinite(Vs[:, :, T - _sd.tail_depths(T, tf_order, B):])):
        raise ValueError("Vs must be finite at the last kept depths")
    return _sd.evaluate(family, param, S, N, M, T, H, K, tf_order, S1, cnt, L, weights, sums, start=start, Constraints=Constraints,
                        tau2=tau2, draws=draws, seed=seed, sweeps=sweeps, max_rounds=max_rounds, summary=summary, q=q,
                        transform=transform, first_sample=first_sample, stability=stability, Ws=Ws, Vs=Vs, lam2=lam2,
                        device=device)


# chain initialisers (utils.py:218-419): non-negative tensor factorisation and the factor PAV projection, on the GPU
from .nmf import bounded_tensor_nmf, factor_pav, tensor_nmf  # noqa: E402,F401


def ep_from_mf(Y, W, V, mode='max', multiplier=2):
    """Gaussian approximation of the likelihood around a factorisation (utils.py:423-438): the means W.V and one
    over-estimated standard deviation for every cell - the root of the largest (mode='max') or `multiplier` times the
    root of the mean (mode='multiplier') per-cell mean squared error of the observed replicates.  Y: 3-D or 4-D with
    NaN for missing entries.  Returns (Mu_ep, Sigma_ep), the ep_approx of ConstrainedNonconjugateBayesianTensorFiltering."""
    import warnings
    Y = np.asarray(Y, dtype=float)
    if Y.ndim == 3:
        Y = Y[..., None]
    M = (W[:, None, None] * V[None]).sum(axis=-1, keepdims=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        sqerr = np.nanmean((Y - M) ** 2, axis=-1)
        if mode == 'max':
            overestimate = np.sqrt(np.nanmax(sqerr))
        elif mode == 'multiplier':
            overestimate = np.sqrt(np.nanmean(sqerr)) * multiplier
        else:
            raise ValueError("mode must be 'max' or 'multiplier'")
    print('Estimated stdev: {}'.format(overestimate))
    return M[..., 0], np.ones(Y.shape[:-1]) * overestimate
