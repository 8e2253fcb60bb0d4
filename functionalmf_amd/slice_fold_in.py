"""Folding new rows into a slice-sampled fit: the embedding of a row the chain never saw, per kept sample, for the models
that have no conjugate row conditional (NonconjugateBayesianTensorFiltering and its constrained subclass).

The row prior of both models is N(0, sigma2 I) (the reference's factor.py:685-686; a new row lies beyond the leading K rows,
so the lower-triangular restriction does not touch it), and given V_s (and U_s) every restriction on a row is linear in w:
the curve constraints  sum_t A[c,t] (w . v_jt) >= C[c]  of every column j, the fixed Row_constraints, and 0 <= w . u_f <= 1.
The feasible set is convex, so elliptical slice sampling (elliptical_slice.py:59-124 with mu = 0) with the restrictions as
a likelihood of minus infinity samples p(w_new | y_new, V_s, U_s): every proposal lies on an ellipse through the current
feasible state, so the bracket always shrinks to something feasible.  `sweeps` updates per (sample, row) from a feasible
start - by default the mean of the fitted rows of the sample, which lies in the (convex) feasible set - and the last state
of every chain is one draw per kept sample.

The data-sized work is the HIP of csrc/btf_slice_fold.h (btf_slice_fold_rows / btf_collect_slice_fold); this module holds
the host halves in plain numpy (importable without a GPU): the DEFINITION the kernel is tested against (`row_statistics`,
`loglik`, `feasible`, `feature_term`, `chain`), the argument checks, and `evaluate`, the one caller of the C entry points.
"""
import numpy as np

from ._analysis import check_q, transform_code
from .likelihoods import gamma_grid_table

# the device likelihood families (NonconjugateBayesianTensorFiltering.LINKS, btf_ess.h:25-37)
FAMILIES = {"poisson": 0, "poisson_log": 0, "poisson_identity": 1, "bernoulli_logit": 2, "gaussian": 3, "negbin_logit": 4,
            "gamma_grid": 5}
GAMMA_GRID = 5
MAX_SUMMARY_SAMPLES = 16384      # the limit of posterior_summary_kernel (one cell's values are sorted in LDS)
DEFAULT_MAX_ROUNDS = 40          # proposals per sweep: ess_max_rounds of the slice-sampled models
# sweeps per (sample, row): the smallest of {4, 8, 16, 32, 64} after which the largest standardised deviation of the mean
# against the quadrature posterior no longer falls ("Folding new rows into a slice-sampled fit", table of
# scripts/slice_fold_in_rate.py --sweeps)
DEFAULT_SWEEPS = 32


def family_code(family):
    if callable(family):
        raise NotImplementedError("slice_fold_in_rows needs a device likelihood: a Python-callable loglikelihood is evaluated "
                                  "on the host only")
    if family not in FAMILIES:
        raise ValueError("family must be one of %s" % (tuple(sorted(FAMILIES)),))
    return FAMILIES[family]


def check_param(family, param):
    """The likelihood parameter as the definition takes it: None (families 0..2), the positive scalar of families 3
    (variance) and 4 (rate), or the gamma-grid table (shape, scale, prob) of likelihoods.gamma_grid_table."""
    code = family_code(family)
    if code in (3, 4):
        if param is None or not np.isscalar(param) or not (float(param) > 0 and np.isfinite(param)):
            raise ValueError("family %r needs param > 0 (the variance / the rate)" % (family,))
        return float(param)
    if code == GAMMA_GRID:
        if isinstance(param, (tuple, list)) and len(param) == 3 and all(np.ndim(v) == 1 for v in param) \
                and len({np.size(v) for v in param}) == 1 and not np.isscalar(param[2]):
            param = GammaTable(*param)
        return gamma_grid_table(param)
    return None


class GammaTable:
    """(shape, scale, prob) arrays as an object gamma_grid_table accepts."""

    def __init__(self, shape, scale, prob):
        self.shape_grid, self.scale_grid, self.probs_grid = shape, scale, prob


def row_statistics(Y_new, family, M, T, R=None):
    """(R, S1 (R,M,T), cnt (R,M,T), L (R,M,T) or None) of the new rows: the sum and the number of the observed replicates
    of every cell and, for the gamma grid, the sum of their logs.  Y_new: (R,M,T) or (R,M,T,nreps), NaN = missing; a row
    with no observation at all is allowed; None (with R): rows without observations.  ValueError on a shape that does not
    match (M, T), an infinite value, or an observed y <= 0 under the gamma grid."""
    code = family_code(family)
    if Y_new is None:
        if R is None or int(R) < 1:
            raise ValueError("Y_new=None needs row_features: the rows come from their features alone")
        z = np.zeros((int(R), M, T))
        return int(R), z, z.copy(), (z.copy() if code == GAMMA_GRID else None)
    if isinstance(Y_new, (tuple, list)):
        raise ValueError("Y_new is one (R,M,T) or (R,M,T,nreps) array")
    Y = np.asarray(Y_new, dtype=float)
    if Y.ndim == 3:
        Y = Y[..., None]
    if Y.ndim != 4 or Y.shape[0] < 1 or Y.shape[1:3] != (M, T) or Y.shape[3] < 1:
        raise ValueError("Y_new %r must be (R,%d,%d) or (R,%d,%d,nreps)" % (np.shape(Y_new), M, T, M, T))
    if R is not None and Y.shape[0] != R:
        raise ValueError("Y_new holds %d rows and row_features %d" % (Y.shape[0], R))
    if np.isinf(Y).any():
        raise ValueError("Y_new holds infinite values (nan marks a missing observation)")
    obs = ~np.isnan(Y)
    S1 = np.ascontiguousarray(np.where(obs, Y, 0.0).sum(axis=3))
    cnt = np.ascontiguousarray(obs.sum(axis=3), dtype=np.float64)
    L = None
    if code == GAMMA_GRID:
        if np.any(Y[obs] <= 0):
            raise ValueError("the gamma_grid likelihood needs every observed y > 0")
        L = np.ascontiguousarray(np.where(obs, np.log(np.where(obs, Y, 1.0)), 0.0).sum(axis=3))
    return Y.shape[0], S1, cnt, L


def _softplus(x):
    return np.logaddexp(0.0, x)


def loglik(family, param, stats_of_row, V, w):
    """Log-likelihood of one row at w, the families of btf_ess.h:25-37 without their state-independent terms (the gamma
    grid: complete).  stats_of_row = (S1, cnt, L) of the row, each (M,T) (L None unless gamma grid); V (M,T,K); param: the
    variance (3), the rate (4) or the table (shape, scale, prob) of likelihoods.gamma_grid_table (5)."""
    K = np.shape(V)[-1]
    eta = np.asarray(V, dtype=float).reshape(-1, K).dot(np.asarray(w, dtype=float))
    return loglik_eta(family, param, stats_of_row, eta)


def loglik_eta(family, param, stats, eta):
    """The same from the linear predictors: stats = (S1, cnt, L) and eta hold one value per cell, in any common shape
    (slice_fold_in_cols evaluates a column's cells with eta_it = w_i . v_t through this)."""
    code = family if isinstance(family, int) else family_code(family)
    S1, cnt, L = stats
    eta = np.reshape(eta, -1)
    S1, cnt = np.reshape(S1, -1), np.reshape(cnt, -1)
    obs = cnt > 0
    if not obs.any() and code != GAMMA_GRID:
        return 0.0
    e, s1, c = eta[obs], S1[obs], cnt[obs]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if code == 0:
            return float(np.sum(s1 * e - c * np.exp(e)))
        if code == 1:
            if np.any(e <= 0):
                return -np.inf
            return float(np.sum(s1 * np.log(e) - c * e))
        if code == 2:
            return float(np.sum(s1 * e - c * _softplus(e)))
        if code == 3:
            return float(np.sum(s1 * e - 0.5 * c * e * e) / param)
        if code == 4:
            return float(np.sum(s1 * e - (s1 + c * param) * _softplus(e)))
        from scipy.special import gammaln, logsumexp
        a, sc, p = param
        keep = p > 0
        a, sc, p = a[keep], sc[keep], p[keep]
        lsp = np.log(p.sum())
        total = lsp * float(np.count_nonzero(~obs))
        if not obs.any():
            return float(total)
        if np.any(e <= 0):
            return -np.inf
        Lo = np.reshape(L, -1)[obs]
        comp = np.log(p)[None] + a[None] * (Lo - c * np.log(e))[:, None] - (s1 / e)[:, None] / sc[None] \
            - c[:, None] * (a * np.log(sc) + gammaln(a))[None]
        return float(total + np.sum(logsumexp(comp, axis=1) - Lo))


def slacks(w, V, Constraints=None, Row_constraints=None, U=None):
    """The slack of every restriction at w, as one array (empty without restrictions): A V_j w - c per (column,
    constraint), a . w - a[K] per row constraint, then w . u_f and 1 - w . u_f per feature."""
    w = np.asarray(w, dtype=float)
    out = []
    if Constraints is not None and len(Constraints):
        C = np.atleast_2d(np.asarray(Constraints, dtype=float))
        eta = np.asarray(V, dtype=float).dot(w)                     # (M,T)
        out.append((eta.dot(C[:, :-1].T) - C[:, -1][None]).reshape(-1))
    if Row_constraints is not None and len(Row_constraints):
        Rc = np.atleast_2d(np.asarray(Row_constraints, dtype=float))
        out.append(Rc[:, :-1].dot(w) - Rc[:, -1])
    if U is not None and len(U):
        p = np.asarray(U, dtype=float).dot(w)
        out += [p, 1.0 - p]
    return np.concatenate(out) if out else np.zeros(0)


def feasible(w, V, Constraints=None, Row_constraints=None, U=None):
    """Every restriction holds at w, by the comparisons of the GASS row update: A V_j w >= c for every column and
    constraint, Row_constraints a . w >= a[K], 0 <= w . u_f <= 1 (NaN fails)."""
    s = slacks(w, V, Constraints, Row_constraints, U)
    return bool(np.all(s >= 0))


def feature_codes(row_features, R=None):
    """(R,F) uint8 codes 0, 1, 2 = missing of a (R,F) array of 0 / 1 / nan; ValueError otherwise."""
    X = np.asarray(row_features, dtype=float)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or (R is not None and X.shape[0] != R):
        raise ValueError("row_features must be (R, F) with F >= 1, got %r" % (X.shape,))
    miss = np.isnan(X)
    if not np.all(miss | (X == 0) | (X == 1)):
        raise ValueError("row_features must hold 0, 1 or nan (missing)")
    return np.ascontiguousarray(np.where(miss, 2, X).astype(np.uint8))


def feature_term(w, U, x_codes):
    """sum_f x log(w . u_f) + (1 - x) log(1 - w . u_f) over the pairs that are not missing (code 2, or nan)."""
    x = np.asarray(x_codes, dtype=float).reshape(-1)
    p = np.asarray(U, dtype=float).dot(np.asarray(w, dtype=float))
    one, zero = x == 1, x == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(np.log(p[one])) + np.sum(np.log(1.0 - p[zero])))


def record_length(K, max_rounds=DEFAULT_MAX_ROUNDS):
    """Numbers one sweep consumes: the K normals, u_h, u_a, then the max_rounds - 1 shrink uniforms."""
    return int(K) + 1 + int(max_rounds)


def chain(start, V, sigma2, family, param=None, stats=None, Constraints=None, Row_constraints=None, U=None, x_codes=None,
          draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS):
    """The chain of one (sample, row) in numpy: elliptical_slice.py:59-124 with mu = 0.  Per sweep nu = sqrt(sigma2) z,
    hh = ll(x) + log(u_h), phi = 2 pi u_a with the bracket [phi - 2 pi, phi]; propose x' = x cos phi + nu sin phi, accept
    when x' is feasible and ll(x') >= hh, otherwise shrink the bracket towards 0 and set phi = min + (max - min) u_next.
    After max_rounds proposals without acceptance the sweep keeps x and is counted.  ll = loglik (+ feature_term with U and
    x_codes); the value of the state is carried over from the accepted proposal.

    start (K,); V (M,T,K); stats = (S1, cnt, L) of the row (None: a row without observations).  draws (sweeps,
    K + 1 + max_rounds): the record of every sweep - K normals, u_h, u_a, the shrink uniforms - or None: drawn from rng (a
    np.random.Generator / RandomState; default: a fresh default_rng()).

    Returns a dict: w (K,) - nan when the start is infeasible or has a non-finite likelihood (failed=True; the chain does
    not run) -, rounds (likelihood evaluations of proposals), unfinished (sweeps that hit the cap), and the smallest
    decision margins met: margin_ll = min |ll(x') - hh| and margin_slack = the smallest absolute constraint slack."""
    code = family if isinstance(family, int) else family_code(family)
    x = np.array(start, dtype=float).reshape(-1)
    K = x.size
    V = np.asarray(V, dtype=float)
    M, T = V.shape[:2]
    if stats is None:
        z = np.zeros((M, T))
        stats = (z, z, z if code == GAMMA_GRID else None)
    sweeps = DEFAULT_SWEEPS if sweeps is None else int(sweeps)
    max_rounds = int(max_rounds)
    rec = record_length(K, max_rounds)
    if draws is not None:
        draws = np.asarray(draws, dtype=float)
        if draws.shape != (sweeps, rec):
            raise ValueError("draws of one chain must be (sweeps, K + 1 + max_rounds) = (%d, %d), got %r" % (sweeps, rec, draws.shape))
    elif rng is None:
        rng = np.random.default_rng()
    restricted = any(v is not None and len(v) for v in (Constraints, Row_constraints, U))
    margin = {"ll": np.inf, "slack": np.inf}

    def ok(w):
        if not restricted:
            return True
        s = slacks(w, V, Constraints, Row_constraints, U)
        margin["slack"] = min(margin["slack"], float(np.min(np.abs(s)))) if s.size else margin["slack"]
        return bool(np.all(s >= 0))

    def ll_of(w):
        v = loglik(code, param, stats, V, w)
        if U is not None and x_codes is not None and len(U):
            v += feature_term(w, U, x_codes)
        return v

    out = {"w": np.full(K, np.nan), "rounds": 0, "unfinished": 0, "failed": True, "margin_ll": np.inf, "margin_slack": np.inf}
    ll = ll_of(x) if ok(x) else np.nan
    if not np.isfinite(ll):
        return out
    sd = np.sqrt(float(sigma2))
    rounds = unfinished = 0
    for sw in range(sweeps):
        if draws is not None:
            d = draws[sw]
        else:
            d = np.concatenate([rng.standard_normal(K), rng.uniform(size=rec - K)])
        nu = sd * d[:K]
        hh = ll + np.log(d[K])
        phi = 2.0 * np.pi * d[K + 1]
        lo, hi = phi - 2.0 * np.pi, phi
        accepted = False
        for rd in range(max_rounds):
            xp = x * np.cos(phi) + nu * np.sin(phi)
            if ok(xp):
                rounds += 1
                llp = ll_of(xp)
                if np.isfinite(llp):
                    margin["ll"] = min(margin["ll"], abs(llp - hh))
                if llp >= hh:
                    x, ll, accepted = xp, llp, True
                    break
            if phi > 0:
                hi = phi
            else:
                lo = phi
            if rd + 1 < max_rounds:
                phi = lo + (hi - lo) * d[K + 2 + rd]
        if not accepted:
            unfinished += 1
    out.update(w=x, rounds=rounds, unfinished=unfinished, failed=False, margin_ll=margin["ll"], margin_slack=margin["slack"])
    return out


def chains(starts, Vs, sigma2, family, param=None, stats=None, Constraints=None, Row_constraints=None, Us=None, x_codes=None,
           draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS):
    """`chain` for every (sample, row): starts (S,R,K), Vs (S,M,T,K), sigma2 (S,), stats = (S1, cnt, L) each (R,M,T), Us
    (S,F,K), x_codes (R,F), draws (S,R,sweeps,K+1+max_rounds).  Returns W (S,R,K), rounds and unfinished (S,R), and the
    smallest margins over all chains."""
    starts = np.asarray(starts, dtype=float)
    S, R, K = starts.shape
    W = np.zeros((S, R, K))
    rounds, unf = np.zeros((S, R), dtype=np.int32), np.zeros((S, R), dtype=np.int32)
    mll = msl = np.inf
    for s in range(S):
        for r in range(R):
            st = None if stats is None else (stats[0][r], stats[1][r], None if stats[2] is None else stats[2][r])
            o = chain(starts[s, r], Vs[s], np.reshape(sigma2, -1)[s], family, param, st, Constraints, Row_constraints,
                      None if Us is None else Us[s], None if x_codes is None else x_codes[r],
                      None if draws is None else draws[s, r], rng, sweeps, max_rounds)
            W[s, r], rounds[s, r], unf[s, r] = o["w"], o["rounds"], o["unfinished"]
            mll, msl = min(mll, o["margin_ll"]), min(msl, o["margin_slack"])
    return {"W": W, "rounds": rounds, "unfinished": unf, "margin_ll": mll, "margin_slack": msl}


def check_constraints(Constraints, Row_constraints, T, K):
    """(Constraints (J,T+1) or None, Row_constraints (n,K+1) or None) as contiguous float64 arrays; ValueError otherwise."""
    from . import _native
    if Constraints is not None:
        Constraints = _native.as_f64(np.atleast_2d(Constraints))
        if Constraints.ndim != 2 or Constraints.shape[1] != T + 1 or not np.all(np.isfinite(Constraints)):
            raise ValueError("Constraints must be a finite (J, ndepth + 1) = (J, %d) array: the bound in the last column" % (T + 1))
        if Constraints.shape[0] == 0:
            Constraints = None
    if Row_constraints is not None:
        Row_constraints = _native.as_f64(np.atleast_2d(Row_constraints))
        if Row_constraints.ndim != 2 or Row_constraints.shape[1] != K + 1 or not np.all(np.isfinite(Row_constraints)):
            raise ValueError("Row_constraints must be a finite (n, nembeds + 1) = (n, %d) array" % (K + 1))
        if Row_constraints.shape[0] == 0:
            Row_constraints = None
    return Constraints, Row_constraints


def check_args(family, param, S, R, K, start=None, draws=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95),
               transform=None, first_sample=0, Us=None, codes=None, have_W=True):
    """Validate and normalise; raises ValueError before any device call.  Returns (family code, param, start (S,R,K) or
    None, draws or None, sweeps, max_rounds, qs, transform code, Us or None)."""
    from . import _native
    code = family_code(family)
    param = check_param(family, param)
    if int(S) < 1 or int(R) < 1:
        raise ValueError("slice_fold_in_rows: at least one sample and one row")
    if not 1 <= int(K) <= 10:
        raise ValueError("slice_fold_in_rows: nembeds must be 1..10")
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("slice_fold_in_rows: %d samples exceed the %d of the summary kernel; thin the samples or pass "
                         "summary=False" % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(R) >= 2 ** 31:
        raise ValueError("slice_fold_in_rows: first_sample must be >= 0 and (first_sample + S) * R below 2^31")
    qs = check_q(q, allow_none=True) if summary else np.zeros(0)
    if sweeps is None:
        sweeps = DEFAULT_SWEEPS
    if int(sweeps) != sweeps or int(sweeps) < 1:
        raise ValueError("sweeps must be a positive integer")
    if int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= 65536:
        raise ValueError("max_rounds must be an integer in 1..65536")
    sweeps, max_rounds = int(sweeps), int(max_rounds)
    if start is not None:
        start = np.asarray(start, dtype=np.float64)
        if start.shape not in ((K,), (R, K), (S, R, K)):
            raise ValueError("start must be (K,), (R,K) or (S,R,K) with S,R,K = %d,%d,%d, got %r" % (S, R, K, start.shape))
        if not np.all(np.isfinite(start)):
            raise ValueError("start must be finite")
        start = np.ascontiguousarray(np.broadcast_to(start, (S, R, K)))
    elif not have_W:
        raise ValueError("slice_fold_in_rows: without start= the fitted rows Ws (S,N,K) are needed (the default start is their mean)")
    if draws is not None:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        want = (S, R, sweeps, record_length(K, max_rounds))
        if draws.shape != want:
            raise ValueError("draws must be (S,R,sweeps,K+1+max_rounds) = %r, got %r" % (want, draws.shape))
        if not np.all(np.isfinite(draws)) or np.any(draws[..., K:] <= 0) or np.any(draws[..., K:] >= 1):
            raise ValueError("draws: finite normals, then uniforms strictly inside (0, 1)")
    if codes is not None:
        if Us is None:
            raise ValueError("row_features needs the feature embeddings U (S,F,K) of every kept sample (results['U'])")
        Us = _native.as_f64(Us)
        if Us.shape != (S, codes.shape[1], K) or not np.all(np.isfinite(Us)):
            raise ValueError("U must be a finite (S,F,K) = (%d,%d,%d) array, got %r" % (S, codes.shape[1], K, Us.shape))
    else:
        Us = None
    return code, param, start, draws, sweeps, max_rounds, qs, tcode, Us


def evaluate(family, param, S, R, M, T, K, S1, cnt, L, start=None, Constraints=None, Row_constraints=None, Us=None, codes=None,
             draws=None, seed=0, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95), transform=None, first_sample=0,
             ctx=None, Vs=None, Ws=None, sigma2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Vs None: the context's first S collected samples (no upload; W, V
    and sigma2 from the collected slots, the likelihood's parameter or table from the context); otherwise Vs (S,M,T,K),
    sigma2 (S,) and - without a start - Ws (S,N,K) are uploaded (stateless entry point).  Returns the dict of
    NonconjugateBayesianTensorFiltering.slice_fold_in_rows."""
    import ctypes
    from . import _native
    code, param, start, draws, sweeps, max_rounds, qs, tcode, Us = check_args(
        family, param, S, R, K, start, draws, sweeps, max_rounds, summary, q, transform, first_sample, Us, codes,
        have_W=Vs is None or Ws is not None)
    Constraints, Row_constraints = check_constraints(Constraints, Row_constraints, T, K)
    W = np.zeros((S, R, K))
    W0 = np.zeros((S, R, K))
    rounds = np.zeros((S, R), dtype=np.int32)
    unf = np.zeros((S, R), dtype=np.int32)
    mean = np.zeros((R, M, T)) if summary else None
    quant = np.zeros((len(qs), R, M, T)) if summary else None
    d = _native.dptr
    ip = lambda a: a.ctypes.data_as(_native._c_ip)
    F = 0 if codes is None else int(codes.shape[1])
    mid = (d(start), d(S1), d(cnt), d(L), d(Constraints), 0 if Constraints is None else int(Constraints.shape[0]),
           d(Row_constraints), 0 if Row_constraints is None else int(Row_constraints.shape[0]), d(Us), F,
           codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if F else None, d(draws), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps,
           max_rounds, int(first_sample), d(W), d(W0), ip(rounds), ip(unf), tcode, d(qs) if len(qs) else None, len(qs), d(mean),
           d(quant) if len(qs) else None)
    if Vs is None:
        ctx.call("btf_collect_slice_fold", code, int(S), int(R), *mid)
    else:
        lib = _native.load()
        par = 0.0 if param is None or code == GAMMA_GRID else (1.0 / param if code == 3 else param)
        tab = param if code == GAMMA_GRID else (None, None, None)
        G = int(tab[0].size) if code == GAMMA_GRID else 0
        N = 0 if Ws is None or start is not None else int(Ws.shape[1])
        _native.check(lib.btf_slice_fold_rows(int(device), code, float(par), d(tab[0]), d(tab[1]), d(tab[2]), G, int(S), int(R), int(M),
                                              int(T), int(K), d(Vs), d(Ws) if start is None else None, N, mid[0], d(sigma2), *mid[1:]),
                      lib, fail_index=False)
    out = {"W": W, "W_start": W0, "rounds": rounds, "unfinished": unf, "nsamples": int(S)}
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
