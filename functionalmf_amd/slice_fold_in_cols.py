"""Folding new columns into a slice-sampled fit: the curves of a column the chain never saw, per kept sample, for the
models that have no conjugate column conditional (NonconjugateBayesianTensorFiltering and its constrained subclass).

Given a kept sample's W_s and lam2_s the new column's curve v (T,K; depth-major, index t K + k) and its four horseshoe+
levels form a small chain of their own, as in fold_in_cols - but the curve has no closed-form draw.  Its prior given the
levels is N(0, (P (x) I_K)^-1), P = Delta' diag(1 / (lam2 tau2)) Delta, and every restriction on it is linear in v given
W_s: sum_t A[q,t] (w_i . v_t) >= C[q] for EVERY fitted row i (the reference's _v_constraints, factor.py:847-854), so the
feasible set is convex.  Plain elliptical slice sampling on the prior ellipse is valid but mixes far too slowly here (the
prior is much wider than the likelihood: DESIGN.md, "Folding new columns into a slice-sampled fit"), so the ellipse is
centred on a Gaussian fit of the likelihood, as the reference does for a constrained column with ep_approx
(factor.py:771-793, :891): with per-cell fits N(Mu_fit | eta, Sigma_fit), weights a_it = 1 / Sigma_fit^2 and sums
a_it Mu_fit enter exactly as the Gaussian weights / sums of fold_in_cols._system,

    Q = blockdiag_t(sum_i a_it w_i w_i') + P (x) I_K,   m = Q^-1 b,   b_t = sum_i a_it Mu_it w_i,

the sweep draws nu = L^-T z (Q = L L'), proposes v' = m + (v - m) cos phi + nu sin phi and accepts when v' is feasible and
r(v') >= r(v) + log u_h, where

    r(v) = loglik(v) + sum_{cells with a fit} eta_it (a_it eta_it / 2 - a_it Mu_it)          eta_it = w_i . v_t

is the log-likelihood divided by the fit (the second term is - log N(Mu_fit | eta, Sigma_fit) without what does not depend
on v).  N(v; m, Q^-1) r(v) 1[feasible] is the conditional of v whatever the fit: THE FIT CHANGES ONLY THE MIXING, NEVER THE
TARGET.  With an exact fit (Gaussian family) r is constant and every proposal is accepted in its first round: the sweep is
the Gibbs draw of fold_in_cols.  The levels are then updated exactly as in fold_in_cols.chain.

The data-sized work is the HIP of csrc/btf_slice_fold_cols.h (btf_slice_fold_cols / btf_collect_slice_fold_cols); this
module holds the host halves in plain numpy (importable without a GPU): the DEFINITION the kernel is tested against
(`chain`), the default fit (`gaussian_fit`), the argument checks, and `evaluate`, the one caller of the C entry points.

The default fit, per observed cell with n replicates, sum S1 and mean ybar = S1 / n, on the scale of eta (delta method;
`multiplier` times the sd, 2 by default - an over-wide fit costs a few more proposals, a too narrow one many):
    gaussian (variance s2)      Mu = ybar                          sd = sqrt(s2 / n)
    poisson_identity            Mu = (S1 + 1/2) / n                sd = sqrt(Mu / n)
    gamma_grid                  Mu = ybar / mbar                   sd = Mu sqrt((m2 / mbar^2 - 1) / n)
                                mbar = sum_g p_g a_g s_g, m2 = sum_g p_g a_g (a_g + 1) s_g^2   (p normalised)
    poisson_log                 Mu = log((S1 + 1/2) / n)           sd = 1 / sqrt(S1 + 1/2)
    negbin_logit (rate r)       Mu = log(mu / r), mu = (S1 + 1/2) / n      sd = sqrt((1 + mu / r) / (n mu))
    bernoulli_logit             Mu = logit(p), p = (S1 + 1/2) / (n + 1)    sd = 1 / sqrt((n + 1) p (1 - p))
Nothing asserts the quality of this fit except the sweeps study behind DEFAULT_SWEEPS.
"""
import numpy as np

from . import fold_in_cols as _fc, slice_fold_in as _sf
from ._analysis import check_q, transform_code

FAMILIES = _sf.FAMILIES
GAMMA_GRID = _sf.GAMMA_GRID
MAX_SUMMARY_SAMPLES = _sf.MAX_SUMMARY_SAMPLES
DEFAULT_MAX_ROUNDS = _sf.DEFAULT_MAX_ROUNDS
LDS_LIMIT = _fc.LDS_LIMIT        # SCOLS_LDS_LIMIT of csrc/btf_slice_fold_cols.h
STABILITY = _fc.STABILITY
STATIC_LDS = 2 * 128 * 16 + 128 * 32      # the exp / log tables and the gamma-grid components of the kernel (static LDS)
# sweeps per (sample, column): the smallest power of two after which the largest standardised difference of the curve
# means no longer falls on z_problem against the stored Gibbs moments, with the default fit (largest |z| at S = 16384:
# 22.1 at 256, 4.3 at 512, 0.8 at 1024, 1.3 at 2048).  At the dose-response-like shape (T = 9, K = 5, 26 constraints, gamma
# grid, a third of 60 rows observed) the difference against a 4096-sweep run is STILL FALLING at 2048 sweeps (largest mean
# error 1.78 reference sd at 256, 0.74 at 1024, 0.35 at 2048): there the default is short of the noise floor, and a closer
# fit= or more sweeps= pay ("Folding new columns into a slice-sampled fit", table of
# scripts/slice_fold_in_cols_rate.py --step sweeps)
DEFAULT_SWEEPS = 1024


def sweep_length(T, K, tf_order, max_rounds=DEFAULT_MAX_ROUNDS):
    """Numbers one sweep consumes: T K normals, u_h, u_a, the max_rounds - 1 shrink uniforms, 4 nD gammas."""
    return int(T) * int(K) + 1 + int(max_rounds) + 4 * _fc.penalty(T, tf_order).shape[0]


def record_length(T, K, tf_order, sweeps, max_rounds=DEFAULT_MAX_ROUNDS):
    """Length of the flat `draws` of one chain: 4 nD start gammas, then `sweeps` records of sweep_length."""
    return 4 * _fc.penalty(T, tf_order).shape[0] + int(sweeps) * sweep_length(T, K, tf_order, max_rounds)


def lds_bytes(T, K, tf_order):
    """LDS one chain's workgroup needs (scols_lds_bytes of csrc/btf_slice_fold_cols.h): the band of Q, (T K) x (half
    bandwidth + 1) doubles; six T K vectors (v, m, nu, v', b, the pivots); the fit blocks T K (K + 1) / 2; the five level
    arrays 5 nD; the prior band T (tf_order + 2); the pair table of the factorisation; and the static tables."""
    T, K, tf = int(T), int(K), int(tf_order)
    n, bw, nD = T * K, _fc.half_bandwidth(K, tf), _fc.penalty(T, tf).shape[0]
    npairs = bw * (bw + 1) // 2
    return 8 * (n * (bw + 1) + 6 * n + T * (K * (K + 1) // 2) + 5 * nD + T * (tf + 2)) + 8 * ((npairs + 3) // 4) + STATIC_LDS


def random_draws(rng, T, K, tf_order, sweeps, max_rounds=DEFAULT_MAX_ROUNDS, size=()):
    """`draws` for `chain` from a numpy Generator or RandomState, in the chain's layout; size: the leading shape (e.g.
    (S, C))."""
    nD, n = _fc.penalty(T, tf_order).shape[0], int(T) * int(K)
    size = tuple(int(x) for x in size)
    parts = [rng.standard_gamma(0.5, size=size + (4 * nD,))]
    shapes = np.ones((4, nD))
    shapes[0] = (K + 1) / 2.0
    for _ in range(int(sweeps)):
        parts.append(rng.normal(size=size + (n,)))
        parts.append(rng.uniform(size=size + (1 + int(max_rounds),)))
        parts.append(rng.standard_gamma(np.broadcast_to(shapes.reshape(-1), size + (4 * nD,))))
    return np.concatenate(parts, axis=-1)


def column_statistics(Y_new, family, N, T):
    """(C, S1 (C,N,T), cnt (C,N,T), L (C,N,T) or None) of the new columns: slice_fold_in.row_statistics on (C,N,T)."""
    try:
        return _sf.row_statistics(Y_new, family, N, T)
    except ValueError as e:
        raise ValueError(str(e).replace("(R,", "(C,"))


def gaussian_fit(Y_new, family, param=None, multiplier=2):
    """(Mu_fit, Sigma_fit), each (C,N,T): the default per-cell Gaussian fit of the likelihood on the scale of eta (the
    formulas of the module's docstring); nan where the cell has no observation.  The fit changes only the mixing of the
    sampler, never its target."""
    code = _sf.family_code(family)
    param = _sf.check_param(family, param)
    Y = np.asarray(Y_new, dtype=float)
    if Y.ndim == 3:
        Y = Y[..., None]
    if Y.ndim != 4:
        raise ValueError("Y_new %r must be (C,N,T) or (C,N,T,nreps)" % (np.shape(Y_new),))
    if not float(multiplier) > 0:
        raise ValueError("multiplier must be positive")
    obs = ~np.isnan(Y)
    n = obs.sum(axis=3).astype(float)
    S1 = np.where(obs, Y, 0.0).sum(axis=3)
    with np.errstate(divide="ignore", invalid="ignore"):
        ybar = S1 / n
        sm = (S1 + 0.5) / n
        if code == 3:
            mu, sd = ybar, np.sqrt(param / n)
        elif code == 1:
            mu, sd = sm, np.sqrt(sm / n)
        elif code == GAMMA_GRID:
            a, s, p = param
            p = p / p.sum()
            mbar, m2 = float(np.sum(p * a * s)), float(np.sum(p * a * (a + 1) * s * s))
            mu = ybar / mbar
            sd = mu * np.sqrt(max(m2 / mbar ** 2 - 1.0, 0.0) / n)
        elif code == 0:
            mu, sd = np.log(sm), 1.0 / np.sqrt(S1 + 0.5)
        elif code == 4:
            mu, sd = np.log(sm / param), np.sqrt((1.0 + sm / param) / (n * sm))
        else:
            p = (S1 + 0.5) / (n + 1.0)
            mu, sd = np.log(p / (1.0 - p)), 1.0 / np.sqrt((n + 1.0) * p * (1.0 - p))
        sd = float(multiplier) * sd
    ok = (n > 0) & np.isfinite(mu) & np.isfinite(sd) & (sd > 0)
    return np.where(ok, mu, np.nan), np.where(ok, sd, np.nan)


def fit_weights(fit, C, N, T):
    """(weights a = 1 / Sigma^2, sums a Mu), each (C,N,T), of fit = (Mu, Sigma); a nan or non-positive sd (or a nan mean)
    means the cell carries no fit (both 0).  fit None / False: no cell has one (the plain prior ellipse: slow)."""
    if fit is None or fit is False:
        z = np.zeros((C, N, T))
        return z, z.copy()
    if not isinstance(fit, (tuple, list)) or len(fit) != 2:
        raise ValueError("fit must be a pair (Mu_fit, Sigma_fit) of (C,N,T) arrays")
    Mu, Sg = np.asarray(fit[0], dtype=float), np.asarray(fit[1], dtype=float)
    if Mu.shape != (C, N, T) or Sg.shape != (C, N, T):
        raise ValueError("fit: Mu_fit %r and Sigma_fit %r must be (C,N,T) = (%d,%d,%d)" % (Mu.shape, Sg.shape, C, N, T))
    if np.isinf(Mu).any() or np.isinf(Sg).any():
        raise ValueError("fit must not hold infinite values (nan: the cell carries no fit)")
    ok = ~np.isnan(Mu) & ~np.isnan(Sg) & (np.nan_to_num(Sg) > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(ok, 1.0 / (np.where(ok, Sg, 1.0) ** 2), 0.0)
    return np.ascontiguousarray(a), np.ascontiguousarray(a * np.where(ok, Mu, 0.0))


def slacks(v, W, Constraints):
    """A (W v') - c for every (fitted row, constraint), as one array (empty without constraints)."""
    if Constraints is None or not len(Constraints):
        return np.zeros(0)
    C = np.atleast_2d(np.asarray(Constraints, dtype=float))
    eta = np.asarray(W, dtype=float).dot(np.asarray(v, dtype=float).T)           # (N,T)
    return (eta.dot(C[:, :-1].T) - C[:, -1][None]).reshape(-1)


def chain(start, W, lam2, tf_order, family, param=None, stats=None, weights=None, sums=None, Constraints=None, tau2=None,
          draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, stability=STABILITY, nu_scale=1.0, track_cond=True):
    """The chain of one (sample, column) in numpy: the definition (see the module's docstring for the method).

    start (T,K); W (N,K); stats = (S1, cnt, L) of the column, each (N,T) (None: a column without observations); weights /
    sums (N,T): fit_weights of the column (None: no fit); Constraints (J,T+1); tau2 (nD,): the local scales held fixed
    (the level update is skipped; the record keeps its layout).  draws: the flat record (record_length) - 4 nD start
    gammas (shape 1/2), then per sweep T K normals, u_h, u_a, max_rounds - 1 shrink uniforms and 4 nD gammas (shapes
    (K + 1) / 2, 1, 1, 1) - or None: drawn from rng.  nu_scale multiplies every nu (the tests perturb the definition with it).

    Returns a dict: v (T,K) - nan when the start is infeasible or has a non-finite likelihood (failed=True; the chain does
    not run) -, tau2 (nD,), rounds (likelihood evaluations of proposals), unfinished (sweeps that hit the cap),
    margin_ll = min |r(v') - hh|, margin_slack = the smallest absolute constraint slack met, cond = the largest cond(Q) (0 with track_cond=False)."""
    code = family if isinstance(family, int) else _sf.family_code(family)
    W = np.asarray(W, dtype=float)
    N, K = W.shape
    v = np.array(start, dtype=float)
    T = v.shape[0]
    if v.shape != (T, K):
        raise ValueError("start must be (T,K)")
    n = T * K
    D = _fc.penalty(T, tf_order)
    nD = D.shape[0]
    sweeps = DEFAULT_SWEEPS if sweeps is None else int(sweeps)
    max_rounds = int(max_rounds)
    per = sweep_length(T, K, tf_order, max_rounds)
    if draws is None:
        draws = random_draws(np.random.default_rng() if rng is None else rng, T, K, tf_order, sweeps, max_rounds)
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if sweeps < 1 or draws.size != 4 * nD + sweeps * per:
        raise ValueError("draws of one chain must hold 4 nD + sweeps (T K + 1 + max_rounds + 4 nD) = %d values, got %d"
                         % (4 * nD + sweeps * per, draws.size))
    if stats is None:
        z = np.zeros((N, T))
        stats = (z, z, z if code == GAMMA_GRID else None)
    S1, cnt, L = (None if a is None else np.asarray(a, dtype=float) for a in stats)
    weights = np.zeros((N, T)) if weights is None else np.asarray(weights, dtype=float)
    sums = np.zeros((N, T)) if sums is None else np.asarray(sums, dtype=float)
    obs = cnt > 0
    st_obs = (S1[obs], cnt[obs], None if L is None else L[obs])
    has_fit = weights > 0
    wf, sf = weights[has_fit], sums[has_fit]
    restricted = Constraints is not None and len(Constraints) > 0
    margin = {"ll": np.inf, "slack": np.inf}
    lo, hi = float(stability), 1.0 / float(stability)

    def ok(x):
        if not restricted:
            return True
        s = slacks(x, W, Constraints)
        margin["slack"] = min(margin["slack"], float(np.min(np.abs(s))))
        return bool(np.all(s >= 0))

    def r_of(x):
        eta = W.dot(x.T)
        val = _sf.loglik_eta(code, param, st_obs, eta[obs]) if obs.any() else 0.0
        ef = eta[has_fit]
        return val + float(np.sum(ef * (0.5 * wf * ef - sf)))

    fixed = tau2 is not None
    if fixed:
        tau, c, b, a = np.asarray(tau2, dtype=float).reshape(nD), None, None, None
    else:
        tau, c, b, a = _fc.start_levels(draws[:4 * nD].reshape(4, nD))
    out = {"v": np.full((T, K), np.nan), "tau2": np.full(nD, np.nan), "rounds": 0, "unfinished": 0, "failed": True,
           "margin_ll": np.inf, "margin_slack": np.inf, "cond": 0.0}
    ll = r_of(v) if ok(v) else np.nan
    if not np.isfinite(ll):
        return out
    A_fit, b_fit = _fc._blocks(weights, sums, W)
    rounds = unfinished = 0
    cond = 0.0
    pos = 4 * nD
    two_pi = 2.0 * np.pi
    for sw in range(sweeps):
        d = draws[pos:pos + per]
        pos += per
        if sw == 0 or not fixed:
            m, Q = _fc._system_of_blocks(A_fit, b_fit, lam2, tau, tf_order)
            m = m.reshape(T, K)
            if track_cond:
                cond = max(cond, float(np.linalg.cond(Q)))
            Lc = np.linalg.cholesky(Q)
        nu = float(nu_scale) * np.linalg.solve(Lc.T, d[:n]).reshape(T, K)
        hh = ll + np.log(d[n])
        phi = two_pi * d[n + 1]
        blo, bhi = phi - two_pi, phi
        accepted = False
        for rd in range(max_rounds):
            xp = m + (v - m) * np.cos(phi) + nu * np.sin(phi)
            if ok(xp):
                rounds += 1
                llp = r_of(xp)
                if np.isfinite(llp):
                    margin["ll"] = min(margin["ll"], abs(llp - hh))
                if llp >= hh:
                    v, ll, accepted = xp, llp, True
                    break
            if phi > 0:
                bhi = phi
            else:
                blo = phi
            if rd + 1 < max_rounds:
                phi = blo + (bhi - blo) * d[n + 2 + rd]
        if not accepted:
            unfinished += 1
        if not fixed:
            g = d[n + 1 + max_rounds:].reshape(4, nD)
            dv = D.dot(v)
            rate = (dv * dv).sum(axis=1) / (2.0 * float(lam2)) + 1.0 / np.clip(c, lo, hi)
            tau = np.clip(rate, lo, hi) / g[0]
            c = np.clip(1.0 / tau + 1.0 / b, lo, hi) / g[1]
            b = np.clip(1.0 / c + 1.0 / a, lo, hi) / g[2]
            a = np.clip(1.0 / b + 1.0, lo, hi) / g[3]
    out.update(v=v, tau2=np.array(tau, dtype=float), rounds=rounds, unfinished=unfinished, failed=False, margin_ll=margin["ll"],
               margin_slack=margin["slack"], cond=cond)
    return out


def chains(starts, Ws, lam2, tf_order, family, param=None, stats=None, weights=None, sums=None, Constraints=None, tau2=None,
           draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, stability=STABILITY, nu_scale=1.0):
    """`chain` for every (sample, column): starts (S,C,T,K), Ws (S,N,K), lam2 (S,), stats = (S1, cnt, L) each (C,N,T),
    weights / sums (C,N,T), tau2 (S,C,nD) or None, draws (S,C,record_length).  Returns V (S,C,T,K), Tau2 (S,C,nD), rounds
    and unfinished (S,C), the smallest margins and the largest cond(Q) over all chains."""
    starts = np.asarray(starts, dtype=float)
    S, C, T, K = starts.shape
    nD = _fc.penalty(T, tf_order).shape[0]
    V, Tau2 = np.zeros((S, C, T, K)), np.zeros((S, C, nD))
    rounds, unf = np.zeros((S, C), dtype=np.int32), np.zeros((S, C), dtype=np.int32)
    mll = msl = np.inf
    cond = 0.0
    for s in range(S):
        for c in range(C):
            st = None if stats is None else (stats[0][c], stats[1][c], None if stats[2] is None else stats[2][c])
            o = chain(starts[s, c], Ws[s], np.reshape(lam2, -1)[s], tf_order, family, param, st,
                      None if weights is None else weights[c], None if sums is None else sums[c], Constraints,
                      None if tau2 is None else tau2[s, c], None if draws is None else draws[s, c], rng, sweeps, max_rounds,
                      stability, nu_scale)
            V[s, c], Tau2[s, c], rounds[s, c], unf[s, c] = o["v"], o["tau2"], o["rounds"], o["unfinished"]
            mll, msl, cond = min(mll, o["margin_ll"]), min(msl, o["margin_slack"]), max(cond, o["cond"])
    return {"V": V, "Tau2": Tau2, "rounds": rounds, "unfinished": unf, "margin_ll": mll, "margin_slack": msl, "cond": cond}


def check_args(family, param, S, C, N, T, K, tf_order, start=None, tau2=None, draws=None, sweeps=None,
               max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95), transform=None, first_sample=0, have_V=True):
    """Validate and normalise; raises ValueError before any device call.  Returns (family code, param, start (S,C,T,K) or
    None, tau2 (S,C,nD) or None, draws or None, sweeps, max_rounds, qs, transform code)."""
    code = _sf.family_code(family)
    param = _sf.check_param(family, param)
    if int(S) < 1 or int(C) < 1 or int(N) < 1:
        raise ValueError("slice_fold_in_cols: at least one sample, one column and one fitted row")
    if not 1 <= int(K) <= 10:
        raise ValueError("slice_fold_in_cols: nembeds must be 1..10")
    if int(tf_order) < 0 or int(T) < 2:
        raise ValueError("slice_fold_in_cols: tf_order >= 0 and ndepth >= 2")
    if _fc.half_bandwidth(K, tf_order) >= 64:
        raise ValueError("slice_fold_in_cols: the half bandwidth (tf_order + 1) nembeds = %d must stay below 64"
                         % _fc.half_bandwidth(K, tf_order))
    need = lds_bytes(T, K, tf_order)
    if need > LDS_LIMIT:
        raise ValueError("slice_fold_in_cols: the band of a column at ndepth %d, nembeds %d, tf_order %d needs %d bytes of LDS, "
                         "beyond the limit of %d bytes a workgroup may hold" % (T, K, tf_order, need, LDS_LIMIT))
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("slice_fold_in_cols: %d samples exceed the %d of the summary kernel; thin the samples or pass "
                         "summary=False" % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(C) >= 2 ** 31:
        raise ValueError("slice_fold_in_cols: first_sample must be >= 0 and (first_sample + S) * C below 2^31")
    qs = check_q(q, allow_none=True) if summary else np.zeros(0)
    if sweeps is None:
        sweeps = DEFAULT_SWEEPS
    if int(sweeps) != sweeps or not 1 <= int(sweeps) < 2 ** 20 - 1:
        raise ValueError("sweeps must be a positive integer (below 2^20 - 1)")
    if int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= 65536:
        raise ValueError("max_rounds must be an integer in 1..65536")
    sweeps, max_rounds = int(sweeps), int(max_rounds)
    nD, n = _fc.penalty(T, tf_order).shape[0], int(T) * int(K)
    if start is not None:
        start = np.asarray(start, dtype=np.float64)
        if start.shape not in ((T, K), (C, T, K), (S, C, T, K)):
            raise ValueError("start must be (T,K), (C,T,K) or (S,C,T,K) with S,C,T,K = %d,%d,%d,%d, got %r" % (S, C, T, K, start.shape))
        if not np.all(np.isfinite(start)):
            raise ValueError("start must be finite")
        start = np.ascontiguousarray(np.broadcast_to(start, (S, C, T, K)))
    elif not have_V:
        raise ValueError("slice_fold_in_cols: without start= the fitted columns Vs (S,M,T,K) are needed (the default start is "
                         "their mean)")
    if tau2 is not None:
        tau2 = np.asarray(tau2, dtype=np.float64)
        if tau2.shape not in ((C, nD), (S, C, nD)):
            raise ValueError("tau2 must be (C,nD) or (S,C,nD) = (%d,%d,%d), got %r" % (S, C, nD, tau2.shape))
        if not (np.all(np.isfinite(tau2)) and np.all(tau2 > 0)):
            raise ValueError("tau2 must be finite and positive")
        tau2 = np.ascontiguousarray(np.broadcast_to(tau2, (S, C, nD)))
    if draws is not None:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        per = sweep_length(T, K, tf_order, max_rounds)
        want = (S, C, 4 * nD + sweeps * per)
        if draws.shape != want:
            raise ValueError("draws must be (S,C,4 nD + sweeps (T K + 1 + max_rounds + 4 nD)) = %r, got %r" % (want, draws.shape))
        if not np.all(np.isfinite(draws)):
            raise ValueError("draws must be finite")
        body = draws[..., 4 * nD:].reshape(S, C, sweeps, per)
        uni = body[..., n:n + 1 + max_rounds]
        if np.any(uni <= 0) or np.any(uni >= 1):
            raise ValueError("draws: the uniforms of every sweep must lie strictly inside (0, 1)")
        if not (np.all(draws[..., :4 * nD] > 0) and np.all(body[..., n + 1 + max_rounds:] > 0)):
            raise ValueError("the gamma variates of draws must be positive")
    return code, param, start, tau2, draws, sweeps, max_rounds, qs, tcode


def evaluate(family, param, S, C, N, T, K, tf_order, S1, cnt, L, weights, sums, start=None, Constraints=None, tau2=None,
             draws=None, seed=0, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95), transform=None,
             first_sample=0, stability=STABILITY, ctx=None, Ws=None, Vs=None, lam2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Ws None: the context's first S collected samples (no upload; W, V
    and lam2 from the collected slots, the likelihood's parameter or table from the context); otherwise Ws (S,N,K), lam2
    (S,) and - without a start - Vs (S,M,T,K) are uploaded (stateless entry point).  S1 / cnt / L: column_statistics;
    weights / sums: fit_weights.  Returns the dict of NonconjugateBayesianTensorFiltering.slice_fold_in_cols."""
    from . import _native
    code, param, start, tau2, draws, sweeps, max_rounds, qs, tcode = check_args(
        family, param, S, C, N, T, K, tf_order, start, tau2, draws, sweeps, max_rounds, summary, q, transform, first_sample,
        have_V=Ws is None or Vs is not None)
    Constraints, _ = _sf.check_constraints(Constraints, None, T, K)
    nD = _fc.penalty(T, tf_order).shape[0]
    V = np.zeros((S, C, T, K))
    V0 = np.zeros((S, C, T, K))
    Tau2 = np.zeros((S, C, nD))
    rounds = np.zeros((S, C), dtype=np.int32)
    unf = np.zeros((S, C), dtype=np.int32)
    mean = np.zeros((N, C, T)) if summary else None
    quant = np.zeros((len(qs), N, C, T)) if summary else None
    d = _native.dptr
    ip = lambda a: a.ctypes.data_as(_native._c_ip)
    tail = (d(start), d(S1), d(cnt), d(L), d(weights), d(sums), d(Constraints), 0 if Constraints is None else int(Constraints.shape[0]),
            d(tau2), d(draws), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, max_rounds, int(first_sample), float(stability), d(V), d(V0),
            d(Tau2), ip(rounds), ip(unf), tcode, d(qs) if len(qs) else None, len(qs), d(mean), d(quant) if len(qs) else None)
    if Ws is None:
        ctx.call("btf_collect_slice_fold_cols", code, int(S), int(C), *tail)
    else:
        lib = _native.load()
        par = 0.0 if param is None or code == GAMMA_GRID else (1.0 / param if code == 3 else param)
        tab = param if code == GAMMA_GRID else (None, None, None)
        G = int(tab[0].size) if code == GAMMA_GRID else 0
        M = 0 if Vs is None or start is not None else int(Vs.shape[1])
        _native.check(lib.btf_slice_fold_cols(int(device), code, float(par), d(tab[0]), d(tab[1]), d(tab[2]), G, int(S), int(C), int(N),
                                              int(T), int(K), int(tf_order), d(Ws), d(Vs) if start is None else None, M, d(lam2),
                                              *tail), lib, fail_index=False)
    out = {"V": V, "V_start": V0, "Tau2": Tau2, "rounds": rounds, "unfinished": unf, "nsamples": int(S)}
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
