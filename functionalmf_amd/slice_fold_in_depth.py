"""Folding new depth slices into a slice-sampled fit: the curves at depths the chain never saw, per kept sample and fitted
column, for the models that have no conjugate column conditional (NonconjugateBayesianTensorFiltering and its constrained
subclass) - the sixth cell of the fold-in family.

The call composes its two neighbours and restates nothing of them.  fold_in_depth defines the PRIOR SIDE: the new penalty
rows R of the operator on T + H points, D'[R] = [D_o | D_n], the offsets off = D_o V_s[j] from the kept tail of the curve,
fresh horseshoe+ levels on the rows of R, and the Gaussian system

    (m, Q) = fold_in_depth._system(a, a Mu, W_s, lam2_s, tau2, off, D_n)

with the per-cell fit weights a = 1 / Sigma_fit^2 and sums a Mu_fit in the place of the Gaussian counts and sums.
slice_fold_in_cols defines the CURVE UPDATE on the H K new coordinates v (H,K; depth-major): nu = L^-T z (Q = L L'),
hh = r(v) + log u_h, phi = 2 pi u_a, propose v' = m + (v - m) cos phi + nu sin phi, accept when v' is feasible and
r(v') >= hh, else shrink the bracket; at most max_rounds proposals, a sweep at the cap keeps its state and counts as
unfinished;

    r(v) = loglik over the observed new cells + sum over fitted cells of eta (a eta / 2 - a Mu),    eta_ih = w_i . v_h.

As there, THE FIT CHANGES ONLY THE MIXING, NEVER THE TARGET, and with an exact fit (Gaussian family) every proposal is
accepted in its first round: the sweep is the Gibbs draw of fold_in_depth.  The levels follow fold_in_depth.chain with
dv = off + D_n v.

The one new ingredient: a constraint on the extended grid may couple a new depth with kept ones (v_{T-1} - v_T >= -1e-2).
`reduce_constraints` keeps the rows of Constraints (J, T + H + 1) with a non-zero at a new depth - the others do not depend
on the new curve - and cuts them to the B trailing kept depths they reach; a state is feasible when

    sum_t A_o[q,t] (w_i . V_old[T - B + t]) + sum_h A_n[q,h] (w_i . v_h) >= c[q]     for EVERY fitted row i and every kept q.

Kept and new eta go through one dot-product routine (`eta_of`) and the terms of a slack are added in ascending depth order, so
a new depth that carries the bits of V_old[T - 1] - the default start - ties exactly: a row (+1, -1) against bound 0
evaluates to exactly 0 and passes.  With Y_new=None the call is the CONSTRAINED FORECAST: the prior continuation truncated
to the feasible set.

The data-sized work is the HIP of csrc/btf_slice_fold_depth.h (btf_slice_fold_depth / btf_collect_slice_fold_depth); this
module holds the host halves in plain numpy (importable without a GPU): the DEFINITION the kernel is tested against
(`chain`), the argument checks, and `evaluate`, the one caller of the C entry points.
"""
import numpy as np

from . import fold_in_cols as _fc, fold_in_depth as _fd, slice_fold_in as _sf, slice_fold_in_cols as _sc
from ._analysis import check_q, transform_code

FAMILIES = _sf.FAMILIES
GAMMA_GRID = _sf.GAMMA_GRID
MAX_SUMMARY_SAMPLES = _sf.MAX_SUMMARY_SAMPLES
DEFAULT_MAX_ROUNDS = _sf.DEFAULT_MAX_ROUNDS
LDS_LIMIT = _fc.LDS_LIMIT        # SDEPTH_LDS_LIMIT of csrc/btf_slice_fold_depth.h
STABILITY = _fc.STABILITY
STATIC_LDS = _sc.STATIC_LDS      # the exp / log tables and the gamma-grid components of the kernel (static LDS)
MAX_GRID = _fd.MAX_GRID
# sweeps per (sample, fitted column), from scripts/slice_fold_in_depth_rate.py --step sweeps (CPU, numpy, the default fit, 256
# replicates): the largest standardised difference of the curve means W v at 8, 16, ..., 1024 sweeps against a chain eight
# times longer than the largest count (8192 sweeps):
#     sweeps                                      8     16     32     64    128    256    512   1024
#     flu-like (Poisson identity, positivity)  12.60  12.17  11.42  10.21   8.74   7.55   6.83   4.38
#     dose-response-like (gamma grid, fit.py)   7.09   6.08   2.97   1.25   2.34   0.90   0.96   2.85
# The dose-response-like slice (T = 9, H = 2, K = 5, 32 constraints on the extended grid) stops falling at 64 sweeps.  At the
# flu-like slice (T = 40, H = 8, K = 10, a third of 50 rows observed) the difference is STILL FALLING at 1024 sweeps, the
# largest count tried (largest mean error 0.86 reference sd at 128, 0.41 at 1024): with fresh horseshoe+ levels and a chain
# that starts on the flat continuation - where the new differences are exactly zero and the levels collapse first - the
# level / curve pair mixes slowly, and the proposals are cheap (1.05 per sweep).  The default is the largest count tried;
# there it is short of the noise floor, and more sweeps= or fixed tau2= pay ("Folding new depth slices into a
# slice-sampled fit").
DEFAULT_SWEEPS = 1024


def reduce_constraints(Constraints, T, H):
    """(A_o (Jn,B), A_n (Jn,H), c (Jn,), B) of Constraints (J, T + H + 1) on the extended grid: the rows with a non-zero at a
    new depth (the others do not depend on the new curve), split into the B trailing kept depths they reach (0: none) and
    the H new depths, and their bounds.  None or an array with zero rows: no constraint (Jn = B = 0)."""
    T, H = int(T), int(H)
    if Constraints is None or np.size(Constraints) == 0:
        return np.zeros((0, 0)), np.zeros((0, H)), np.zeros(0), 0
    C = np.atleast_2d(np.asarray(Constraints, dtype=np.float64))
    if C.ndim != 2 or C.shape[1] != T + H + 1 or not np.all(np.isfinite(C)):
        raise ValueError("Constraints must be a finite (J, ndepth + horizon + 1) = (J, %d) array on the extended grid: the bound "
                         "in the last column" % (T + H + 1))
    keep = np.any(C[:, T:T + H] != 0.0, axis=1)
    C = C[keep]
    reach = np.flatnonzero(np.any(C[:, :T] != 0.0, axis=0))
    B = T - int(reach[0]) if reach.size else 0
    return np.ascontiguousarray(C[:, T - B:T]), np.ascontiguousarray(C[:, T:T + H]), np.ascontiguousarray(C[:, -1]), B


def eta_of(W, x):
    """w_i . x_t for every row of W (N,K) and every depth of x (D,K), the K terms added in ascending order: (N,D).  Every
    element goes through the same elementwise operations whatever the shapes are, so equal depths give equal bits."""
    W, x = np.asarray(W, dtype=float), np.asarray(x, dtype=float)
    eta = np.zeros((W.shape[0], x.shape[0]))
    for k in range(W.shape[1]):
        eta += W[:, k, None] * x[None, :, k]
    return eta


def reduced_slacks(v, W, V_old, reduced):
    """The slack of every (fitted row, kept constraint) at the new curve v (H,K), as one array (empty without constraints):
    the terms of a slack added in ascending depth order over the B kept and the H new depths, minus the bound."""
    A_o, A_n, c, B = reduced
    if not c.size:
        return np.zeros(0)
    V_old = np.asarray(V_old, dtype=float)
    T = V_old.shape[0]
    eta = eta_of(W, np.concatenate([V_old[T - B:], np.asarray(v, dtype=float)], axis=0))             # (N, B + H)
    A = np.concatenate([A_o, A_n], axis=1)
    acc = np.zeros((eta.shape[0], c.size))
    for t in np.flatnonzero(np.any(A != 0.0, axis=0)):
        acc += eta[:, t, None] * A[None, :, t]
    return (acc - c[None]).reshape(-1)


def tail_depths(T, tf_order, B=0):
    """Kept depths the chain reads: the last max(min(T, tf_order + 1), B)."""
    return max(_fd.tail_depths(T, tf_order), int(B))


def sweep_length(T, H, K, tf_order, max_rounds=DEFAULT_MAX_ROUNDS):
    """Numbers one sweep consumes: H K normals, u_h, u_a, the max_rounds - 1 shrink uniforms, 4 nR gammas."""
    return int(H) * int(K) + 1 + int(max_rounds) + 4 * _fd.new_rows(T, H, tf_order)[0].size


def record_length(T, H, K, tf_order, sweeps, max_rounds=DEFAULT_MAX_ROUNDS):
    """Length of the flat `draws` of one chain: 4 nR start gammas, then `sweeps` records of sweep_length."""
    return 4 * _fd.new_rows(T, H, tf_order)[0].size + int(sweeps) * sweep_length(T, H, K, tf_order, max_rounds)


def lds_bytes(T, H, K, tf_order, B=0):
    """LDS one chain's workgroup needs (sdepth_lds_bytes of csrc/btf_slice_fold_depth.h): the count of
    fold_in_depth.lds_bytes with six H K vectors (v, m, nu, v', b, the pivots) in the place of four, the kept tail of
    max(min(T, tf_order + 1), B) depths, and the static tables of slice_fold_in_cols."""
    T, H, K, tf = int(T), int(H), int(K), int(tf_order)
    return _fd.lds_bytes(T, H, K, tf) + 8 * (2 * H * K + (tail_depths(T, tf, B) - _fd.tail_depths(T, tf)) * K) + STATIC_LDS


def random_draws(rng, T, H, K, tf_order, sweeps, max_rounds=DEFAULT_MAX_ROUNDS, size=()):
    """`draws` for `chain` from a numpy Generator or RandomState, in the chain's layout; size: the leading shape (e.g.
    (S, M))."""
    nR, n = _fd.new_rows(T, H, tf_order)[0].size, int(H) * int(K)
    size = tuple(int(x) for x in size)
    parts = [rng.standard_gamma(0.5, size=size + (4 * nR,))]
    shapes = np.ones((4, nR))
    shapes[0] = (K + 1) / 2.0
    for _ in range(int(sweeps)):
        parts.append(rng.normal(size=size + (n,)))
        parts.append(rng.uniform(size=size + (1 + int(max_rounds),)))
        parts.append(rng.standard_gamma(np.broadcast_to(shapes.reshape(-1), size + (4 * nR,))))
    return np.concatenate(parts, axis=-1)


def _view(Y_new, N, M):
    """Y_new (N,M,H) or (N,M,H,nreps) as its (M,N,H[,nreps]) view; ValueError on another shape."""
    if isinstance(Y_new, (tuple, list)):
        raise ValueError("Y_new is one (N,M,H) or (N,M,H,nreps) array")
    Y = np.asarray(Y_new, dtype=float)
    if Y.ndim not in (3, 4) or Y.shape[:2] != (int(N), int(M)) or min(Y.shape[2:]) < 1:
        raise ValueError("Y_new %r must be (%d,%d,H) or (%d,%d,H,nreps) with H >= 1" % (np.shape(Y_new), N, M, N, M))
    return np.swapaxes(Y, 0, 1)


def slice_statistics(Y_new, family, N, M, horizon=None):
    """(H, S1 (M,N,H), cnt (M,N,H), L (M,N,H) or None) of the new depth slices: slice_fold_in.row_statistics on the (M,N,H)
    view of Y_new (N,M,H) or (N,M,H,nreps), nan = missing.  Y_new None with horizon=H: no data at all (the constrained
    forecast)."""
    code = _sf.family_code(family)
    N, M = int(N), int(M)
    if Y_new is None:
        if horizon is None or int(horizon) != horizon or int(horizon) < 1:
            raise ValueError("slice_fold_in_depth: without Y_new, horizon must be a positive integer")
        z = np.zeros((M, N, int(horizon)))
        return int(horizon), z, z.copy(), (z.copy() if code == GAMMA_GRID else None)
    Yv = _view(Y_new, N, M)
    H = Yv.shape[2]
    if horizon is not None and int(horizon) != H:
        raise ValueError("slice_fold_in_depth: horizon %r does not match the %d new depths of Y_new" % (horizon, H))
    _, S1, cnt, L = _sf.row_statistics(Yv, family, N, H)
    return H, S1, cnt, L


def default_fit(Y_new, family, param, N, M, multiplier=2):
    """slice_fold_in_cols.gaussian_fit on the (M,N,H) view of Y_new: (Mu_fit, Sigma_fit), each (M,N,H); None without data."""
    if Y_new is None:
        return None
    return _sc.gaussian_fit(_view(Y_new, N, M), family, param, multiplier=multiplier)


def chain(V_old, W, lam2, tf_order, family, param=None, stats=None, weights=None, sums=None, Constraints=None, horizon=None,
          start=None, tau2=None, draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, stability=STABILITY, nu_scale=1.0,
          track_cond=True, on_sweep=None):
    """The chain of one (sample, fitted column) in numpy: the definition (see the module's docstring for the method).

    V_old (T,K) the kept curve V_s[j]; W (N,K); stats = (S1, cnt, L) of the column's new slice, each (N,H) (None: no
    observation - horizon= then gives H); weights / sums (N,H): slice_fold_in_cols.fit_weights of the slice (None: no
    fit); Constraints (J, T + H + 1) on the extended grid, or the tuple `reduce_constraints` returns; start (H,K) (None:
    V_old[T - 1] at every new depth); tau2 (nR,): the local scales held fixed (the level update is skipped; the record keeps
    its layout).  draws: the flat record (record_length) - 4 nR start gammas (shape 1/2), then per sweep H K normals, u_h,
    u_a, max_rounds - 1 shrink uniforms and 4 nR gammas (shapes (K + 1) / 2, 1, 1, 1) - or None: drawn from rng.  nu_scale
    multiplies every nu (the tests perturb the definition with it).  on_sweep(r, v (H,K)): called with the state after sweep r.

    Returns a dict: v (H,K) - nan when the start is infeasible or has a non-finite r (failed=True; the chain does not run)
    -, tau2 (nR,), rounds (likelihood evaluations of proposals), unfinished (sweeps that hit the cap), margin_ll =
    min |r(v') - hh|, margin_slack = the smallest absolute constraint slack met, cond = the largest cond(Q) (0 with
    track_cond=False)."""
    code = family if isinstance(family, int) else _sf.family_code(family)
    W = np.asarray(W, dtype=float)
    N, K = W.shape
    V_old = _fd._kept(V_old, K)
    T = V_old.shape[0]
    if stats is not None:
        H = np.shape(stats[1])[1]
    elif start is not None:
        H = np.shape(start)[0]
    elif horizon is not None:
        H = int(horizon)
    else:
        raise ValueError("without stats and start, horizon= gives the number of new depths")
    v = np.tile(V_old[T - 1], (H, 1)) if start is None else np.array(start, dtype=float)
    if v.shape != (H, K):
        raise ValueError("start must be (H,K)")
    n = H * K
    _, D_o, D_n = _fd.new_rows(T, H, tf_order)
    nR = D_n.shape[0]
    off = D_o.dot(V_old)
    reduced = Constraints if isinstance(Constraints, tuple) else reduce_constraints(Constraints, T, H)
    sweeps = DEFAULT_SWEEPS if sweeps is None else int(sweeps)
    max_rounds = int(max_rounds)
    per = sweep_length(T, H, K, tf_order, max_rounds)
    if draws is None:
        draws = random_draws(np.random.default_rng() if rng is None else rng, T, H, K, tf_order, sweeps, max_rounds)
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if sweeps < 1 or draws.size != 4 * nR + sweeps * per:
        raise ValueError("draws of one chain must hold 4 nR + sweeps (H K + 1 + max_rounds + 4 nR) = %d values, got %d"
                         % (4 * nR + sweeps * per, draws.size))
    if stats is None:
        z = np.zeros((N, H))
        stats = (z, z, z if code == GAMMA_GRID else None)
    S1, cnt, L = (None if a is None else np.asarray(a, dtype=float) for a in stats)
    weights = np.zeros((N, H)) if weights is None else np.asarray(weights, dtype=float)
    sums = np.zeros((N, H)) if sums is None else np.asarray(sums, dtype=float)
    obs = cnt > 0
    st_obs = (S1[obs], cnt[obs], None if L is None else L[obs])
    has_fit = weights > 0
    wf, sf = weights[has_fit], sums[has_fit]
    restricted = reduced[2].size > 0
    margin = {"ll": np.inf, "slack": np.inf}
    lo, hi = float(stability), 1.0 / float(stability)

    def ok(x):
        if not restricted:
            return True
        s = reduced_slacks(x, W, V_old, reduced)
        margin["slack"] = min(margin["slack"], float(np.min(np.abs(s))))
        return bool(np.all(s >= 0))

    def r_of(x):
        eta = eta_of(W, x)
        val = _sf.loglik_eta(code, param, st_obs, eta[obs]) if obs.any() else 0.0
        ef = eta[has_fit]
        return val + float(np.sum(ef * (0.5 * wf * ef - sf)))

    fixed = tau2 is not None
    if fixed:
        tau, c, b, a = np.asarray(tau2, dtype=float).reshape(nR), None, None, None
    else:
        tau, c, b, a = _fc.start_levels(draws[:4 * nR].reshape(4, nR))
    out = {"v": np.full((H, K), np.nan), "tau2": np.full(nR, np.nan), "rounds": 0, "unfinished": 0, "failed": True,
           "margin_ll": np.inf, "margin_slack": np.inf, "cond": 0.0}
    ll = r_of(v) if ok(v) else np.nan
    if not np.isfinite(ll):
        return out
    rounds = unfinished = 0
    cond = 0.0
    pos = 4 * nR
    two_pi = 2.0 * np.pi
    for sw in range(sweeps):
        d = draws[pos:pos + per]
        pos += per
        if sw == 0 or not fixed:
            m, Q = _fd._system(weights, sums, W, lam2, tau, off, D_n)
            m = m.reshape(H, K)
            if track_cond:
                cond = max(cond, float(np.linalg.cond(Q)))
            Lc = np.linalg.cholesky(Q)
        nu = float(nu_scale) * np.linalg.solve(Lc.T, d[:n]).reshape(H, K)
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
            g = d[n + 1 + max_rounds:].reshape(4, nR)
            dv = off + D_n.dot(v)
            rate = (dv * dv).sum(axis=1) / (2.0 * float(lam2)) + 1.0 / np.clip(c, lo, hi)
            tau = np.clip(rate, lo, hi) / g[0]
            c = np.clip(1.0 / tau + 1.0 / b, lo, hi) / g[1]
            b = np.clip(1.0 / c + 1.0 / a, lo, hi) / g[2]
            a = np.clip(1.0 / b + 1.0, lo, hi) / g[3]
        if on_sweep is not None:
            on_sweep(sw, v)
    out.update(v=v, tau2=np.array(tau, dtype=float), rounds=rounds, unfinished=unfinished, failed=False, margin_ll=margin["ll"],
               margin_slack=margin["slack"], cond=cond)
    return out


def chains(Vs, Ws, lam2, tf_order, family, param=None, stats=None, weights=None, sums=None, Constraints=None, horizon=None,
           starts=None, tau2=None, draws=None, rng=None, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, stability=STABILITY,
           nu_scale=1.0):
    """`chain` for every (sample, fitted column): Vs (S,M,T,K), Ws (S,N,K), lam2 (S,), stats = (S1, cnt, L) each (M,N,H),
    weights / sums (M,N,H), starts (S,M,H,K) or None, tau2 (S,M,nR) or None, draws (S,M,record_length).  Returns V
    (S,M,H,K), Tau2 (S,M,nR), rounds and unfinished (S,M), failed (S,M), the smallest margins and the largest cond(Q)."""
    Vs = np.asarray(Vs, dtype=float)
    S, M, T, K = Vs.shape
    H = np.shape(stats[1])[2] if stats is not None else (np.shape(starts)[2] if starts is not None else int(horizon))
    nR = _fd.new_rows(T, H, tf_order)[0].size
    reduced = Constraints if isinstance(Constraints, tuple) else reduce_constraints(Constraints, T, H)
    V, Tau2 = np.zeros((S, M, H, K)), np.zeros((S, M, nR))
    rounds, unf = np.zeros((S, M), dtype=np.int32), np.zeros((S, M), dtype=np.int32)
    failed = np.zeros((S, M), dtype=bool)
    mll = msl = np.inf
    cond = 0.0
    for s in range(S):
        for j in range(M):
            st = None if stats is None else (stats[0][j], stats[1][j], None if stats[2] is None else stats[2][j])
            o = chain(Vs[s, j], Ws[s], np.reshape(lam2, -1)[s], tf_order, family, param, st,
                      None if weights is None else weights[j], None if sums is None else sums[j], reduced, H,
                      None if starts is None else starts[s, j], None if tau2 is None else tau2[s, j],
                      None if draws is None else draws[s, j], rng, sweeps, max_rounds, stability, nu_scale)
            V[s, j], Tau2[s, j], rounds[s, j], unf[s, j], failed[s, j] = o["v"], o["tau2"], o["rounds"], o["unfinished"], o["failed"]
            mll, msl, cond = min(mll, o["margin_ll"]), min(msl, o["margin_slack"]), max(cond, o["cond"])
    return {"V": V, "Tau2": Tau2, "rounds": rounds, "unfinished": unf, "failed": failed, "margin_ll": mll, "margin_slack": msl,
            "cond": cond}


def check_args(family, param, S, M, N, T, H, K, tf_order, start=None, tau2=None, draws=None, sweeps=None,
               max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95), transform=None, first_sample=0, B=0, horizon=None):
    """Validate and normalise; raises ValueError before any device call.  B: the kept depths the constraints reach
    (reduce_constraints); horizon: checked against H when given.  Returns (family code, param, start (S,M,H,K) or None,
    tau2 (S,M,nR) or None, draws or None, sweeps, max_rounds, qs, transform code)."""
    code = _sf.family_code(family)
    param = _sf.check_param(family, param)
    if int(S) < 1 or int(M) < 1 or int(N) < 1:
        raise ValueError("slice_fold_in_depth: at least one sample, one column and one fitted row")
    if not 1 <= int(K) <= 10:
        raise ValueError("slice_fold_in_depth: nembeds must be 1..10")
    if int(tf_order) < 0 or int(T) < 2 or int(H) < 1:
        raise ValueError("slice_fold_in_depth: tf_order >= 0, ndepth >= 2 and horizon >= 1")
    if horizon is not None and (int(horizon) != horizon or int(horizon) != int(H)):
        raise ValueError("slice_fold_in_depth: horizon %r does not match the %d new depths of Y_new" % (horizon, H))
    if int(T) + int(H) > MAX_GRID:
        raise ValueError("slice_fold_in_depth: ndepth + horizon must stay within %d" % MAX_GRID)
    if (int(tf_order) + 1) * int(K) >= 64:
        raise ValueError("slice_fold_in_depth: the half bandwidth (tf_order + 1) nembeds = %d must stay below 64"
                         % ((int(tf_order) + 1) * int(K)))
    if not 0 <= int(B) <= int(T):
        raise ValueError("slice_fold_in_depth: the constraints reach %r kept depths of %d" % (B, T))
    need = lds_bytes(T, H, K, tf_order, B)
    if need > LDS_LIMIT:
        raise ValueError("slice_fold_in_depth: the band of %d new depths at nembeds %d, tf_order %d with a kept tail of %d depths "
                         "needs %d bytes of LDS, beyond the limit of %d bytes a workgroup may hold"
                         % (H, K, tf_order, tail_depths(T, tf_order, B), need, LDS_LIMIT))
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("slice_fold_in_depth: %d samples exceed the %d of the summary kernel; thin the samples or pass "
                         "summary=False" % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(M) >= 2 ** 31:
        raise ValueError("slice_fold_in_depth: first_sample must be >= 0 and (first_sample + S) * ncols below 2^31")
    qs = check_q(q, allow_none=True) if summary else np.zeros(0)
    if sweeps is None:
        sweeps = DEFAULT_SWEEPS
    if int(sweeps) != sweeps or not 1 <= int(sweeps) < 2 ** 20 - 1:
        raise ValueError("sweeps must be a positive integer (below 2^20 - 1)")
    if int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= 65536:
        raise ValueError("max_rounds must be an integer in 1..65536")
    sweeps, max_rounds = int(sweeps), int(max_rounds)
    nR, n = _fd.new_rows(T, H, tf_order)[0].size, int(H) * int(K)
    if start is not None:
        start = np.asarray(start, dtype=np.float64)
        if start.shape not in ((H, K), (M, H, K), (S, M, H, K)):
            raise ValueError("start must be (H,K), (M,H,K) or (S,M,H,K) with S,M,H,K = %d,%d,%d,%d, got %r" % (S, M, H, K, start.shape))
        if not np.all(np.isfinite(start)):
            raise ValueError("start must be finite")
        start = np.ascontiguousarray(np.broadcast_to(start, (S, M, H, K)))
    if tau2 is not None:
        tau2 = np.asarray(tau2, dtype=np.float64)
        if tau2.shape not in ((M, nR), (S, M, nR)):
            raise ValueError("tau2 must be (M,nR) or (S,M,nR) = (%d,%d,%d), got %r" % (S, M, nR, tau2.shape))
        if not (np.all(np.isfinite(tau2)) and np.all(tau2 > 0)):
            raise ValueError("tau2 must be finite and positive")
        tau2 = np.ascontiguousarray(np.broadcast_to(tau2, (S, M, nR)))
    if draws is not None:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        per = sweep_length(T, H, K, tf_order, max_rounds)
        want = (S, M, 4 * nR + sweeps * per)
        if draws.shape != want:
            raise ValueError("draws must be (S,M,4 nR + sweeps (H K + 1 + max_rounds + 4 nR)) = %r, got %r" % (want, draws.shape))
        if not np.all(np.isfinite(draws)):
            raise ValueError("draws must be finite")
        body = draws[..., 4 * nR:].reshape(S, M, sweeps, per)
        uni = body[..., n:n + 1 + max_rounds]
        if np.any(uni <= 0) or np.any(uni >= 1):
            raise ValueError("draws: the uniforms of every sweep must lie strictly inside (0, 1)")
        if not (np.all(draws[..., :4 * nR] > 0) and np.all(body[..., n + 1 + max_rounds:] > 0)):
            raise ValueError("the gamma variates of draws must be positive")
    return code, param, start, tau2, draws, sweeps, max_rounds, qs, tcode


def evaluate(family, param, S, N, M, T, H, K, tf_order, S1, cnt, L, weights, sums, start=None, Constraints=None, tau2=None,
             draws=None, seed=0, sweeps=None, max_rounds=DEFAULT_MAX_ROUNDS, summary=True, q=(5, 95), transform=None,
             first_sample=0, stability=STABILITY, ctx=None, Ws=None, Vs=None, lam2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Ws None: the context's first S collected samples (no upload; W, the
    tail of V and lam2 from the collected slots, the likelihood's parameter or table from the context); otherwise Ws
    (S,N,K), Vs (S,M,T,K) - its last tail_depths are uploaded - and lam2 (S,) (stateless entry point).  S1 / cnt / L:
    slice_statistics; weights / sums: slice_fold_in_cols.fit_weights on (M,N,H); Constraints (J, T + H + 1) on the
    extended grid or None.  Returns the dict of NonconjugateBayesianTensorFiltering.slice_fold_in_depth."""
    from . import _native
    A_o, A_n, c, B = reduce_constraints(Constraints, T, H)
    code, param, start, tau2, draws, sweeps, max_rounds, qs, tcode = check_args(
        family, param, S, M, N, T, H, K, tf_order, start, tau2, draws, sweeps, max_rounds, summary, q, transform, first_sample, B)
    Jn = int(c.size)
    cons = np.ascontiguousarray(np.concatenate([A_o, A_n, c[:, None]], axis=1)) if Jn else None
    nR = _fd.new_rows(T, H, tf_order)[0].size
    V = np.zeros((S, M, H, K))
    V0 = np.zeros((S, M, H, K))
    Tau2 = np.zeros((S, M, nR))
    rounds = np.zeros((S, M), dtype=np.int32)
    unf = np.zeros((S, M), dtype=np.int32)
    mean = np.zeros((N, M, H)) if summary else None
    quant = np.zeros((len(qs), N, M, H)) if summary else None
    d = _native.dptr
    ip = lambda a: a.ctypes.data_as(_native._c_ip)
    tail = (d(start), d(S1), d(cnt), d(L), d(weights), d(sums), d(cons), Jn, int(B), d(tau2), d(draws),
            int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, max_rounds, int(first_sample), float(stability), d(V), d(V0), d(Tau2), ip(rounds),
            ip(unf), tcode, d(qs) if len(qs) else None, len(qs), d(mean), d(quant) if len(qs) else None)
    if Ws is None:
        ctx.call("btf_collect_slice_fold_depth", code, int(S), int(H), *tail)
    else:
        lib = _native.load()
        par = 0.0 if param is None or code == GAMMA_GRID else (1.0 / param if code == 3 else param)
        tab = param if code == GAMMA_GRID else (None, None, None)
        G = int(tab[0].size) if code == GAMMA_GRID else 0
        Vt = np.ascontiguousarray(Vs[:, :, T - tail_depths(T, tf_order, B):, :], dtype=np.float64)
        _native.check(lib.btf_slice_fold_depth(int(device), code, float(par), d(tab[0]), d(tab[1]), d(tab[2]), G, int(S), int(N), int(M),
                                               int(T), int(H), int(K), int(tf_order), d(Ws), d(Vt), d(lam2), *tail), lib,
                      fail_index=False)
    out = {"V": V, "V_start": V0, "Tau2": Tau2, "rounds": rounds, "unfinished": unf, "nsamples": int(S)}
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
