"""Folding new depth slices into a fitted posterior: the curves at depths the chain never saw, per kept sample and column.

The trend-filtering prior of a column couples a new depth with the last tf_order + 1 kept depths of the same column, through
penalty rows whose horseshoe+ local scales nobody has sampled.  Let D' = penalty(T + H, tf_order) be the operator on the
extended grid, R its NEW ROWS (those with a non-zero in the columns T..T+H-1, nR of them) and D'[R] = [D_o | D_n] their split
into kept and new depths.  Rows of D' that touch kept depths only do not depend on the new curve and drop out of its
conditional, so no kept Tau2 is read.  Given a kept sample's W_s, V_s[j], nu2_s and lam2_s, the H new depths v (H x K,
depth-major: index t K + k) of column j and the levels (tau2, c, b, a) of the rows of R form a small Gibbs chain:

    start    (tau2, c, b, a) = fold_in_cols.start_levels(g0), g0 (4, nR) ~ Gamma(1/2, 1)
    sweep    off = D_o V_s[j] (nR, K);  Q = blockdiag_t(A_t) + (D_n' diag(1 / (lam2 tau2)) D_n) (x) I_K
             rhs = b - vec(D_n' diag(1 / (lam2 tau2)) off);  v = Q^-1 rhs + L^-T z,  Q = L L'
             the levels as fold_in_cols.chain with dv = off + D_n v and the same clips

the fold_in_cols chain with a system H K wide, a right-hand side from the kept curve, and one chain per (sample, FITTED
column).  The last boundary row of an odd-order operator on T points (the lower-order difference that closes the grid) is an
interior row on T + H points: it belongs to R with its interior coefficients and gets a fresh scale like every other row of
R; the scale the T-point fit sampled for it is not carried over.  D_n has full column rank, so a column slice with no
observation at all is allowed (Q is then the prior's precision): with no data the call is the model's FORECAST, and with
sweeps=1 that draw is exact (the levels of the start are the prior's).  The forecast is honest but weak: fresh local scales
on the low-order rows shrink the continuation towards flat, and its curves are heavy-tailed.  The data-informed update -
some rows observed at the new depths - is the point of the feature.  As in fold_in_rows and fold_in_cols the new data does
not inform W, the kept depths or the hyper-parameters.  Binomial slices open every sweep with omega_it ~ PG(n_it, w_i . v_t)
from the current v, which starts at the last kept depth V_s[j, T - 1] for every new t.

The data-sized work is the HIP of csrc/btf_fold_in_depth.h (btf_fold_in_depth / btf_collect_fold_in_depth); this module holds
the host halves in plain numpy (importable without a GPU): the DEFINITION (`conditional`, `chain`) the kernel is compared
with draw for draw, the argument checks, and `evaluate`, the one caller of the C entry points.
"""
import numpy as np

from ._analysis import check_q, transform_code
from .fold_in_cols import (FAMILIES, MAX_SUMMARY_SAMPLES, MAX_TRIALS, LDS_LIMIT, STABILITY, family_code, penalty, polya_gamma,
                           start_levels)

# sweeps of the chain per (sample, column): the smallest power of two after which the largest standardised difference of
# the curve means W v against a long chain no longer falls.  Against 256 sweeps it still falls from 64 to 128 at the C3-like
# slice, so the grid was extended against 1024 sweeps: it reaches the noise floor at 64 at the flu-like slice and at 128 at
# the C3-like one ("Folding new depth slices in", table of scripts/fold_in_depth_rate.py --step sweeps)
DEFAULT_SWEEPS = 128
MAX_GRID = 8192                  # FOLDD_MAX_GRID of csrc/btf_fold_in_depth.h: ndepth + horizon (the penalty on the extended grid is dense on the host)


def new_rows(T, H, tf_order):
    """(R, D_o (nR, T), D_n (nR, H)): the rows of D' = penalty(T + H, tf_order) with a non-zero at a new depth, split into
    kept and new depths.  For T >= tf_order + 1, nR = H, 2 H + 1, 3 H + 2 at tf_order 0, 1, 2; D_o reaches back at most
    tf_order + 1 kept depths and D_n has full column rank."""
    T, H = int(T), int(H)
    if H < 1 or T < 2 or int(tf_order) < 0:
        raise ValueError("fold_in_depth: horizon >= 1, ndepth >= 2 and tf_order >= 0")
    D = penalty(T + H, tf_order)
    R = np.flatnonzero(np.any(D[:, T:] != 0.0, axis=1))
    return R, D[R][:, :T], D[R][:, T:]


def draws_length(T, H, K, tf_order, sweeps):
    """Length of the flat `draws` of one chain: 4 nR + sweeps (H K + 4 nR)."""
    nR = new_rows(T, H, tf_order)[0].size
    return 4 * nR + int(sweeps) * (int(H) * int(K) + 4 * nR)


def half_bandwidth(H, K, tf_order):
    """Of Q in depth-major order: (tf_order + 1) K as in fold_in_cols, cut at the H K - 1 of a system that is narrower."""
    return min((int(tf_order) + 1) * int(K), int(H) * int(K) - 1)


def tail_depths(T, tf_order):
    """Kept depths the chain reads: the last min(T, tf_order + 1)."""
    return min(int(T), int(tf_order) + 1)


def lds_bytes(T, H, K, tf_order):
    """LDS one chain's workgroup needs (foldd_lds_bytes of csrc/btf_fold_in_depth.h): the band of Q, (H K) x (half bandwidth
    + 1) doubles, and the side arrays - right-hand sides, pivots and b 4 H K, the likelihood blocks H K (K + 1) / 2, the
    five level arrays 5 nR, the offsets nR K, the prior band H (tf_order + 2), the kept tail min(T, tf_order + 1) K - and
    the pair table of the factorisation."""
    T, H, K, tf = int(T), int(H), int(K), int(tf_order)
    n, bw, nR = H * K, half_bandwidth(H, K, tf), new_rows(T, H, tf)[0].size
    npairs = bw * (bw + 1) // 2
    return 8 * (n * (bw + 1) + 4 * n + H * (K * (K + 1) // 2) + 5 * nR + nR * K + H * (tf + 2) + tail_depths(T, tf) * K) \
        + 8 * ((npairs + 3) // 4)


def _slice(Y_slice):
    Y = np.asarray(Y_slice, dtype=float)
    if Y.ndim == 2:
        Y = Y[..., None]
    if Y.ndim != 3:
        raise ValueError("Y_slice %r must be (N,H) or (N,H,nreps)" % (np.shape(Y_slice),))
    obs = ~np.isnan(Y)
    return obs.sum(axis=2).astype(float), np.where(obs, Y, 0.0).sum(axis=2)


def _system(weights, sums, W, lam2, tau2, off, D_n):
    """(mean, Q) from per-cell weights and weighted sums (N,H), the offsets off (nR,K) and D_n (nR,H)."""
    if weights.shape[0] != W.shape[0]:
        raise ValueError("the slice %r does not match W %r" % (weights.shape, W.shape))
    H, K = weights.shape[1], W.shape[1]
    A = np.einsum("it,ik,il->tkl", weights, W, W)
    b = sums.T.dot(W).reshape(-1)
    w = 1.0 / (float(lam2) * np.asarray(tau2, dtype=float))
    Q = np.kron(D_n.T.dot(D_n * w[:, None]), np.eye(K))
    for t in range(H):
        Q[t * K:(t + 1) * K, t * K:(t + 1) * K] += A[t]
    rhs = b - D_n.T.dot(w[:, None] * off).reshape(-1)
    return np.linalg.solve(Q, rhs), Q


def _kept(V_old, K):
    V_old = np.asarray(V_old, dtype=float)
    if V_old.ndim != 2 or V_old.shape[1] != K or V_old.shape[0] < 2:
        raise ValueError("V_old %r must be (T,%d) with T >= 2" % (V_old.shape, K))
    return V_old


def conditional(Y_slice, W, V_old, nu2, lam2, tau2, tf_order):
    """The Gaussian conditional of the H new depths of one column in numpy: the definition the kernel is tested against.
    Y_slice (N,H) or (N,H,nreps), nan = missing; W (N,K); V_old (T,K) the kept curve; tau2 (nR,) the scales of the new
    rows.  Returns (mean (H K,), Q (H K, H K)), depth-major: the Schur conditional of fold_in_cols.conditional on the
    (T + H)-point grid given the kept depths - the same Q_nn block, mean Q_nn^-1 (b_n - Q_no v_old)."""
    W = np.asarray(W, dtype=float)
    V_old = _kept(V_old, W.shape[1])
    cnt, ysum = _slice(Y_slice)
    _, D_o, D_n = new_rows(V_old.shape[0], cnt.shape[1], tf_order)
    return _system(cnt / float(nu2), ysum / float(nu2), W, lam2, tau2, D_o.dot(V_old), D_n)


def chain(Y_slice, W, V_old, nu2, lam2, tf_order, sweeps, draws, family="gaussian", trials=None, stability=STABILITY,
          on_system=None, on_sweep=None, seed=None):
    """The whole chain of one (sample, column) on the flat `draws` (length draws_length): the start block g0 (4, nR) of unit
    Gamma(1/2, 1) variates, then per sweep z (H K standard normals) and g (4, nR) with g[0] ~ Gamma((K + 1) / 2, 1) and
    g[1..3] ~ Gamma(1, 1) - the layout of fold_in_cols.chain with nR in the place of nD.  Sweep: (mean, Q) = conditional,
    v = mean + L^-T z with Q = L L'; dv = off + D_n v, rate = sum_k dv_k^2 / (2 lam2) + 1 / clip(c), tau2 = clip(rate) /
    g[0]; c = clip(1 / tau2 + 1 / b) / g[1], b = clip(1 / c + 1 / a) / g[2], a = clip(1 / b + 1) / g[3].
    A slice without data is Y_slice = np.full((N,H), nan).
    family="binomial": Y_slice is (Y, N) or Y with trials= (default 1), nu2 is not read, and every sweep first draws omega_it
    ~ PG(n_it, w_i . v_t) from the current v (v_t = V_old[T - 1] at the start; fold_in_cols.polya_gamma on numpy's generator
    seeded by `seed`): A_t = sum_i omega_it w_i w_i', b_t = sum_i (y_it - n_it / 2) w_i.
    on_system(Q): called with every precision the chain factors; on_sweep(r, v (H,K)): with the state after sweep r (the
    chain of r + 1 sweeps on the leading part of `draws` ends there).  Returns (v (H,K), mean (H,K), tau2 (nR,)) of the
    last sweep."""
    code = family_code(family)
    W = np.asarray(W, dtype=float)
    K = W.shape[1]
    V_old = _kept(V_old, K)
    T = V_old.shape[0]
    if code == FAMILIES["gaussian"]:
        cnt, ysum = _slice(Y_slice)
        weights, sums = cnt / float(nu2), ysum / float(nu2)
    else:
        pair = isinstance(Y_slice, (tuple, list))
        Yb = np.asarray(Y_slice[0] if pair else Y_slice, dtype=float)
        if Yb.ndim != 2:
            raise ValueError("Binomial Y_slice must be (N,H)")
        Nb = np.broadcast_to(np.asarray(1.0 if (trials is None and not pair) else (Y_slice[1] if pair else trials), dtype=float),
                             Yb.shape)
        _, ntr, y = slice_statistics((Yb[:, None], Nb[:, None]), family, W.shape[0], 1)
        ntr, y = ntr[0].T, y[0].T                                      # (N,H)
        sums = np.where(ntr > 0, y - ntr / 2, 0.0)
        pg_rng = np.random.default_rng(seed)
    H = sums.shape[1]
    _, D_o, D_n = new_rows(T, H, tf_order)
    nR, n = D_n.shape[0], H * K
    off = D_o.dot(V_old)
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if int(sweeps) < 1 or draws.size != 4 * nR + int(sweeps) * (n + 4 * nR):
        raise ValueError("draws must hold 4 nR + sweeps (H K + 4 nR) = %d values, got %d" % (4 * nR + int(sweeps) * (n + 4 * nR),
                                                                                             draws.size))
    lo, hi = float(stability), 1.0 / float(stability)
    tau2, c, b, a = start_levels(draws[:4 * nR].reshape(4, nR))
    pos = 4 * nR
    v = np.tile(V_old[T - 1], H)
    for r in range(int(sweeps)):
        z, g = draws[pos:pos + n], draws[pos + n:pos + n + 4 * nR].reshape(4, nR)
        pos += n + 4 * nR
        if code == FAMILIES["binomial"]:
            weights = polya_gamma(pg_rng, ntr, W.dot(v.reshape(H, K).T))
        mean, Q = _system(weights, sums, W, lam2, tau2, off, D_n)
        if on_system is not None:
            on_system(Q)
        L = np.linalg.cholesky(Q)
        v = mean + np.linalg.solve(L.T, z)
        dv = off + D_n.dot(v.reshape(H, K))
        rate = (dv * dv).sum(axis=1) / (2.0 * float(lam2)) + 1.0 / np.clip(c, lo, hi)
        tau2 = np.clip(rate, lo, hi) / g[0]
        c = np.clip(1.0 / tau2 + 1.0 / b, lo, hi) / g[1]
        b = np.clip(1.0 / c + 1.0 / a, lo, hi) / g[2]
        a = np.clip(1.0 / b + 1.0, lo, hi) / g[3]
        if on_sweep is not None:
            on_sweep(r, v.reshape(H, K))
    return v.reshape(H, K), mean.reshape(H, K), tau2


def random_draws(rng, T, H, K, tf_order, sweeps, size=()):
    """`draws` for `chain` from a numpy Generator or RandomState (standard_gamma / normal), in the chain's layout; size: the
    leading shape (e.g. (S, M))."""
    nR, n = new_rows(T, H, tf_order)[0].size, int(H) * int(K)
    size = tuple(int(x) for x in size)
    parts = [rng.standard_gamma(0.5, size=size + (4 * nR,))]
    shapes = np.ones((4, nR))
    shapes[0] = (K + 1) / 2.0
    for _ in range(int(sweeps)):
        parts.append(rng.normal(size=size + (n,)))
        parts.append(rng.standard_gamma(np.broadcast_to(shapes.reshape(-1), size + (4 * nR,))))
    return np.concatenate(parts, axis=-1)


def slice_statistics(Y_new, family, N, M, trials=None, horizon=None):
    """(H, weights (M,H,N), sums (M,H,N)) of the new depth slices, in the kernel's [column][depth][row] layout.  Gaussian:
    observed replicates and their sum per cell of Y_new (N,M,H) or (N,M,H,nreps), nan = missing; Binomial: trials and
    successes of the observed cells of a (Y, N) pair, or of Y with trials= (default 1) (a cell with nan in either, or
    without trials, is missing).  Y_new None with horizon=H: no data at all (the forecast).  ValueError on a shape that does
    not match (N, M), on H < 1 and on infinite values."""
    code = family_code(family)
    N, M = int(N), int(M)
    if Y_new is None:
        if horizon is None or int(horizon) != horizon or int(horizon) < 1:
            raise ValueError("fold_in_depth: without Y_new, horizon must be a positive integer")
        z = np.zeros((M, int(horizon), N))
        return int(horizon), z, z.copy()
    if code == FAMILIES["gaussian"]:
        if isinstance(Y_new, (tuple, list)):
            raise ValueError("Gaussian slices are one (N,M,H) or (N,M,H,nreps) array, not a pair")
        Y = np.asarray(Y_new, dtype=float)
        if Y.ndim == 3:
            Y = Y[..., None]
        if Y.ndim != 4 or Y.shape[:2] != (N, M) or Y.shape[2] < 1 or Y.shape[3] < 1:
            raise ValueError("Y_new %r must be (%d,%d,H) or (%d,%d,H,nreps) with H >= 1" % (np.shape(Y_new), N, M, N, M))
        if np.isinf(Y).any():
            raise ValueError("Y_new holds infinite values (nan marks a missing observation)")
        obs = ~np.isnan(Y)
        cnt, ysum = obs.sum(axis=3).astype(np.float64), np.where(obs, Y, 0.0).sum(axis=3)
    else:
        if isinstance(Y_new, (tuple, list)):
            if len(Y_new) != 2:
                raise ValueError("Binomial slices are a (Y, N) pair")
            Y, Ntr = np.asarray(Y_new[0], dtype=float), np.asarray(Y_new[1], dtype=float)
        else:
            Y = np.asarray(Y_new, dtype=float)
            Ntr = np.ones(Y.shape) if trials is None else np.broadcast_to(np.asarray(trials, dtype=float), Y.shape)
        if Y.ndim != 3 or Y.shape[:2] != (N, M) or Y.shape[2] < 1 or Ntr.shape != Y.shape:
            raise ValueError("Binomial Y_new %r / trials %r must be (%d,%d,H) with H >= 1" % (Y.shape, Ntr.shape, N, M))
        if np.isinf(Y).any() or np.isinf(Ntr).any():
            raise ValueError("Y_new holds infinite values (nan marks a missing observation)")
        obs = ~(np.isnan(Y) | np.isnan(Ntr)) & (np.nan_to_num(Ntr) > 0)
        cnt, ysum = np.where(obs, Ntr, 0.0), np.where(obs, Y, 0.0)
        if np.any(cnt != np.floor(cnt)) or np.any(cnt > MAX_TRIALS):
            raise ValueError("Binomial trial counts must be integers up to %d (larger counts are not folded in yet)" % MAX_TRIALS)
        if np.any(ysum < 0) or np.any(ysum > cnt):
            raise ValueError("Binomial successes must lie in [0, trials]")
    H = cnt.shape[2]
    if horizon is not None and int(horizon) != H:
        raise ValueError("fold_in_depth: horizon %r does not match the %d new depths of Y_new" % (horizon, H))
    return H, np.ascontiguousarray(cnt.transpose(1, 2, 0)), np.ascontiguousarray(ysum.transpose(1, 2, 0))


def check_args(family, S, M, T, H, K, tf_order, draws=None, sweeps=None, summary=True, q=(5, 95), transform=None, first_sample=0):
    """Validate and normalise; raises ValueError before any device call.  Returns (family code, draws or None, qs,
    transform code, sweeps)."""
    code = family_code(family)
    if int(S) < 1 or int(M) < 1:
        raise ValueError("fold_in_depth: at least one sample and one column")
    if not 1 <= int(K) <= 10:
        raise ValueError("fold_in_depth: nembeds must be 1..10")
    if int(tf_order) < 0 or int(T) < 2 or int(H) < 1:
        raise ValueError("fold_in_depth: tf_order >= 0, ndepth >= 2 and horizon >= 1")
    if int(T) + int(H) > MAX_GRID:
        raise ValueError("fold_in_depth: ndepth + horizon must stay within %d" % MAX_GRID)
    if (int(tf_order) + 1) * int(K) >= 64:
        raise ValueError("fold_in_depth: the half bandwidth (tf_order + 1) nembeds = %d must stay below 64"
                         % ((int(tf_order) + 1) * int(K)))
    need = lds_bytes(T, H, K, tf_order)
    if need > LDS_LIMIT:
        raise ValueError("fold_in_depth: the band of %d new depths at nembeds %d, tf_order %d needs %d bytes of LDS, beyond the "
                         "limit of %d bytes a workgroup may hold" % (H, K, tf_order, need, LDS_LIMIT))
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("fold_in_depth: %d samples exceed the %d of the summary kernel; thin the samples or pass summary=False"
                         % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(M) >= 2 ** 31:
        raise ValueError("fold_in_depth: first_sample must be >= 0 and (first_sample + S) * ncols below 2^31")
    qs = check_q(q, allow_none=True) if summary else np.zeros(0)
    if sweeps is None:
        sweeps = DEFAULT_SWEEPS
    if int(sweeps) != sweeps or not 1 <= int(sweeps) < 2 ** 20 - 1:
        raise ValueError("sweeps must be a positive integer (below 2^20 - 1)")
    sweeps = int(sweeps)
    if draws is not None:
        if code != FAMILIES["gaussian"]:
            raise ValueError("draws replaces the device generator for the Gaussian model only (the Binomial chain also draws "
                             "Polya-Gamma variates); pass seed=")
        nR, n = new_rows(T, H, tf_order)[0].size, int(H) * int(K)
        L = 4 * nR + sweeps * (n + 4 * nR)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.shape != (S, M, L):
            raise ValueError("draws must be (S,M,4 nR + sweeps (H K + 4 nR)) = (%d,%d,%d), got %r" % (S, M, L, draws.shape))
        if not np.all(np.isfinite(draws)):
            raise ValueError("draws must be finite")
        gam = np.ones(L, dtype=bool)
        for r in range(sweeps):
            gam[4 * nR + r * (n + 4 * nR):4 * nR + r * (n + 4 * nR) + n] = False
        if not np.all(draws[..., gam] > 0):
            raise ValueError("the gamma variates of draws must be positive")
    return code, draws, qs, tcode, sweeps


def evaluate(family, S, N, M, T, H, K, tf_order, weights, sums, draws=None, seed=0, sweeps=None, summary=True, q=(5, 95),
             transform=None, first_sample=0, stability=STABILITY, ctx=None, Ws=None, Vs=None, nu2=None, lam2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Ws None: the context's first S collected samples (no upload; the
    tail of V, nu2 and lam2 are read where they lie); otherwise Ws (S,N,K), Vs (S,M,T,K) - its last min(T, tf_order + 1)
    depths are uploaded - nu2 (S,), lam2 (S,) (stateless entry point).  weights / sums: slice_statistics.  Returns the dict
    of BayesianTensorFiltering.fold_in_depth."""
    from . import _native
    code, draws, qs, tcode, sweeps = check_args(family, S, M, T, H, K, tf_order, draws, sweeps, summary, q, transform, first_sample)
    gauss = code == FAMILIES["gaussian"]
    nR = new_rows(T, H, tf_order)[0].size
    V = np.zeros((S, M, H, K))
    Vm = np.zeros((S, M, H, K))
    Tau2 = np.zeros((S, M, nR))
    mean = np.zeros((N, M, H)) if summary else None
    quant = np.zeros((len(qs), N, M, H)) if summary else None
    d = _native.dptr
    cnt, trials = (weights, None) if gauss else (None, weights)
    tail = (d(cnt), d(sums), d(trials), d(draws), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, int(first_sample), float(stability),
            d(V), d(Vm), d(Tau2), tcode, d(qs) if len(qs) else None, len(qs), d(mean), d(quant) if len(qs) else None)
    if Ws is None:
        ctx.call("btf_collect_fold_in_depth", code, int(S), int(H), *tail)
    else:
        lib = _native.load()
        Vt = np.ascontiguousarray(Vs[:, :, T - tail_depths(T, tf_order):, :], dtype=np.float64)
        _native.check(lib.btf_fold_in_depth(int(device), code, int(S), int(N), int(M), int(T), int(H), int(K), int(tf_order), d(Ws),
                                            d(Vt), d(nu2), d(lam2), *tail), lib)
    out = {"V": V, "Tau2": Tau2, "nsamples": int(S)}
    if gauss:
        out["V_mean"] = Vm
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
