"""Folding new columns into a fitted posterior: the curves of a column the chain never saw, per kept sample.

Given W the columns of V are conditionally independent (the reference's factor.py:378: _resample_V walks them one by one),
but a column's prior N(0, (I_K (x) Delta' diag(1 / (lam2 tau2)) Delta)^-1) hangs on horseshoe+ local scales tau2 of its own,
which nobody has sampled for a NEW column.  They do not have to be: given a kept sample's W_s, nu2_s and lam2_s the new
column's curve V_c and its four horseshoe+ levels form a small Gibbs chain of their own, with the conditionals of
_resample_V for one column (factor.py:378-409) and of _resample_Tau2 for one column (factor.py:136-141), started from the
prior draw of the levels (sample_horseshoe_plus with the clip of _init_Tau2).  The last state of `sweeps` rounds is a draw
from p(V_c | y_c, W_s, nu2_s, lam2_s) up to the chain's finite length, and one chain per kept sample integrates W and the
hyper-parameters over the posterior.  As in fold_in_rows the new data does NOT inform W or the hyper-parameters.  Binomial
columns open every round with omega_it ~ PG(n_it, w_i . v_t) from the current v, starting at v = 0 (factor.py:437-460).

The data-sized work is the HIP of csrc/btf_fold_in_cols.h (btf_fold_in_cols / btf_collect_fold_in_cols); this module holds
the host halves in plain numpy (importable without a GPU): the DEFINITION (`conditional`, `chain`) the kernel is compared
with draw for draw, the argument checks, and `evaluate`, the one caller of the C entry points.
Coordinates of a column are depth-major: index t * K + k.
"""
import numpy as np

from ._analysis import check_q, transform_code
from .utils import bayes_grid_penalty

FAMILIES = {"gaussian": 0, "binomial": 1}
MAX_SUMMARY_SAMPLES = 16384      # the limit of posterior_summary_kernel (one cell's values are sorted in LDS)
MAX_TRIALS = 32                  # FOLD_CHAIN_MAX_TRIALS of csrc/btf_fold_chain.h: the counts drawn exactly, as fold_in.MAX_TRIALS
LDS_LIMIT = 156 * 1024           # FOLDC_LDS_LIMIT of csrc/btf_fold_in_cols.h: what one workgroup may hold of a CU's 160 KiB of LDS
STABILITY = 1e-6                 # the models' default `stability`
TAU2_START_CLIP = 9.0            # _init_Tau2
PG_TERMS = 200                   # terms of the sum-of-gammas series `chain` draws its Polya-Gamma variates from (host only)
# rounds of the chain per (sample, column): the smallest power of two after which the largest standardised difference of
# the curve means W v against a long chain no longer falls.  Against 256 rounds it falls at every step of 1..64 at both
# shapes; against 1024 rounds it stops falling at 128 at the dose-response-like shape and reaches the noise floor only at
# 512 at the C3-like one (DESIGN.md 4g'', "Folding new columns in", table of scripts/fold_in_cols_rate.py --step sweeps)
DEFAULT_SWEEPS = 512


def family_code(family):
    if family not in FAMILIES:
        raise ValueError("family must be one of %s" % (tuple(FAMILIES),))
    return FAMILIES[family]


_PENALTY = {}


def penalty(T, tf_order):
    """Delta = utils.bayes_grid_penalty(T, tf_order) as a dense (nD, T) array (read-only, cached)."""
    key = (int(T), int(tf_order))
    if key not in _PENALTY:
        D = np.asarray(bayes_grid_penalty(*key).todense(), dtype=float)
        D.setflags(write=False)
        _PENALTY[key] = D
    return _PENALTY[key]


def draws_length(T, K, tf_order, sweeps):
    """Length of the flat `draws` of one chain: 4 nD + sweeps (T K + 4 nD)."""
    nD = penalty(T, tf_order).shape[0]
    return 4 * nD + int(sweeps) * (int(T) * int(K) + 4 * nD)


def half_bandwidth(K, tf_order):
    """Of Q in depth-major order: within a depth the offsets reach K - 1, across depths the prior couples (t, k) with
    (t + d, k), d <= tf_order + 1, at offset d K - so (tf_order + 1) K (the bound (tf_order + 1) K + K - 1, safe for any
    order of the coordinates within a depth, is not needed)."""
    return (int(tf_order) + 1) * int(K)


def lds_bytes(T, K, tf_order):
    """LDS one chain's workgroup needs (foldc_lds_bytes of csrc/btf_fold_in_cols.h): the band of Q, (T K) x (half bandwidth
    + 1) doubles, and the side arrays - right-hand sides, pivots and b 4 T K, the likelihood blocks T K (K + 1) / 2, the
    five level arrays 5 nD, the prior band T (tf_order + 2) - and the pair table of the factorisation."""
    T, K, tf = int(T), int(K), int(tf_order)
    n, bw, nD = T * K, half_bandwidth(K, tf), penalty(T, tf).shape[0]
    npairs = bw * (bw + 1) // 2
    return 8 * (n * (bw + 1) + 4 * n + T * (K * (K + 1) // 2) + 5 * nD + T * (tf + 2)) + 8 * ((npairs + 3) // 4)


def _column(Y_col):
    Y = np.asarray(Y_col, dtype=float)
    if Y.ndim == 2:
        Y = Y[..., None]
    if Y.ndim != 3:
        raise ValueError("Y_col %r must be (N,T) or (N,T,nreps)" % (np.shape(Y_col),))
    obs = ~np.isnan(Y)
    return obs.sum(axis=2).astype(float), np.where(obs, Y, 0.0).sum(axis=2)


def _system(weights, sums, W, lam2, tau2, tf_order):
    """(mean, Q) from per-cell weights and weighted sums (N,T): A_t = sum_i weights_it w_i w_i', b_t = sum_i sums_it w_i."""
    return _system_of_blocks(*_blocks(weights, sums, W), lam2, tau2, tf_order)


def _blocks(weights, sums, W):
    """(A (T,K,K), b (T K,)) of _system: what does not depend on the levels."""
    if weights.shape[0] != W.shape[0]:
        raise ValueError("the column %r does not match W %r" % (weights.shape, W.shape))
    return np.einsum("it,ik,il->tkl", weights, W, W), sums.T.dot(W).reshape(-1)


def _system_of_blocks(A, b, lam2, tau2, tf_order):
    T, K = A.shape[:2]
    D = penalty(T, tf_order)
    P = D.T.dot(D / (float(lam2) * np.asarray(tau2, dtype=float))[:, None])
    Q = np.kron(P, np.eye(K))
    for t in range(T):
        Q[t * K:(t + 1) * K, t * K:(t + 1) * K] += A[t]
    return np.linalg.solve(Q, b), Q


def conditional(Y_col, W, nu2, lam2, tau2, tf_order):
    """The Gaussian conditional of one new column in numpy: the definition the kernel is tested against.
    Y_col (N,T) or (N,T,nreps), nan = missing; W (N,K); tau2 (nD,).  Returns (mean (T K,), Q (T K, T K)), depth-major: Q
    has the block A_t = sum_i cnt_it w_i w_i' / nu2 on the diagonal at depth t plus P = Delta' diag(1 / (lam2 tau2)) Delta on
    every embedding dimension (the kron(I_K, P) of factor.py:404-405, permuted); b_t = sum_i ysum_it w_i / nu2 and
    mean = Q^-1 b."""
    cnt, ysum = _column(Y_col)
    return _system(cnt / float(nu2), ysum / float(nu2), np.asarray(W, dtype=float), lam2, tau2, tf_order)


def start_levels(g0):
    """(tau2, c, b, a) of a new column from unit Gamma(1/2, 1) variates g0 (4, nD): sample_horseshoe_plus with the clip of
    _init_Tau2."""
    a = 1.0 / g0[0]
    b = 1.0 / (a * g0[1])
    c = 1.0 / (b * g0[2])
    return np.minimum(1.0 / (c * g0[3]), TAU2_START_CLIP), c, b, a


def polya_gamma(rng, n, psi, terms=PG_TERMS):
    """PG(n, psi) elementwise by the sum-of-gammas series (Polson, Scott & Windle 2013, eq. 2) cut at `terms` terms, the
    mean of the rest added: the host stand-in for the exact device sampler.  n = 0 gives 0."""
    n, psi = np.asarray(n, dtype=float), np.asarray(psi, dtype=float)
    k = np.arange(1, terms + 1) - 0.5
    den = k * k + (psi[..., None] / (2 * np.pi)) ** 2
    g = rng.standard_gamma(np.broadcast_to(np.maximum(n, 1e-300)[..., None], den.shape))
    x = (g / den).sum(axis=-1) / (2 * np.pi ** 2)
    a = np.abs(psi)
    full = np.where(a > 1e-8, np.tanh(a / 2) / (2 * np.maximum(a, 1e-8)), 0.25) * n        # E PG(n, psi)
    x = x + full - (n[..., None] / den).sum(axis=-1) / (2 * np.pi ** 2)
    return np.where(n > 0, x, 0.0)


def chain(Y_col, W, nu2, lam2, tf_order, sweeps, draws, family="gaussian", trials=None, stability=STABILITY, on_system=None,
          on_sweep=None, seed=None):
    """The whole chain of one (sample, column) on the flat `draws` (length draws_length): the start block g0 (4, nD) of unit
    Gamma(1/2, 1) variates, then per sweep z (T K standard normals) and g (4, nD) with g[0] ~ Gamma((K + 1) / 2, 1) and
    g[1..3] ~ Gamma(1, 1).  Sweep: (mean, Q) = conditional, v = mean + L^-T z with Q = L L' (lower Cholesky, natural
    depth-major order); rate = sum_k (Delta v_k)^2 / (2 lam2) + 1 / clip(c), tau2 = clip(rate) / g[0]; c = clip(1 / tau2 +
    1 / b) / g[1], b = clip(1 / c + 1 / a) / g[2], a = clip(1 / b + 1) / g[3] (factor.py:136-141: 1 / gamma(shape, 1 / x) is
    x / standard_gamma(shape)).
    family="binomial": Y_col is (Y, N) or Y with trials= (default 1), nu2 is not read, and every sweep first draws omega_it ~
    PG(n_it, w_i . v_t) from the current v (v = 0 at the start; `polya_gamma` on numpy's generator seeded by `seed`):
    A_t = sum_i omega_it w_i w_i', b_t = sum_i (y_it - n_it / 2) w_i.  `draws` still supplies the normals and the gammas.
    on_system(Q): called with every precision the chain factors; on_sweep(r, v (T,K)): with the state after sweep r (the
    chain of r + 1 sweeps on the leading part of `draws` ends there).  Returns (v (T,K), mean (T,K), tau2 (nD,)) of the
    last sweep."""
    code = family_code(family)
    W = np.asarray(W, dtype=float)
    K = W.shape[1]
    if code == FAMILIES["gaussian"]:
        cnt, ysum = _column(Y_col)
        weights, sums = cnt / float(nu2), ysum / float(nu2)
    else:
        pair = isinstance(Y_col, (tuple, list))
        Yb = np.asarray(Y_col[0] if pair else Y_col, dtype=float)
        Nb = np.broadcast_to(np.asarray(1.0 if (trials is None and not pair) else (Y_col[1] if pair else trials), dtype=float), Yb.shape)
        _, ntr, y = column_statistics((Yb[None], Nb[None]), family, W.shape[0], Yb.shape[1] if Yb.ndim == 2 else -1)
        ntr, y = ntr[0], y[0]
        sums = np.where(ntr > 0, y - ntr / 2, 0.0)
        pg_rng = np.random.default_rng(seed)
    T = sums.shape[1]
    D = penalty(T, tf_order)
    nD, n = D.shape[0], T * K
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if int(sweeps) < 1 or draws.size != 4 * nD + int(sweeps) * (n + 4 * nD):
        raise ValueError("draws must hold 4 nD + sweeps (T K + 4 nD) = %d values, got %d" % (4 * nD + int(sweeps) * (n + 4 * nD),
                                                                                             draws.size))
    lo, hi = float(stability), 1.0 / float(stability)
    tau2, c, b, a = start_levels(draws[:4 * nD].reshape(4, nD))
    pos = 4 * nD
    v = np.zeros(n)
    for r in range(int(sweeps)):
        z, g = draws[pos:pos + n], draws[pos + n:pos + n + 4 * nD].reshape(4, nD)
        pos += n + 4 * nD
        if code == FAMILIES["binomial"]:
            weights = polya_gamma(pg_rng, ntr, W.dot(v.reshape(T, K).T))
        mean, Q = _system(weights, sums, W, lam2, tau2, tf_order)
        if on_system is not None:
            on_system(Q)
        L = np.linalg.cholesky(Q)
        v = mean + np.linalg.solve(L.T, z)
        dv = D.dot(v.reshape(T, K))
        rate = (dv * dv).sum(axis=1) / (2.0 * float(lam2)) + 1.0 / np.clip(c, lo, hi)
        tau2 = np.clip(rate, lo, hi) / g[0]
        c = np.clip(1.0 / tau2 + 1.0 / b, lo, hi) / g[1]
        b = np.clip(1.0 / c + 1.0 / a, lo, hi) / g[2]
        a = np.clip(1.0 / b + 1.0, lo, hi) / g[3]
        if on_sweep is not None:
            on_sweep(r, v.reshape(T, K))
    return v.reshape(T, K), mean.reshape(T, K), tau2


def random_draws(rng, T, K, tf_order, sweeps, size=()):
    """`draws` for `chain` from a numpy Generator or RandomState (standard_gamma / normal), in the chain's layout; size: the
    leading shape (e.g. (S, C))."""
    nD, n = penalty(T, tf_order).shape[0], int(T) * int(K)
    size = tuple(int(x) for x in size)
    parts = [rng.standard_gamma(0.5, size=size + (4 * nD,))]
    shapes = np.ones((4, nD))
    shapes[0] = (K + 1) / 2.0
    for _ in range(int(sweeps)):
        parts.append(rng.normal(size=size + (n,)))
        parts.append(rng.standard_gamma(np.broadcast_to(shapes.reshape(-1), size + (4 * nD,))))
    return np.concatenate(parts, axis=-1)


def column_statistics(Y_new, family, N, T, trials=None):
    """(C, weights (C,N,T), sums (C,N,T)) of the new columns.  Gaussian: observed replicates and their sum per cell; Binomial:
    trials and successes of the observed cells (a cell with nan in either, or without trials, is missing).  ValueError on a
    shape that does not match (N, T)."""
    code = family_code(family)
    if code == FAMILIES["gaussian"]:
        if isinstance(Y_new, (tuple, list)):
            raise ValueError("Gaussian columns are one (C,N,T) or (C,N,T,nreps) array, not a pair")
        Y = np.asarray(Y_new, dtype=float)
        if Y.ndim == 3:
            Y = Y[..., None]
        if Y.ndim != 4 or Y.shape[0] < 1 or Y.shape[1:3] != (N, T) or Y.shape[3] < 1:
            raise ValueError("Y_new %r must be (C,%d,%d) or (C,%d,%d,nreps)" % (np.shape(Y_new), N, T, N, T))
        if np.isinf(Y).any():
            raise ValueError("Y_new holds infinite values (nan marks a missing observation)")
        obs = ~np.isnan(Y)
        return Y.shape[0], np.ascontiguousarray(obs.sum(axis=3), dtype=np.float64), \
            np.ascontiguousarray(np.where(obs, Y, 0.0).sum(axis=3))
    if isinstance(Y_new, (tuple, list)):
        if len(Y_new) != 2:
            raise ValueError("Binomial columns are a (Y, N) pair")
        Y, Ntr = np.asarray(Y_new[0], dtype=float), np.asarray(Y_new[1], dtype=float)
    else:
        Y = np.asarray(Y_new, dtype=float)
        Ntr = np.ones(Y.shape) if trials is None else np.broadcast_to(np.asarray(trials, dtype=float), Y.shape)
    if Y.ndim != 3 or Y.shape[0] < 1 or Y.shape[1:] != (N, T) or Ntr.shape != Y.shape:
        raise ValueError("Binomial Y_new %r / trials %r must be (C,%d,%d)" % (Y.shape, Ntr.shape, N, T))
    obs = ~(np.isnan(Y) | np.isnan(Ntr)) & (np.nan_to_num(Ntr) > 0)
    n = np.where(obs, Ntr, 0.0)
    y = np.where(obs, Y, 0.0)
    if np.any(n != np.floor(n)) or np.any(n > MAX_TRIALS) or not np.all(np.isfinite(n)):
        raise ValueError("Binomial trial counts must be integers up to %d (larger counts are not folded in yet)" % MAX_TRIALS)
    if np.any(y < 0) or np.any(y > n) or not np.all(np.isfinite(y)):
        raise ValueError("Binomial successes must lie in [0, trials]")
    return Y.shape[0], np.ascontiguousarray(n), np.ascontiguousarray(y)


def check_args(family, S, C, T, K, tf_order, draws=None, sweeps=None, summary=True, q=(5, 95), transform=None, first_sample=0):
    """Validate and normalise; raises ValueError before any device call.  Returns (family code, draws or None, qs,
    transform code, sweeps)."""
    code = family_code(family)
    if int(S) < 1:
        raise ValueError("fold_in_cols: at least one sample")
    if not 1 <= int(K) <= 10:
        raise ValueError("fold_in_cols: nembeds must be 1..10")
    if int(tf_order) < 0 or int(T) < 2:
        raise ValueError("fold_in_cols: tf_order >= 0 and ndepth >= 2")
    if half_bandwidth(K, tf_order) >= 64:
        raise ValueError("fold_in_cols: the half bandwidth (tf_order + 1) nembeds = %d must stay below 64" % half_bandwidth(K, tf_order))
    need = lds_bytes(T, K, tf_order)
    if need > LDS_LIMIT:
        raise ValueError("fold_in_cols: the band of a column at ndepth %d, nembeds %d, tf_order %d needs %d bytes of LDS, beyond "
                         "the limit of %d bytes a workgroup may hold" % (T, K, tf_order, need, LDS_LIMIT))
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("fold_in_cols: %d samples exceed the %d of the summary kernel; thin the samples or pass summary=False"
                         % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(C) >= 2 ** 31:
        raise ValueError("fold_in_cols: first_sample must be >= 0 and (first_sample + S) * C below 2^31")
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
        nD, n = penalty(T, tf_order).shape[0], int(T) * int(K)
        L = 4 * nD + sweeps * (n + 4 * nD)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.shape != (S, C, L):
            raise ValueError("draws must be (S,C,4 nD + sweeps (T K + 4 nD)) = (%d,%d,%d), got %r" % (S, C, L, draws.shape))
        if not np.all(np.isfinite(draws)):
            raise ValueError("draws must be finite")
        gam = np.ones(L, dtype=bool)
        for r in range(sweeps):
            gam[4 * nD + r * (n + 4 * nD):4 * nD + r * (n + 4 * nD) + n] = False
        if not np.all(draws[..., gam] > 0):
            raise ValueError("the gamma variates of draws must be positive")
    return code, draws, qs, tcode, sweeps


def evaluate(family, S, C, N, T, K, tf_order, weights, sums, draws=None, seed=0, sweeps=None, summary=True, q=(5, 95),
             transform=None, first_sample=0, stability=STABILITY, ctx=None, Ws=None, nu2=None, lam2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Ws None: the context's first S collected samples (no upload; nu2
    and lam2 from the collected scalars); otherwise Ws (S,N,K), nu2 (S,), lam2 (S,) are uploaded (stateless entry point).
    weights / sums: column_statistics.  Returns the dict of BayesianTensorFiltering.fold_in_cols."""
    from . import _native
    code, draws, qs, tcode, sweeps = check_args(family, S, C, T, K, tf_order, draws, sweeps, summary, q, transform, first_sample)
    gauss = code == FAMILIES["gaussian"]
    nD = penalty(T, tf_order).shape[0]
    V = np.zeros((S, C, T, K))
    Vm = np.zeros((S, C, T, K))
    Tau2 = np.zeros((S, C, nD))
    mean = np.zeros((N, C, T)) if summary else None
    quant = np.zeros((len(qs), N, C, T)) if summary else None
    d = _native.dptr
    cnt, trials = (weights, None) if gauss else (None, weights)
    tail = (d(cnt), d(sums), d(trials), d(draws), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, int(first_sample), float(stability),
            d(V), d(Vm), d(Tau2), tcode, d(qs) if len(qs) else None, len(qs), d(mean), d(quant) if len(qs) else None)
    if Ws is None:
        ctx.call("btf_collect_fold_in_cols", code, int(S), int(C), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_fold_in_cols(int(device), code, int(S), int(C), int(N), int(T), int(K), int(tf_order), d(Ws), d(nu2),
                                           d(lam2), *tail), lib)
    out = {"V": V, "Tau2": Tau2, "nsamples": int(S)}
    if gauss:
        out["V_mean"] = Vm
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
