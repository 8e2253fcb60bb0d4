"""Folding new columns and new depth slices into a fitted Negative-Binomial posterior.

Given the rate the Negative-Binomial model is the Binomial one on pseudo-data (the reference's factor.py:506-511, 553): a cell
with c observed replicates, their sum ysum and rate r has

    omega ~ PG(ysum + c r, w_i . v_t)        kappa = (ysum - c r) / 2

in the place of the Binomial cell's PG(n, .) and y - n / 2.  Everything else is the chain of fold_in_cols.chain /
fold_in_depth.chain (family="binomial"): the same start (v = 0 for a new column, the last kept depth for new depths), the
same levels, the same layout of `draws`.  The pseudo-trial counts are real-valued and unbounded, so the Binomial fold-ins -
whose exact sampler takes integers up to 32 - cannot be reused by passing (Y, Y + R); the device draws the weights with the
sampler of the Negative-Binomial sweeps (the sum-of-gammas series below 200, a moment-matched normal from there on).

THE RATE of a new column or depth is the kept sample's rate when the fitted layout (`rdims`) does not vary along the folded
axis: (S, N|1, 1, T|1) for columns, (S, N|1, M|1, 1) for depths.  Where it does vary the fit says nothing about the new
entity's rate and the caller passes rate=: (S,) plus a shape that broadcasts against the new tensor.  Sampling a rate for
a new column or depth is out of scope, as is pg_exact=True.

NEW ROWS (`chain_rows`, `evaluate_rows`; csrc/btf_negbin_fold_rows.h, btf_negbin_fold_in_rows) are the chain of
fold_in.py's Binomial rows on the same pseudo-data, from w = 0 with the prior N(0, sigma2 I).  Where the fit has one rate per
row (rdims=(1, 2), R (S,N,1,1)) a new row has no kept rate: the chain then SAMPLES one scalar rate for it, by the model's own
random-walk Metropolis step on log r (factor.py:513-554 restricted to the one row) in front of every sweep.

The data-sized work is the HIP of csrc/btf_fold_chain.h (negbin_draw_depth, negbin_accumulate) in the third family of
fold_cols_kernel / fold_depth_kernel (btf_negbin_fold_in_cols / btf_negbin_fold_in_depth); this module holds the host halves
in plain numpy (importable without a GPU): the DEFINITION (`chain_cols`, `chain_depth`), the argument checks, and `evaluate`,
the one caller of the C entry points.  With `draws` and `omega` together a chain is a deterministic function of its inputs:
that is the replay the kernels are tested against.
"""
import math

import numpy as np

from . import fold_in_cols as _fc
from . import fold_in_depth as _fd

LDS_LIMIT = _fc.LDS_LIMIT
STABILITY = _fc.STABILITY
MAX_PSEUDO_TRIALS = 1e15         # b = ysum + c r must stay below it (negbin_fold_cells_check of csrc/btf_analysis.hip)
# "cols", "depth": the Binomial family's.  "rows": a chain with a SAMPLED rate (a fixed rate runs fold_in.DEFAULT_INNER_SWEEPS,
# the Binomial rows' count): the smallest power of two after which the largest |z| of the means of log r and ilogit(w . v)
# against a chain four times as long no longer falls ("Folding new rows into a Negative-Binomial fit", table of
# scripts/negbin_fold_in_rows_rate.py --step sweeps)
DEFAULT_SWEEPS = {"cols": _fc.DEFAULT_SWEEPS, "depth": _fd.DEFAULT_SWEEPS, "rows": 128}
MAX_ROW_SWEEPS = 1 << 20         # sweeps and nmetropolis of a row chain: keeps the generator's counter ranges apart


def cell_statistics(Y, shape, what="Y_new"):
    """(cnt, ysum), each `shape`: the observed replicates of a cell and their sum.  Y: counts shaped `shape` or `shape` +
    (nreps,), nan = missing.  ValueError on another shape and on counts that are not finite, non-negative integers."""
    given = np.shape(Y)
    Y = np.asarray(Y, dtype=float)
    shape = tuple(int(x) for x in shape)
    if Y.ndim == len(shape):
        Y = Y[..., None]
    if Y.ndim != len(shape) + 1 or Y.shape[:-1] != shape or Y.shape[-1] < 1 or min(shape) < 1:
        raise ValueError("%s %r must be %r or %r + (nreps,)" % (what, given, shape, shape))
    obs = ~np.isnan(Y)
    y = np.where(obs, Y, 0.0)
    if not np.all(np.isfinite(y)) or np.any(y < 0) or np.any(y != np.floor(y)):
        raise ValueError("%s: counts must be finite, non-negative integers (nan marks a missing value)" % what)
    return np.ascontiguousarray(obs.sum(axis=-1), dtype=np.float64), np.ascontiguousarray(y.sum(axis=-1))


def slice_cells(Y_new, N, M, horizon=None):
    """(H, cnt (N,M,H), ysum (N,M,H)) of new depth slices: cell_statistics of Y_new (N,M,H) or (N,M,H,nreps), or, with
    Y_new None and horizon=H, no data at all (the forecast)."""
    N, M = int(N), int(M)
    if Y_new is None:
        if horizon is None or int(horizon) != horizon or int(horizon) < 1:
            raise ValueError("negbin_fold_in_depth: without Y_new, horizon must be a positive integer")
        z = np.zeros((N, M, int(horizon)))
        return int(horizon), z, z.copy()
    shape = np.shape(Y_new)
    if len(shape) not in (3, 4) or shape[2] < 1:
        raise ValueError("Y_new %r must be (%d,%d,H) or (%d,%d,H,nreps) with H >= 1" % (shape, N, M, N, M))
    H = int(shape[2])
    if horizon is not None and int(horizon) != H:
        raise ValueError("negbin_fold_in_depth: horizon %r does not match the %d new depths of Y_new" % (horizon, H))
    cnt, ysum = cell_statistics(Y_new, (N, M, H))
    return H, cnt, ysum


def rate_strides(rate):
    """(compact array, strides) of a rate (S, C|1, N|1, T|1) in the kernels' order (sample, chain, row, depth): the strides
    in doubles of the C-contiguous array, 0 on an axis of extent 1 (shared)."""
    rate = np.ascontiguousarray(rate, dtype=np.float64)
    if rate.ndim != 4:
        raise ValueError("the rate must have four axes (sample, chain, row, depth), got %r" % (rate.shape,))
    strides, step = [0] * 4, 1
    for a in (3, 2, 1, 0):
        if rate.shape[a] > 1:
            strides[a] = step
            step *= rate.shape[a]
    return rate, tuple(strides)


def resolve_rate(axis, R, rate, S, C, N, T, needed=True):
    """The rate of the new entities as (S, C|1, N|1, T|1) in the kernels' order.  axis "cols": C new columns of (C,N,T);
    "depth": C = M fitted columns and T = H new depths of (N,M,H).  rate: (S,) plus a shape that broadcasts against the
    new tensor, or None: R = results["R"], (S,) plus the model's rate shape over (N,M,T), which must not vary along the
    folded axis.  needed=False (no cell is observed, so no rate is read): without rate= a rate of 1 stands in.  ValueError on
    shapes and on rates that are not finite and positive."""
    S, C, N, T = int(S), int(C), int(N), int(T)
    new = (C, N, T) if axis == "cols" else (N, C, T)
    if rate is None and not needed:
        return np.ones((S, 1, 1, 1))
    if rate is not None:
        r = np.asarray(rate, dtype=float)
        if r.ndim == 0 or r.shape[0] != S:
            raise ValueError("rate must hold one rate (tensor) per sample: leading dimension %d, got %r" % (S, r.shape))
        tail = r.shape[1:]
        if int(np.prod(tail, dtype=np.int64)) == 1:
            tail = (1, 1, 1)
        if len(tail) != 3 or any(e not in (1, full) for e, full in zip(tail, new)):
            raise ValueError("rate %r: every axis after the first must be 1 or the new tensor's %r" % (r.shape, new))
        r = r.reshape((S,) + tuple(tail))
    else:
        if R is None:
            raise ValueError('results holds no "R": pass rate=')
        r = np.asarray(R, dtype=float)
        if r.ndim == 0 or r.shape[0] != S:
            raise ValueError('results["R"] must hold one rate (tensor) per sample: leading dimension %d, got %r' % (S, r.shape))
        tail = r.shape[1:]
        if int(np.prod(tail, dtype=np.int64)) == 1:
            tail = (1, 1, 1)
        if len(tail) != 3:
            raise ValueError('results["R"] %r must be (S,) plus the rate shape over (rows, columns, depths)' % (r.shape,))
        folded, name = (1, "column") if axis == "cols" else (2, "depth")
        if tail[folded] != 1:
            raise ValueError("the fitted rate varies along the %ss (R %r): the fit says nothing about the rate of a new %s - "
                             "pass rate=" % (name, r.shape, name))
        r = r.reshape((S,) + tuple(tail))
        if axis == "cols":
            r = r.transpose(0, 2, 1, 3)                      # (S, N|1, 1, T|1) -> (S, 1, N|1, T|1)
        if any(e not in (1, full) for e, full in zip(r.shape[1:], new)):
            raise ValueError('results["R"] %r does not match the model' % (np.shape(R),))
    if axis == "depth":
        r = r.transpose(0, 2, 1, 3)                          # (S, N|1, M|1, H|1) -> (S, M|1, N|1, H|1)
    if not np.all(np.isfinite(r)) or np.any(r <= 0):
        raise ValueError("rates must be finite and positive")
    return np.ascontiguousarray(r)


def lds_bytes(N, T, K, tf_order, horizon=None):
    """LDS one chain's workgroup needs (btf_negbin_fold_lds_bytes): the count of fold_in_cols.lds_bytes (horizon None) or
    fold_in_depth.lds_bytes plus 8 N bytes for the Polya-Gamma weights of one depth."""
    base = _fc.lds_bytes(T, K, tf_order) if horizon is None else _fd.lds_bytes(T, horizon, K, tf_order)
    return base + 8 * int(N)


def check_args(axis, S, C, N, T, K, tf_order, horizon=None, draws=None, omega=None, sweeps=None, summary=True, q=(5, 95),
               transform=None, first_sample=0):
    """Validate and normalise; raises ValueError before any device call.  axis "cols": C new columns of T depths; "depth":
    C = M fitted columns, T kept depths, horizon new ones.  draws: as fold_in_cols / fold_in_depth take it, but only with
    omega (S,C,sweeps,N,T|H) beside it.  Returns (draws or None, omega or None, qs, transform code, sweeps)."""
    if axis not in ("cols", "depth"):
        raise ValueError("axis must be 'cols' or 'depth'")
    if draws is not None and omega is None:
        raise ValueError("draws replaces the device generator only with omega= beside it (the chain also draws Polya-Gamma "
                         "variates); pass seed=")
    if int(N) < 1:
        raise ValueError("negbin_fold_in: at least one row")
    # the siblings' checks under the family name "gaussian": sizes, sweeps, q, transform and first_sample do not depend on the
    # family, and "gaussian" is the branch that validates `draws` (shape, finite, positive gammas) where "binomial" refuses it
    if axis == "cols":
        _, draws, qs, tcode, sweeps = _fc.check_args("gaussian", S, C, T, K, tf_order, draws, sweeps, summary, q, transform, first_sample)
        D = int(T)
    else:
        _, draws, qs, tcode, sweeps = _fd.check_args("gaussian", S, C, T, horizon, K, tf_order, draws, sweeps, summary, q, transform,
                                                     first_sample)
        D = int(horizon)
    need = lds_bytes(N, T, K, tf_order, None if axis == "cols" else horizon)
    if need > LDS_LIMIT:
        raise ValueError("negbin_fold_in: the band and the weights of a depth at nrows %d, ndepth %d, nembeds %d, tf_order %d need %d "
                         "bytes of LDS, beyond the limit of %d bytes a workgroup may hold" % (N, D, K, tf_order, need, LDS_LIMIT))
    if float(sweeps) * int(N) * D >= 9.0e15:
        raise ValueError("negbin_fold_in: sweeps * nrows * depths must stay below 9e15")
    if omega is not None:
        omega = np.asarray(omega, dtype=np.float64)
        if omega.shape != (S, C, sweeps, N, D):
            raise ValueError("omega must be (S,C,sweeps,N,depths) = %r, got %r" % ((S, C, sweeps, N, D), omega.shape))
        if not np.all(np.isfinite(omega)) or np.any(omega < 0):
            raise ValueError("omega must be finite and non-negative")
    return draws, omega, qs, tcode, sweeps


def _pseudo(cnt, ysum, rate):
    """(b, kappa) (N,T) of a column's cells: b = ysum + c r and kappa = (ysum - c r) / 2 where observed, 0 elsewhere."""
    r = np.broadcast_to(np.asarray(rate, dtype=float), cnt.shape)
    if np.any(r[cnt > 0] <= 0) or not np.all(np.isfinite(r)):
        raise ValueError("rates must be finite and positive")
    seen = cnt > 0
    return np.where(seen, ysum + cnt * r, 0.0), np.where(seen, (ysum - cnt * r) / 2, 0.0)


def _levels(tau2, c, b, a, dv, lam2, g, lo, hi):
    rate = (dv * dv).sum(axis=1) / (2.0 * float(lam2)) + 1.0 / np.clip(c, lo, hi)
    tau2 = np.clip(rate, lo, hi) / g[0]
    c = np.clip(1.0 / tau2 + 1.0 / b, lo, hi) / g[1]
    b = np.clip(1.0 / c + 1.0 / a, lo, hi) / g[2]
    a = np.clip(1.0 / b + 1.0, lo, hi) / g[3]
    return tau2, c, b, a


def _omega_of(omega, sweeps, shape):
    if omega is None:
        return None
    omega = np.asarray(omega, dtype=float)
    if omega.shape != (int(sweeps),) + tuple(shape):
        raise ValueError("omega must be (sweeps,N,depths) = %r, got %r" % ((int(sweeps),) + tuple(shape), omega.shape))
    return omega


def chain_cols(Y_col, W, rate, lam2, tf_order, sweeps, draws, omega=None, stability=STABILITY, on_system=None, on_sweep=None, seed=None):
    """The whole chain of one (sample, new column): fold_in_cols.chain(family="binomial") with the cell's trials and kappa
    replaced by b = ysum + c r and (ysum - c r) / 2.  Y_col (N,T) or (N,T,nreps) counts, nan = missing; rate broadcasts
    against (N,T); draws: the flat layout of fold_in_cols.chain (draws_length).  omega (sweeps,N,T): the weights in the place
    of every Polya-Gamma draw (read where the cell is observed); None: fold_in_cols.polya_gamma on numpy's generator seeded
    by `seed`, called as fold_in_cols.chain calls it.  on_system(Q), on_sweep(r, v): as fold_in_cols.chain.  Returns (v (T,K), mean (T,K), tau2 (nD,)) of the last sweep."""
    W = np.asarray(W, dtype=float)
    N, K = W.shape
    Y = np.asarray(Y_col, dtype=float)
    cnt, ysum = cell_statistics(Y, Y.shape[:2], "Y_col")
    if cnt.shape[0] != N:
        raise ValueError("the column %r does not match W %r" % (cnt.shape, W.shape))
    b_pg, sums = _pseudo(cnt, ysum, rate)
    T = cnt.shape[1]
    omega = _omega_of(omega, sweeps, (N, T))
    pg_rng = np.random.default_rng(seed) if omega is None else None
    D = _fc.penalty(T, tf_order)
    nD, n = D.shape[0], T * K
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if int(sweeps) < 1 or draws.size != 4 * nD + int(sweeps) * (n + 4 * nD):
        raise ValueError("draws must hold 4 nD + sweeps (T K + 4 nD) = %d values, got %d" % (4 * nD + int(sweeps) * (n + 4 * nD), draws.size))
    lo, hi = float(stability), 1.0 / float(stability)
    tau2, c, b, a = _fc.start_levels(draws[:4 * nD].reshape(4, nD))
    pos = 4 * nD
    v = np.zeros(n)
    for r in range(int(sweeps)):
        z, g = draws[pos:pos + n], draws[pos + n:pos + n + 4 * nD].reshape(4, nD)
        pos += n + 4 * nD
        if omega is None:
            weights = _fc.polya_gamma(pg_rng, b_pg, W.dot(v.reshape(T, K).T))
        else:
            weights = np.where(cnt > 0, omega[r], 0.0)
        mean, Q = _fc._system_of_blocks(*_fc._blocks(weights, sums, W), lam2, tau2, tf_order)
        if on_system is not None:
            on_system(Q)
        v = mean + np.linalg.solve(np.linalg.cholesky(Q).T, z)
        tau2, c, b, a = _levels(tau2, c, b, a, D.dot(v.reshape(T, K)), lam2, g, lo, hi)
        if on_sweep is not None:
            on_sweep(r, v.reshape(T, K))
    return v.reshape(T, K), mean.reshape(T, K), tau2


def chain_depth(Y_slice, W, V_old, rate, lam2, tf_order, sweeps, draws, omega=None, stability=STABILITY, on_system=None, on_sweep=None, seed=None):
    """The whole chain of one (sample, fitted column) over H new depths: fold_in_depth.chain(family="binomial") with the
    cell's trials and kappa replaced by b = ysum + c r and (ysum - c r) / 2.  Y_slice (N,H) or (N,H,nreps) counts, nan =
    missing (all nan: the forecast); V_old (T,K) the kept curve; rate broadcasts against (N,H); draws: the flat layout of
    fold_in_depth.chain.  omega (sweeps,N,H) as in chain_cols.  Returns (v (H,K), mean (H,K), tau2 (nR,))."""
    W = np.asarray(W, dtype=float)
    N, K = W.shape
    V_old = _fd._kept(V_old, K)
    T = V_old.shape[0]
    Y = np.asarray(Y_slice, dtype=float)
    cnt, ysum = cell_statistics(Y, Y.shape[:2], "Y_slice")
    if cnt.shape[0] != N:
        raise ValueError("the slice %r does not match W %r" % (cnt.shape, W.shape))
    b_pg, sums = _pseudo(cnt, ysum, rate)
    H = cnt.shape[1]
    omega = _omega_of(omega, sweeps, (N, H))
    pg_rng = np.random.default_rng(seed) if omega is None else None
    _, D_o, D_n = _fd.new_rows(T, H, tf_order)
    nR, n = D_n.shape[0], H * K
    off = D_o.dot(V_old)
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if int(sweeps) < 1 or draws.size != 4 * nR + int(sweeps) * (n + 4 * nR):
        raise ValueError("draws must hold 4 nR + sweeps (H K + 4 nR) = %d values, got %d" % (4 * nR + int(sweeps) * (n + 4 * nR), draws.size))
    lo, hi = float(stability), 1.0 / float(stability)
    tau2, c, b, a = _fc.start_levels(draws[:4 * nR].reshape(4, nR))
    pos = 4 * nR
    v = np.tile(V_old[T - 1], H)
    for r in range(int(sweeps)):
        z, g = draws[pos:pos + n], draws[pos + n:pos + n + 4 * nR].reshape(4, nR)
        pos += n + 4 * nR
        if omega is None:
            weights = _fc.polya_gamma(pg_rng, b_pg, W.dot(v.reshape(H, K).T))
        else:
            weights = np.where(cnt > 0, omega[r], 0.0)
        mean, Q = _fd._system(weights, sums, W, lam2, tau2, off, D_n)
        if on_system is not None:
            on_system(Q)
        v = mean + np.linalg.solve(np.linalg.cholesky(Q).T, z)
        tau2, c, b, a = _levels(tau2, c, b, a, off + D_n.dot(v.reshape(H, K)), lam2, g, lo, hi)
        if on_sweep is not None:
            on_sweep(r, v.reshape(H, K))
    return v.reshape(H, K), mean.reshape(H, K), tau2


def evaluate(axis, S, C, N, T, K, tf_order, cnt, ysum, rate, Ws, lam2, Vs=None, horizon=None, draws=None, omega=None, seed=0,
             sweeps=None, summary=True, q=(5, 95), transform=None, first_sample=0, stability=STABILITY, device=0):
    """Run the device evaluation and unpack it (stateless: the samples are always uploaded).  axis "cols": cnt, ysum (C,N,T)
    from cell_statistics, Ws (S,N,K); "depth": cnt, ysum (N,M,H), C = M, Vs (S,M,T,K) - its last min(T, tf_order + 1)
    depths are uploaded.  rate: resolve_rate's array.  lam2 (S,).  Returns the dict of fold_in_cols / fold_in_depth."""
    from . import _native
    draws, omega, qs, tcode, sweeps = check_args(axis, S, C, N, T, K, tf_order, horizon, draws, omega, sweeps, summary, q, transform,
                                                 first_sample)
    if float(np.max(ysum, initial=0.0)) + float(np.max(cnt, initial=0.0)) * float(rate.max()) >= MAX_PSEUDO_TRIALS:
        raise ValueError("ysum + count * rate must stay below %g" % MAX_PSEUDO_TRIALS)
    cols = axis == "cols"
    D = int(T) if cols else int(horizon)
    nlev = _fc.penalty(T, tf_order).shape[0] if cols else _fd.new_rows(T, D, tf_order)[0].size
    rate, rs = rate_strides(rate)
    if omega is not None:
        omega = np.ascontiguousarray(omega.transpose(0, 1, 2, 4, 3))          # the kernels' [depth][row]
    if not cols:                                                              # the kernels' [column][depth][row]
        cnt, ysum = np.ascontiguousarray(cnt.transpose(1, 2, 0)), np.ascontiguousarray(ysum.transpose(1, 2, 0))
    V = np.zeros((S, C, D, K))
    Vm = np.zeros((S, C, D, K))
    Tau2 = np.zeros((S, C, nlev))
    mean = np.zeros((N, C, D)) if summary else None
    quant = np.zeros((len(qs), N, C, D)) if summary else None
    d = _native.dptr
    lib = _native.load()
    tail = (d(lam2), d(cnt), d(ysum), d(rate)) + rs + (d(omega), d(draws), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, int(first_sample),
                                                        float(stability), d(V), d(Vm), d(Tau2), tcode, d(qs) if len(qs) else None,
                                                        len(qs), d(mean), d(quant) if len(qs) else None)
    if cols:
        rc = lib.btf_negbin_fold_in_cols(int(device), int(S), int(C), int(N), int(T), int(K), int(tf_order), d(Ws), *tail)
    else:
        Vt = np.ascontiguousarray(Vs[:, :, T - _fd.tail_depths(T, tf_order):, :], dtype=np.float64)
        rc = lib.btf_negbin_fold_in_depth(int(device), int(S), int(N), int(C), int(T), D, int(K), int(tf_order), d(Ws), d(Vt), *tail)
    _native.check(rc, lib)
    out = {"V": V, "V_mean": Vm, "Tau2": Tau2, "nsamples": int(S)}
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out


# ---------------------------------------------------------------- new rows, with a fixed or a sampled rate

_lgamma = np.vectorize(math.lgamma, otypes=[float])


def row_histograms(Y_new):
    """(yv (R,B), h (R,B)) of new rows Y_new (R,...) with nan = missing: the distinct counts of every row in ascending order
    and how often each was observed, padded to the widest row with h = 0 (and yv = 0).  The count part of a row's likelihood
    ratio is a sum over its histogram: a Metropolis step costs the number of distinct counts, not M T nreps.  B >= 1."""
    Y = np.asarray(Y_new, dtype=float)
    if Y.ndim < 2 or Y.shape[0] < 1:
        raise ValueError("Y_new %r must hold one block of cells per new row" % (Y.shape,))
    seen = Y[~np.isnan(Y)]
    if not np.all(np.isfinite(seen)) or np.any(seen < 0) or np.any(seen != np.floor(seen)):
        raise ValueError("Y_new: counts must be finite, non-negative integers (nan marks a missing value)")
    rows = []
    for i in range(Y.shape[0]):
        y = Y[i].reshape(-1)
        rows.append(np.unique(y[~np.isnan(y)], return_counts=True))
    B = max([1] + [len(v) for v, _ in rows])
    yv, h = np.zeros((len(rows), B)), np.zeros((len(rows), B))
    for i, (v, n) in enumerate(rows):
        yv[i, :len(v)], h[i, :len(v)] = v, n
    return yv, h


def failure_log_sum(cnt, psi):
    """L = sum_cells c log(1 - P), P = ilogit(clip(psi, -10, 10)): log(1 - P) = -log1p(exp(clip(psi)))."""
    x = np.clip(np.asarray(psi, dtype=float), -10.0, 10.0)
    return float(np.where(cnt > 0, -cnt * np.log1p(np.exp(x)), 0.0).sum())


def rate_loglik_ratio(yv, h, cand, r, L):
    """The log-likelihood ratio of a row's rate (factor.py:531-536 summed over the row): sum over the histogram of
    h [rise(yv, cand) - rise(yv, r)], plus (cand - r) L.  The bracket is formed as [lgamma(yv + cand) - lgamma(yv + r)] -
    [lgamma(cand) - lgamma(r)]: each difference is of two nearby numbers, so a large count (lgamma(5000 + r) is about 4e4)
    does not leave its rounding in the small ratio."""
    yv, h = np.asarray(yv, dtype=float), np.asarray(h, dtype=float)
    cand, r = float(cand), float(r)
    count = np.where((h > 0) & (yv > 0), (_lgamma(yv + cand) - _lgamma(yv + r)) - (math.lgamma(cand) - math.lgamma(r)), 0.0)
    return float((h * count).sum() + (cand - r) * L)


def metropolis_step(logr, n, u, yv, h, L, rpropstdev, rstdev):
    """One random-walk step on log r with the normal n and the uniform u (factor.py:522-550 for one rate):
    returns (log r afterwards, accepted, prob, cand)."""
    r = math.exp(logr)
    cand_log = logr + float(rpropstdev) * float(n)
    cand = math.exp(cand_log)
    prior = (logr * logr - cand_log * cand_log) / (2.0 * float(rstdev) ** 2)
    prob = math.exp(min(max(prior + rate_loglik_ratio(yv, h, cand, r, L), -10.0), 1.0))
    accepted = bool(u <= prob and cand > 1.0)                 # the floor is the model's own (factor.py:547)
    return (cand_log if accepted else logr), accepted, prob, cand


def draws_length_rows(K, sweeps, nmetropolis=0):
    """Values in the flat `draws` of one row chain: per sweep nmetropolis normals, nmetropolis uniforms (a sampled rate; 0
    with a fixed one), then K normals."""
    return int(sweeps) * (2 * int(nmetropolis) + int(K))


def random_draws_rows(rs, K, sweeps, nmetropolis=0, size=()):
    """`draws` of chain_rows from a numpy RandomState: size + (draws_length_rows,)."""
    size, nm = tuple(size), int(nmetropolis)
    d = np.empty(size + (int(sweeps), 2 * nm + int(K)))
    d[..., :nm] = rs.normal(size=size + (int(sweeps), nm))
    d[..., nm:2 * nm] = rs.uniform(size=size + (int(sweeps), nm))
    d[..., 2 * nm:] = rs.normal(size=size + (int(sweeps), int(K)))
    return d.reshape(size + (-1,))


def chain_rows(Y_row, V, sigma2, rate, sweeps, draws, omega=None, rate_init=None, nmetropolis=30, rpropstdev=0.1, rstdev=1, seed=None,
               on_system=None, on_sweep=None, on_accept=None, pg_terms=None):
    """The whole chain of one (sample, new row), from w = 0.  Y_row (M,T) or (M,T,nreps) counts, nan = missing; V (M,T,K).
    rate: broadcasts against (M,T) and is held; None: the row has ONE scalar rate, started at rate_init and sampled.  One
    sweep, in the order of the model's resample (rate, weights, w), with psi = V w:
      rate     (sampled) L = failure_log_sum(c, psi) once, then nmetropolis times metropolis_step on the row's histogram
      weights  where c > 0: omega ~ PG(ysum + c r, psi) - omega[sweep] (sweeps,M,T) when given, else fold_in_cols.polya_gamma
               on numpy's generator seeded by `seed` (pg_terms: its terms)
      row      Q = sum omega v v' + I / sigma2, b = sum kappa v with kappa = (ysum - c r) / 2, w = Q^-1 b + L^-T z, Q = L L'
    draws: flat, per sweep nmetropolis normals and nmetropolis uniforms (sampled only), then K normals (draws_length_rows).
    on_system(Q); on_sweep(sweep, w, r); on_accept(sweep, step, prob, u, cand).  Returns (w (K,), mean (K,), rate, share of
    the chain's Metropolis steps that were accepted) at the last sweep; with a fixed rate: the rate as given, and None."""
    V = np.asarray(V, dtype=float)
    if V.ndim != 3:
        raise ValueError("V must be (M,T,K), got %r" % (V.shape,))
    M, T, K = V.shape
    Y = np.asarray(Y_row, dtype=float)
    cnt, ysum = cell_statistics(Y, (M, T), "Y_row")
    sampled = rate is None
    sweeps, nm = int(sweeps), int(nmetropolis) if sampled else 0
    if sampled:
        if rate_init is None or not (np.isfinite(rate_init) and float(rate_init) > 0):
            raise ValueError("a sampled rate starts at rate_init, finite and positive")
        if nm < 1:
            raise ValueError("nmetropolis must be at least 1")
        logr = math.log(float(rate_init))
        yv, h = row_histograms(Y[None])
    draws = np.asarray(draws, dtype=float).reshape(-1)
    if sweeps < 1 or draws.size != draws_length_rows(K, sweeps, nm):
        raise ValueError("draws must hold sweeps (2 nmetropolis + K) = %d values, got %d" % (draws_length_rows(K, max(sweeps, 0), nm), draws.size))
    omega = _omega_of(omega, sweeps, (M, T))
    pg_rng = np.random.default_rng(seed) if omega is None else None
    Vf = V.reshape(M * T, K)
    w, pos, nacc = np.zeros(K), 0, 0
    for sw in range(sweeps):
        psi = Vf.dot(w).reshape(M, T)
        if sampled:
            L = failure_log_sum(cnt, psi)
            ns, us = draws[pos:pos + nm], draws[pos + nm:pos + 2 * nm]
            pos += 2 * nm
            for step in range(nm):
                logr, acc, prob, cand = metropolis_step(logr, ns[step], us[step], yv[0], h[0], L, rpropstdev, rstdev)
                nacc += acc
                if on_accept is not None:
                    on_accept(sw, step, prob, us[step], cand)
            r = math.exp(logr)
        else:
            r = rate
        b_pg, kappa = _pseudo(cnt, ysum, r)
        if omega is None:
            weights = _fc.polya_gamma(pg_rng, b_pg, psi) if pg_terms is None else _fc.polya_gamma(pg_rng, b_pg, psi, terms=int(pg_terms))
        else:
            weights = np.where(cnt > 0, omega[sw], 0.0)
        Q = (Vf * weights.reshape(-1, 1)).T.dot(Vf) + np.eye(K) / float(sigma2)
        if on_system is not None:
            on_system(Q)
        mean = np.linalg.solve(Q, Vf.T.dot(kappa.reshape(-1)))
        w = mean + np.linalg.solve(np.linalg.cholesky(Q).T, draws[pos:pos + K])
        pos += K
        if on_sweep is not None:
            on_sweep(sw, w, r)
    return w, mean, (r if sampled else rate), (nacc / float(sweeps * nm) if sampled else None)


def resolve_row_rate(R_fit, rate, sample_rate, S, R, M, T):
    """Where the rate of R new rows of (M,T) cells comes from: ("fixed", (S, R|1, M|1, T|1)) or ("sampled", None).
      rate given, (S,) plus a shape that broadcasts against (R,M,T)       fixed, as given
      R_fit (S,1,M|1,T|1): the fitted layout does not vary along rows     fixed, the kept sample's
      R_fit (S,N,1,1), N > 1: one rate per row                            sampled, one scalar per (sample, new row)
      any other layout that varies along rows                             ValueError asking for rate=
    sample_rate=True forces sampling (and refuses rate=); False without a usable fixed rate is a ValueError."""
    S, R, M, T = int(S), int(R), int(M), int(T)
    new = (R, M, T)

    def positive(r):
        if not np.all(np.isfinite(r)) or np.any(r <= 0):
            raise ValueError("rates must be finite and positive")
        return np.ascontiguousarray(r)

    if rate is not None:
        if sample_rate:
            raise ValueError("rate= holds the rate of the new rows; sample_rate=True samples it: pass one of them")
        r = np.asarray(rate, dtype=float)
        if r.ndim == 0 or r.shape[0] != S:
            raise ValueError("rate must hold one rate (tensor) per sample: leading dimension %d, got %r" % (S, r.shape))
        tail = r.shape[1:]
        if int(np.prod(tail, dtype=np.int64)) == 1:
            tail = (1, 1, 1)
        if len(tail) != 3 or any(e not in (1, full) for e, full in zip(tail, new)):
            raise ValueError("rate %r: every axis after the first must be 1 or the new rows' %r" % (r.shape, new))
        return "fixed", positive(r.reshape((S,) + tuple(tail)))
    if sample_rate:
        return "sampled", None
    if R_fit is None:
        raise ValueError('results holds no "R": pass rate=, or sample_rate=True with rate_init=')
    r = np.asarray(R_fit, dtype=float)
    if r.ndim == 0 or r.shape[0] != S:
        raise ValueError('results["R"] must hold one rate (tensor) per sample: leading dimension %d, got %r' % (S, r.shape))
    tail = r.shape[1:]
    if int(np.prod(tail, dtype=np.int64)) == 1:
        tail = (1, 1, 1)
    if len(tail) != 3:
        raise ValueError('results["R"] %r must be (S,) plus the rate shape over (rows, columns, depths)' % (r.shape,))
    if tail[0] == 1:
        if any(e not in (1, full) for e, full in zip(tail[1:], new[1:])):
            raise ValueError('results["R"] %r does not match the model' % (np.shape(R_fit),))
        return "fixed", positive(r.reshape((S,) + tuple(tail)))
    if tail[1:] == (1, 1):
        if sample_rate is not None:                             # (False: asked not to sample)
            raise ValueError("the fit has one rate per row (R %r) and says nothing about the rate of a new row: sample_rate=False "
                             "needs rate=" % (r.shape,))
        return "sampled", None
    raise ValueError("the fitted rate varies along the rows and along another axis (R %r): the fit says nothing about the rate of a "
                     "new row - pass rate=" % (r.shape,))


def default_rate_init(R_fit, S):
    """(S,): the geometric mean of every kept sample's rates."""
    if R_fit is None:
        raise ValueError('results holds no "R" to start a sampled rate from: pass rate_init=')
    r = np.asarray(R_fit, dtype=float)
    if r.ndim == 0 or r.shape[0] != int(S):
        raise ValueError('results["R"] must hold one rate (tensor) per sample: leading dimension %d, got %r' % (S, r.shape))
    r = r.reshape(int(S), -1)
    if not np.all(np.isfinite(r)) or np.any(r <= 0):
        raise ValueError("rates must be finite and positive")
    return np.exp(np.log(r).mean(axis=1))


def resolve_rate_init(rate_init, R_fit, S, R):
    """rate_init (S,) or (S,R) as (S,R); None: default_rate_init.  Finite and positive."""
    S, R = int(S), int(R)
    r0 = default_rate_init(R_fit, S) if rate_init is None else np.asarray(rate_init, dtype=float)
    if r0.shape == (S,):
        r0 = np.repeat(r0[:, None], R, axis=1)
    if r0.shape != (S, R):
        raise ValueError("rate_init must be (S,) or (S,R) = (%d,) or (%d,%d), got %r" % (S, S, R, r0.shape))
    if not np.all(np.isfinite(r0)) or np.any(r0 <= 0):
        raise ValueError("rate_init must be finite and positive")
    return np.ascontiguousarray(r0, dtype=np.float64)


def check_args_rows(S, R, M, T, K, sampled, nmetropolis=30, rpropstdev=0.1, rstdev=1, draws=None, omega=None, sweeps=None, summary=True,
                    q=(5, 95), transform=None, first_sample=0):
    """Validate and normalise; raises ValueError before any device call.  draws (S,R,draws_length_rows) only with omega
    (S,R,sweeps,M,T) beside it.  Returns (z (S,R,sweeps,K) or None, mh (S,R,sweeps,2,nmetropolis) or None, omega or None, qs,
    transform code, sweeps, nmetropolis (0 with a fixed rate))."""
    from . import fold_in as _fr
    if draws is not None and omega is None:
        raise ValueError("draws replaces the device generator only with omega= beside it (the chain also draws Polya-Gamma "
                         "variates); pass seed=")
    if int(R) < 1 or int(M) < 1 or int(T) < 1:
        raise ValueError("negbin_fold_in_rows: at least one new row and one cell")
    if float(R) * int(M) * int(T) >= 2 ** 31:
        raise ValueError("negbin_fold_in_rows: R * M * T must stay below 2^31")
    _, _, qs, tcode, _ = _fr.check_args("gaussian", S, R, K, None, summary, q, transform, None, first_sample)
    if sweeps is None:
        sweeps = DEFAULT_SWEEPS["rows"] if sampled else _fr.DEFAULT_INNER_SWEEPS
    if int(sweeps) != sweeps or not 1 <= int(sweeps) <= MAX_ROW_SWEEPS:
        raise ValueError("sweeps must be an integer in 1..%d" % MAX_ROW_SWEEPS)
    sweeps, nm = int(sweeps), 0
    if sampled:
        if int(nmetropolis) != nmetropolis or not 1 <= int(nmetropolis) <= MAX_ROW_SWEEPS:
            raise ValueError("nmetropolis must be an integer in 1..%d when the rate is sampled" % MAX_ROW_SWEEPS)
        nm = int(nmetropolis)
        if not (np.isfinite(rpropstdev) and rpropstdev > 0 and np.isfinite(rstdev) and rstdev > 0):
            raise ValueError("rpropstdev and rstdev must be finite and positive")
    z = mh = None
    if draws is not None:
        draws = np.asarray(draws, dtype=np.float64)
        L = draws_length_rows(K, sweeps, nm)
        if draws.shape != (S, R, L):
            raise ValueError("draws must be (S,R,sweeps (2 nmetropolis + K)) = %r, got %r" % ((S, R, L), draws.shape))
        if not np.all(np.isfinite(draws)):
            raise ValueError("draws must be finite")
        d = draws.reshape(S, R, sweeps, 2 * nm + K)
        z = np.ascontiguousarray(d[..., 2 * nm:])
        if sampled:
            mh = np.ascontiguousarray(d[..., :2 * nm].reshape(S, R, sweeps, 2, nm))
            if np.any(mh[:, :, :, 1] <= 0) or np.any(mh[:, :, :, 1] >= 1):
                raise ValueError("draws: the uniforms must lie inside (0, 1)")
    if omega is not None:
        omega = np.asarray(omega, dtype=np.float64)
        if omega.shape != (S, R, sweeps, M, T):
            raise ValueError("omega must be (S,R,sweeps,M,T) = %r, got %r" % ((S, R, sweeps, M, T), omega.shape))
        if not np.all(np.isfinite(omega)) or np.any(omega < 0):
            raise ValueError("omega must be finite and non-negative")
    return z, mh, omega, qs, tcode, sweeps, nm


def evaluate_rows(S, R, M, T, K, Y_new, Vs, sigma2, rate=None, rate_init=None, nmetropolis=30, rpropstdev=0.1, rstdev=1, draws=None,
                  omega=None, seed=0, sweeps=None, summary=True, q=(5, 95), transform=None, first_sample=0, device=0):
    """Run the device evaluation of new rows and unpack it (stateless: the samples are always uploaded).  Y_new (R,M,T) or
    (R,M,T,nreps); Vs (S,M,T,K); sigma2 (S,); rate: resolve_row_rate's array, or None with rate_init (S,R): a sampled
    rate.  Returns the dict of negbin_fold_in_rows."""
    from . import _native
    sampled = rate is None
    cnt, ysum = cell_statistics(Y_new, (R, M, T))
    z, mh, omega, qs, tcode, sweeps, nm = check_args_rows(S, R, M, T, K, sampled, nmetropolis, rpropstdev, rstdev, draws, omega, sweeps,
                                                          summary, q, transform, first_sample)
    rmax = float(np.max(rate_init)) if sampled else float(rate.max())       # (a sampled rate is bounded where it starts)
    if float(np.max(ysum, initial=0.0)) + float(np.max(cnt, initial=0.0)) * rmax >= MAX_PSEUDO_TRIALS:
        raise ValueError("ysum + count * rate must stay below %g" % MAX_PSEUDO_TRIALS)
    d = _native.dptr
    if sampled:
        yv, h = row_histograms(Y_new)
        rate_args = (None, 0, 0, 0, 0, d(rate_init), d(yv), d(h), yv.shape[1])
    else:
        rate, rs = rate_strides(rate)
        rate_args = (d(rate),) + rs + (None, None, None, 0)
    if omega is not None:
        omega = np.ascontiguousarray(omega.reshape(S, R, sweeps, M * T).transpose(0, 2, 3, 1))      # the kernel's [sweep][cell][row]
    W, Wm = np.zeros((S, R, K)), np.zeros((S, R, K))
    Rout = np.zeros((S, R)) if sampled else None
    acc = np.zeros((S, R)) if sampled else None
    mean = np.zeros((R, M, T)) if summary else None
    quant = np.zeros((len(qs), R, M, T)) if summary else None
    lib = _native.load()
    rc = lib.btf_negbin_fold_in_rows(int(device), int(S), int(R), int(M), int(T), int(K), d(Vs), d(sigma2), d(cnt), d(ysum), *rate_args,
                                     nm, float(rpropstdev), float(rstdev), d(omega), d(z), d(mh), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps,
                                     int(first_sample), d(W), d(Wm), d(Rout), d(acc), tcode, d(qs) if len(qs) else None, len(qs), d(mean),
                                     d(quant) if len(qs) else None)
    _native.check(rc, lib)
    out = {"W": W, "W_mean": Wm, "nsamples": int(S)}
    if sampled:
        out["R"], out["accept"] = Rout, acc
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
