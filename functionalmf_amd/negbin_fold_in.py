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
the new entity is out of scope, as are new ROWS and pg_exact=True.

The data-sized work is the HIP of csrc/btf_fold_chain.h (negbin_draw_depth, negbin_accumulate) in the third family of
fold_cols_kernel / fold_depth_kernel (btf_negbin_fold_in_cols / btf_negbin_fold_in_depth); this module holds the host halves
in plain numpy (importable without a GPU): the DEFINITION (`chain_cols`, `chain_depth`), the argument checks, and `evaluate`,
the one caller of the C entry points.  With `draws` and `omega` together a chain is a deterministic function of its inputs:
that is the replay the kernels are tested against.
"""
import numpy as np

from . import fold_in_cols as _fc
from . import fold_in_depth as _fd

LDS_LIMIT = _fc.LDS_LIMIT
STABILITY = _fc.STABILITY
MAX_PSEUDO_TRIALS = 1e15         # b = ysum + c r must stay below it (negbin_fold_cells_check of csrc/btf_analysis.hip)
DEFAULT_SWEEPS = {"cols": _fc.DEFAULT_SWEEPS, "depth": _fd.DEFAULT_SWEEPS}     # the Binomial family's


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
