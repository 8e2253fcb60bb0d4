"""Folding new rows into a fitted posterior: the embedding of a row the chain never saw, per kept sample.

Given V the rows of W are conditionally independent (the reference's factor.py:333: the independence the project shards
on) and the prior of a row is N(0, sigma2 I).  For a NEW row with observations y (any missing pattern) and kept sample s

    Q_s = sum_{(j,t) observed} c_jt v_jt^s v_jt^s' / nu2_s + I / sigma2_s        b_s = sum ysum_jt v_jt^s / nu2_s
    w_new^s ~ N(Q_s^-1 b_s, Q_s^-1)

(c_jt observed replicates of the cell, ysum_jt their sum) - what _resample_W (factor.py:333-362) does for a row of the
fitted tensor - and one draw per kept sample is a draw from p(w_new | y_new, training data) with V and the hyper-parameters
integrated over the posterior: exact for the Gaussian model.  For the Binomial model the same holds inside a short
Polya-Gamma chain per (sample, row) started from w = 0: omega_jt ~ PG(n_jt, w . v_jt), then the Gaussian draw with weights
omega and kappa = y - n / 2 (factor.py:437-460).  The data-sized work is the HIP of csrc/btf_fold_in.h (btf_fold_in_rows /
btf_collect_fold_in); this module holds the host halves in plain numpy (importable without a GPU): the DEFINITION
(`conditional`, `draw`), the argument checks, and `evaluate`, the one caller of the C entry points.
"""
import numpy as np

from ._analysis import check_q, transform_code

FAMILIES = {"gaussian": 0, "binomial": 1}
MAX_SUMMARY_SAMPLES = 16384      # the limit of posterior_summary_kernel (one cell's values are sorted in LDS)
MAX_TRIALS = 32                  # FOLD_MAX_TRIALS of csrc/btf_fold_in.h: the counts pg_exact=None draws exactly
# rounds of the Binomial inner chain per (sample, row): the smallest count after which the largest |z| of the mean against
# the quadrature posterior no longer falls ("Folding new rows in", table of scripts/fold_in_rate.py --sweeps)
DEFAULT_INNER_SWEEPS = 4


def family_code(family):
    if family not in FAMILIES:
        raise ValueError("family must be one of %s" % (tuple(FAMILIES),))
    return FAMILIES[family]


def conditional(Y_row, V, nu2, sigma2):
    """The Gaussian conditional of one new row in numpy: the definition the kernel is tested against.
    Y_row (M,T) or (M,T,nreps), nan = missing; V (M,T,K).  Returns (mean, Q) with Q = sum c v v' / nu2 + I / sigma2 and
    mean = Q^-1 b, b = sum ysum v / nu2."""
    Y = np.asarray(Y_row, dtype=float)
    V = np.asarray(V, dtype=float)
    if Y.ndim == 2:
        Y = Y[..., None]
    M, T, K = V.shape
    if Y.shape[:2] != (M, T):
        raise ValueError("Y_row %r does not match V %r" % (Y.shape, V.shape))
    obs = ~np.isnan(Y)
    c = obs.sum(axis=2).astype(float).reshape(-1)
    ysum = np.where(obs, Y, 0.0).sum(axis=2).reshape(-1)
    Vf = V.reshape(M * T, K)
    Q = (Vf * c[:, None]).T.dot(Vf) / float(nu2) + np.eye(K) / float(sigma2)
    b = Vf.T.dot(ysum) / float(nu2)
    return np.linalg.solve(Q, b), Q


def draw(mean, Q, z):
    """w = mean + L^-T z with Q = L L' (factor.py:357-362 with its normals z)."""
    L = np.linalg.cholesky(np.asarray(Q, dtype=float))
    return np.asarray(mean, dtype=float) + np.linalg.solve(L.T, np.asarray(z, dtype=float))


def row_statistics(Y_new, family, M, T, trials=None):
    """(R, weights (R,M,T), sums (R,M,T)) of the new rows.  Gaussian: observed replicates and their sum per cell; Binomial:
    trials and successes of the observed cells (a cell with nan in either, or without trials, is missing).  ValueError on a
    shape that does not match (M, T)."""
    code = family_code(family)
    if code == FAMILIES["gaussian"]:
        if isinstance(Y_new, (tuple, list)):
            raise ValueError("Gaussian rows are one (R,M,T) or (R,M,T,nreps) array, not a pair")
        Y = np.asarray(Y_new, dtype=float)
        if Y.ndim == 3:
            Y = Y[..., None]
        if Y.ndim != 4 or Y.shape[0] < 1 or Y.shape[1:3] != (M, T) or Y.shape[3] < 1:
            raise ValueError("Y_new %r must be (R,%d,%d) or (R,%d,%d,nreps)" % (np.shape(Y_new), M, T, M, T))
        if np.isinf(Y).any():
            raise ValueError("Y_new holds infinite values (nan marks a missing observation)")
        obs = ~np.isnan(Y)
        return Y.shape[0], np.ascontiguousarray(obs.sum(axis=3), dtype=np.float64), \
            np.ascontiguousarray(np.where(obs, Y, 0.0).sum(axis=3))
    if isinstance(Y_new, (tuple, list)):
        if len(Y_new) != 2:
            raise ValueError("Binomial rows are a (Y, N) pair")
        Y, N = np.asarray(Y_new[0], dtype=float), np.asarray(Y_new[1], dtype=float)
    else:
        Y = np.asarray(Y_new, dtype=float)
        N = np.ones(Y.shape) if trials is None else np.broadcast_to(np.asarray(trials, dtype=float), Y.shape)
    if Y.ndim != 3 or Y.shape[0] < 1 or Y.shape[1:] != (M, T) or N.shape != Y.shape:
        raise ValueError("Binomial Y_new %r / trials %r must be (R,%d,%d)" % (Y.shape, N.shape, M, T))
    obs = ~(np.isnan(Y) | np.isnan(N)) & (np.nan_to_num(N) > 0)
    n = np.where(obs, N, 0.0)
    y = np.where(obs, Y, 0.0)
    if np.any(n != np.floor(n)) or np.any(n > MAX_TRIALS) or not np.all(np.isfinite(n)):
        raise ValueError("Binomial trial counts must be integers up to %d (larger counts are not folded in yet)" % MAX_TRIALS)
    if np.any(y < 0) or np.any(y > n) or not np.all(np.isfinite(y)):
        raise ValueError("Binomial successes must lie in [0, trials]")
    return Y.shape[0], np.ascontiguousarray(n), np.ascontiguousarray(y)


def check_args(family, S, R, K, z=None, summary=True, q=(5, 95), transform=None, inner_sweeps=None, first_sample=0):
    """Validate and normalise; raises ValueError before any device call.  Returns (family code, z or None, qs, transform
    code, inner_sweeps)."""
    code = family_code(family)
    if int(S) < 1:
        raise ValueError("fold_in_rows: at least one sample")
    if not 1 <= int(K) <= 10:
        raise ValueError("fold_in_rows: nembeds must be 1..10")
    tcode = transform_code(transform)
    if summary and int(S) > MAX_SUMMARY_SAMPLES:
        raise ValueError("fold_in_rows: %d samples exceed the %d of the summary kernel; thin the samples or pass summary=False"
                         % (S, MAX_SUMMARY_SAMPLES))
    if int(first_sample) < 0 or (int(first_sample) + int(S)) * int(R) >= 2 ** 31:
        raise ValueError("fold_in_rows: first_sample must be >= 0 and (first_sample + S) * R below 2^31")
    qs = check_q(q, allow_none=True) if summary else np.zeros(0)
    if z is not None:
        if code != FAMILIES["gaussian"]:
            raise ValueError("z replaces the device generator for the Gaussian model only (the Binomial chain also draws Polya-Gamma variates)")
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.shape != (S, R, K):
            raise ValueError("z must be (S,R,K) = (%d,%d,%d), got %r" % (S, R, K, z.shape))
        if not np.all(np.isfinite(z)):
            raise ValueError("z must be finite")
    if inner_sweeps is None:
        inner_sweeps = DEFAULT_INNER_SWEEPS
    if int(inner_sweeps) != inner_sweeps or int(inner_sweeps) < 1:
        raise ValueError("inner_sweeps must be a positive integer")
    return code, z, qs, tcode, int(inner_sweeps)


def evaluate(family, S, R, M, T, K, weights, sums, z=None, seed=0, summary=True, q=(5, 95), transform=None, inner_sweeps=None,
             first_sample=0, ctx=None, Vs=None, nu2=None, sigma2=None, device=0):
    """Run the device evaluation and unpack it.  ctx with Vs None: the context's first S collected samples (no upload, nu2
    and sigma2 from the collected scalars); otherwise Vs (S,M,T,K), nu2 (S,), sigma2 (S,) are uploaded (stateless entry
    point).  weights / sums: row_statistics.  Returns the dict of BayesianTensorFiltering.fold_in_rows."""
    from . import _native
    code, z, qs, tcode, sweeps = check_args(family, S, R, K, z, summary, q, transform, inner_sweeps, first_sample)
    gauss = code == FAMILIES["gaussian"]
    W = np.zeros((S, R, K))
    Wm = np.zeros((S, R, K)) if gauss else None
    mean = np.zeros((R, M, T)) if summary else None
    quant = np.zeros((len(qs), R, M, T)) if summary else None
    d = _native.dptr
    cnt, trials = (weights, None) if gauss else (None, weights)
    tail = (d(cnt), d(sums), d(trials), d(z), int(seed) & 0xFFFFFFFFFFFFFFFF, sweeps, int(first_sample), d(W), d(Wm), tcode,
            d(qs) if len(qs) else None, len(qs), d(mean), d(quant) if len(qs) else None)
    if Vs is None:
        ctx.call("btf_collect_fold_in", code, int(S), int(R), *tail)
    else:
        lib = _native.load()
        _native.check(lib.btf_fold_in_rows(int(device), code, int(S), int(R), int(M), int(T), int(K), d(Vs), d(nu2), d(sigma2), *tail),
                      lib)
    out = {"W": W, "nsamples": int(S)}
    if gauss:
        out["W_mean"] = Wm
    if summary:
        out["mean"], out["quantiles"] = mean, quant
    return out
