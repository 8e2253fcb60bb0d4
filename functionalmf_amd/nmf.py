"""Non-negative tensor factorisation and the factor PAV projection on the GPU: the chain initialisers of the reference's
examples (functionalmf.utils.tensor_nmf, utils.py:276-420, and factor_pav, utils.py:218-252).  tensor_nmf is the plain
factorisation; bounded_tensor_nmf adds the reference's max_entry projection and its row_features.

The host draws the starting point (numpy's legacy stream, in the reference's order) and builds compact statistics of the
data once: per cell the sum of the observed replicates and their count, plus the within-cell sum of squares.  Every ALS
step - the NNLS solves of all rows, of all (column, depth) cells, the PAV projection and the stopping rule - runs on the
device (csrc/btf_nmf.h); the host reads the factors once, at the end.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _native

MAX_NEMBEDS = 10


def _as_Y4(Y):
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 3:
        Y = Y[..., None]
    if Y.ndim != 4 or min(Y.shape) < 1:
        raise ValueError("Y must be (N, M, T) or (N, M, T, R) with every dimension at least 1, got %s" % (Y.shape,))
    if Y.shape[3] > 255:
        raise ValueError("at most 255 replicates per cell")
    if np.isinf(Y).any():
        raise ValueError("Y must be finite or nan (missing)")
    return Y


def _check_finite(name, a):
    """A given factor holding nan or inf would make every dual of the device's NNLS compare false: each system would come
    back as the 1e-3 floor and the run would spend max_steps.  Refused here, as scipy's nnls refuses it in the reference."""
    if a is not None and not np.isfinite(np.asarray(a, dtype=np.float64)).all():
        raise ValueError("%s must be finite" % name)


def nmf_statistics(Y):
    """(S, counts, ssw) of Y (N,M,T[,R]): S (N, M*T) float64 = sum of the observed replicates of each cell, counts
    (N, M*T) uint8 = their number, or None when nothing is missing, and ssw = sum over observed entries of
    (y - cell mean)^2."""
    Y = _as_Y4(Y)
    N, M, T, R = Y.shape
    obs = ~np.isnan(Y)
    Y0 = np.where(obs, Y, 0.0)
    S = Y0.sum(axis=3)
    cnt = obs.sum(axis=3)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, S / np.maximum(cnt, 1), 0.0)
    ssw = float(np.sum(np.where(obs, Y0 - mean[..., None], 0.0) ** 2)) if R > 1 else 0.0
    counts = None if bool(obs.all()) else np.ascontiguousarray(cnt.reshape(N, M * T), dtype=np.uint8)
    return np.ascontiguousarray(S.reshape(N, M * T)), counts, ssw


class NMFData:
    """The statistics of one data tensor uploaded to a device (btf_nmf_create); `run` can be called repeatedly."""

    def __init__(self, Y, nembeds, device=0):
        Y = _as_Y4(Y)
        self.shape = Y.shape
        self.nembeds = int(nembeds)
        S, counts, ssw = nmf_statistics(Y)
        self.complete = counts is None
        self.lib = _native.load()
        self.h = C.c_void_p()
        self._bounded = False
        N, M, T, R = Y.shape
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint8)) if counts is not None else None
        _native.check(self.lib.btf_nmf_create(C.byref(self.h), int(device), N, M, T, R, self.nembeds, _native.dptr(S), cp, ssw),
                      self.lib)

    def close(self):
        if getattr(self, "h", None):
            self.lib.btf_nmf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, W, V, max_steps=30, monotone=False, tol=1e-4, verbose=False, fit_W=True, fit_V=True, timing=False,
            max_entry=None, row_features=None, R=None):
        """ALS from (W, V); returns (W, V, info) with new arrays.  info: steps, rmse (one per step run) and, with
        timing=True, device_ms (device time of the queued steps).  max_entry: every fitted row, cell and feature row whose
        entries exceed it is projected (see bounded_tensor_nmf).  row_features X (N, F), nan = missing, with the
        starting R (F, K): info["R"] is the fitted R.  With either, info also holds projected_rows (N,), projected_cells
        (M, T) and projected_features (F,), the systems projected in the last step run, and projected (per step: their
        number)."""
        W = np.array(W, dtype=np.float64, order="C", copy=True)
        V = np.array(V, dtype=np.float64, order="C", copy=True)
        N, M, T = self.shape[:3]
        for name, a in (("W", W), ("V", V), ("R", R)):
            _check_finite(name, a)
        if max_entry is not None and not (np.isfinite(max_entry) and max_entry > 0):
            raise ValueError("max_entry must be positive and finite, got %r" % (max_entry,))
        if (row_features is None) != (R is None):
            raise ValueError("row_features and R come together")
        steps = C.c_int32(0)
        hist = np.zeros(max(int(max_steps), 1))
        ms = np.zeros(1)
        if max_entry is None and row_features is None:
            if self._bounded:                               # a handle that ran bounded before: back to the plain state
                self._set(0.0, None)
            _native.check(self.lib.btf_nmf_run(self.h, _native.dptr(W), _native.dptr(V), int(bool(fit_W)), int(bool(fit_V)),
                                               int(bool(monotone)), int(max_steps), float(tol), int(bool(verbose)),
                                               C.byref(steps), _native.dptr(hist), _native.dptr(ms) if timing else None),
                          self.lib)
            flags = nproj = None
        else:
            F = 0
            if row_features is not None:
                X = _check_features(row_features, N)
                F = X.shape[1]
                R = np.array(R, dtype=np.float64, order="C", copy=True)
                if R.shape != (F, self.nembeds):
                    raise ValueError("R must be (%d, %d), got %s" % (F, self.nembeds, R.shape))
            self._set(0.0 if max_entry is None else float(max_entry), X if F else None)
            flags = np.zeros(N + M * T + F, dtype=np.uint8)
            nproj = np.zeros(max(int(max_steps), 1), dtype=np.int32)
            _native.check(self.lib.btf_nmf_run_bounded(
                self.h, _native.dptr(W), _native.dptr(V), _native.dptr(R) if F else None, int(bool(fit_W)), int(bool(fit_V)),
                int(bool(monotone)), int(max_steps), float(tol), int(bool(verbose)), C.byref(steps), _native.dptr(hist),
                _native.dptr(ms) if timing else None, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                nproj.ctypes.data_as(C.POINTER(C.c_int32))), self.lib)
        info = {"steps": int(steps.value), "rmse": hist[:steps.value].copy()}
        if timing:
            info["device_ms"] = float(ms[0])
        if flags is not None:
            info["projected_rows"] = flags[:N].astype(bool)
            info["projected_cells"] = flags[N:N + M * T].astype(bool).reshape(M, T)
            info["projected_features"] = flags[N + M * T:].astype(bool)
            info["projected"] = nproj[:steps.value].copy()
            if row_features is not None:
                info["R"] = R
        return W, V, info

    def _set(self, max_entry, X):
        """Bounds and features of the handle for the next run (btf_nmf_set_bounds / btf_nmf_set_row_features)."""
        _native.check(self.lib.btf_nmf_set_bounds(self.h, max_entry), self.lib)
        if X is None:
            _native.check(self.lib.btf_nmf_set_row_features(self.h, 0, None, None), self.lib)
        else:
            obs = ~np.isnan(X)
            SX = np.ascontiguousarray(np.where(obs, X, 0.0))
            op = None if bool(obs.all()) else np.ascontiguousarray(obs, dtype=np.uint8)
            _native.check(self.lib.btf_nmf_set_row_features(self.h, X.shape[1], _native.dptr(SX),
                                                            op.ctypes.data_as(C.POINTER(C.c_uint8)) if op is not None else None),
                          self.lib)
        self._bounded = max_entry > 0 or X is not None


def _check_features(row_features, N):
    X = np.asarray(row_features, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != N or X.shape[1] < 1:
        raise ValueError("row_features must be (%d, F) with F >= 1, got %s" % (N, X.shape))
    if np.isinf(X).any():
        raise ValueError("row_features must be finite or nan (missing)")
    return X


def _check_nembeds(nembeds):
    if isinstance(nembeds, bool) or int(nembeds) != nembeds or not 1 <= int(nembeds) <= MAX_NEMBEDS:
        raise ValueError("nembeds must be an integer in 1..%d, got %r" % (MAX_NEMBEDS, nembeds))
    return int(nembeds)


def tensor_nmf(Y, nembeds, max_steps=30, monotone=False, tol=1e-4, verbose=False, max_entry=None, W=None, V=None,
               fit_W=True, fit_V=True, row_features=None, device=0, return_info=False):
    """Non-negative factorisation Y[i,j,t,r] ~ W[i] . V[j,t] by alternating NNLS, optionally with each column's curves
    W_i . V[j] non-increasing in t (monotone=True, factor_pav after every V step).  Drop-in for
    functionalmf.utils.tensor_nmf (utils.py:276-419): the same starting point under np.random.seed, the same steps and
    stopping rule.  Returns (W, V) float64 of shapes (N, K) and (M, T, K), or (W, V, info) with return_info=True: info
    holds `steps` (ALS steps run) and `rmse` (per step: sqrt of the residual sum of squares).  Given W / V are not
    modified.  `max_entry` and `row_features` raise NotImplementedError here: bounded_tensor_nmf takes them.

    A given W or V (or R of bounded_tensor_nmf) holding nan or inf, and +-inf in Y, raise ValueError before any device
    call; nan in Y is a missing entry.  The reference refuses such input too: its scipy.optimize.nnls calls
    (utils.py:335, 366, 395) check the design matrix, built from the fixed factor, and the data with asarray_chkfinite.
    It does so in the first solve that meets the value; here every argument is checked up front."""
    if max_entry is not None:
        raise NotImplementedError("tensor_nmf: max_entry (the reference's SLSQP projection) is bounded_tensor_nmf's")
    if row_features is not None:
        raise NotImplementedError("tensor_nmf: row_features (side information) is bounded_tensor_nmf's")
    W, V, info = _als(Y, nembeds, None, None, None, max_steps, monotone, tol, verbose, W, V, fit_W, fit_V, device)
    if return_info:
        return W, V, info
    return W, V


def _als(Y, nembeds, max_entry, row_features, R, max_steps, monotone, tol, verbose, W, V, fit_W, fit_V, device):
    """The argument checks, the reference's starting point and the run shared by tensor_nmf and bounded_tensor_nmf."""
    K = _check_nembeds(nembeds)
    Yarr = np.asarray(Y)
    if Yarr.ndim not in (3, 4) or min(Yarr.shape) < 1:
        raise ValueError("Y must be (N, M, T) or (N, M, T, R), got shape %s" % (Yarr.shape,))
    N, M, T = Yarr.shape[:3]
    if int(max_steps) != max_steps or max_steps < 0:
        raise ValueError("max_steps must be a non-negative integer")
    if W is not None and np.shape(W) != (N, K):
        raise ValueError("W must be (%d, %d), got %s" % (N, K, np.shape(W)))
    if V is not None and np.shape(V) != (M, T, K):
        raise ValueError("V must be (%d, %d, %d), got %s" % (M, T, K, np.shape(V)))
    if max_entry is not None and not (np.isfinite(max_entry) and max_entry > 0):
        raise ValueError("max_entry must be positive and finite, got %r" % (max_entry,))
    for name, a in (("W", W), ("V", V), ("R", R)):
        _check_finite(name, a)
    if np.isinf(np.asarray(Yarr, dtype=np.float64)).any():
        raise ValueError("Y must be finite or nan (missing)")
    X = None
    if row_features is not None:
        X = _check_features(row_features, N)
        if R is not None and np.shape(R) != (X.shape[1], K):
            raise ValueError("R must be (%d, %d), got %s" % (X.shape[1], K, np.shape(R)))
    elif R is not None:
        raise ValueError("R given without row_features")
    # the reference's starting point, from the legacy global stream in its order (utils.py:283-295)
    if W is None:
        W = np.random.gamma(1, 1, size=(N, K))
        if N > 1:
            W[np.triu_indices(K, k=1)] = 0
    if V is None:
        V = np.random.gamma(1, 1, size=(M, T, K))
    if X is not None and R is None:
        R = np.random.gamma(1, 1, size=(X.shape[1], K))
    data = NMFData(Yarr, K, device=device)
    try:
        return data.run(W, V, max_steps=int(max_steps), monotone=monotone, tol=tol, verbose=verbose, fit_W=fit_W,
                        fit_V=fit_V, max_entry=max_entry, row_features=X, R=R)
    finally:
        data.close()


def bounded_tensor_nmf(Y, nembeds, max_entry=None, row_features=None, R=None, max_steps=30, monotone=False, tol=1e-4,
                       verbose=False, W=None, V=None, fit_W=True, fit_V=True, device=0, return_info=False):
    """tensor_nmf with the reference's `max_entry` and `row_features` (utils.py:294-295, 326-347, 369-377, 384-407).

    max_entry: after its NNLS solve every row of W (leading d = min(K, i+1) entries) and every cell V[j,t] whose fitted
    entries W V' exceed max_entry is replaced by the least-squares solution under 0 <= W V' <= max_entry over all cells
    (rows) and x >= 1e-6: SLSQP in the reference, an exact dual active-set solve on the device here, so the two agree to
    SLSQP's stopping slack.  With monotone=True and data in [0, 1] the result starts a [0,1] + monotone constrained chain.

    row_features X (N, F), nan = missing: side information per row.  R (F, K) is drawn after W and V from the legacy
    stream (or given, to restart from a state); the observed X[i] join row i's system with R as their design rows, and
    after the V step every R[f] = max(NNLS(W[obs], X[obs, f]), 1e-3), projected like a cell; a feature nobody observed
    keeps its value.  The rmse and the stopping rule use Y only.

    Returns (W, V), or (W, V, R) with row_features, with info appended when return_info=True (NMFData.run lists its
    keys).  Without max_entry and row_features the result is tensor_nmf's, bit for bit."""
    W, V, info = _als(Y, nembeds, max_entry, row_features, R, max_steps, monotone, tol, verbose, W, V, fit_W, fit_V, device)
    out = (W, V) if row_features is None else (W, V, info.pop("R"))
    return out + (info,) if return_info else out


def factor_pav(W, V, in_place=False, device=0):
    """Pool-adjacent-violators projection of V so that W @ V[t] does not increase with t, for every row of W
    (functionalmf.utils.factor_pav, utils.py:218-252).  V is one column's (T, K) block or a batch (M, T, K); each
    column is projected on its own.  Returns V projected (the given array itself with in_place=True)."""
    W = np.asarray(W)
    Varr = np.asarray(V)
    if W.ndim != 2 or Varr.ndim not in (2, 3) or W.shape[1] != Varr.shape[-1] or min(W.shape) < 1 or min(Varr.shape) < 1:
        raise ValueError("W must be (N, K) and V (T, K) or (M, T, K) with the same K")
    K = _check_nembeds(W.shape[1])
    Wc = _native.as_f64(W)
    out = np.array(Varr, dtype=np.float64, order="C", copy=True)
    V3 = out.reshape((1,) + out.shape) if out.ndim == 2 else out
    M, T = V3.shape[:2]
    lib = _native.load()
    _native.check(lib.btf_nmf_pav(int(device), W.shape[0], M, T, K, _native.dptr(Wc), _native.dptr(V3)), lib)
    if in_place:
        if not isinstance(V, np.ndarray):
            raise ValueError("in_place=True needs V to be a numpy array")
        V[...] = out
        return V
    return out
