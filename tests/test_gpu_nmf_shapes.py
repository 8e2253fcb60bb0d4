"""tensor_nmf, bounded_tensor_nmf and factor_pav (csrc/btf_nmf.h) where the fixtures of test_gpu_nmf.py and
test_gpu_nmf_bounded.py never go: every nembeds 1..10, the ragged edges of the launch geometry (a last wave of one cell,
a last 1024-cell chunk of one cell, a last slab of one or two rows, the 256-row slabs of more than 1024 rows, 255
replicates), NNLS systems whose support is chosen, degenerate systems, the PAV kernel's block-strided loops and its
largest column, and the max_entry projection at nembeds 6..9.  Every reference is float64 numpy / scipy written here.

  1. Half-steps (max_steps=1, fit_V=False or fit_W=False) on data built so that the solution x* of every full-rank system
     is known: with G = A'A, a support P, x*_P >= 0.05 and multipliers mu >= 0.05 off P, b = A x* - A G^-1 mu makes x* the
     unique NNLS solution with strict complementarity (A'(b - A x*) = -mu).  A system with fewer observed design rows
     than unknowns (3 cells for up to 10 unknowns at (5, 1, 3, 1) and (1025, 1, 3, 2)) has no unique solution: its data is
     b = A x0 with x0 >= 0, the optimal residual is 0, and the fit is compared as in part 2.
  2. Degenerate systems against a brute force over all supports.
  3. factor_pav against a numpy transcription of the sweep documented above nmf_pav_kernel.
  4. The max_entry projection at nembeds 6..9 by a KKT certificate.
"""
import itertools

import numpy as np
import pytest
from scipy.optimize import nnls

from functionalmf_amd import _native, utils

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
FLOOR = 1e-3
XMIN = 1e-6


def _rmse(Y, W, V):
    Y4 = Y if Y.ndim == 4 else Y[..., None]
    return np.sqrt(np.nansum((Y4 - np.einsum("nk,mtk->nmt", W, V)[..., None]) ** 2))


# ---------------------------------------------------------------------------------------------------------------- part 1
ALL_K = list(range(1, 11))
HALF_SHAPES = [((5, 1, 3, 1), [1, 3, 6, 7, 8, 9, 10]),        # 3-D Y, ssw = 0, M T < 64, every row truncated for K > 5
               ((67, 5, 13, 2), ALL_K),                      # M T = 65; two solve workgroups, RB tail of 3, slab of 3 rows
               ((130, 25, 41, 3), [2, 4, 6, 7, 8, 9, 10]),   # M T = 1025: a chunk of one cell; a last slab of 2 rows
               ((1025, 1, 3, 2), ALL_K),                     # 256-row slabs, the last of one row
               ((3, 1, 2, 255), [2])]                        # the largest replicate count of the u8 counts
HALF_CASES = [(shape, K, miss) for shape, ks in HALF_SHAPES for K in ks for miss in (False, True)]


def _observed(N, MT, R, K, rs):
    """Which replicates are observed: whole cells and single replicates dropped, then cells given back until every row
    keeps min(d, M T) observed cells and every cell min(K, N) observed rows."""
    obs = np.ones((N, MT, R), dtype=bool)
    obs[rs.uniform(size=(N, MT)) < 0.12] = False
    if R > 1:
        obs &= (rs.uniform(size=(N, MT, R)) >= 0.12) | ~obs.any(axis=2, keepdims=True)
    for i in range(N):
        gone = np.flatnonzero(~obs[i].any(axis=1))
        short = min(min(K, i + 1), MT) - (MT - gone.size)
        if short > 0:
            obs[i, rs.choice(gone, short, replace=False)] = True
    for c in range(MT):
        gone = np.flatnonzero(~obs[:, c].any(axis=1))
        short = min(K, N) - (N - gone.size)
        if short > 0:
            obs[rs.choice(gone, short, replace=False), c] = True
    if obs.all():                                            # nothing could be dropped: one entry goes all the same
        obs[0, MT - 1, R - 1] = False
    return obs


def _all_supports(d):
    return [np.array(m, dtype=bool) for m in itertools.product([False, True], repeat=d)]


def _build_half(side, W0, Vm, obs, rs):
    """The systems of one half-step (side "W": one per row, design = the cells' v_jt[:d]; side "V": one per cell, design =
    the rows of W0), each with its constructed data, and the data tensor Y (N, M T, R) with nan where nothing is observed.
    Every replicate of a cell is its target plus an offset that sums to zero over the cell's observed replicates."""
    N, K = W0.shape
    MT = Vm.shape[0]
    R = obs.shape[2]
    cnt = obs.sum(axis=2)
    systems = []
    for s in range(N if side == "W" else MT):
        d = min(K, s + 1) if side == "W" else K
        D = Vm[:, :d] if side == "W" else W0
        c = (cnt[s] if side == "W" else cnt[:, s]).astype(float)
        G = (D * c[:, None]).T @ D
        nobs = int((c > 0).sum())
        cond = float(np.linalg.cond(G)) if nobs >= d else np.inf
        systems.append(dict(d=d, D=D, c=c, G=G, nobs=nobs, cond=cond, exact=nobs >= d and cond < 1e8))
    full = [q for q in systems if q["exact"] and q["d"] == K]
    if K <= 6 and len(full) >= 2 ** K:                       # every support, each at least once
        masks = _all_supports(K)
        order = rs.permutation(len(full))
        for n, o in enumerate(order):
            full[o]["P"] = masks[n % len(masks)]
    else:
        for n, q in enumerate(full):
            q["P"] = np.zeros(K, bool) if n == 0 else np.ones(K, bool) if n == 1 else rs.uniform(size=K) < 0.5
    Yc = np.zeros((N, MT))
    for q_i, q in enumerate(systems):
        d, D = q["d"], q["D"]
        if q["exact"]:
            if "P" not in q:
                q["P"] = rs.uniform(size=d) < 0.6
            P = q["P"]
            q["x"] = np.where(P, rs.uniform(0.05, 2.0, size=d), 0.0)
            mu = np.where(P, 0.0, rs.uniform(0.05, 1.0, size=d))
            b = D @ (q["x"] - np.linalg.solve(q["G"], mu))
        else:
            x0 = np.zeros(d)
            x0[rs.choice(d, min(2, d), replace=False)] = rs.uniform(20.0, 40.0, size=min(2, d))
            b = D @ x0
        q["b"] = b
        if side == "W":
            Yc[q_i] = b
        else:
            Yc[:, q_i] = b
    off = np.where(obs, rs.normal(0.0, 0.1, size=obs.shape), 0.0)
    off -= np.where(obs, (off.sum(axis=2) / np.maximum(cnt, 1))[..., None], 0.0)
    Y = np.where(obs, Yc[..., None] + off, np.nan)
    return systems, Y


def _check_half(systems, X1, X0, Y, side):
    """The assertions of part 1 on the fitted factor X1 (X0: what was given); returns (worst error / bound of the device,
    the same for a float64 numpy solve of the same normal equations, number of systems with a constructed solution)."""
    S = np.nansum(Y, axis=2)
    worst = worst_np = 0.0
    nexact = 0
    for s, q in enumerate(systems):
        d, D, c = q["d"], q["D"], q["c"]
        x = X1[s, :d]
        assert np.isfinite(x).all(), (side, s)
        assert np.array_equal(X1[s, d:], X0[s, d:]), (side, s)                 # never fitted: the given bits
        if q["exact"]:
            nexact += 1
            P, xs = q["P"], q["x"]
            assert (x[~P] == FLOOR).all(), (side, s, x, xs)
            bound = 50 * q["cond"] * EPS * np.max(np.abs(xs))
            if P.any():
                err = float(np.max(np.abs(x[P] - xs[P])))
                h = D.T @ (S[s] if side == "W" else S[:, s])
                err_np = float(np.max(np.abs(np.linalg.solve(q["G"][np.ix_(P, P)], h[P]) - xs[P])))
                worst, worst_np = max(worst, err / bound), max(worst_np, err_np / bound)
                assert err <= bound, (side, s, err, bound, err_np)
        elif q["nobs"] == 0:
            assert (x == FLOOR).all(), (side, s, x)
        else:                                                # consistent data, optimal residual 0: compare the fit
            b = q["b"]
            reach = FLOOR * np.sum(np.sqrt(c @ D ** 2))
            norm_b = np.sqrt(c @ b ** 2)
            assert norm_b >= 1e3 * reach, (side, s, norm_b, reach)             # or the check below is vacuous
            res = np.sqrt(c @ (D @ x - b) ** 2)
            assert res <= reach + 1e-9 * norm_b, (side, s, res, reach)
    return worst, worst_np, nexact


@pytest.mark.parametrize("shape,K,miss", HALF_CASES, ids=["%dx%dx%dx%d-K%d-%s" % (s + (k, "missing" if m else "complete"))
                                                          for s, k, m in HALF_CASES])
def test_half_steps_reproduce_constructed_nnls_solutions(shape, K, miss):
    """One W half-step and one V half-step from given dense gamma factors on data whose NNLS solutions are constructed:
    entries on the support within 50 cond(G) eps max|x*| of x*, entries off it exactly 1e-3, entries past d and the
    other factor bit-identical to the input, rmse[0] within 1e-11 of numpy's residual norm of the returned factors.
    For K <= 6 every one of the 2^K supports appears wherever a half-step has that many full systems (rows at
    (130, 25, 41, 3) and (1025, 1, 3, 2), cells at (67, 5, 13, 2) and (130, 25, 41, 3)); above, and in the truncated rows,
    the supports are random and include the empty and the full one.
    Measured on an MI355X over all 70 cases: the worst entry lies at 0.084 of the bound on the W side and 0.114 on the
    V side (a float64 numpy solve of the same normal equations: 0.113 and 0.073), the rmse within 1.1e-12 relative (at
    (5, 1, 3, 1) nembeds 8, where the fit is exact up to the 1e-3 floor and the residual is all cancellation)."""
    N, M, T, R = shape
    MT = M * T
    rs = np.random.RandomState(1000 * K + N + (7 if miss else 0))
    W0 = rs.gamma(1.0, 1.0, size=(N, K)) + 0.05
    Vm = rs.gamma(1.0, 1.0, size=(MT, K)) + 0.05
    V0 = Vm.reshape(M, T, K)
    obs = _observed(N, MT, R, K, rs) if miss else np.ones((N, MT, R), dtype=bool)
    assert obs.all() != miss
    out = {}
    for side in ("W", "V"):
        systems, Y = _build_half(side, W0, Vm, obs, rs)
        for q in systems:                                    # the CPU-side conditions on the input
            if q["exact"]:
                assert q["nobs"] >= q["d"] and np.linalg.matrix_rank(q["G"]) == q["d"]
            if N >= 67 and (side == "V" or q["d"] <= MT):
                assert q["exact"], (side, q["d"], q["nobs"], q["cond"])
        full = [q for q in systems if q["exact"] and q["d"] == K]
        if K <= 6 and len(full) >= 2 ** K:
            assert len({tuple(q["P"]) for q in full}) == 2 ** K
        if len(full) >= 2:
            assert any(q["P"].all() for q in full) and any(not q["P"].any() for q in full)
        Y = Y.reshape(N, M, T, R)
        if R == 1:
            Y = Y[..., 0]                                    # the 3-D form: ssw = 0
        W1, V1, info = utils.tensor_nmf(Y, K, max_steps=1, W=W0, V=V0, fit_W=side == "W", fit_V=side == "V",
                                        return_info=True)
        assert info["steps"] == 1
        if side == "W":
            assert np.array_equal(V1, V0)
            worst = _check_half(systems, W1, W0, Y.reshape(N, MT, R), side)
        else:
            assert np.array_equal(W1, W0)
            worst = _check_half(systems, V1.reshape(MT, K), Vm, Y.reshape(N, MT, R), side)
        want = _rmse(Y, W1, V1)
        rel = abs(info["rmse"][0] - want) / want
        out[side] = worst + (rel,)
        assert rel <= 1e-11, (side, info["rmse"][0], want)
    print("half-steps", shape, "K", K, "missing" if miss else "complete",
          " ".join("%s: err/bound %.3g (numpy %.3g) over %d constructed systems, rmse rel %.2g" % ((k,) + v)
                   for k, v in out.items()))
    assert out["W"][2] > 0 and (out["V"][2] > 0 or N < K)


# ---------------------------------------------------------------------------------------------------------------- part 2
KINDS = ["duplicate", "zero_column", "negative", "zero", "few_rows", "no_rows", "scaled", "collinear"]
UNIQUE = ("negative", "zero", "scaled", "collinear")


def _brute_nnls(A, b):
    """The NNLS solution by enumeration: least squares on every support (lstsq on A itself, its columns scaled to unit
    length so that the badly scaled kind is solved as accurately as the others), the non-negative candidates, the
    smallest residual."""
    d = A.shape[1]
    norms = np.linalg.norm(A, axis=0)
    norms[norms == 0] = 1.0
    if not np.allclose(norms, 1.0):
        x, r = _brute_nnls(A / norms, b)
        return x / norms, r
    best, best_r = np.zeros(d), float(np.linalg.norm(b))
    for m in itertools.product([False, True], repeat=d):
        P = np.array(m, dtype=bool)
        if not P.any():
            continue
        xp = np.linalg.lstsq(A[:, P], b, rcond=None)[0]
        if (xp >= 0).all():
            x = np.zeros(d)
            x[P] = xp
            r = float(np.linalg.norm(A @ x - b))
            if r < best_r:
                best, best_r = x, r
    return best, best_r


@pytest.mark.parametrize("side", ["rows", "cells"])
@pytest.mark.parametrize("K", [2, 4, 7, 10])
@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_systems_match_a_brute_force_over_the_supports(kind, K, side):
    """(13, 3, 5, 2), one half-step per kind: no error, finite output, and for a handful of systems (truncated rows, full
    ones, the special one) the brute force's solution.  Where the solution is unique (negative and zero data: x = 0;
    badly scaled and nearly collinear columns) the comparison of part 1, against the brute force's x clipped at 1e-3;
    for the columns scaled over 1e-4 .. 1e4 in the equilibrated variables x_k |a_k| with the condition number of the
    unit-diagonal Gram, because cond(G) itself is about 1e16 there (its bound would be vacuous) while scaling columns
    changes neither the problem nor the relative error of a Cholesky solve.  Elsewhere the fit is unique but x is not:
    |A x - b| <= |A x_ref - b| + 1e-3 sum |a_k| + 1e-9 |b|, with the data scaled so that the optimal residual and fit are
    at least 1e3 times the middle term.  scipy's nnls is not used: on rank-deficient systems its fits were found
    20 - 46 % away from a better solution.
    Measured on an MI355X: unique solutions at most 0.073 of the bound (collinear, nembeds 4, rows); elsewhere the
    residual exceeds the brute force's by at most 0.64 of the floor's reach (a cell observed in 2 rows, nembeds 7) and
    by under 0.03 of it in every other kind."""
    N, M, T, R = 13, 3, 5, 2
    MT = M * T
    rs = np.random.RandomState(100 * K + KINDS.index(kind) + (50 if side == "cells" else 0))
    W0 = rs.gamma(1.0, 1.0, size=(N, K)) + 0.05
    Vm = rs.gamma(1.0, 1.0, size=(MT, K)) + 0.05
    F = Vm if side == "rows" else W0                         # the fixed factor: its columns are the design's
    if kind == "duplicate":
        F[:, 1] = 2.0 * F[:, 0]
    elif kind == "zero_column":
        F[:, min(1, K - 1)] = 0.0
    elif kind == "scaled":
        F *= 10.0 ** rs.permutation(np.linspace(-4.0, 4.0, K))
    elif kind == "collinear":
        F[:] = F[:, :1] * (1.0 + 1e-4 * rs.normal(size=F.shape))
    sc = 10.0 * K                                            # the data's scale: see the docstring's last condition
    mean = W0 @ Vm.T
    mean *= 6.0 / mean.mean()
    Y = sc * (mean[..., None] + rs.normal(size=(N, MT, R)))
    special = 11 if side == "rows" else 7                    # the system that few_rows / no_rows starve
    if kind == "negative":
        Y = -np.abs(Y) - 1.0
    elif kind == "zero":
        Y[:] = 0.0
    elif kind in ("few_rows", "no_rows"):
        sl = (special,) if side == "rows" else (slice(None), special)
        keep = np.zeros(MT if side == "rows" else N, dtype=bool)
        if kind == "few_rows":
            keep[[2, 9]] = True
            vals = Y[sl].copy()
            vals[2] = sc * (5.0 + rs.uniform(size=R))
            vals[9] = -sc * (5.0 + rs.uniform(size=R))
            Y[sl] = vals
        Y[sl] = np.where(keep[:, None], Y[sl], np.nan)
    W1, V1, info = utils.tensor_nmf(Y.reshape(N, M, T, R), K, max_steps=1, W=W0, V=Vm.reshape(M, T, K),
                                    fit_W=side == "rows", fit_V=side == "cells", return_info=True)
    assert info["steps"] == 1 and np.isfinite(W1).all() and np.isfinite(V1).all() and np.isfinite(info["rmse"]).all()
    X1 = W1 if side == "rows" else V1.reshape(MT, K)
    assert X1.min() >= FLOOR
    if side == "rows":
        assert np.array_equal(V1.reshape(MT, K), Vm)
        chosen = sorted({0, 1, K - 1, min(K, N - 1), N - 1, special})
    else:
        assert np.array_equal(W1, W0)
        chosen = sorted({0, 1, MT - 1, special})
    worst = {"x": 0.0, "fit": -np.inf}
    for s in chosen:
        d = min(K, s + 1) if side == "rows" else K
        y = (Y[s] if side == "rows" else Y[:, s]).ravel()
        ok = ~np.isnan(y)
        A = np.repeat(F[:, :d], R, axis=0)[ok]
        b = y[ok]
        x = X1[s, :d]
        if not ok.any():
            assert (x == FLOOR).all(), (s, x)                # no observation: the floor, no error
            continue
        xr, res_r = _brute_nnls(A, b)
        if kind in UNIQUE:
            G = A.T @ A
            if kind == "scaled":
                n = np.sqrt(np.diag(G))
                cond, scale = np.linalg.cond(G / np.outer(n, n)), n
            else:
                cond, scale = (np.linalg.cond(G) if xr.any() else 1.0), np.ones(d)
            want = np.maximum(xr, FLOOR)
            assert (x[xr <= FLOOR] == FLOOR).all(), (s, x, xr)
            bound = 50 * cond * EPS * np.max(np.abs(want * scale))
            err = float(np.max(np.abs((x - want) * scale)))
            worst["x"] = max(worst["x"], err / bound)
            assert err <= bound, (s, err, bound, x, want)
        else:
            norms = np.linalg.norm(A, axis=0)
            reach = FLOOR * norms.sum()
            assert res_r >= 1e3 * reach and np.linalg.norm(A @ xr) >= 1e3 * reach, (s, res_r, np.linalg.norm(A @ xr), reach)
            res = float(np.linalg.norm(A @ x - b))
            worst["fit"] = max(worst["fit"], (res - res_r) / reach)
            assert res <= res_r + reach + 1e-9 * np.linalg.norm(b), (s, res, res_r, reach)
    print("degenerate", kind, "K", K, side, "worst err/bound %.3g, worst (|A x - b| - |A x_ref - b|) / reach %.3g"
          % (worst["x"], worst["fit"]))


# ---------------------------------------------------------------------------------------------------------------- part 3
def _pav_sweep(W, V):
    """The sweep documented above nmf_pav_kernel, in numpy: passes over the pairs (t, t+1) left to right; a pair violates
    when w_i . v_t - w_i . v_{t+1} < 0 for any row; the two pools merge into (w0 v_t + w1 v_{t+1}) / (w0 + w1) and the
    sweep goes on from the merged pool's last member; passes repeat until one merges nothing.  Returns the projected
    V, the pools, the number of merges and the smallest |d0 - d1| between different pools over the largest |w . v|."""
    V = np.array(V, dtype=np.float64)
    T = V.shape[0]
    pool = np.arange(T)
    merges, margin, scale = 0, np.inf, 0.0
    while True:
        merged = False
        t = 0
        while t < T - 1:
            d0, d1 = W @ V[t], W @ V[t + 1]
            scale = max(scale, float(np.abs(d0).max()), float(np.abs(d1).max()))
            if pool[t] != pool[t + 1]:
                margin = min(margin, float(np.abs(d0 - d1).min()))
            if not ((d0 - d1) < 0).any():
                t += 1
                continue
            in0, in1 = pool == pool[t], pool == pool[t + 1]
            w0, w1 = int(in0.sum()), int(in1.sum())
            V[in0 | in1] = (w0 * V[t] + w1 * V[t + 1]) / (w0 + w1)
            pool[in1] = pool[t]
            merged = True
            merges += 1
            t += w1
        if not merged:
            break
    return V, pool, merges, (margin / scale if scale > 0 and np.isfinite(margin) else np.inf)


def _trend(N, T, K, seed, noise=0.25):
    """W >= 0 and a V whose curves decrease on the whole, with noise: pools of a few depths, not one block."""
    rs = np.random.RandomState(seed)
    W = rs.gamma(1.0, 1.0, size=(N, K)) + 0.05
    V = rs.uniform(0.5, 1.5, size=K) * (1.2 - np.linspace(0.0, 1.0, T))[:, None]
    V += noise * rs.uniform(-1, 1, size=(T, K)) / np.sqrt(K)
    return W, V


def _check_pav(W, V, got):
    ref, pool, merges, margin = _pav_sweep(W, V)
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert rel <= 1e-12, rel
    Mu = W @ got.T
    assert (np.diff(Mu, axis=1) <= 1e-12 * np.abs(Mu).max()).all()
    for p in np.unique(pool):
        mean = V[pool == p].mean(axis=0)
        assert np.max(np.abs(got[pool == p] - mean)) <= 1e-12 * np.max(np.abs(V)), p
    assert np.array_equal(utils.factor_pav(W, got), got)               # a projected column is a fixed point, bit for bit
    return rel, pool, merges, margin


PAV_SHAPES = [(1, 1, 1), (1, 2, 1), (257, 64, 7), (600, 257, 10), (3, 300, 2), (3, 780, 10)]


@pytest.mark.parametrize("N,T,K", PAV_SHAPES, ids=["%dx%dx%d" % s for s in PAV_SHAPES])
def test_factor_pav_at_block_stride_and_lds_edges(N, T, K):
    """factor_pav against the numpy sweep to 1e-12 where the kernel's tid-strided loops take more than one trip (more than
    256 rows, depths or pool entries) and at the largest column that fits 64 KB of LDS, (3, 780, 10); W @ P[t] does not
    increase, every pool is the mean of the input over it, and projecting twice changes no bit.  The inputs are a
    decreasing trend plus noise (random V pools to a single block under hundreds of rows) and are checked here to keep
    at least 4 pools after at least 4 merges, one pool of 3 or more depths, and every vote 1e-10 clear of a tie.
    Measured on an MI355X: at most 2.6e-16 relative from the numpy sweep (13 .. 80 pools after 51 .. 700 merges; the
    closest vote is 4.4e-9 of the largest curve value from a tie, at (600, 257, 10))."""
    W, V = _trend(N, T, K, seed=N + T + K)
    if T == 2:
        V = V[::-1].copy()                                   # one violation, one merge
    ref, pool, merges, margin = _pav_sweep(W, V)
    if T >= 64:
        sizes = np.bincount(pool)
        found = (len(np.unique(pool)), merges, int(sizes.max()), margin)
        assert found[0] >= 4 and merges >= 4 and sizes.max() >= 3 and margin > 1e-10, found
    Vin = V.copy()
    got = utils.factor_pav(W, V)
    assert np.array_equal(V, Vin) and got.shape == V.shape
    rel, pool, merges, margin = _check_pav(W, V, got)
    print("factor_pav", (N, T, K), "rel %.3g, %d pools after %d merges, margin %.3g" % (rel, len(np.unique(pool)), merges,
                                                                                          margin))


def test_factor_pav_of_a_batch_projects_each_column():
    N, M, T, K = 40, 3, 50, 4
    W, _ = _trend(N, T, K, seed=1)
    V = np.stack([_trend(N, T, K, seed=10 + j, noise=0.2 + 0.2 * j)[1] for j in range(M)])
    got = utils.factor_pav(W, V)
    assert got.shape == (M, T, K)
    for j in range(M):
        rel, pool, merges, margin = _check_pav(W, V[j], got[j])
        assert merges >= 4 and margin > 1e-10
        assert np.array_equal(utils.factor_pav(W, V[j]), got[j])       # alone or in a batch: the same bits


def test_factor_pav_of_one_row_is_isotonic_regression():
    """N = K = 1, W = 1: the classic non-increasing isotonic regression (pool adjacent violators with a stack of block
    means), unique, so the order of the merges does not matter."""
    rs = np.random.RandomState(3)
    for T in (2, 17, 300):
        v = np.linspace(1.0, 0.0, T) + 0.3 * rs.normal(size=T)
        blocks = []                                          # [sum, count]
        for y in v:
            blocks.append([y, 1])
            while len(blocks) > 1 and blocks[-2][0] / blocks[-2][1] < blocks[-1][0] / blocks[-1][1]:
                s, n = blocks.pop()
                blocks[-1][0] += s
                blocks[-1][1] += n
        want = np.concatenate([np.full(n, s / n) for s, n in blocks])
        got = utils.factor_pav(np.ones((1, 1)), v[:, None])[:, 0]
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), T
        assert (np.diff(got) <= 0).all()


def test_factor_pav_of_an_increasing_column_cascades_into_one_pool():
    """(3, 780, 10), every embedding increasing: 779 merges in one pass, each with the pool grown so far.  Measured on
    an MI355X: 3.3e-15 relative from the numpy sweep."""
    N, T, K = 3, 780, 10
    rs = np.random.RandomState(5)
    W = rs.gamma(1.0, 1.0, size=(N, K)) + 0.05
    V = np.cumsum(rs.uniform(0.5, 1.5, size=(T, K)), axis=0)
    ref, pool, merges, margin = _pav_sweep(W, V)
    assert merges == T - 1 and len(np.unique(pool)) == 1 and margin > 1e-10
    got = utils.factor_pav(W, V)
    rel, _, _, _ = _check_pav(W, V, got)
    assert np.max(np.abs(got - V.mean(axis=0))) <= 1e-12 * np.abs(V).max()
    print("factor_pav increasing (3, 780, 10): rel %.3g" % rel)


def test_one_depth_more_than_fits_is_refused():
    """T = 781 at nembeds 10 needs 65604 bytes of LDS: BTF_EINVAL from factor_pav and from tensor_nmf(monotone=True)."""
    with pytest.raises(_native.BTFError) as e:
        utils.factor_pav(np.ones((2, 10)), np.ones((781, 10)))
    assert e.value.code == _native.BTF_EINVAL
    with pytest.raises(_native.BTFError) as e:
        utils.tensor_nmf(np.ones((2, 1, 781)), 10, max_steps=1, monotone=True, W=np.ones((2, 10)), V=np.ones((1, 781, 10)))
    assert e.value.code == _native.BTF_EINVAL
    W, V = utils.tensor_nmf(np.ones((2, 1, 781)), 10, max_steps=1, W=np.ones((2, 10)), V=np.ones((1, 781, 10)))
    assert np.isfinite(W).all() and np.isfinite(V).all()     # without the projection the depth is fine


def test_monotone_run_at_nembeds_8_leaves_every_column_a_fixed_point_of_factor_pav():
    N, M, T, R, K = 30, 3, 12, 2, 8
    rs = np.random.RandomState(8)
    Wt = rs.gamma(2.0, 0.5, size=(N, K))
    Vt = -np.sort(-rs.gamma(2.0, 0.5, size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", Wt, Vt)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))
    np.random.seed(2)
    W, V, info = utils.tensor_nmf(Y, K, max_steps=3, monotone=True, tol=-1.0, return_info=True)
    assert info["steps"] == 3
    Mu = np.einsum("nk,mtk->nmt", W, V)
    assert (np.diff(Mu, axis=2) <= 1e-12 * np.abs(Mu).max()).all()
    for j in range(M):
        assert np.array_equal(utils.factor_pav(W, V[j]), V[j]), j
    assert np.array_equal(utils.factor_pav(W, V), V)
    assert abs(info["rmse"][-1] - _rmse(Y, W, V)) <= 1e-11 * _rmse(Y, W, V)


# ---------------------------------------------------------------------------------------------------------------- part 4
HI = 0.999


def _bounded_case(K, miss, side):
    """(20, 4, 9, 2) with data in [0, 1.2]: the first seed whose half-step has at least 5 systems whose clipped NNLS
    solution overshoots max_entry, none of them within 1e-6 of it.  Returns the inputs and, per system, (d, design,
    counts, G, h, clipped NNLS solution, overshoot)."""
    N, M, T, R = 20, 4, 9, 2
    MT = M * T
    for seed in range(50):
        rs = np.random.RandomState(10000 + 100 * K + 10 * seed + (1 if miss else 0) + (2 if side == "V" else 0))
        Wt = rs.dirichlet(0.5 * np.ones(K), size=N)
        Vt = rs.uniform(0.05, 1.3, size=(MT, K))
        Y = np.clip((Wt @ Vt.T)[..., None] + rs.normal(0, 0.08, size=(N, MT, R)), 0.0, 1.2)
        if miss:
            Y[rs.uniform(size=(N, MT)) < 0.06] = np.nan
            Y[rs.uniform(size=Y.shape) < 0.06] = np.nan
        W0 = rs.dirichlet(0.5 * np.ones(K), size=N) + 0.02
        Vm = rs.uniform(0.05, 1.3, size=(MT, K))
        S, cnt = np.nansum(Y, axis=2), (~np.isnan(Y)).sum(axis=2).astype(float)
        systems = []
        for s in range(N if side == "W" else MT):
            d = min(K, s + 1) if side == "W" else K
            D = Vm[:, :d] if side == "W" else W0
            c = cnt[s] if side == "W" else cnt[:, s]
            y = (Y[s] if side == "W" else Y[:, s]).ravel()
            ok = ~np.isnan(y)
            x = np.maximum(nnls(np.repeat(D, R, axis=0)[ok], y[ok])[0], FLOOR)
            systems.append(dict(d=d, D=D, G=(D * c[:, None]).T @ D, h=D.T @ (S[s] if side == "W" else S[:, s]), x=x,
                                over=float((D @ x).max() - HI)))
        over = np.array([q["over"] for q in systems])
        conds = [np.linalg.cond(q["G"]) for q in systems]
        if (over > 1e-6).sum() >= 5 and not (np.abs(over) <= 1e-6).any() and max(conds) < 1e8:
            return Y.reshape(N, M, T, R), W0, Vm.reshape(M, T, K), systems
    raise AssertionError("no seed gives 5 projected systems")


@pytest.mark.parametrize("side", ["W", "V"])
@pytest.mark.parametrize("miss", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("K", [6, 7, 8, 9])
def test_max_entry_projection_satisfies_the_kkt_conditions(K, miss, side):
    """One bounded half-step per side at nembeds 6..9: exactly the systems whose clipped NNLS solution overshoots
    max_entry are projected (at least 5 of them), each projected x is feasible (1e-9 on the rows, 1e-12 on x >= 1e-6)
    and stationary: G x - h is a non-negative combination of the normals of the constraints with slack below 1e-9, up
    to 1e3 cond(G) eps |h|; the others carry the plain NNLS result, bit for bit.
    Measured on an MI355X: 5 .. 10 projected systems per half-step; the rows overshoot max_entry by at most 2.2e-16, x
    falls below 1e-6 by at most 1.5e-16, and the part of G x - h outside the cone of the active normals is at most
    1.1e-4 of the bound."""
    Y, W0, V0, systems = _bounded_case(K, miss, side)
    N, M, T, _ = Y.shape
    kw = dict(max_steps=1, W=W0, V=V0, fit_W=side == "W", fit_V=side == "V", return_info=True)
    Wb, Vb, info = utils.bounded_tensor_nmf(Y, K, max_entry=HI, **kw)
    Wp, Vp, _ = utils.tensor_nmf(Y, K, **kw)
    Xb, Xp = (Wb, Wp) if side == "W" else (Vb.reshape(M * T, K), Vp.reshape(M * T, K))
    flags = info["projected_rows"] if side == "W" else info["projected_cells"].ravel()
    want = np.array([q["over"] > 0 for q in systems])
    assert np.array_equal(flags, want), (np.flatnonzero(flags), np.flatnonzero(want))
    assert int(info["projected"][0]) == int(want.sum()) >= 5
    assert not (info["projected_cells"] if side == "W" else info["projected_rows"]).any()
    worst = {"upper": -np.inf, "lower": -np.inf, "xmin": -np.inf, "stationarity / bound": 0.0}
    for s, q in enumerate(systems):
        d, D, G, h = q["d"], q["D"], q["G"], q["h"]
        x = Xb[s, :d]
        assert np.array_equal(Xb[s, d:], (W0 if side == "W" else V0.reshape(-1, K))[s, d:])
        if not want[s]:
            assert np.array_equal(Xb[s], Xp[s]), s
            assert np.allclose(x, q["x"], rtol=1e-9, atol=1e-12), (s, x, q["x"])
            continue
        cx = D @ x
        worst["upper"] = max(worst["upper"], float(cx.max() - HI))
        worst["lower"] = max(worst["lower"], float(-cx.min()))
        worst["xmin"] = max(worst["xmin"], float(XMIN - x.min()))
        assert cx.max() <= HI + 1e-9 and cx.min() >= -1e-9 and x.min() >= XMIN - 1e-12, (s, cx.max(), cx.min(), x.min())
        normals = [-D[q_] for q_ in np.flatnonzero(HI - cx < 1e-9)] + [D[q_] for q_ in np.flatnonzero(cx < 1e-9)] + \
                  [np.eye(d)[k] for k in np.flatnonzero(x - XMIN < 1e-9)]
        assert normals, s                                    # projected, so the unconstrained minimiser was cut off
        g = G @ x - h
        left = nnls(np.array(normals).T, g)[1]
        bound = 1e3 * np.linalg.cond(G) * EPS * np.linalg.norm(h)
        worst["stationarity / bound"] = max(worst["stationarity / bound"], left / bound)
        assert left <= bound, (s, left, bound, len(normals))
    print("projection K", K, "missing" if miss else "complete", side, "projected", int(want.sum()), worst)
