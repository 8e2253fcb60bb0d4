"""Measurements behind slice_fold_in_depth; appends JSON lines to profiles/r27_slice_fold_in_depth_rate.jsonl.

    python scripts/slice_fold_in_depth_rate.py --step sweeps  (no GPU) the chain's mixing from
                                                  functionalmf_amd.slice_fold_in_depth.chain alone, numpy's generator, the
                                                  default fit: the largest standardised difference of the curve means W v
                                                  between 8, 16, ..., 1024 sweeps and a chain eight times longer than the
                                                  largest count, over replicate chains, at a flu-like Poisson slice (identity
                                                  link under positivity, N = 50 rows with a third observed, T = 40 kept
                                                  weeks, H = 8, K = 10, tf_order 2) and a dose-response-like gamma-grid
                                                  slice (N = 60, T = 9 kept doses, H = 2, K = 5, the fit.py constraints on the
                                                  extended grid): what DEFAULT_SWEEPS is chosen from
    python scripts/slice_fold_in_depth_rate.py --step rate    slice_fold_in_depth on S = 500 uploaded samples, K = 5, default
                                                  sweeps, host wall clock with all transfers and the summary, min of 3:
                                                  politics-like (19,19,228), Poisson identity with positivity, H = 8;
                                                  dose-response (1024,256,9), gamma grid, H = 2; C3 (512,256,64), Poisson
                                                  identity with 127 constraints, H = 8 - against the numpy definition per
                                                  chain (timed on a few chains, scaled to S * M: EXTRAPOLATED), against
                                                  slice_fold_in_cols per chain and sweep at the same shape in the same run,
                                                  and the share of the feasibility pass (the call without constraints)
                                                  (--samples S: another number of kept samples, recorded as nsamples)
    python scripts/slice_fold_in_depth_rate.py --step margin  RMSE of the fold-in's mean against the truth at the new depths
                                                  over the RMSE of a model fitted on all T + H depths, 5 data seeds
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r27_slice_fold_in_depth_rate.jsonl")
GRID = (8, 16, 32, 64, 128, 256, 512, 1024)
LONG = 8 * GRID[-1]


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def fit_constraints(T, at_most_one=False):
    """Positivity, (at most one,) monotone decreasing with slack 1e-2: the rows of doseresponse/fit.py:58-61."""
    C_zero = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(T - i - 2), [-1e-2]]) for i in range(T - 1)])
    C_one = np.concatenate([np.eye(T) * -1, np.full((T, 1), -1)], axis=1)
    return np.concatenate([C_zero, C_one, C_mono] if at_most_one else [C_zero, C_mono], axis=0)


def gamma_grid(G, rs):
    """(shape, scale, prob) of a gamma grid with G components."""
    return np.linspace(2.0, 6.0, G), rs.gamma(2.0, 0.5, size=G) / 10.0, np.full(G, 1.0 / G)


def mixing_problem(name, seed=0):
    """(family, param, W, V_old, Y (N,H,nreps), lam2, Constraints on the extended grid, tf_order): one kept state, a third
    of the rows observed at every new depth."""
    rs = np.random.RandomState(seed)
    if name == "flu-like":
        N, T, H, K = 50, 40, 8, 10
        W = rs.uniform(0.5, 1.5, size=(N, K)) / K
        season = 6.0 + 4.0 * np.sin(np.arange(T + H) / 6.0)
        v = season[:, None] * rs.uniform(0.6, 1.4, size=(1, K)) * np.exp(0.05 * np.cumsum(rs.normal(size=(T + H, K)), axis=0))
        Y = rs.poisson(W.dot(v[T:].T)).astype(float)[..., None]
        family, param = "poisson_identity", None
        Cons = np.concatenate([np.eye(T + H), np.zeros((T + H, 1))], axis=1)
    else:
        N, T, H, K = 60, 9, 2, 5
        W = rs.uniform(0.5, 1.5, size=(N, K)) / K
        v = rs.uniform(0.5, 1.0, size=(1, K)) * np.linspace(1.0, 0.25, T + H)[:, None]
        family, param = "gamma_grid", gamma_grid(6, rs)
        a, s, p = param
        eta = W.dot(v[T:].T)
        g = rs.choice(a.size, size=eta.shape + (2,), p=p)
        Y = rs.gamma(a[g], s[g] * eta[..., None])
        Cons = fit_constraints(T + H, True)
    Y[rs.permutation(N)[N // 3:]] = np.nan
    return family, param, W, v[:T], Y, 0.1, Cons, 2


def _replicates(args):
    name, seeds = args
    from functionalmf_amd import slice_fold_in as sf, slice_fold_in_cols as sc, slice_fold_in_depth as sd
    family, param, W, V_old, Y, lam2, Cons, tf = mixing_problem(name)
    N, H = Y.shape[:2]
    p = sf.check_param(family, param)
    _, S1, cnt, L = sf.row_statistics(Y[None], family, N, H)
    a, b = sc.fit_weights(sc.gaussian_fit(Y[None], family, p), 1, N, H)
    stats = (S1[0], cnt[0], None if L is None else L[0])
    red = sd.reduce_constraints(Cons, V_old.shape[0], H)
    keep = {s: [] for s in GRID + (LONG,)}
    rounds = unf = 0
    for seed in seeds:
        def on_sweep(r, v):
            if r + 1 in keep:
                keep[r + 1].append(W.dot(v.T))
        o = sd.chain(V_old, W, lam2, tf, family, p, stats, a[0], b[0], red, rng=np.random.default_rng(seed), sweeps=LONG,
                     track_cond=False, on_sweep=on_sweep)
        assert not o["failed"]
        rounds, unf = rounds + o["rounds"], unf + o["unfinished"]
    return {s: np.array(v) for s, v in keep.items()}, rounds, unf


def step_sweeps(replicates, only=None, workers=8):
    for name in ("flu-like", "dose-response-like"):
        if only and only != name:
            continue
        seeds = 2027 + np.arange(replicates)
        with ProcessPoolExecutor(workers) as pool:
            parts = list(pool.map(_replicates, [(name, [int(x) for x in seeds[w::workers]]) for w in range(workers)]))
        keep = {s: np.concatenate([p[0][s] for p in parts]) for s in GRID + (LONG,)}
        rounds, unf = sum(p[1] for p in parts), sum(p[2] for p in parts)
        ref = keep[LONG]
        family, _, W, V_old, Y, _, Cons, tf = mixing_problem(name)
        for s in GRID:
            d = keep[s].mean(axis=0) - ref.mean(axis=0)
            se = np.sqrt((keep[s].var(axis=0, ddof=1) + ref.var(axis=0, ddof=1)) / replicates)
            emit(step="sweeps", problem=name, family=family, shape=[W.shape[0], V_old.shape[0], Y.shape[1]], nembeds=W.shape[1],
                 tf_order=tf, constraints=int(Cons.shape[0]), replicates=replicates, sweeps=s, against=LONG,
                 max_abs_z=float(np.abs(d / se).max()), rms_z=float(np.sqrt(np.mean((d / se) ** 2))),
                 max_abs_diff_in_reference_sd=float(np.abs(d / ref.std(axis=0, ddof=1)).max()),
                 proposals_per_sweep=rounds / float(replicates * LONG), unfinished=int(unf))


# ---------------------------------------------------------------------------------------------------------------- GPU steps
def rate_problem(name, N, M, T, H, K, family, S, seed=0):
    """S kept states around positive factors with falling curves (feasible under positivity and the monotone rows), new
    slices with half the rows observed."""
    rs = np.random.RandomState(seed)
    W = rs.uniform(0.5, 1.5, size=(N, K)) / K
    V = rs.uniform(0.5, 1.0, size=(M, 1, K)) * np.linspace(1.0, 0.3, T + H)[None, :, None]
    if family == "poisson_identity":
        V *= 8.0
        param = None
        Y = rs.poisson(np.einsum("nk,mtk->nmt", W, V[:, T:])).astype(float)
    else:
        param = gamma_grid(50, rs)
        a, s, p = param
        eta = np.einsum("nk,mtk->nmt", W, V[:, T:])
        g = rs.choice(a.size, size=eta.shape, p=p)
        Y = rs.gamma(a[g], s[g] * eta)
    Y[rs.permutation(N)[N // 2:]] = np.nan
    Ws = W[None] * np.exp(0.02 * rs.normal(size=(S, N, K)))
    Vs = V[None, :, :T] * (1.0 + 0.02 * rs.uniform(-1, 1, size=(S, 1, 1, 1)))
    return Ws, np.ascontiguousarray(Vs), np.full(S, 0.1), Y, param


def rate_case(name, N, M, T, H, K, family, Cons, Cc, S=500, repeats=3, numpy_chains=2):
    from functionalmf_amd import slice_fold_in as sf, slice_fold_in_cols as sc, slice_fold_in_depth as sd, utils
    Ws, Vs, lam2, Y, param = rate_problem(name, N, M, T, H, K, family, S)
    kw = dict(lam2=lam2, likelihood_param=param, tf_order=2, seed=1)
    utils.slice_fold_in_depth(Y, Ws[:2], Vs[:2], family, Constraints=Cons, lam2=lam2[:2], likelihood_param=param, seed=1, sweeps=2)   # warm-up
    t_all, t_free, rounds = [], [], 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = utils.slice_fold_in_depth(Y, Ws, Vs, family, Constraints=Cons, **kw)
        t_all.append(time.perf_counter() - t0)
        print("%s: call %d of %d: %.3f s" % (name, len(t_all), repeats, t_all[-1]), file=sys.stderr, flush=True)
    t0 = time.perf_counter()                                           # (an observation: once)
    utils.slice_fold_in_depth(Y, Ws, Vs, family, Constraints=None, **kw)
    t_free.append(time.perf_counter() - t0)
    assert np.all(np.isfinite(out["V"]))
    print("%s: slice_fold_in_depth %.3f s, without constraints %.3f s" % (name, min(t_all), min(t_free)), file=sys.stderr, flush=True)
    # the host route: the numpy definition per chain, timed on a few chains and scaled to S * M
    p = sf.check_param(family, param)
    _, S1, cnt, L = sd.slice_statistics(Y, family, N, M)
    a, b = sc.fit_weights(sd.default_fit(Y, family, p, N, M), M, N, H)
    red = sd.reduce_constraints(Cons, T, H)
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    for c in range(numpy_chains):
        s, j = c % S, c % M
        sd.chain(Vs[s, j], Ws[s], lam2[s], 2, family, p, (S1[j], cnt[j], None if L is None else L[j]), a[j], b[j], red, rng=rng,
                 track_cond=False)
    host = (time.perf_counter() - t0) / numpy_chains * S * M
    # slice_fold_in_cols at the same shape in the same run: M of the fitted columns' first T depths as "new" columns
    Mc = min(M, 16)
    Yc = np.ascontiguousarray(np.repeat(Y[:, :Mc, :1], T, axis=2).transpose(1, 0, 2))
    per_cols = cols_rounds = refused = None
    try:                                                               # (an observation: once)
        t0 = time.perf_counter()
        oc = utils.slice_fold_in_cols(Yc, Ws, family, lam2=lam2, Vs=Vs, likelihood_param=param, Constraints=Cc, tf_order=2, seed=1,
                                      sweeps=sd.DEFAULT_SWEEPS, summary=False)
        per_cols = (time.perf_counter() - t0) / (S * Mc * sd.DEFAULT_SWEEPS)
        cols_rounds = float(oc["rounds"].mean()) / sd.DEFAULT_SWEEPS
    except (ValueError, RuntimeError) as e:                            # (a T K-wide band beyond the LDS limit, or the columns' default start refused)
        refused = str(e)
    per_depth = min(t_all) / (S * M * sd.DEFAULT_SWEEPS)
    emit(step="rate", case=name, family=family, shape=[N, M, T], horizon=H, nembeds=K, nsamples=S, chains=S * M, sweeps=sd.DEFAULT_SWEEPS,
         model_constraints=int(Cc.shape[0]), constraints_on_extended_grid=int(Cons.shape[0]), reduced_constraints=int(red[2].size), kept_depths_reached=int(red[3]),
         repeats=repeats, seconds_min=min(t_all), seconds_without_constraints_min=min(t_free),
         feasibility_share=1.0 - min(t_free) / min(t_all), proposals_per_sweep=float(out["rounds"].mean()) / sd.DEFAULT_SWEEPS,
         unfinished=int(out["unfinished"].sum()), numpy_seconds_extrapolated=host, numpy_chains_timed=numpy_chains,
         speedup_over_numpy_extrapolated=host / min(t_all), seconds_per_chain_and_sweep=per_depth,
         slice_fold_in_cols_seconds_per_chain_and_sweep=per_cols, slice_fold_in_cols_columns=Mc,
         slice_fold_in_cols_proposals_per_sweep=cols_rounds, slice_fold_in_cols_refused=refused, kernel_trace=False)


def step_rate(only=None, S=500):
    pos = lambda D: np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
    # (name, N, M, T, H, K, family, the model's constraints on the extended grid, the same on the T-point grid for the columns call)
    cases = (("politics-like (19,19,228) K=5 H=8", 19, 19, 228, 8, 5, "poisson_identity", pos(236), pos(228)),
             ("dose-response (1024,256,9) K=5 H=2", 1024, 256, 9, 2, 5, "gamma_grid", fit_constraints(11, True), fit_constraints(9, True)),
             ("C3 (512,256,64) K=5 H=8", 512, 256, 64, 8, 5, "poisson_identity", fit_constraints(72), fit_constraints(64)))
    for c in cases:
        if only is None or c[0].startswith(only):
            rate_case(*c, S=S)


def step_margin(sweeps=None):
    """RMSE of the fold-in's posterior mean at the new depths over that of a model fitted on all T + H depths."""
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering as Model
    N, M, T, H, K = 40, 12, 20, 4, 3
    for seed in range(5):
        rs = np.random.RandomState(seed)
        W = rs.uniform(0.5, 1.5, size=(N, K)) / K
        V = 8.0 * rs.uniform(0.5, 1.0, size=(M, 1, K)) * np.linspace(1.0, 0.3, T + H)[None, :, None]
        truth = np.einsum("nk,mtk->nmt", W, V)
        Y = rs.poisson(truth).astype(float)
        pos = lambda D: np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
        means = []
        for D in (T, T + H):
            np.random.seed(seed)
            m = Model(N, M, D, "poisson_identity", pos(D), nembeds=K, tf_order=2, W_init=W.copy(), V_init=V[:, :D].copy(), rng="device",
                      device_seed=seed + 1)
            res = m.run_gibbs(Y[:, :, :D], nburn=200, nsamples=200, verbose=False)
            if D == T:
                out = m.slice_fold_in_depth(Y[:, :, T:], results=res, Constraints=pos(T + H), seed=seed + 11, sweeps=sweeps)
                means.append(out["mean"])
            else:
                means.append(np.einsum("snk,smtk->nmt", res["W"], res["V"][:, :, T:]) / res["W"].shape[0])
        rf, rc = (float(np.sqrt(np.mean((mu - truth[:, :, T:]) ** 2))) for mu in means)
        emit(step="margin", data_seed=seed, shape=[N, M, T], horizon=H, nembeds=K, rmse_fold_in=rf, rmse_in_chain=rc, ratio=rf / rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["sweeps", "rate", "margin"], required=True)
    ap.add_argument("--problem", default=None)
    ap.add_argument("--replicates", type=int, default=128)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--samples", type=int, default=500, help="kept samples of the rate step (500: what the records report; the "
                    "dose-response shape at 1024 sweeps takes minutes per call there, a smaller S is labelled in its record)")
    a = ap.parse_args()
    if a.step == "sweeps":
        return step_sweeps(a.replicates, a.problem, a.workers)
    if a.step == "rate":
        return step_rate(a.problem, a.samples)
    step_margin()


if __name__ == "__main__":
    main()
