"""Measurements behind slice_fold_in_cols; appends JSON lines to profiles/r24_slice_fold_in_cols_rate.jsonl.

    python scripts/slice_fold_in_cols_rate.py                 every step below, each in a child process under its own time limit
    python scripts/slice_fold_in_cols_rate.py --step sweeps   what DEFAULT_SWEEPS is chosen from, with the default fit and the
                                                              device generator (the kernel replays the numpy definition draw for
                                                              draw: tests/test_gpu_slice_fold_in_cols.py, test 1): the largest
                                                              standardised difference of the curve means at 32 ... 2048 sweeps
                                                              - z_problem (N = 12, T = 6, K = 2, Gaussian) against the stored
                                                              moments of the exact Gibbs chain, S = 16384 chains, and a
                                                              dose-response-like shape (N = 60 rows with a third observed,
                                                              T = 9, K = 5, 26 constraints, gamma grid) against a 4096-sweep
                                                              run, S = 4096 chains each
    python scripts/slice_fold_in_cols_rate.py --step margin   fold-in RMSE / in-chain RMSE over 5 data seeds (test 7's set-up)
    python scripts/slice_fold_in_cols_rate.py --step time     slice_fold_in_cols with uploaded results, host wall clock with all
                                                              transfers and the summary, min of 3: the dose-response shape
                                                              (1024,256,9), K = 5, G = 50, 26 constraints, S = 500, 30 rows
                                                              observed, C = 8 and C = 64; C3 (512,256,64) Poisson identity with
                                                              127 constraints, C = 8 - against the loop a user could write
                                                              before: per kept sample a C-column constrained model with W fixed
                                                              at W_s runs `sweeps` rounds of _resample_V + _resample_Tau2 (timed
                                                              on a few samples and scaled), and against one V step of a fitted
                                                              model of the shape in the same run
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r24_slice_fold_in_cols_rate.jsonl")
STEPS = (("sweeps", 300), ("margin", 420), ("time", 540))
SWEEP_GRID = (32, 64, 128, 256, 512, 1024, 2048)
LONG = 4096


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def test_module(name="test_gpu_slice_fold_in_cols"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))           # (its conftest)
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dose_like_problem(N=60, T=9, K=5, G=50, seed=0):
    """One kept state of a dose-response-like fit and one new column observed on a third of its rows: positive rows,
    falling curves below one, gamma-grid data, the 26 constraints of the dose-response application."""
    t = test_module("test_host_slice_fold_in")
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    v = np.zeros((T, K))
    v[-1] = rs.gamma(2.0, 0.2, size=K)
    for d in range(T - 2, -1, -1):
        v[d] = v[d + 1] + rs.gamma(1.0, 0.2, size=K) * (rs.rand() < 0.7)
    W *= 0.8 / W.dot(v.T).max()
    lik = t.gamma_table(G, rs)
    Y = t.draw_rows("gamma_grid", lik, W.dot(v.T)[None], 3, rs)
    Y[0, rs.permutation(N)[N // 3:]] = np.nan
    return W, v, Y, lik, t.fit_constraints(T, True)


def step_sweeps():
    from functionalmf_amd import slice_fold_in_cols as sc, utils
    t = test_module()
    W, Y, nu2, lam2 = t.z_problem()
    S = 16384
    for sweeps in SWEEP_GRID:
        out = utils.slice_fold_in_cols(Y[None], np.repeat(W[None], S, axis=0), "gaussian", lam2=np.full(S, lam2), likelihood_param=nu2,
                                       start=np.zeros((Y.shape[1], W.shape[1])), seed=12345, sweeps=sweeps, summary=False)
        V = out["V"][:, 0]
        g = t.z_against_gibbs.__globals__["load_golden"]("fold_in_cols_numpy_replicates.npz")
        emit(step="sweeps", problem="z_problem against the Gibbs moments", nsamples=S, sweeps=sweeps, largest_z=t.z_against_gibbs(V),
             sd_ratio_max=float(np.sqrt(V.var(axis=0, ddof=1) / g["var"]).max()),
             largest_mean_error_in_gibbs_sd=float(np.max(np.abs(V.mean(axis=0) - g["mean"]) / np.sqrt(g["var"]))),
             proposals_per_sweep=float(out["rounds"].mean() / sweeps), unfinished=int(out["unfinished"].sum()),
             default=sweeps == sc.DEFAULT_SWEEPS)
    W, v, Y, lik, Cons = dose_like_problem()
    S = 4096
    Ws = np.repeat(W[None], S, axis=0)
    kw = dict(lam2=np.full(S, 0.1), likelihood_param=lik, Constraints=Cons, start=0.9 * v, summary=False)
    curves = lambda out: np.einsum("nk,stk->snt", W, out["V"][:, 0])
    ref = curves(utils.slice_fold_in_cols(Y, Ws, "gamma_grid", seed=1, sweeps=LONG, **kw))
    for sweeps in SWEEP_GRID:
        out = utils.slice_fold_in_cols(Y, Ws, "gamma_grid", seed=2, sweeps=sweeps, **kw)
        c = curves(out)
        se = np.sqrt(c.var(axis=0, ddof=1) / S + ref.var(axis=0, ddof=1) / S)
        emit(step="sweeps", problem="dose-response-like against %d sweeps" % LONG, nsamples=S, sweeps=sweeps,
             largest_z=float(np.max(np.abs(c.mean(axis=0) - ref.mean(axis=0)) / se)),
             sd_ratio_max=float(np.sqrt(c.var(axis=0, ddof=1) / ref.var(axis=0, ddof=1)).max()),
             largest_mean_error_in_reference_sd=float(np.max(np.abs(c.mean(axis=0) - ref.mean(axis=0)) / ref.std(axis=0, ddof=1))),
             proposals_per_sweep=float(out["rounds"].mean() / sweeps), unfinished=int(out["unfinished"].sum()),
             default=sweeps == sc.DEFAULT_SWEEPS)


def step_margin():
    t = test_module()
    for seed in range(5):
        fold, chain, base = t.fold_vs_chain(seed)
        emit(step="margin", data_seed=seed, rmse_fold_in=fold, rmse_in_chain=chain, rmse_mean_curve=base, ratio=fold / chain)


def timing_case(name, family, N, M, T, K, S, C, nobs=30, repeats=3, loop_samples=2, G=50):
    from functionalmf_amd import slice_fold_in_cols as sc, utils
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    t = test_module("test_host_slice_fold_in")
    rs = np.random.RandomState(0)
    W = rs.gamma(2.0, 0.5, size=(N, K))
    V = np.zeros((M + C, T, K))
    V[:, -1] = rs.gamma(2.0, 0.2, size=(M + C, K))
    for d in range(T - 2, -1, -1):
        V[:, d] = V[:, d + 1] + rs.gamma(1.0, 0.2, size=(M + C, K)) * (rs.rand(M + C, 1) < 0.5)
    gg = family == "gamma_grid"
    W *= (0.6 if gg else 20.0) / np.einsum("nk,mtk->nmt", W, V).max()
    lik = t.gamma_table(G, rs) if gg else None
    Cons = t.fit_constraints(T, gg)
    Ws = W[None] * np.exp(0.05 * rs.normal(size=(S, N, K)))
    Vs = V[None, :M] * (1.0 + 0.05 * rs.uniform(-1, 1, size=(S, 1, 1, 1)))
    Y_new = t.draw_rows(family, lik, np.einsum("nk,ctk->cnt", W, V[M:]), 3, rs)
    Y_new[:, np.setdiff1d(np.arange(N), rs.choice(N, size=nobs, replace=False))] = np.nan
    kw = dict(lam2=np.full(S, 0.1), Vs=Vs, likelihood_param=lik, Constraints=Cons, seed=1)
    utils.slice_fold_in_cols(Y_new, Ws, family, **kw)                  # warm-up: code objects, allocations
    t_fold, t_draw = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = utils.slice_fold_in_cols(Y_new, Ws, family, **kw)
        t_fold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        utils.slice_fold_in_cols(Y_new, Ws, family, summary=False, **kw)
        t_draw.append(time.perf_counter() - t0)
    # what a user could do before: a C-column constrained model per kept sample with W fixed at the sample's
    Yc = np.ascontiguousarray(Y_new.transpose(1, 0, 2, 3))
    t0 = time.perf_counter()
    for s in range(loop_samples):
        np.random.seed(s)
        small = ConstrainedNonconjugateBayesianTensorFiltering(N, C, T, family, Cons, likelihood_param=lik, nembeds=K, tf_order=2,
                                                               W_true=Ws[s], V_init=np.repeat(Vs[s].mean(axis=0)[None], C, axis=0),
                                                               lam2_true=0.1, sigma2_true=1.0, rng="device")
        small._bind_data(Yc)
        for _ in range(sc.DEFAULT_SWEEPS):
            small._resample_V(Yc)
            small._resample_Tau2()
        small.V
    loop = (time.perf_counter() - t0) / loop_samples * S
    # one V step of a fitted model of the shape, in the same run
    np.random.seed(9)
    Yfit = t.draw_rows(family, lik, np.einsum("nk,mtk->nmt", W, V[:M]), 1, rs)
    big = ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, family, Cons, likelihood_param=lik, nembeds=K, tf_order=2,
                                                         W_init=W.copy(), V_init=V[:M].copy(), rng="device")
    big._bind_data(Yfit)
    big._resample_V(Yfit)
    big.V
    t0 = time.perf_counter()
    for _ in range(3):
        big._resample_V(Yfit)
    big.V
    v_step = (time.perf_counter() - t0) / 3
    emit(step="time", case=name, family=family, shape=[N, M, T], nembeds=K, nsamples=S, ncols_new=C, rows_observed=nobs,
         ncons=int(Cons.shape[0]), sweeps=sc.DEFAULT_SWEEPS, repeats=repeats, lds_bytes=sc.lds_bytes(T, K, 2),
         slice_fold_in_cols_seconds_min=min(t_fold), chains_only_seconds_min=min(t_draw),
         proposals_per_sweep=float(out["rounds"].mean() / sc.DEFAULT_SWEEPS), unfinished=int(out["unfinished"].sum()),
         loop_seconds_scaled_from=loop_samples, loop_seconds=loop, speedup=loop / min(t_fold), v_step_seconds=v_step,
         v_steps_per_call=min(t_fold) / v_step, kernel_trace=False)


def step_time():
    timing_case("dose-response (1024,256,9) C=8", "gamma_grid", 1024, 256, 9, 5, 500, 8)
    timing_case("dose-response (1024,256,9) C=64", "gamma_grid", 1024, 256, 9, 5, 500, 64)
    timing_case("C3 (512,256,64) C=8", "poisson_identity", 512, 256, 64, 5, 500, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step is None:                     # every step in a child of its own, under its own time limit; stop at the first failure
        for step, limit in STEPS:
            rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step])
            if rc != 0:
                sys.exit("step %s ended with status %d: nothing more is started on the GPU" % (step, rc))
        return
    {"sweeps": step_sweeps, "margin": step_margin, "time": step_time}[a.step]()


if __name__ == "__main__":
    main()
