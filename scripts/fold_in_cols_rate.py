"""Measurements behind fold_in_cols; appends JSON lines to profiles/r23_fold_in_cols_rate.jsonl.

    python scripts/fold_in_cols_rate.py --step sweeps   (no GPU) the chain's mixing from functionalmf_amd.fold_in_cols.chain
                                                        alone, numpy's generator: the largest standardised difference of
                                                        the curve means W v between 1, 2, ..., 64 sweeps and 256 sweeps
                                                        over replicate chains, at a dose-response-like shape (N = 60 rows
                                                        with a third observed, T = 9, K = 5, tf_order 2) and a C3-like one
                                                        (T = 64): what DEFAULT_SWEEPS is chosen from
    python scripts/fold_in_cols_rate.py --step golden   (no GPU) the numpy reference of test 5 (tests/golden/)
    python scripts/fold_in_cols_rate.py                 every GPU step below, each in a child process under its own time limit
    python scripts/fold_in_cols_rate.py --step zscore   device generator against numpy's (tests/test_gpu_fold_in_cols.py, test 5)
    python scripts/fold_in_cols_rate.py --step binomial Binomial bias against the one-column model's own chain (test 6), S = 16384
    python scripts/fold_in_cols_rate.py --step margin   fold-in RMSE / in-chain RMSE over 5 data seeds (test 7's set-up)
    python scripts/fold_in_cols_rate.py --step time     fold_in_cols on S = 1000 device-collected samples, host wall clock, min
                                                        of 3: C = 8 and C = 64 at C3 (512,256,64), K = 5, and C = 8 at a
                                                        dose-response shape (1024,256,9), K = 5 - against the loop a user
                                                        could write before: per kept sample a one-column model given
                                                        W_true = W_s and the kept scalars runs DEFAULT_SWEEPS rounds of
                                                        _resample_V + _resample_Tau2 (timed on 25 samples and scaled)
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
OUT = os.path.join(ROOT, "profiles", "r23_fold_in_cols_rate.jsonl")
STEPS = (("zscore", 300), ("binomial", 420), ("margin", 420), ("time", 540))
SWEEP_GRID = (1, 2, 4, 8, 16, 32, 64)
LONG = 256                     # --long N: the reference length; the grid then runs on in powers of two up to N / 2


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def test_module():
    sys.path.insert(0, os.path.join(ROOT, "tests"))           # (its conftest)
    spec = importlib.util.spec_from_file_location("test_gpu_fold_in_cols", os.path.join(ROOT, "tests", "test_gpu_fold_in_cols.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mixing_problem(T, N=60, K=5, seed=0):
    """N rows, a third of them observed (all depths), smooth curves plus noise; one kept state (W, nu2, lam2)."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    v = 0.3 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = W.dot(v.T) + rs.normal(0, 0.5, size=(N, T))
    Y[rs.permutation(N)[N // 3:]] = np.nan
    return W, Y, 0.25, 0.1


def step_sweeps(replicates=200, only=None, LONG=LONG):
    from functionalmf_amd import fold_in_cols as fc
    SWEEP_GRID = tuple(2 ** k for k in range(20) if 2 ** k <= max(64, LONG // 2))
    for name, T in (("dose-response-like", 9), ("C3-like", 64)):
        if only and only != name:
            continue
        W, Y, nu2, lam2 = mixing_problem(T)
        K = W.shape[1]
        keep = {s: np.zeros((replicates,) + Y.shape) for s in SWEEP_GRID + (LONG,)}
        rng = np.random.default_rng(2025)
        for rep in range(replicates):
            draws = fc.random_draws(rng, T, K, 2, LONG)

            def on_sweep(r, v, rep=rep):
                if r + 1 in keep:
                    keep[r + 1][rep] = W.dot(v.T)
            fc.chain(Y, W, nu2, lam2, 2, LONG, draws, on_sweep=on_sweep)
        ref = keep[LONG]
        for s in SWEEP_GRID:
            d = keep[s].mean(axis=0) - ref.mean(axis=0)
            se = np.sqrt((keep[s].var(axis=0, ddof=1) + ref.var(axis=0, ddof=1)) / replicates)
            emit(step="sweeps", problem=name, shape=[Y.shape[0], T], nembeds=K, tf_order=2, replicates=replicates, sweeps=s,
                 against=LONG, max_abs_z=float(np.abs(d / se).max()), rms_z=float(np.sqrt(np.mean((d / se) ** 2))),
                 max_abs_diff=float(np.abs(d).max()))


def step_golden():
    """(no GPU) the numpy reference of test 5: tests/golden/fold_in_cols_numpy_replicates.npz."""
    from functionalmf_amd import fold_in_cols as fc
    t = test_module()
    W, Y, nu2, lam2 = t.z_problem()
    a = t.numpy_replicates(W, Y, nu2, lam2, t.Z_SAMPLES, t.Z_SEEDS[0])
    b = t.numpy_replicates(W, Y, nu2, lam2, t.Z_SAMPLES, t.Z_SEEDS[1])
    z = t.two_sample_z(b, a)
    np.savez(os.path.join(ROOT, "tests", "golden", "fold_in_cols_numpy_replicates.npz"), mean=a.mean(axis=0), var=a.var(axis=0, ddof=1),
             first=a[:8], nsamples=t.Z_SAMPLES, sweeps=fc.DEFAULT_SWEEPS, seed=t.Z_SEEDS[0], z_numpy_vs_numpy=z)
    emit(step="golden", nsamples=t.Z_SAMPLES, sweeps=fc.DEFAULT_SWEEPS, max_abs_z_numpy_vs_numpy=z)


def step_zscore():
    t = test_module()
    z, zref = t.device_generator_z()
    emit(step="zscore", nsamples=t.Z_SAMPLES, max_abs_z_device_vs_numpy=z, max_abs_z_numpy_vs_numpy=zref)


def step_binomial(S=16384):
    t = test_module()
    for sweeps in (None,):
        diff, se = t.binomial_bias(S, sweeps)
        emit(step="binomial", nsamples=S, sweeps=sweeps, max_abs_diff=diff, oracle_mcse=se)


def step_margin():
    t = test_module()
    for seed in range(5):
        fold, chain, zero = t.fold_vs_chain(seed)
        emit(step="margin", data_seed=seed, rmse_fold_in=fold, rmse_in_chain=chain, rmse_predict_zero=zero, ratio=fold / chain)


def timing_case(name, N, M, T, K, S, C, repeats=3, loop_samples=25):
    from functionalmf_amd import fold_in_cols as fc
    from functionalmf_amd.factor import GaussianBayesianTensorFiltering
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M + C, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.5, size=(N, M + C, T))
    Y_new = np.ascontiguousarray(Y[:, M:].transpose(1, 0, 2))
    Y_new[:, rs.permutation(N)[N // 3:]] = np.nan                      # a third of the rows tested on the new columns
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(np.ascontiguousarray(Y[:, :M]), nburn=20, nsamples=S, verbose=False)
    model.fold_in_cols(Y_new, seed=1)                                  # warm-up: code objects, allocations
    t_fold, t_draw = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.fold_in_cols(Y_new, seed=1)
        t_fold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        model.fold_in_cols(Y_new, seed=1, summary=False)
        t_draw.append(time.perf_counter() - t0)
    # what a user could do before: a one-column model per new column with W fixed at the kept sample's
    np.random.seed(2)
    Yc = np.ascontiguousarray(Y_new[0][:, None, :])
    t0 = time.perf_counter()
    for s in range(loop_samples):
        np.random.seed(s)
        small = GaussianBayesianTensorFiltering(N, 1, T, nembeds=K, W_true=res["W"][s], nu2_true=float(res["nu2"][s, 0]),
                                                lam2_true=float(res["lam2"][s, 0]), sigma2_true=float(res["sigma2"][s, 0]))
        for _ in range(fc.DEFAULT_SWEEPS):
            small._resample_V(Yc)
            small._resample_Tau2()
        small.V
    loop = (time.perf_counter() - t0) / loop_samples * S * C
    emit(step="time", case=name, shape=[N, M, T], nembeds=K, nsamples=S, ncols_new=C, sweeps=fc.DEFAULT_SWEEPS, repeats=repeats,
         fold_in_cols_seconds_min=min(t_fold), fold_in_cols_chains_only_seconds_min=min(t_draw),
         loop_seconds_scaled_from=loop_samples, loop_seconds=loop, speedup=loop / min(t_fold), kernel_trace=False)


def step_time():
    timing_case("dose-response (1024,256,9) C=8", 1024, 256, 9, 5, 1000, 8)
    timing_case("C3 (512,256,64) C=8", 512, 256, 64, 5, 1000, 8)
    timing_case("C3 (512,256,64) C=64", 512, 256, 64, 5, 1000, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["sweeps", "golden"])
    ap.add_argument("--problem", default=None)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--long", type=int, default=LONG)
    a = ap.parse_args()
    if a.step is None:                     # every step in a child of its own, under its own time limit; stop at the first failure
        for step, limit in STEPS:
            rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step])
            if rc != 0:
                sys.exit("step %s ended with status %d: nothing more is started on the GPU" % (step, rc))
        return
    if a.step == "sweeps":
        return step_sweeps(a.replicates, a.problem, a.long)
    if a.step == "golden":
        return step_golden()
    {"zscore": step_zscore, "binomial": step_binomial, "margin": step_margin, "time": step_time}[a.step]()


if __name__ == "__main__":
    main()
