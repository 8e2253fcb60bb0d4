"""Measurements behind fold_in_rows (one run on the GPU); appends JSON lines to profiles/r13_fold_in_rate.jsonl.

    python scripts/fold_in_rate.py                 every step below, each in a child process under its own time limit
    python scripts/fold_in_rate.py --step sweeps   Binomial inner_sweeps: z-scores of the mean against the quadrature posterior
                                                   (the set-up of tests/test_gpu_fold_in.py, test 6) for 1..32 rounds, S = 65536
    python scripts/fold_in_rate.py --step margin   fold-in RMSE / in-chain RMSE over 5 data seeds (test 7's set-up)
    python scripts/fold_in_rate.py --step time     fold_in_rows against what a user could do before: an R-row model bound to
                                                   Y_new and, per kept sample, V = V_s, nu2, sigma2, _resample_W() (uploads
                                                   included), at C3 (S = 1000, R = 64, K = 5, half the columns observed,
                                                   device-collected) and at the flu shape (50,1,370), R = 8
    python scripts/fold_in_rate.py --step once     one C3 call, untimed (for a kernel trace)
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
OUT = os.path.join(ROOT, "profiles", "r13_fold_in_rate.jsonl")
STEPS = (("sweeps", 420), ("margin", 420), ("time", 540))


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_fold_in", os.path.join(ROOT, "tests", "test_gpu_fold_in.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def step_sweeps(S=65536):
    from functionalmf_amd import utils
    t = test_module()
    V, sigma2, Y, N = t.binomial_problem()
    m, C = t.quadrature_posterior(V, sigma2, Y, N)
    Vs, s2 = np.repeat(V[None], S, axis=0), np.full(S, sigma2)
    se = np.sqrt(np.diag(C) / S)
    for n in (1, 2, 4, 8, 16, 32):
        W = utils.fold_in_rows((Y, N), Vs, "binomial", sigma2=s2, seed=2024, summary=False, inner_sweeps=n)["W"][:, 0]
        d = W.mean(axis=0) - m
        emit(step="sweeps", inner_sweeps=n, nsamples=S, posterior_mean=m.tolist(), diff=d.tolist(), z=(d / se).tolist(),
             max_abs_z=float(np.abs(d / se).max()), max_abs_diff=float(np.abs(d).max()),
             cov_max_abs_diff=float(np.abs(np.cov(W.T) - C).max()))


def step_margin():
    t = test_module()
    for seed in range(5):
        fold, chain, zero = t.fold_vs_chain(seed)
        emit(step="margin", data_seed=seed, rmse_fold_in=fold, rmse_in_chain=chain, rmse_prior_mean=zero, ratio=fold / chain)


def timing_case(name, N, M, T, K, S, R, repeats, once=False):
    from functionalmf_amd.factor import GaussianBayesianTensorFiltering
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N + R, K)), 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.5, size=(N + R, M, T))
    Y_new = Y[N:].copy()
    if M > 1:
        Y_new[:, 1::2] = np.nan
    else:
        Y_new[:, :, 1::2] = np.nan
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y[:N], nburn=20, nsamples=S, verbose=False)
    if once:
        model.fold_in_rows(Y_new, seed=1)
        return
    model.fold_in_rows(Y_new, seed=1)                         # warm-up: code objects, allocations
    t_fold, t_draw = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.fold_in_rows(Y_new, seed=1)
        t_fold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        model.fold_in_rows(Y_new, seed=1, summary=False)
        t_draw.append(time.perf_counter() - t0)
    # what a user could do before: an R-row model bound to the new rows, one W half-sweep per kept state
    np.random.seed(2)
    small = GaussianBayesianTensorFiltering(R, M, T, nembeds=K, rng="device")
    Ws = np.zeros((S, R, K))

    def loop():
        for s in range(S):
            small.V = res["V"][s]
            small.nu2, small.sigma2 = float(res["nu2"][s, 0]), float(res["sigma2"][s, 0])
            small._resample_W(Y_new)
            Ws[s] = small.W
    loop_ts = []
    for _ in range(max(1, repeats // 2)):
        t0 = time.perf_counter()
        loop()
        loop_ts.append(time.perf_counter() - t0)
    fmas = float(S) * R * M * T * (K * (K + 1) // 2 + K)
    emit(step="time", case=name, shape=[N, M, T], nembeds=K, nsamples=S, nrows_new=R, repeats=repeats,
         fold_in_seconds_min=min(t_fold), fold_in_seconds_median=float(np.median(t_fold)),
         fold_in_draw_only_seconds_min=min(t_draw), loop_seconds_min=min(loop_ts), speedup=min(loop_ts) / min(t_fold),
         accumulation_fmas=fmas)


def step_time(once=False):
    timing_case("flu (50,1,370)", 50, 1, 370, 5, 1000, 8, 5, once)
    timing_case("C3 (512,256,64)", 512, 256, 64, 5, 1000, 64, 5, once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["once"])
    a = ap.parse_args()
    if a.step is None:                     # every step in a child of its own, under its own time limit; stop at the first failure
        for step, limit in STEPS:
            rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step])
            if rc != 0:
                sys.exit("step %s ended with status %d: nothing more is started on the GPU" % (step, rc))
        return
    {"sweeps": step_sweeps, "margin": step_margin, "time": step_time, "once": lambda: step_time(once=True)}[a.step]()


if __name__ == "__main__":
    main()
