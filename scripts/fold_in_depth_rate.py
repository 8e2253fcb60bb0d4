"""Measurements behind fold_in_depth; appends JSON lines to profiles/r26_fold_in_depth_rate.jsonl.

    python scripts/fold_in_depth_rate.py --step sweeps   (no GPU) the chain's mixing from functionalmf_amd.fold_in_depth.chain
                                                         alone, numpy's generator: the largest standardised difference of
                                                         the curve means W v between 1, 2, ..., 128 sweeps and 256 sweeps
                                                         over replicate chains, at a flu-like slice (N = 50 rows with a
                                                         third observed, T = 40 kept depths, H = 8, K = 10, tf_order 2) and
                                                         a C3-like one (N = 60, K = 5): what DEFAULT_SWEEPS is chosen from
    python scripts/fold_in_depth_rate.py --step golden   (no GPU) the numpy references of tests 3, 4 and 5 (tests/golden/)
    python scripts/fold_in_depth_rate.py --step oracle   (no GPU) the Binomial reference alone (the last part of --step golden)
    python scripts/fold_in_depth_rate.py --step job      (no GPU) RMSE with data / RMSE of the forecast at the hidden rows
                                                         from the numpy definition over 5 data seeds (test 6's recipe)
    python scripts/fold_in_depth_rate.py                 every GPU step below, each in a child process under its own time limit
    python scripts/fold_in_depth_rate.py --step zscore   device generator against numpy's (tests 3 and 4)
    python scripts/fold_in_depth_rate.py --step binomial Binomial bias against a long run of the numpy definition (test 5), S = 16384
    python scripts/fold_in_depth_rate.py --step jobgpu   test 6's ratio on the device over 5 data seeds
    python scripts/fold_in_depth_rate.py --step time     fold_in_depth on S = 1000 device-collected samples, host wall clock with
                                                         transfers and the summary, min of 3: the flu shape (50,1,370), K = 10,
                                                         H = 8; C3 (512,256,64), K = 5, H = 8; the dose-response shape
                                                         (1024,256,9), K = 5, H = 2 - against the numpy definition per chain
                                                         (timed on a few chains, scaled to S * M: EXTRAPOLATED) and one V step
                                                         of the fitted model in the same run; the summary kernel's share is the
                                                         difference to a call with summary=False
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
OUT = os.path.join(ROOT, "profiles", "r26_fold_in_depth_rate.jsonl")
STEPS = (("zscore", 240), ("binomial", 240), ("jobgpu", 240), ("time", 560))
LONG = 256


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def test_module():
    sys.path.insert(0, os.path.join(ROOT, "tests"))           # (its conftest)
    spec = importlib.util.spec_from_file_location("test_gpu_fold_in_depth", os.path.join(ROOT, "tests", "test_gpu_fold_in_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mixing_problem(N, T, H, K, seed=0):
    """N rows, a third of them observed at every new depth, random-walk curves plus noise; one kept state."""
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    v = 0.3 * np.cumsum(rs.normal(size=(T + H, K)), axis=0)
    Y = W.dot(v[T:].T) + rs.normal(0, 0.5, size=(N, H))
    Y[rs.permutation(N)[N // 3:]] = np.nan
    return W, v[:T], Y, 0.25, 0.1


def step_sweeps(replicates=200, only=None, LONG=LONG):
    from functionalmf_amd import fold_in_depth as fd
    grid = tuple(2 ** k for k in range(20) if 2 ** k <= LONG // 2)
    for name, (N, T, H, K) in (("flu-like", (50, 40, 8, 10)), ("C3-like", (60, 40, 8, 5))):
        if only and only != name:
            continue
        W, V_old, Y, nu2, lam2 = mixing_problem(N, T, H, K)
        keep = {s: np.zeros((replicates,) + Y.shape) for s in grid + (LONG,)}
        rng = np.random.default_rng(2026)
        for rep in range(replicates):
            draws = fd.random_draws(rng, T, H, K, 2, LONG)

            def on_sweep(r, v, rep=rep):
                if r + 1 in keep:
                    keep[r + 1][rep] = W.dot(v.T)
            fd.chain(Y, W, V_old, nu2, lam2, 2, LONG, draws, on_sweep=on_sweep)
        ref = keep[LONG]
        for s in grid:
            d = keep[s].mean(axis=0) - ref.mean(axis=0)
            se = np.sqrt((keep[s].var(axis=0, ddof=1) + ref.var(axis=0, ddof=1)) / replicates)
            emit(step="sweeps", problem=name, shape=[N, T, H], nembeds=K, tf_order=2, replicates=replicates, sweeps=s, against=LONG,
                 max_abs_z=float(np.abs(d / se).max()), rms_z=float(np.sqrt(np.mean((d / se) ** 2))), max_abs_diff=float(np.abs(d).max()))


def step_golden():
    """(no GPU) tests/golden/fold_in_depth_numpy_replicates.npz and fold_in_depth_binomial_oracle.npz."""
    from functionalmf_amd import fold_in_depth as fd
    t = test_module()
    fa, fb = t.forecast_replicates(t.Z_SAMPLES, t.Z_SEEDS[0]), t.forecast_replicates(t.Z_SAMPLES, t.Z_SEEDS[1])
    ks = t.ks_two_sample(fb, fa)
    W, V_old, Y, nu2, lam2 = t.z_problem()
    a = t.numpy_replicates(W, V_old, Y, nu2, lam2, t.Z_SAMPLES, t.Z_SEEDS[0])
    b = t.numpy_replicates(W, V_old, Y, nu2, lam2, t.Z_SAMPLES, t.Z_SEEDS[1])
    z = t.two_sample_z(b, a)
    np.savez(os.path.join(ROOT, "tests", "golden", "fold_in_depth_numpy_replicates.npz"), forecast=fa, ks_numpy_vs_numpy=ks,
             mean=a.mean(axis=0), var=a.var(axis=0, ddof=1), first=a[:8], nsamples=t.Z_SAMPLES, sweeps=fd.DEFAULT_SWEEPS,
             seed=t.Z_SEEDS[0], z_numpy_vs_numpy=z)
    emit(step="golden", nsamples=t.Z_SAMPLES, sweeps=fd.DEFAULT_SWEEPS, ks_numpy_vs_numpy=ks, ks_limit=float(t.KS_LIMIT),
         max_abs_z_numpy_vs_numpy=z)
    step_oracle()


def step_oracle():
    """(no GPU) the Binomial reference of test 5: 64 independent long runs of the numpy definition."""
    t = test_module()
    m, se = t.binomial_oracle_chain()
    np.savez(os.path.join(ROOT, "tests", "golden", "fold_in_depth_binomial_oracle.npz"), mean=m, se=se)
    emit(step="golden", what="binomial oracle", chains=64, sweeps_kept=1024, burn=1024, oracle_mcse_max=float(se.max()))


def step_job():
    """(no GPU) test 6's recipe on the numpy definition, numpy's generator."""
    from functionalmf_amd import fold_in_depth as fd
    t = test_module()
    for seed in range(5):
        Ws, Vs, nu2, lam2, Y, truth, hid = t.job_problem(seed)
        S, M, T, K = Vs.shape
        H = Y.shape[2]
        rng = np.random.default_rng(100 + seed)
        means = []
        for data in (Y, np.full(Y.shape, np.nan)):
            acc = np.zeros(truth.shape)
            for s in range(S):
                for j in range(M):
                    v = fd.chain(data[:, j], Ws[s], Vs[s, j], nu2[s], lam2[s], 2, fd.DEFAULT_SWEEPS,
                                 fd.random_draws(rng, T, H, K, 2, fd.DEFAULT_SWEEPS))[0]
                    acc[:, j] += Ws[s].dot(v.T) / S
            means.append(acc)
        carry = np.einsum("snk,smk->nm", Ws, Vs[:, :, -1]) / S
        rd, rf = t.job_rmse(means[0], means[1], truth, hid)
        rc = t.job_rmse(np.repeat(carry[:, :, None], H, axis=2), means[1], truth, hid)[0]
        emit(step="job", where="numpy definition", data_seed=seed, sweeps=fd.DEFAULT_SWEEPS, rmse_with_data=rd, rmse_forecast=rf,
             rmse_carry_last_forward=rc, ratio=rd / rf)


def step_jobgpu():
    t = test_module()
    for seed in range(5):
        rd, rf = t.does_the_job(seed)
        emit(step="job", where="device", data_seed=seed, rmse_with_data=rd, rmse_forecast=rf, ratio=rd / rf)


def step_zscore():
    t = test_module()
    g = t.numpy_reference()
    ks = t.ks_two_sample(t.device_forecast(), g["forecast"])
    z, zref = t.device_generator_z()
    emit(step="zscore", nsamples=t.Z_SAMPLES, ks_device_vs_numpy=ks, ks_numpy_vs_numpy=float(g["ks_numpy_vs_numpy"]),
         ks_limit=float(t.KS_LIMIT), max_abs_z_device_vs_numpy=z, max_abs_z_numpy_vs_numpy=zref)


def step_binomial(S=16384):
    t = test_module()
    diff, se = t.binomial_bias(S)
    emit(step="binomial", nsamples=S, sweeps=None, max_abs_diff=diff, oracle_mcse=se)


def timing_case(name, N, M, T, K, H, S, repeats=3, numpy_chains=8):
    from functionalmf_amd import fold_in_depth as fd
    from functionalmf_amd.factor import GaussianBayesianTensorFiltering
    rs = np.random.RandomState(0)
    W, V = rs.normal(size=(N, K)), 0.1 * np.cumsum(rs.normal(size=(M, T + H, K)), axis=1)
    Y = np.einsum("nk,mtk->nmt", W, V) + rs.normal(0, 0.5, size=(N, M, T + H))
    Y_fit, Y_new = np.ascontiguousarray(Y[:, :, :T]), np.ascontiguousarray(Y[:, :, T:])
    Y_new[rs.permutation(N)[N // 2:]] = np.nan                         # half the rows report at the new depths
    np.random.seed(1)
    model = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, rng="device")
    res = model.run_gibbs(Y_fit, nburn=20, nsamples=S, verbose=False)
    model.fold_in_depth(Y_new, seed=1)                                 # warm-up: code objects, allocations
    t_fold, t_draw = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.fold_in_depth(Y_new, seed=1)
        t_fold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        model.fold_in_depth(Y_new, seed=1, summary=False)
        t_draw.append(time.perf_counter() - t0)
    print("%s: fold_in_depth %.3f s, chains only %.3f s" % (name, min(t_fold), min(t_draw)), file=sys.stderr, flush=True)
    # the host route: the numpy definition per chain, timed on a few chains and scaled to S * M
    rng = np.random.default_rng(3)
    t0 = time.perf_counter()
    for c in range(numpy_chains):
        s, j = c % S, c % M
        fd.chain(Y_new[:, j], res["W"][s], res["V"][s, j], float(res["nu2"][s, 0]), float(res["lam2"][s, 0]), model.tf_order,
                 fd.DEFAULT_SWEEPS, fd.random_draws(rng, T, H, K, model.tf_order, fd.DEFAULT_SWEEPS))
    host = (time.perf_counter() - t0) / numpy_chains * S * M
    # one V step of the fitted model, in the same run (queued and waited for)
    t_v = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        model._resample_V(Y_fit)
        model.V
        t_v.append(time.perf_counter() - t0)
    t_v = t_v[1:]                                                      # (the first one re-binds the data)
    emit(step="time", case=name, shape=[N, M, T], horizon=H, nembeds=K, nsamples=S, chains=S * M, sweeps=fd.DEFAULT_SWEEPS, repeats=repeats,
         fold_in_depth_seconds_min=min(t_fold), chains_only_seconds_min=min(t_draw), summary_seconds=min(t_fold) - min(t_draw),
         numpy_seconds_extrapolated=host, numpy_chains_timed=numpy_chains, speedup_over_numpy_extrapolated=host / min(t_fold),
         v_step_seconds_min=min(t_v), ratio_to_v_step=min(t_fold) / min(t_v), kernel_trace=False)


def step_time():
    timing_case("flu (50,1,370) K=10 H=8", 50, 1, 370, 10, 8, 1000)
    timing_case("dose-response (1024,256,9) K=5 H=2", 1024, 256, 9, 5, 2, 1000)
    timing_case("C3 (512,256,64) K=5 H=8", 512, 256, 64, 5, 8, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["sweeps", "golden", "oracle", "job"])
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
    {"golden": step_golden, "oracle": step_oracle, "job": step_job, "zscore": step_zscore, "binomial": step_binomial, "jobgpu": step_jobgpu,
     "time": step_time}[a.step]()


if __name__ == "__main__":
    main()
