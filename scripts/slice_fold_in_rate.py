"""Measurements behind slice_fold_in_rows (one run on the GPU); appends JSON lines to profiles/r21_slice_fold_in_rate.jsonl.

    python scripts/slice_fold_in_rate.py                 every step below, each in a child process under its own time limit
    python scripts/slice_fold_in_rate.py --step sweeps   sweeps per chain: the mean against the quadrature posterior (the
                                                         set-ups of tests/test_gpu_slice_fold_in.py, tests 6 and 7) for
                                                         4..64 sweeps, S = 65536
    python scripts/slice_fold_in_rate.py --step margin   fold-in RMSE / in-chain RMSE over 5 data seeds (test 9's set-up)
    python scripts/slice_fold_in_rate.py --step time     slice_fold_in_rows against what a user could do before - an R-row
                                                         model per kept sample with V = V_s and the model's own _resample_W,
                                                         `sweeps` times (timed on LOOP_SAMPLES of the samples and scaled) -
                                                         and against one W step of the fitted model, at the dose-response
                                                         shape (S = 500, R = 8 and R = 64) and at C3 (512,256,64) Poisson
                                                         identity with 127 constraints
No kernel trace is collected here: the times are host wall clock around the whole call (uploads and summary included).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r21_slice_fold_in_rate.jsonl")
STEPS = (("sweeps", 420), ("margin", 420), ("time", 540))
LOOP_SAMPLES = 25


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def step_sweeps(S=65536):
    import test_gpu_slice_fold_in as t
    for name in ("poisson", "gamma_grid", "bernoulli", "features"):
        c = t.features_case() if name == "features" else t.quadrature_case(name)
        m, C = c["m"], c["C"]
        se = np.sqrt(np.diag(C) / S)
        for n in (4, 8, 16, 32, 64):
            out = t.run_features_case(S, 2024, sweeps=n) if name == "features" else t.run_quadrature_case(name, S, 2024, sweeps=n)
            W = out["W"][:, 0]
            d = W.mean(axis=0) - m
            emit(step="sweeps", case=name, sweeps=n, nsamples=S, posterior_mean=m.tolist(), diff=d.tolist(), z=(d / se).tolist(),
                 max_abs_z=float(np.abs(d / se).max()), max_abs_diff=float(np.abs(d).max()),
                 cov_max_abs_diff=float(np.abs(np.cov(W.T) - C).max()), rounds_per_chain=float(out["rounds"].mean()),
                 unfinished=int(out["unfinished"].sum()))


def step_margin():
    import test_gpu_slice_fold_in as t
    for seed in range(5):
        fold, chain, start = t.fold_vs_chain(seed)
        emit(step="margin", data_seed=seed, rmse_fold_in=fold, rmse_in_chain=chain, rmse_start=start, ratio=fold / chain)


def timing_case(name, family, S, R, N, M, T, K, G, repeats=3):
    import test_gpu_slice_fold_in as t
    from functionalmf_amd import slice_fold_in as sf
    from functionalmf_amd import utils
    from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
    Ws, Vs, sigma2, Y_new, lik, Cons = t.dose_response_inputs(S=S, R=R, N=N, M=M, T=T, K=K, G=G)
    if family == "poisson_identity":
        Cons = t.fit_constraints(T)
        Vs = 20.0 * Vs
        rs = np.random.RandomState(5)
        Y_new = np.where(np.isnan(Y_new), np.nan, rs.poisson(np.einsum("rk,mtk->rmt", Ws[0, :R], Vs[0]))[..., None].astype(float))
        lik = None
    kw = dict(sigma2=sigma2, Ws=Ws, likelihood_param=lik, Constraints=Cons, seed=3)
    out = utils.slice_fold_in_rows(Y_new, Vs, family, **kw)                  # warm-up: code objects, allocations
    ts, td = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        utils.slice_fold_in_rows(Y_new, Vs, family, **kw)
        ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        utils.slice_fold_in_rows(Y_new, Vs, family, summary=False, **kw)
        td.append(time.perf_counter() - t0)
    # what a user could do before: an R-row model bound to the new rows, `sweeps` W steps per kept state
    np.random.seed(2)
    mk = lambda n, W0: ConstrainedNonconjugateBayesianTensorFiltering(n, M, T, family, Cons, likelihood_param=lik, nembeds=K,
                                                                      W_init=W0, V_init=Vs[0].copy(), rng="device", device_seed=3)
    small = mk(R, np.ascontiguousarray(out["W_start"][0]))
    Wl = np.zeros((LOOP_SAMPLES, R, K))

    def loop():
        for s in range(LOOP_SAMPLES):
            small.V = Vs[s]
            small.W = out["W_start"][s]
            small.sigma2 = float(sigma2[s])
            for _ in range(sf.DEFAULT_SWEEPS):
                small._resample_W(Y_new)
            Wl[s] = small.W
    loop()
    tl = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        loop()
        tl.append(time.perf_counter() - t0)
    loop_all = min(tl) * S / LOOP_SAMPLES
    # one W step of the fitted model at that shape
    big = mk(N, np.ascontiguousarray(Ws[0]))
    Yb = np.full((N, M, T, 1), np.nan)
    Yb[:R] = Y_new[..., :1]
    big._resample_W(Yb)
    big.sync()
    tw = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        big._resample_W(Yb)
        big.sync()
        tw.append(time.perf_counter() - t0)
    emit(step="time", case=name, family=family, shape=[N, M, T], nembeds=K, nsamples=S, nrows_new=R, sweeps=sf.DEFAULT_SWEEPS,
         constraints=int(Cons.shape[0]), repeats=repeats, slice_fold_in_seconds_min=min(ts), slice_fold_in_seconds_median=float(np.median(ts)),
         slice_fold_in_draw_only_seconds_min=min(td), loop_samples=LOOP_SAMPLES, loop_seconds_min_on_those=min(tl),
         loop_seconds_scaled_to_all=loop_all, speedup_over_loop=loop_all / min(ts), model_w_step_seconds_min=min(tw),
         w_steps_per_call=min(ts) / min(tw), rounds_per_chain=float(out["rounds"].mean()),
         pairs_without_capped_sweep=float(np.mean(out["unfinished"] == 0)), kernel_trace=False)


def step_time():
    timing_case("dose-response (1024,256,9) R=8", "gamma_grid", 500, 8, 1024, 256, 9, 5, 50)
    timing_case("dose-response (1024,256,9) R=64", "gamma_grid", 500, 64, 1024, 256, 9, 5, 50)
    timing_case("C3 (512,256,64) R=8", "poisson_identity", 500, 8, 512, 256, 64, 5, 50)


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
