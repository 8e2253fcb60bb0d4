"""Measurements behind negbin_fold_in_cols / negbin_fold_in_depth; appends JSON lines to profiles/r28_negbin_fold_in_rate.jsonl.

    python scripts/negbin_fold_in_rate.py --step sweeps  (no GPU) the chains' mixing from negbin_fold_in.chain_cols / chain_depth
                                                         alone, numpy's generator: the largest standardised difference of the
                                                         success probabilities ilogit(W v) between 1, 2, ..., 128 sweeps and
                                                         256 sweeps over replicate chains, at a count column (N = 40 rows, a
                                                         third observed, T = 12, K = 3) and a count slice (T = 12, H = 4) - the
                                                         check that the Binomial family's default sweeps serve this family too
    python scripts/negbin_fold_in_rate.py --step oracle  (no GPU) the reference of the large-count test: a long run of
                                                         chain_cols at R = 50 with counts into the hundreds, its mean of
                                                         ilogit(W v) and batch-means standard error
                                                         (tests/golden/negbin_fold_in_oracle.npz)
    python scripts/negbin_fold_in_rate.py                every GPU step below, each in a child process under its own time limit
    python scripts/negbin_fold_in_rate.py --step bias    S = 16384: the largest |difference| of the means of ilogit(W v) between
                                                         the NB fold-ins and the Binomial fold-ins on (Y, Y + R) (columns,
                                                         depths), and between negbin_fold_in_cols and the oracle at large
                                                         counts - the allowances of tests/test_gpu_negbin_fold_in.py are twice
                                                         these
    python scripts/negbin_fold_in_rate.py --step rate    S = 500 uploaded samples, half the rows observed, host wall clock with
                                                         all transfers and the summary, min of 3: flu (50,1,370) K = 10, H = 8;
                                                         politics-like (19,19,228) K = 5, H = 8; C3 (512,256,64) K = 5, C = 8
                                                         columns and H = 8 depths - against the numpy definition per chain (timed
                                                         on a few chains, scaled: EXTRAPOLATED) and, as an observation, the
                                                         Binomial fold-in in the same run on (Y, Y + R) clipped to 32 trials
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
OUT = os.path.join(ROOT, "profiles", "r28_negbin_fold_in_rate.jsonl")
GOLDEN = os.path.join(ROOT, "tests", "golden", "negbin_fold_in_oracle.npz")
STEPS = (("bias", 300), ("rate", 560))
LONG = 256


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def test_module():
    sys.path.insert(0, os.path.join(ROOT, "tests"))           # (its conftest)
    spec = importlib.util.spec_from_file_location("test_gpu_negbin_fold_in", os.path.join(ROOT, "tests", "test_gpu_negbin_fold_in.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ilogit(x):
    return 1.0 / (1.0 + np.exp(-x))


def count_problem(N, T, K, rate, seed=0, observed=1.0 / 3):
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(N, K))
    v = 0.4 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = rs.negative_binomial(rate, 1.0 - ilogit(W.dot(v.T))).astype(float)
    Y[rs.permutation(N)[int(N * observed):]] = np.nan
    return W, v, Y


def step_sweeps(replicates=100, LONG=LONG):
    from functionalmf_amd import fold_in_cols as fc, fold_in_depth as fd, negbin_fold_in as nf
    N, T, K, H, tf, rate, lam2 = 40, 12, 3, 4, 2, 5.0, 0.1
    W, v, Y = count_problem(N, T + H, K, rate)
    grid = [1, 2, 4, 8, 16, 32, 64, 128]
    for axis in ("cols", "depth"):
        states = {g: [] for g in grid + [LONG]}
        rng = np.random.default_rng(1)
        for rep in range(replicates):
            def on_sweep(r, x, rep=rep):
                if r + 1 in states:
                    states[r + 1].append(ilogit(W.dot(x.T)))
            if axis == "cols":
                nf.chain_cols(Y[:, :T], W, rate, lam2, tf, LONG, fc.random_draws(rng, T, K, tf, LONG), on_sweep=on_sweep, seed=rep)
            else:
                nf.chain_depth(Y[:, T:], W, v[:T], rate, lam2, tf, LONG, fd.random_draws(rng, T, H, K, tf, LONG), on_sweep=on_sweep,
                               seed=rep)
        ref = np.array(states[LONG])
        for g in grid:
            x = np.array(states[g])
            z = np.abs(x.mean(axis=0) - ref.mean(axis=0)) / np.sqrt(x.var(axis=0, ddof=1) / replicates + ref.var(axis=0, ddof=1) / replicates)
            emit(step="sweeps", axis=axis, shape=[N, T, K], horizon=H, rate=rate, replicates=replicates, sweeps=g, against=LONG,
                 max_standardised_difference=float(z.max()))


def large_count_problem():
    """N = 16, T = 6, K = 2, R = 50: y + R between a few dozen and several hundred, on both sides of PG_NORMAL_B = 200."""
    rs = np.random.RandomState(4)
    N, T, K, rate = 16, 6, 2, 50.0
    W = rs.normal(size=(N, K))
    v = np.array([0.9, 0.5]) + 0.25 * np.cumsum(rs.normal(size=(T, K)), axis=0)
    Y = rs.negative_binomial(rate, 1.0 - ilogit(W.dot(v.T))).astype(float)
    Y[rs.uniform(size=(N, T)) < 0.15] = np.nan
    return W, Y, rate, 0.1


def step_oracle(nburn=1000, nsweeps=60000, batches=30):
    from functionalmf_amd import fold_in_cols as fc, negbin_fold_in as nf
    W, Y, rate, lam2 = large_count_problem()
    N, T = Y.shape
    K = W.shape[1]
    b = np.where(np.isnan(Y), 0.0, Y + rate)
    kept = []

    def on_sweep(r, x):
        if r >= nburn:
            kept.append(ilogit(W.dot(x.T)))
    t0 = time.perf_counter()
    nf.chain_cols(Y, W, rate, lam2, 2, nburn + nsweeps, fc.random_draws(np.random.default_rng(11), T, K, 2, nburn + nsweeps),
                  on_sweep=on_sweep, seed=12)
    p = np.array(kept)
    bm = p.reshape(batches, nsweeps // batches, N, T).mean(axis=1)
    mean, se = p.mean(axis=0), bm.std(axis=0, ddof=1) / np.sqrt(batches)
    np.savez_compressed(GOLDEN, W=W, Y=Y, rate=rate, lam2=lam2, mean=mean, se=se, nburn=nburn, nsweeps=nsweeps)
    emit(step="oracle", shape=[N, T, K], rate=rate, nburn=nburn, sweeps=nsweeps, batches=batches, max_mcse=float(se.max()),
         pseudo_trials_min=float(b[b > 0].min()), pseudo_trials_max=float(b.max()), cells_in_normal_range=int((b >= 200).sum()),
         cells_in_series_range=int(((b > 0) & (b < 200)).sum()), seconds=time.perf_counter() - t0)


def step_bias(S=16384):
    t = test_module()
    for axis in ("cols", "depth"):
        d, se5 = t.nb_vs_binomial(axis, S)
        emit(step="bias", what="nb_vs_binomial_" + axis, nsamples=S, max_abs_diff=float(d.max()), five_se_there=float(se5.reshape(-1)[np.argmax(d)]))
    d, se5, se = t.large_count_bias(S)
    emit(step="bias", what="large_counts_vs_oracle", nsamples=S, max_abs_diff=float(d.max()), five_se_there=float(se5.reshape(-1)[np.argmax(d)]),
         oracle_mcse=se)


def timing_case(name, axis, N, M, T, K, D, S=500, repeats=3, numpy_chains=4, rate=5.0):
    """axis "cols": D = C new columns on T depths; "depth": D = H new depths of the M fitted columns."""
    from functionalmf_amd import fold_in_cols as fc, fold_in_depth as fd, negbin_fold_in as nf, utils
    rs = np.random.RandomState(0)
    Ws = rs.normal(size=(S, N, K)) * 0.6
    Vs = 0.2 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2)
    lam2, R = np.full(S, 0.1), np.full(S, rate)
    tf = 2
    if axis == "cols":
        chains, sweeps = S * D, fc.DEFAULT_SWEEPS
        Y = rs.negative_binomial(rate, 0.5, size=(D, N, T)).astype(float)
        Y[:, rs.permutation(N)[N // 2:]] = np.nan                          # half the rows observed
        run = lambda: utils.negbin_fold_in_cols(Y, Ws, R, lam2=lam2, tf_order=tf, seed=1)
        Yb = np.minimum(Y, 32 - rate)
        binom = lambda: utils.fold_in_cols((Yb, Yb + rate), Ws, "binomial", lam2=lam2, tf_order=tf, seed=1)
        rng = np.random.default_rng(3)
        one = lambda c: nf.chain_cols(Y[c % D], Ws[c % S], rate, 0.1, tf, sweeps, fc.random_draws(rng, T, K, tf, sweeps), seed=c)
    else:
        chains, sweeps = S * M, fd.DEFAULT_SWEEPS
        Y = rs.negative_binomial(rate, 0.5, size=(N, M, D)).astype(float)
        Y[rs.permutation(N)[N // 2:]] = np.nan
        run = lambda: utils.negbin_fold_in_depth(Y, Ws, Vs, R, lam2=lam2, tf_order=tf, seed=1)
        Yb = np.minimum(Y, 32 - rate)
        binom = lambda: utils.fold_in_depth((Yb, Yb + rate), Ws, Vs, "binomial", lam2=lam2, tf_order=tf, seed=1)
        rng = np.random.default_rng(3)
        one = lambda c: nf.chain_depth(Y[:, c % M], Ws[c % S], Vs[c % S, c % M], rate, 0.1, tf, sweeps,
                                       fd.random_draws(rng, T, D, K, tf, sweeps), seed=c)
    run()                                                                  # warm-up: code objects, allocations
    binom()
    t_nb, t_bi = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        t_nb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        binom()
        t_bi.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for c in range(numpy_chains):
        one(c)
    host = (time.perf_counter() - t0) / numpy_chains * chains
    print("%s: NB %.3f s, Binomial %.3f s, numpy (extrapolated) %.0f s" % (name, min(t_nb), min(t_bi), host), file=sys.stderr, flush=True)
    emit(step="rate", case=name, axis=axis, shape=[N, M, T], new=D, nembeds=K, nsamples=S, chains=chains, sweeps=sweeps, repeats=repeats,
         negbin_fold_in_seconds_min=min(t_nb), numpy_seconds_extrapolated=host, numpy_chains_timed=numpy_chains,
         speedup_over_numpy_extrapolated=host / min(t_nb), binomial_fold_in_seconds_min=min(t_bi),
         ratio_to_binomial_fold_in=min(t_nb) / min(t_bi), kernel_trace=False)


def step_rate():
    timing_case("flu (50,1,370) K=10 H=8", "depth", 50, 1, 370, 10, 8)
    timing_case("politics-like (19,19,228) K=5 H=8", "depth", 19, 19, 228, 5, 8)
    timing_case("C3 (512,256,64) K=5 H=8", "depth", 512, 256, 64, 5, 8, numpy_chains=2)
    timing_case("C3 (512,256,64) K=5 C=8", "cols", 512, 256, 64, 5, 8, numpy_chains=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["sweeps", "oracle"])
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--long", type=int, default=LONG)
    a = ap.parse_args()
    if a.step is None:                     # every step in a child of its own, under its own time limit; stop at the first failure
        for step, limit in STEPS:
            rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step])
            if rc != 0:
                sys.exit("step %s ended with status %d: nothing more is started on the GPU" % (step, rc))
        return
    if a.step == "sweeps":
        return step_sweeps(a.replicates, a.long)
    {"oracle": step_oracle, "bias": step_bias, "rate": step_rate}[a.step]()


if __name__ == "__main__":
    main()
