"""Measurements behind negbin_fold_in_rows; appends JSON lines to profiles/r29_negbin_fold_in_rows_rate.jsonl.

    python scripts/negbin_fold_in_rows_rate.py --step sweeps  (no GPU) the mixing of a chain with a SAMPLED rate, from
                                                         negbin_fold_in.chain_rows alone on numpy's generator: over replicate
                                                         chains, the largest |z| of the paired difference of the means of log r
                                                         and of ilogit(w . v) between L sweeps and 4 L sweeps, L = 1, 2, ..., at a
                                                         politics-like row ((M,T) = (19,228), K = 5) and a flu-like row ((1,370),
                                                         K = 10), half the cells observed, the model's default Metropolis step
                                                         (nmetropolis 30, rpropstdev 0.1, rstdev 1): DEFAULT_SWEEPS["rows"] is
                                                         the smallest power of two after which it no longer falls
    python scripts/negbin_fold_in_rows_rate.py --step oracle  (no GPU) the reference of the sampled-rate test: chain_rows on 32768
                                                         numpy seeds at (M,T) = (3,4), K = 2, 2 replicates, 8 sweeps, nmetropolis 4;
                                                         the means of log r, w and ilogit(w . v) with their standard errors, and
                                                         the shift of the host stand-in sampler - the same at 4 PG_TERMS terms,
                                                         32768 more seeds (tests/golden/negbin_fold_in_rows_oracle.npz)
    python scripts/negbin_fold_in_rows_rate.py --step rate    (GPU) S = 500 uploaded samples, half the cells observed, default
                                                         sweeps, host wall clock with all transfers and the summary, min of 3, a
                                                         fixed and a sampled rate: politics-like (19,19,228) K = 5, R = 4; flu
                                                         (50,1,370) K = 10, R = 8; C3 (512,256,64) K = 5, R = 64 - against the
                                                         numpy definition per chain (timed on a few chains, scaled: EXTRAPOLATED)
                                                         and, as an observation, the Binomial fold_in_rows in the same run at the
                                                         same sweeps on (Y, Y + r) clipped to 32 trials
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r29_negbin_fold_in_rows_rate.jsonl")
GOLDEN = os.path.join(ROOT, "tests", "golden", "negbin_fold_in_rows_oracle.npz")
NMETROPOLIS, RPROPSTDEV, RSTDEV = 30, 0.1, 1.0           # the model's defaults
ORACLE = dict(M=3, T=4, K=2, nreps=2, sweeps=8, nmetropolis=4, rpropstdev=0.3, rstdev=1.0, rate_init=2.5, sigma2=1.5, nchains=32768)


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def ilogit(x):
    return 1.0 / (1.0 + np.exp(-x))


def count_row(M, T, K, rate, seed, observed=0.5, scale=0.6):
    """(V (M,T,K), Y (M,T)): a row of Negative-Binomial counts with rate `rate` at success probabilities ilogit(V w)."""
    rs = np.random.RandomState(seed)
    V = scale * np.cumsum(rs.normal(size=(M, T, K)), axis=1) / np.sqrt(np.arange(1, T + 1))[None, :, None]
    p = ilogit(V.dot(rs.normal(size=K)))
    Y = rs.negative_binomial(rate, 1.0 - np.clip(p, 0.02, 0.98)).astype(float)
    Y[rs.uniform(size=Y.shape) > observed] = np.nan
    return V, Y


# ---------------------------------------------------------------------------------------------------------- sweeps (CPU)
def _sweeps_chain(job):
    from functionalmf_amd import negbin_fold_in as nf
    name, M, T, K, rate, rate_init, longest, rep = job
    V, Y = count_row(M, T, K, rate, seed=1)
    rng = np.random.default_rng(1000 + rep)
    draws = nf.random_draws_rows(rng, K, longest, NMETROPOLIS)
    keep = {}
    Vf = V.reshape(-1, K)

    def on_sweep(sw, w, r):
        if (sw + 1) & sw == 0:                                             # after 1, 2, 4, ... sweeps
            keep[sw + 1] = np.concatenate([[np.log(r)], ilogit(Vf.dot(w))])

    nf.chain_rows(Y, V, 1.0, None, longest, draws, rate_init=rate_init, nmetropolis=NMETROPOLIS, rpropstdev=RPROPSTDEV, rstdev=RSTDEV,
                  seed=rep, on_sweep=on_sweep)
    return keep


def step_sweeps(replicates, longest, procs):
    cases = (("politics-like row (19,228) K=5", 19, 228, 5, 5.0, 2.0), ("flu-like row (1,370) K=10", 1, 370, 10, 20.0, 5.0))
    with multiprocessing.Pool(procs) as pool:
        for name, M, T, K, rate, rate_init in cases:
            kept = pool.map(_sweeps_chain, [(name, M, T, K, rate, rate_init, longest, rep) for rep in range(replicates)])
            L = 1
            while 4 * L <= longest:
                d = np.array([k[L] - k[4 * L] for k in kept])             # paired: the same chain after L and after 4 L sweeps
                z = np.abs(d.mean(axis=0)) / np.maximum(d.std(axis=0, ddof=1) / np.sqrt(replicates), 1e-300)
                emit(step="sweeps", case=name, sweeps=L, against=4 * L, replicates=replicates, nmetropolis=NMETROPOLIS, rpropstdev=RPROPSTDEV,
                     rate_true=rate, rate_init=rate_init, z_log_r=float(z[0]), z_ilogit_max=float(z[1:].max()), z_max=float(z.max()),
                     mean_log_r=float(np.mean([k[L][0] for k in kept])), mean_log_r_against=float(np.mean([k[4 * L][0] for k in kept])))
                L *= 2


# ---------------------------------------------------------------------------------------------------------- oracle (CPU)
def oracle_problem():
    o = ORACLE
    rs = np.random.RandomState(29)
    V = 0.8 * rs.normal(size=(o["M"], o["T"], o["K"]))
    Y = rs.negative_binomial(4.0, 0.4, size=(o["M"], o["T"], o["nreps"])).astype(float)
    Y[0, 1, 0] = Y[2, 3, 1] = np.nan
    Y[1, 2] = np.nan                                                       # a missing cell
    return V, Y


def _oracle_chunk(job):
    from functionalmf_amd import negbin_fold_in as nf
    seeds, terms = job
    o = ORACLE
    V, Y = oracle_problem()
    Vf = V.reshape(-1, o["K"])
    out = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        draws = nf.random_draws_rows(rng, o["K"], o["sweeps"], o["nmetropolis"])
        w, _, r, _ = nf.chain_rows(Y, V, o["sigma2"], None, o["sweeps"], draws, rate_init=o["rate_init"], nmetropolis=o["nmetropolis"],
                                   rpropstdev=o["rpropstdev"], rstdev=o["rstdev"], seed=rng, pg_terms=terms)
        out.append(np.concatenate([[np.log(r)], w, ilogit(Vf.dot(w))]))
    return np.array(out)


def step_oracle(procs):
    from functionalmf_amd import fold_in_cols as fc
    o = ORACLE
    n, K = o["nchains"], o["K"]
    V, Y = oracle_problem()
    stats = {}
    with multiprocessing.Pool(procs) as pool:
        for terms, first in ((fc.PG_TERMS, 0), (4 * fc.PG_TERMS, 10 ** 6)):
            chunks = [(list(range(first + c, first + min(c + 128, n))), terms) for c in range(0, n, 128)]
            x = np.concatenate(pool.map(_oracle_chunk, chunks))
            stats[terms] = (x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(n))
    mean, se = stats[fc.PG_TERMS]
    diff = np.abs(mean - stats[4 * fc.PG_TERMS][0])
    parts = {"logr": slice(0, 1), "w": slice(1, 1 + K), "p": slice(1 + K, None)}
    rec = {"shift_" + k: float(diff[s].max()) for k, s in parts.items()}
    np.savez(GOLDEN, V=V, Y=Y, nchains=n, pg_terms=fc.PG_TERMS, **{k: o[k] for k in ("sweeps", "nmetropolis", "rpropstdev", "rstdev", "rate_init", "sigma2")},
             **{"mean_" + k: mean[s] for k, s in parts.items()}, **{"se_" + k: se[s] for k, s in parts.items()}, **rec)
    emit(step="oracle", nchains=n, pg_terms=[fc.PG_TERMS, 4 * fc.PG_TERMS], mean_log_r=float(mean[0]), se_log_r=float(se[0]),
         se_w_max=float(se[parts["w"]].max()), se_ilogit_max=float(se[parts["p"]].max()),
         se_of_the_shift_max={k: float(np.sqrt(se[s] ** 2 + stats[4 * fc.PG_TERMS][1][s] ** 2).max()) for k, s in parts.items()}, **rec)


# ---------------------------------------------------------------------------------------------------------- rate (GPU)
def timing_case(name, M, T, K, R, S=500, repeats=3, numpy_chains=4, rate=5.0):
    from functionalmf_amd import fold_in, negbin_fold_in as nf, utils
    rs = np.random.RandomState(0)
    Vs = 0.2 * np.cumsum(rs.normal(size=(S, M, T, K)), axis=2)
    sigma2 = np.full(S, 1.0)
    Y = rs.negative_binomial(rate, 0.5, size=(R, M, T)).astype(float)
    Y[rs.uniform(size=Y.shape) < 0.5] = np.nan                            # half the cells observed
    Yb = np.minimum(Y, 32 - rate)
    rng = np.random.default_rng(3)
    for mode in ("fixed", "sampled"):
        sampled = mode == "sampled"
        sweeps = nf.DEFAULT_SWEEPS["rows"] if sampled else fold_in.DEFAULT_INNER_SWEEPS
        nm = NMETROPOLIS if sampled else 0
        if sampled:
            run = lambda: utils.negbin_fold_in_rows(Y, Vs, sigma2, sample_rate=True, rate_init=np.full(S, rate), nmetropolis=NMETROPOLIS,
                                                    rpropstdev=RPROPSTDEV, rstdev=RSTDEV, seed=1)
        else:
            run = lambda: utils.negbin_fold_in_rows(Y, Vs, sigma2, rate=np.full(S, rate), seed=1)
        binom = lambda: utils.fold_in_rows((Yb, Yb + rate), Vs, "binomial", sigma2=sigma2, seed=1, inner_sweeps=sweeps)
        one = lambda c: nf.chain_rows(Y[c % R], Vs[c % S], 1.0, None if sampled else rate, sweeps, nf.random_draws_rows(rng, K, sweeps, nm),
                                      rate_init=rate, nmetropolis=NMETROPOLIS, rpropstdev=RPROPSTDEV, rstdev=RSTDEV, seed=c)
        out = run()                                                        # warm-up: code objects, allocations
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
        host = (time.perf_counter() - t0) / numpy_chains * S * R
        print("%s, %s rate: NB %.3f s, Binomial %.3f s, numpy (extrapolated) %.0f s" % (name, mode, min(t_nb), min(t_bi), host),
              file=sys.stderr, flush=True)
        extra = dict(accept_mean=float(out["accept"].mean()), rate_mean=float(out["R"].mean())) if sampled else {}
        emit(step="rate", case=name, mode=mode, shape_new_rows=[R, M, T], nembeds=K, nsamples=S, chains=S * R, sweeps=sweeps, nmetropolis=nm,
             repeats=repeats, negbin_fold_in_rows_seconds_min=min(t_nb), numpy_seconds_extrapolated=host, numpy_chains_timed=numpy_chains,
             speedup_over_numpy_extrapolated=host / min(t_nb), binomial_fold_in_rows_seconds_min=min(t_bi),
             ratio_to_binomial_fold_in_rows=min(t_nb) / min(t_bi), kernel_trace=False, **extra)


def step_rate():
    timing_case("politics-like (19,19,228) K=5 R=4", 19, 228, 5, 4)
    timing_case("flu (50,1,370) K=10 R=8", 1, 370, 10, 8)
    timing_case("C3 (512,256,64) K=5 R=64", 256, 64, 5, 64, numpy_chains=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["sweeps", "oracle", "rate"], required=True)
    ap.add_argument("--replicates", type=int, default=64)
    ap.add_argument("--long", type=int, default=1024, help="sweeps: the longest chain (L runs up to a quarter of it); about 7 minutes on 8 cores")
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    if a.step == "sweeps":
        return step_sweeps(a.replicates, a.long, a.procs)
    if a.step == "oracle":
        return step_oracle(a.procs)
    step_rate()


if __name__ == "__main__":
    main()
