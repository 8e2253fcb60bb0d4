/* btf.h - C ABI of the MI355X-native Gibbs core for Bayesian Tensor Filtering.
 *
 * This is the drop-in boundary for the hot path of tansey/functionalmf
 *   run_gibbs -> resample -> _resample_W / _resample_V / _resample_nu2
 * (reference functionalmf/factor.py:306-460, functionalmf/fast_mvn.py:10-74).
 * The reference has no FFI layer of its own: the boundary there is the Python
 * method contract of the model object.  Each entry point below
 * names the reference code whose *body* it replaces; the Python classes in
 * functionalmf_amd/factor.py keep the reference's method names and call these
 * through ctypes (see INTEGRATION.md for the binding a maintainer would add to
 * functionalmf/factor.py itself).
 *
 * Conventions
 *   - plain C types only; all arrays are float64, C-contiguous, caller-owned and
 *     borrowed for the duration of the call;
 *   - every function returns a BTF_* status; text via btf_last_error();
 *   - one ctx = one Markov chain on one GPU; calls on a ctx must be serialised by
 *     the caller; different ctxs may live on different threads / devices;
 *   - "step" functions only enqueue work on the ctx's HIP stream; results are
 *     visible after btf_sync() or any btf_get_* (which synchronise);
 *   - NaN marks a missing observation (reference convention);
 *   - dims: N=nrows, M=ncols, T=ndepth, R=nreps, K=nembeds, nD = rows of the
 *     trend-filter penalty Delta (utils.py:66-90).
 */
#ifndef BTF_H_
#define BTF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct btf_ctx btf_ctx;

enum {
  BTF_OK = 0,
  BTF_EINVAL = 1, /* bad argument / unsupported shape                          */
  BTF_EHIP = 2,   /* a HIP runtime call failed (text in btf_last_error)        */
  BTF_ENOTPD = 3, /* a conditional precision was not positive definite (after
                     the jitter retries for V; immediately for W, as
                     np.linalg.cholesky raises at factor.py:357).  Where the
                     reference would warn forever (fast_mvn.py:69-72) this
                     returns instead.  btf_fail_index() names the row/column.  */
  BTF_ESTATE = 4  /* call order: data / state not set yet                      */
};

enum { BTF_COMPAT_REFERENCE = 0, BTF_COMPAT_EXACT = 1 };

/* kernel ids for btf_kernel_times() */
enum {
  BTF_K_STATS = 0,   /* one-time sufficient statistics                      */
  BTF_K_W_ACCUM = 1, /* streaming Gram/mean accumulation, W half-sweep      */
  BTF_K_W_SOLVE = 2, /* batched KxK Cholesky + draw per row                 */
  BTF_K_V_ACCUM = 3, /* streaming Gram/mean accumulation, V half-sweep      */
  BTF_K_V_BANDED = 4,/* block-banded Cholesky sampler per column (fast_mvn) */
  BTF_K_GRAM = 5,    /* K x K Gram of the fixed factor (complete-data path) */
  BTF_K_PROD = 6,    /* small reductions (NB log-likelihood partials); the per-row outer products of the weighted
                        path are formed inside the accumulation since round 2 */
  BTF_K_SSE = 7,     /* residual sum of squares for nu2                     */
  BTF_K_PG = 8,      /* Polya-Gamma draws                                   */
  BTF_K_NB = 9,      /* Negative-Binomial rate update: MH log-likelihood ratio */
  BTF_K_PRIOR = 10,  /* prior band Delta' diag(1/(lam2 Tau2_j)) Delta of every column (factor.py:404-405) */
  BTF_K_EIG = 11,    /* eigen-system of the K x K Gram (spectral sampler)   */
  BTF_K_HYPER = 12,  /* device hyper-parameter draws: Tau2 chain, nu2/sigma2, lam2 */
  BTF_K_ESS = 13,    /* elliptical slice sampling: prior draws, proposals, likelihood passes, decisions */
  BTF_K_CRITERIA = 14, /* model-selection criteria: per-curve log-likelihood over the kept samples (btf_crit_eval, btf_crit_loo) */
  BTF_K_COUNT = 15
};

/* btf_set_option keys / values */
enum {
  BTF_OPT_SAMPLER = 0,       /* V half-sweep sampler, BTF_SAMPLER_*                                   */
  BTF_OPT_NB_HISTOGRAMS = 1, /* 1 (default): Negative-Binomial rate update from per-row count
                                histograms where they apply; 0: always the full-tensor kernel          */
  BTF_OPT_FUSE_GRAM = 2,     /* 1 (default): W'W / V'V partials come out of the preceding solve kernel */
  BTF_OPT_CURVE_COUNTS = 4,  /* 1 (default): Gaussian data whose replicate counts do not vary along the depth axis
                                (whole curves missing, as Y[:3,:3] = NaN in the reference's examples) run the
                                complete-data kernels plus per-row / per-column corrections (same conditionals as the
                                weighted form of factor.py:343-346, :388-391); 0: always the weighted form         */
  BTF_OPT_FUSED_SWEEP = 6,   /* 1 (default): full sweeps with device-resident scalars on complete Gaussian data run as FOUR launches -
                                the spectral V sampler leaves every column's part of the residual sum of squares behind, nu2 | rest
                                and sigma2 | rest of the next sweep ride in its W accumulation launch as a side workgroup
                                (btf_queue_scalars), lam2 | rest in the V accumulation launch (btf_queue_lam2) - instead of six
                                (a residual reduction and a scalar-draw launch between W accumulation and W solve).  Same
                                conditionals, same Philox streams; the sums are formed in another order (rounding).  0: six.   */
  BTF_OPT_FUSED_STEP = 7,    /* Latency kernels as parts of the streaming launches (csrc/btf_fused.h), complete Gaussian data.
                                0: a W+V step is four launches.
                                1 (default): the spectral sampler of _resample_V (factor.py:377-409, fast_mvn.py:35-47) is the TAIL
                                of the V accumulation launch - a tile of 128 (column, depth) outputs is whole columns (ndepth 32, 64
                                or 128; tf_order 2; nembeds <= 8; other shapes run the four-launch form), their sums go from the
                                reduction straight into the sampler's layout; the prior band of the columns is precomputed
                                (prior_band_kernel, only when Tau2 / lam2 changed) and loaded at kernel start.
                                2: also the batched K x K solve of _resample_W (factor.py:349-362), by "owner" workgroups of the W
                                accumulation launch that wait for their tile's streaming workgroups: two launches.
                                All three walk the same chain bit for bit (tests/test_gpu_fused.py).  Measured on MI355X at
                                (512,256,64) nembeds 5: 41.2 / 38.7 / 42.2 us per step. */
  BTF_OPT_FUSED_DATAFLOW = 8,/* 1 (default): where the fused V launch of BTF_OPT_FUSED_STEP >= 1 allows it - one chunk per tile, the
                                precomputed prior band, nembeds <= 6 - its tail is the BARRIER-FREE form (csrc/btf_fused.h,
                                v_fused_df): the chain wave of a column factors A_k = g_k I + P_j (fast_mvn.py:38) the moment its own
                                stream ends, while the other waves still stream, reduce and rotate; LDS counters order the
                                stages.  Bit-identical to the barrier tail and to the four-launch form.  Measured at
                                (512,256,64) nembeds 5: 20.4 us per V launch against 21.0.  0: the barrier tail. */
  BTF_OPT_GRAM_ASIDE = 9,    /* 1 (default): the per-column shares V_j'V_j of the Gram that the next W half-sweep needs are not formed at
                                the end of the fused V launch (BTF_OPT_FUSED_STEP >= 1: its tails store V and leave) but by side
                                workgroups of the NEXT W accumulation launch, beside its stream, from V as stored - whole contexts,
                                complete Gaussian data, nembeds <= 8; anything else that needs the shares first gets them from a small
                                launch of the same device function.  Same operations in the same order: bit-identical
                                (tests/test_gpu_gram_aside.py).  Acts on bare W+V steps only: inside full sweeps (the V launch also leaves
                                the residual parts) and under BTF_OPT_FUSED_STEP 2 the tails keep forming the shares, whatever the
                                value.  0: the tails form the shares.                          */
  BTF_OPT_SPLIT_ACCUM = 5,   /* sharded Gaussian contexts: 1 - the streaming accumulation of a half-sweep runs in two launches: the
                                chunks that reduce over this rank's OWN block of the fixed factor (its columns of V for the W
                                half-sweep, its rows of W for the V half-sweep) are queued right behind the kernel that drew
                                that block - they need no exchange - and the remaining chunks by the next half-sweep call, behind
                                the all-gather (btf_comm_fork / btf_comm_join order a communication stream against them).
                                Same partial sums, same results.  0 (default): one launch.                              */
  BTF_OPT_PG_EXACT = 3       /* Polya-Gamma sampler of btf_pg_draw (what pypolyagamma's pgdrawv does at factor.py:459).
                                0 (default): every integer trial count up to 32 by Devroye's exact alternating-series
                                sampler, summed b times, as pypolyagamma does (flat per-lane work-queue kernels: f32
                                squeeze, f64 decisions inside the guard bands); larger and non-integer counts by the
                                sum-of-gammas series with a moment-matched remainder (approximate; validated against the
                                exact sampler).  Count data (btf_set_data_counts: pseudo-trial counts sum(y) + n r, integers
                                only by accident): the series for every cell.
                                1: exact for every count below 200 - floor(b) Devroye draws plus a 128-term series for a
                                fractional part.
                                2: the series for every count (opt-in; the round-2 default for counts >= 3).
                                Counts >= 200: moment-matched normal in every mode.                             */
};
enum {
  BTF_SAMPLER_BANDED = 0,   /* block-banded LDL' in the declared elimination order (btf_get_V_order):
                               twisted two-chain kernel where it applies; default                     */
  BTF_SAMPLER_SPECTRAL = 1, /* complete Gaussian data only: rotate by the eigenvectors of the shared
                               K x K likelihood block, K scalar banded chains per column (falls back to
                               BANDED for weighted data); square root documented at btf_resample_V     */
  BTF_SAMPLER_CHAIN = 2,    /* single chain, depth-major order                                         */
  BTF_SAMPLER_GENERIC = 3,  /* any-size kernel (band in LDS or HBM scratch), depth-major order         */
  BTF_SAMPLER_BANDED_NOPANEL = 4 /* BANDED without the panelised MFMA factorisation (A/B aid)          */
};

/* ---- lifetime ------------------------------------------------------------
 * Replaces the array allocations of BayesianTensorFiltering.__init__
 * (factor.py:24-110) on the device side.  `stream` is a hipStream_t to run on
 * (e.g. torch.cuda.current_stream().cuda_stream) or NULL for a private one. */
int btf_create(btf_ctx** out, int nrows, int ncols, int ndepth, int nembeds,
               int tf_order, int device, void* stream);
void btf_destroy(btf_ctx* ctx);
const char* btf_last_error(const btf_ctx* ctx);
int btf_fail_index(const btf_ctx* ctx);

/* ---- sharding (multi-GPU) --------------------------------------
 * This ctx updates rows [row0,row0+nrows_local) in the W half-sweep and columns
 * [col0,col0+ncols_local) in the V half-sweep.  Must precede btf_set_data_*.
 * Default: everything.  W and V are replicated: after each half-sweep the updated block is
 * all-gathered - btf_allgather_W / btf_allgather_V below (the ctx's own RCCL communicator), or by
 * the caller on the device pointers btf_dev_W / btf_dev_V. */
int btf_set_shard(btf_ctx* ctx, int row0, int nrows_local, int col0, int ncols_local);
/* compat=REFERENCE in a sharded run (compat caveat).  The cached likelihood weights of quirks Q1/Q2 come from
 * a SOURCE row / column (factor.py:320,349: row nembeds-1 for every later row when the data hold no NaN;
 * factor.py:394-401: the last column at which the NaN pattern changed), which may lie outside the rank's blocks.  With
 * contiguous blocks at most ONE such row and ONE such column exist per rank (the row sources are nembeds-1 or the row
 * itself; the column sources never decrease and are a column's own index or its left neighbour's source).  Declare them
 * here (global indices, -1: none), after btf_set_shard and before the upload: every row slab handed to
 * btf_set_data_* / btf_set_omega then has nrows_local + 1 rows, the source row LAST, every column slab
 * ncols_local + 1 columns, the source column last (btf_set_data_counts keeps taking the whole tensor).  The halo is
 * never updated and never enters a sum (nobs, SSE); only its weights are read - by the stale-weight accumulation
 * (btf_set_stale_sources maps a source equal to the halo onto its slot) - and btf_pg_draw draws them from the streams
 * of the source's global cells, i.e. the values the owning rank draws.  A changed halo invalidates the uploaded data. */
int btf_set_shard_halo(btf_ctx* ctx, int halo_row, int halo_col);
void* btf_stream(btf_ctx* ctx); /* the hipStream_t every step function of this ctx enqueues on (the one passed
                                  to btf_create, or the private one): collectives on the ctx's buffers and event
                                  timing must be ordered against it */
/* Ordering a communication stream (the one the all-gathers of W / V are issued on) against the ctx's stream:
 * btf_comm_fork makes `comm_stream` wait for the kernel that drew this rank's block in the last half-sweep (not for work
 * queued behind it: BTF_OPT_SPLIT_ACCUM); btf_comm_join makes the ctx's stream wait for everything queued on
 * `comm_stream` so far.  hipStream_t handles; no host synchronisation. */
int btf_comm_fork(btf_ctx* ctx, void* comm_stream);
int btf_comm_join(btf_ctx* ctx, void* comm_stream);
/* ---- the ctx-owned communicator ("ctx owns device buffers, streams, RCCL communicators"; 8(e)) -----------
 * The exchange of a sharded run - given V the rows of W are independent (factor.py:333), given W the columns of V are
 * (factor.py:378), so each half-sweep ends in ONE all-gather of the freshly drawn blocks - issued by the library
 * itself: ncclAllGather / ncclAllReduce of RCCL, in place on the ctx's own W / V / scalar buffers and on the ctx's own
 * stream (stream-ordered, no host synchronisation).  RCCL is bound at run time (csrc/btf_comm.h): a process that never
 * calls these never maps it.  One process per GPU, one ctx per process and communicator.
 *
 *   rank 0:      btf_comm_unique_id(id, BTF_COMM_ID_BYTES)       (ncclGetUniqueId)
 *   the caller:  hands the 128 bytes to every rank over any channel it has (MPI, a file, a socket, torch.distributed)
 *   every rank:  btf_set_shard(blocks of btf_comm_block) ... btf_comm_init(ctx, rank, world, id, BTF_COMM_ID_BYTES)
 *   every sweep: btf_resample_W -> btf_allgather_W -> btf_resample_V -> btf_allgather_V
 *
 * btf_comm_block: the block [lo, lo + len) of an axis of n rows / columns that rank `rank` of `world` owns - equal
 * chunks ceil(n / world), the tail ranks short or empty (the only decomposition one in-place all-gather reassembles;
 * W and V are allocated with 64 spare rows / columns for it, hence world <= 64).  The all-gathers return BTF_ESTATE
 * if btf_set_shard was given anything else.
 * btf_allgather_W / _V: all-gather of the block this rank drew in the last half-sweep.  With BTF_OPT_SPLIT_ACCUM the
 * gather runs on a communication stream of the ctx, ordered by btf_comm_fork / btf_comm_join as described there.
 * btf_allreduce_sse: sums the device scalar HYP_SSE (slot 4 of btf_dev_hyp) over the ranks - the one exchange of a
 * sharded nu2 draw (btf_draw_scalars which | 8, this call, which | 16).
 * btf_allreduce_sum: sums n <= 16 host doubles over the ranks, in place (observation counts at set-up, the host-side
 * nu2 draw's residual sum of squares).  Synchronises.
 * btf_comm_rehearse: a timing aid - ONE process plays rank `rank` of `world`: a one-rank communicator, and every
 * all-gather moves the full gathered message (world x chunk doubles) from one scratch buffer to another, so the step
 * pays RCCL's call and the message's bytes but the blocks of the other ranks are never refreshed: not a sampler.
 * btf_comm_info: out[8] = {has communicator, its rank, its size, gather rank, gather world, rehearsal, RCCL version
 * code, ncclCommCount}; out[0] is 2 for the peer-window transport below.
 *
 * The peer-window transport (csrc/btf_comm.h) runs the same four collectives without RCCL: every rank maps the W / V
 * buffers and a mailbox of every other rank (hipIpc handles: processes of one node whose GPUs can map each other) and one
 * kernel per collective stores this rank's block straight into the peers' buffers, flags it and waits for theirs - one
 * launch, two flag round trips.  It is also the only device-side transport for several ranks on ONE GPU.
 *   every rank:  btf_peer_export(ctx, desc, BTF_PEER_DESC_BYTES)
 *   the caller:  all-gathers the descriptors over its channel (MPI_Allgather, torch.distributed)
 *   every rank:  btf_peer_init(ctx, rank, world, descs, world * BTF_PEER_DESC_BYTES)       (descs rank-major)
 * after which btf_allgather_W / _V, btf_allreduce_sse and btf_allreduce_sum use it (btf_comm_info out[0] == 2), under
 * the rule of every collective library: all ranks issue the same sequence of collectives.  Sums are taken in rank order
 * on every rank (identical bits everywhere).  A peer that never arrives turns, after BTF_PEER_TIMEOUT_MS (default
 * 20000), into BTF_EHIP at the next step's status check - not into a hung GPU.  btf_comm_destroy tears it down.          */
#define BTF_COMM_ID_BYTES 128
#define BTF_PEER_DESC_BYTES 256
int btf_peer_export(btf_ctx* ctx, unsigned char* desc, int nbytes);
int btf_peer_init(btf_ctx* ctx, int rank, int world, const unsigned char* descs, int nbytes);
int btf_comm_unique_id(unsigned char* id, int nbytes);
int btf_comm_block(int n, int rank, int world, int32_t* lo, int32_t* len);
int btf_comm_init(btf_ctx* ctx, int rank, int world, const unsigned char* id, int nbytes);
int btf_comm_rehearse(btf_ctx* ctx, int rank, int world);
int btf_comm_destroy(btf_ctx* ctx);
int btf_comm_info(btf_ctx* ctx, int32_t* out);
int btf_allgather_W(btf_ctx* ctx);
int btf_allgather_V(btf_ctx* ctx);
int btf_allreduce_sse(btf_ctx* ctx);
int btf_allreduce_sum(btf_ctx* ctx, double* vals, int n);
/* btf_set_W / btf_set_V for an exchange staged through the host: the caller's own block is unchanged, so chunks already
 * accumulated from it (BTF_OPT_SPLIT_ACCUM) stay valid. */
int btf_set_gathered_W(btf_ctx* ctx, const double* W);
int btf_set_gathered_V(btf_ctx* ctx, const double* V);
void* btf_dev_W(btf_ctx* ctx); /* device double[N][K]    */
void* btf_dev_V(btf_ctx* ctx); /* device double[M][T][K] */

/* ---- data -----------------------------------------------------------------
 * Hoists what factor.py:329-330 and :374-375 recompute every half-sweep
 * (replicate counts and NaN-means) into one pass.  y_rows is the row slab
 * Y[row0:row0+nrows_local] of shape (nrows_local,M,T,R); y_cols is the column
 * slab Y[:,col0:col0+ncols_local] of shape (N,ncols_local,T,R).  Unsharded:
 * pass the same pointer twice.                                               */
int btf_set_data_gaussian(btf_ctx* ctx, const double* y_rows, const double* y_cols, int nreps);
/* Binomial data tuple (Y, N) of factor.py:437-460; same slab convention, R=1. */
int btf_set_data_binomial(btf_ctx* ctx, const double* succ_rows, const double* trials_rows,
                          const double* succ_cols, const double* trials_cols);
/* Quirks Q1/Q2: which row / column the cached likelihood weights
 * come from in compat=REFERENCE.  src_row[N], src_col[M] (global indices);
 * NULL = identity.  Only consulted by the weighted kernels.  Call after
 * btf_set_data_*; a source outside this ctx's shard that is not its declared halo
 * (btf_set_shard_halo) is BTF_EINVAL.                                           */
int btf_set_stale_sources(btf_ctx* ctx, const int32_t* src_row, const int32_t* src_col);

/* ---- Negative-Binomial counts (unsharded contexts) -----------------
 * counts: (N,M,T,nreps) C-order, NaN = missing; kept on the device.  The model is the
 * Binomial one on pseudo-data Y = sum_r y_r, N = sum_r (y_r + R) (factor.py:494-511, :552):
 * btf_nb_set_rate builds those (both layouts) from the rate R; afterwards btf_pg_draw /
 * btf_resample_W / btf_resample_V run as for btf_set_data_binomial.
 * shared[d] != 0: one R value is shared along dim d of (rows, cols, depth) (the reference's
 * `rdims`); R and cand are C-contiguous over the unshared dims.
 * btf_nb_loglik replaces the data-sized part of one random-walk MH step of
 * NegativeBinomialBTF._resample_R (factor.py:533-541): ll[e] = sum over replicates and shared
 * dims of lgamma(y+cand)-lgamma(cand)-lgamma(y+R)+lgamma(R)+(cand-R) log(1-p),
 * p = ilogit(clip(w.v,-10,10)), NaN observations dropped.  Synchronises.  When R is shared
 * along (cols, depth) and every count is an integer < 1024 the sum is evaluated from per-row
 * count histograms (built once at upload) and one pass per sweep for sum cnt*log(1-p): an MH
 * step then reads 8 KB per row instead of the count tensor.
 * Sharded contexts (btf_set_shard) pass the WHOLE (nrows, ncols, ndepth, nreps) tensor as well: the rate
 * update is a function of all of it and every rank computes it (same streams, same result), while
 * the augmented Binomial model is kept for the rank's row and column slabs only.              */
int btf_set_data_counts(btf_ctx* ctx, const double* counts, int nreps);
int btf_nb_loglik(btf_ctx* ctx, const double* R, const double* cand, const int32_t* shared3, double* ll);
int btf_nb_set_rate(btf_ctx* ctx, const double* R, const int32_t* shared3);
/* rng="device": the whole MH loop of NegativeBinomialBTF._resample_R (nsteps random-walk steps,
 * proposals and accept/reject from Philox) plus the pseudo-data rebuild, without a host round
 * trip.  R_in: start value (NULL: continue from the rate on the device).  Needs the histogram
 * form (see btf_nb_loglik); BTF_ESTATE otherwise.  btf_nb_get_rate fetches R (synchronises).   */
int btf_nb_mh(btf_ctx* ctx, uint64_t seed, int nsteps, double rpropstdev, double rstdev, const int32_t* shared3,
              const double* R_in);
int btf_nb_get_rate(btf_ctx* ctx, double* R, const int32_t* shared3);

/* ---- state ---------------------------------------------------------------- */
int btf_set_W(btf_ctx* ctx, const double* W);            /* (N,K)      */
int btf_get_W(btf_ctx* ctx, double* W);
int btf_set_V(btf_ctx* ctx, const double* V);            /* (M,T,K)    */
int btf_get_V(btf_ctx* ctx, double* V);
/* Tau2 NULL: keep the device copy (only lam2 / sigma2 move).  A non-NULL Tau2, or a lam2 that differs from the last
 * one, invalidates the precomputed prior band of the V half-sweep (prior_band_kernel runs again before the next one):
 * a host loop that re-sends unchanged hyper-parameters every sweep should pass NULL.  Reading the scalars back
 * (btf_get_scalars) invalidates nothing.                                                                       */
int btf_set_hyper(btf_ctx* ctx, const double* Tau2 /* (M,nD) */, double lam2, double sigma2);
/* Horseshoe+ local scales on the device (rng="device" only - the draws
 * come from Philox, not from the legacy numpy stream).  btf_set_tau_chain uploads the three
 * auxiliary levels Tau2_a/b/c (M,nD); btf_resample_Tau2 replaces the per-column loop of
 * BTF._resample_Tau2 (factor.py:134-141) for all columns at once, updating Tau2 and the chain
 * in place on the device, and returns lsum[j] = sum_r dsq[j,r]/Tau2_new[j,r] (the per-column
 * terms of the lam2 rate, factor.py:148-150) when lsum_out != NULL (synchronises).  With
 * device-resident scalars enabled the lam2 argument is ignored.                             */
int btf_set_tau_chain(btf_ctx* ctx, const double* Tau2_a, const double* Tau2_b, const double* Tau2_c);
int btf_get_tau(btf_ctx* ctx, double* Tau2, double* Tau2_a, double* Tau2_b, double* Tau2_c); /* a,b,c may be NULL */
int btf_resample_Tau2(btf_ctx* ctx, uint64_t seed, double lam2, double stability, double* lsum_out /* (M) or NULL */);
/* Device-resident scalars only: the NEXT btf_w_accum launch also runs this horseshoe+ update, as side workgroups
 * beside the stream (Tau2 | V, lam2 does not depend on nu2 / sigma2: the same conditionals as btf_resample_Tau2 after
 * the scalar draws; same Philox streams).  The lam2-rate terms stay on the device for btf_draw_lam2. */
int btf_queue_Tau2(btf_ctx* ctx, uint64_t seed, double stability);
/* ... and the NEXT drawing btf_draw_scalars launch also draws lam2 | rest (a second workgroup of that launch; the
 * lam2-rate terms must be on the device by then: a Tau2 update queued with btf_queue_Tau2, or btf_resample_Tau2). */
int btf_queue_lam2(btf_ctx* ctx, uint64_t seed, int compat);
/* (if no btf_draw_scalars launch takes it, the V accumulation launch of the next btf_resample_V carries it as a side workgroup)
 * nu2 | rest (which & 1) and sigma2 | rest (which & 2) as a side workgroup of the NEXT W accumulation launch (btf_w_accum /
 * btf_resample_W): possible on complete Gaussian data, unsharded, when the spectral V sampler of the previous half-sweep left
 * the per-column residual parts behind (BTF_OPT_FUSED_SWEEP) and nothing has touched W or V since.  *queued = 1: queued, the
 * W solve of this sweep will read the new values; 0: not possible now - draw them with btf_draw_scalars.  Replaces the
 * residual pass of factor.py:411-416 and the two gamma draws of genlasso.py:160-164 / factor.py:130-132. */
int btf_queue_scalars(btf_ctx* ctx, uint64_t seed, int which, double nu2_a, double nu2_b, double sigma2_a, double sigma2_b,
                      int32_t* queued);

/* n whole Gibbs sweeps (nu2, sigma2, Tau2 chain, lam2, W, V: GaussianBTF.resample, factor.py:306-311 over :112-128)
 * queued by one call: scalar-noise Gaussian data, device-resident scalars, unsharded.  Seeds: sweep s uses
 * seed_base + draws0 + 5 s + k, k = 1..5 for (Tau2, lam2, nu2/sigma2, W, V) - the sequence the Python driver
 * consumes (functionalmf_amd/factor.py:_next_seed), so both drivers walk the same chain.  Nothing is read back;
 * errors of the factorisations surface at the next btf_sync. */
int btf_gibbs_sweeps(btf_ctx* ctx, int nsweeps, uint64_t seed_base, uint64_t draws0, int compat, double nu2_a, double nu2_b,
                     double sigma2_a, double sigma2_b, double stability, double eps0, int attempts);
/* n W+V updates - _resample_W then _resample_V (factor.py:313-409), device normals - queued by ONE call: what a host loop
 * of btf_resample_W(NULL, seed_base + draws0 + 2 s + 1, compat); btf_resample_V(NULL, seed_base + draws0 + 2 s + 2, ...)
 * over s = 0 .. n-1 does, without a round trip through the caller between the launches (the same launches, the same
 * seeds: the same chain).  Unsharded contexts; no host synchronisation.                                              */
int btf_wv_steps(btf_ctx* ctx, int n, uint64_t seed_base, uint64_t draws0, int compat, double eps0, int attempts);
int btf_set_nu2(btf_ctx* ctx, double nu2);               /* Gaussian scalar noise variance */
/* Device-resident scalar hyper-parameters (rng="device" only, unsharded
 * contexts).  After btf_device_scalars(ctx,1) the half-sweep, prior-band and Tau2 kernels read
 * nu2 (Gaussian data), sigma2 and lam2 from a small device array instead of the host copies, and
 *   btf_draw_scalars: nu2 | rest (which&1; runs the residual reduction of factor.py:411-416 and the
 *                     inverse-gamma draw of genlasso.py:160-164) and sigma2 | rest (which&2;
 *                     factor.py:130-132) - priors InvGamma(a,b);
 *   btf_draw_lam2:    lam2, lam2_a | rest (factor.py:143-153; compat selects quirk Q3's rate), from
 *                     the per-column sums the preceding btf_resample_Tau2 left on the device
 * draw them there from Philox streams, so that a full Gibbs sweep queues without a host round
 * trip.  btf_set_scalars uploads values, btf_get_scalars (synchronises) returns
 * {nu2, sigma2, lam2, lam2_a, SSE of the last nu2 draw, sum W^2 of the last sigma2 draw}.      */
/* Sharded contexts: the residual sum of squares of nu2 | rest is a sum over the ranks' row slabs.  btf_draw_scalars
 * with which | 8 only reduces this rank's share into the device scalar out6[4] (btf_dev_hyp() + 4 doubles); the caller
 * all-reduces that one double over the ranks (RCCL, on btf_stream) and calls btf_draw_scalars with which | 16, which
 * draws from it - every rank the same value (same seed).  btf_set_global_nobs: the observation count over all
 * ranks (a constant of the data set).  sigma2, Tau2, lam2 need no exchange: W and V are replicated.            */
void* btf_dev_hyp(btf_ctx* ctx);
int btf_set_global_nobs(btf_ctx* ctx, double nobs);
int btf_set_scalar_slot(btf_ctx* ctx, int slot, double value);  /* one entry of the btf_get_scalars array (staged exchanges) */
int btf_device_scalars(btf_ctx* ctx, int enable);
int btf_set_scalars(btf_ctx* ctx, double nu2, double sigma2, double lam2, double lam2_a);
int btf_get_scalars(btf_ctx* ctx, double* out6);
int btf_draw_scalars(btf_ctx* ctx, uint64_t seed, int which, double nu2_a, double nu2_b, double sigma2_a, double sigma2_b);
int btf_draw_lam2(btf_ctx* ctx, uint64_t seed, int compat);
int btf_set_omega(btf_ctx* ctx, const double* omega_rows, const double* omega_cols); /* Binomial: PG draws, slabs as data */
int btf_get_omega(btf_ctx* ctx, double* omega_rows);     /* (nrows_local,M,T) */

/* ---- half-sweeps ----------------------------------------------------------
 * btf_resample_W replaces the body of GaussianBTF._resample_W (factor.py:313-362)
 * [and BinomialBTF._resample_W :437-440]: for every local row i, d=min(i+1,K):
 *   Q_i = sum_{j,t} c_ijt v_jt v_jt' + I/sigma2,  m_i = sum c_ijt ybar_ijt v_jt,
 *   W[i,:d] = Q_i^-1 m_i + L_i^-T z_i.
 * z: host array of the sum_i min(i+1,K) standard normals of ALL rows in row
 * order (the legacy-RNG stream of factor.py:361), or NULL to draw them on the
 * device (Philox4x32-10 keyed by `seed`).                                     */
/* btf_w_accum queues the first phase of btf_resample_W alone (the streaming accumulation, which
 * depends on the data and on V only); the next btf_resample_W then goes straight to the solve.
 * Between the two, btf_draw_scalars(which | 4) can take the residual sum of squares of nu2 | rest
 * from the same partials instead of a pass of its own over the data.                          */
int btf_w_accum(btf_ctx* ctx, int compat);
int btf_resample_W(btf_ctx* ctx, const double* z, uint64_t seed, int compat);
/* btf_resample_V replaces GaussianBTF._resample_V (factor.py:364-409) including
 * its call into sample_mvn_from_precision (fast_mvn.py:35-47, :62-68): for every
 * local column j the (K*T)x(K*T) precision  kron(W,I)'C kron(W,I) + I_K (x)
 * Delta' diag(1/(lam2 Tau2_j)) Delta  is formed in depth-major order (t,k), factored
 * as a block-banded LDL' in the declared elimination order P (btf_get_V_order), and
 * V[j] = Q^-1 mu + P' L^-T z  is drawn.
 * z: host (M, K*T) normals, row j for column j, indexed in the factor's
 * elimination order, or NULL for device Philox.  eps0/attempts: the
 * force_psd jitter schedule (eps0*10^a added cumulatively, <= attempts).      */
int btf_resample_V(btf_ctx* ctx, const double* z, uint64_t seed, int compat,
                   double eps0, int attempts);
int btf_get_V_attempts(btf_ctx* ctx, int32_t* tries /* (ncols_local) */);
/* The elimination order P the V half-sweep of this context uses (after btf_set_data_*):
 * order[i] = depth-major index t*K+k of the i-th pivot, i = 0..K*T-1.  Identity for the
 * single-chain kernels; for the default twisted kernel: depths 0..ts-1 ascending, then depths
 * T-1..ts+tf+1 descending (k descending), then the separator depths ts..ts+tf.  z[j][i] is
 * the normal that multiplies pivot i (this is CHOLMOD's P() in fast_mvn.py:44).            */
int btf_get_V_order(btf_ctx* ctx, int32_t* order /* (K*T) */);
/* BTF_SAMPLER_SPECTRAL (complete Gaussian data: every depth of every column has the same K x K
 * likelihood block G = (R/nu2) W'W, factor.py:396-398 with constant weights).  In the reference's own
 * k-major ordering of the unknowns (factor.py:409) Q_j = G (x) I_T + I_K (x) P_j with P_j the prior
 * precision of factor.py:404-405; with G = U diag(g) U' the draw is
 *   V[j] = Q_j^-1 mu + (U (x) I_T) blockdiag_k(L_k^-T D_k^-1/2) z,   g_k I + P_j = L_k D_k L_k',
 * z[j][k*T + t] multiplying pivot t of system k - a square root of Q_j^-1 like fast_mvn.py:44's
 * P' L^-T, same mean term, same jitter schedule (the shift is added to every g_k).  U: eigenvectors in
 * ascending order of eigenvalue, each with its largest-magnitude entry positive.
 * btf_get_V_sampler reports the BTF_SAMPLER_* the next V half-sweep of this context will run.  */
/* The eigen-solver the spectral sampler uses, stand-alone (one-wave cyclic Jacobi, K <= 10): sums `nparts`
 * packed-lower K x K matrices parts[p][r(r+1)/2 + c], returns out[0..K-1] eigenvalues ascending,
 * out[K + r*K + c] component r of eigenvector c (largest-magnitude entry positive), out[K+K*K] sweeps. */
int btf_sym_eig(int device, int nembeds, int nparts, const double* parts, double* out, const double* warm_from);

/* Measurement aid: rate (GB/s) of a plain streaming read of `bytes` of device memory, averaged over `reps`
 * launches - the practical read ceiling bench.py reports beside the spec peak (roofline.read_ceiling_GBs). */
int btf_read_probe(int device, size_t bytes, int reps, double* gb_per_s);
/* Which form of the likelihood part the half-sweeps of this context run (after btf_set_data_*):
 *   BTF_LIK_COMPLETE      complete Gaussian data: K sums per cell, one shared Gram (factor.py:347-348, :392-393)
 *   BTF_LIK_WEIGHTED      per-cell weights (missing replicates, Polya-Gamma omegas): K + K(K+1)/2 sums per cell
 *   BTF_LIK_CURVE_COUNTS  replicate counts constant along the depth axis: the complete-data stream plus per-row /
 *                         per-column corrections (BTF_OPT_CURVE_COUNTS) - the same conditionals as the weighted form */
enum { BTF_LIK_COMPLETE = 0, BTF_LIK_WEIGHTED = 1, BTF_LIK_CURVE_COUNTS = 2 };
int btf_get_likelihood_form(btf_ctx* ctx, int32_t* form);
/* Checkpoint / resume (the reference keeps no state between runs - genlasso.py:57-66 returns the samples; SURVEY
 * section 5): besides the caller's seeds, the rng="device" draws of W and V are keyed by how many W / V half-sweeps
 * this context has run.  A chain continued in another context gets the same draws after handing these two over.
 * btf_set_draw_counters also forgets the spectral sampler's eigen warm start (the next V half-sweep solves the K x K
 * eigenproblem from scratch), so a chain that calls it with its own counters and one restored elsewhere continue
 * identically. */
int btf_get_draw_counters(btf_ctx* ctx, uint64_t* w_half_sweeps, uint64_t* v_half_sweeps);
int btf_set_draw_counters(btf_ctx* ctx, uint64_t w_half_sweeps, uint64_t v_half_sweeps);
/* Algorithmic bytes per cell one accumulation launch streams for the bound data: 8 (linear statistic alone: complete data,
 * curve counts), 9 (+ replicate counts as bytes; or Binomial pseudo-data kappa = Y - N/2 as bytes + f64 weights when
 * the counts are integers up to 127), 16 (f64 statistic + f64 weights).  bench.py's roofline uses it. */
int btf_get_accum_bytes_per_cell(btf_ctx* ctx, double* bytes);

/* warm_from: NULL (cyclic Jacobi from the identity) or the `out` of a nearby matrix, refined by the
 * Ogita-Aishima iteration (the path the sampler takes from the second sweep on; out[K+K*K] = 0 then). */
int btf_set_option(btf_ctx* ctx, int option, int value);
int btf_get_V_sampler(btf_ctx* ctx, int32_t* which);

/* Residual sum of squares and observation count over the LOCAL rows: the two
 * numbers GaussianBTF._resample_nu2 (factor.py:411-416, genlasso.py:157-160)
 * reduces the whole tensor for.  Synchronises.                                */
int btf_sse(btf_ctx* ctx, double* sse, double* nobs);
/* The same in two halves: btf_sse_begin enqueues the reduction (and a copy of W) without
 * waiting; btf_sse_end synchronises, returns the two numbers and, if W_out != NULL, the
 * (N,K) factor as it was when btf_sse_begin was called.  Lets the host queue a whole sweep. */
int btf_sse_begin(btf_ctx* ctx);
int btf_sse_end(btf_ctx* ctx, double* sse, double* nobs, double* W_out);
/* omega_ijt ~ PG(Ntrials_ijt, w_i . v_jt) on the device: replaces the
 * pypolyagamma call at factor.py:459 (own RNG: Philox keyed by seed).         */
int btf_pg_draw(btf_ctx* ctx, uint64_t seed);

/* Stand-alone batch of PG(b_i, psi_i) draws from the same device sampler (used to
 * validate its distribution; element i uses the Philox stream (seed, i)).      */
int btf_pg_batch(int device, int64_t n, const double* b, const double* psi, uint64_t seed, double* out);
/* the same with the sampler chosen by `mode`: 0 / 1 / 2 as BTF_OPT_PG_EXACT; 3: the f64 Devroye sampler for every
 * count below 200 (the round-2 exact kernel: the reference the flat sampler is tested against); 4: as 1 with every
 * trip of the flat sampler repeated in f64 (validation of its fallback: same decisions, same draws up to f32 rounding) */
int btf_pg_batch_mode(int device, int64_t n, const double* b, const double* psi, uint64_t seed, int mode, double* out);

int btf_sync(btf_ctx* ctx); /* waits; returns BTF_ENOTPD if a step failed since the last sync */
/* Host-only self-test of the index arithmetic behind the kernels' tables, LDS layouts, elimination orders and chunk maps
 * (no GPU, no HIP call): 0, or the source line of the first failed check.  scripts/asan_host.sh runs it on a build of the
 * host side with -fsanitize=address,undefined (the reference has no native code to sanitise; SURVEY section 5 aux). */
int btf_host_selftest(void);

/* ---- structured-Gaussian sampler (the fast_mvn equivalent, stand-alone) ----
 * Batched draw  x_b = Q_b^-1 mu_b + L_b^-T z_b,  L_b L_b' = Q_b (+ jitter), for
 * symmetric banded precisions given as lower band by columns:
 * band[b][c][a] = Q_b[c+a, c], a = 0..bw.  mu_part and/or z may be NULL (zero /
 * device Philox).  Replaces sample_mvn_from_precision(Q, mu_part=..., sparse=True)
 * (fast_mvn.py:10-74) for banded Q in the given ordering.                     */
int btf_mvn_banded(int device, int batch, int n, int bw, const double* band,
                   const double* mu_part, const double* z, uint64_t seed,
                   double eps0, int attempts, double* x_out, int32_t* tries_out);

/* Dense forms of fast_mvn (the sparse=False branches: sample_mvn_from_precision fast_mvn.py:49-60,
 * sample_mvn_from_covariance fast_mvn.py:126-142, reached through the dispatcher sample_mvn :145-179).
 * A: batch row-major n x n matrices (only the lower triangle is read), n <= 1024.
 *   form & BTF_MVN_PRECISION: A is a precision Q:  x = Lt^-1 z + Q^-1 mu_part   (or + mu),  L L' = Q
 *   otherwise A is a covariance S:                 x = L z + S mu_part          (or + mu),  L L' = S
 *   form & BTF_MVN_FACTOR: A already IS the lower Cholesky factor L (chol_factor=True)
 * mu / mu_part: [batch][n] or NULL (at most one).  z: [batch][n] standard normals (the reference draws
 * np.random.normal(size=n) after the factorisation) or NULL: Philox(seed).  Not positive definite: eps0 is added to
 * the diagonal cumulatively, x10 per retry, at most `attempts` times (fast_mvn.py:62-68, :133-139); then
 * BTF_ENOTPD with the batch index in the message (the reference's dense branches raise LinAlgError / warn forever).
 * tries_out: [batch] retries used, or NULL. */
enum { BTF_MVN_PRECISION = 1, BTF_MVN_FACTOR = 2 };
int btf_mvn_dense(int device, int batch, int n, const double* A, int form, const double* mu, const double* mu_part,
                  const double* z, uint64_t seed, double eps0, int attempts, double* x_out, int32_t* tries_out);

/* ---- elliptical slice sampling for non-conjugate likelihoods -----------------
 * Replaces NonconjugateBayesianTensorFiltering._resample_W / _resample_V (factor.py:567-590): a prior draw nu
 * (sample_mvn_from_precision on the packed prior precision of factor.py:155-195 - for V the banded sampler with
 * the likelihood switched off, same declared order as btf_resample_V with BTF_SAMPLER_BANDED) and the slice loop
 * of elliptical_slice_ (elliptical_slice.py:59-124).  The likelihood callback of the reference becomes a device
 * likelihood over the statistics btf_set_data_gaussian hoisted (counts y, NaN = missing):
 *   link 0  Poisson, log link:       sum_cells  S1 (w.v) - cnt exp(w.v)
 *   link 1  Poisson, identity link:  sum_cells  S1 log(w.v) - cnt (w.v),  -inf where w.v <= 0
 *   link 2  Bernoulli / Binomial, logit link (S1 successes of cnt trials):  S1 (w.v) - cnt log(1 + exp(w.v))
 *   link 3  Gaussian, identity link, known variance s2 (parameter 1/s2):     (S1 (w.v) - cnt (w.v)^2 / 2) / s2
 *   link 4  Negative-Binomial, logit link, known rate r (parameter r):      S1 (w.v) - (S1 + cnt r) log(1 + exp(w.v))
 * - every one a function of the hoisted statistics S1 = sum_r y, cnt = observed replicates; the state-independent terms
 * (- sum lgamma(y+1), the Gaussian's - sum y^2 / 2 s2 - n log(2 pi s2) / 2, the Negative-Binomial's log binomial
 * coefficients) are left to the caller.  Parameters: btf_set_likelihood_param.  what: 0 = W, 1 = V.  Unsharded contexts.
 *   link 5  gamma grid (the dose-response likelihood, doseresponse/empirical_bayes.py:9-33): an empirical-Bayes mixture of
 *           gammas, component g = (shape a_g, scale s_g, weight p_g; weights used as given), per cell with observed
 *           replicates y_r:  log sum_g p_g prod_r Gamma(y_r; a_g, scale = s_g (w.v))
 *             = logsumexp_g [log p_g + (a_g - 1) L - S1 / (s_g w.v) - cnt (a_g log(s_g w.v) + lgamma a_g)],  L = sum_r log y
 *           - the COMPLETE value (nothing is left to the caller).  A cell without observations contributes log sum_g p_g
 *           (the reference's nansum; 0 for normalised weights); w.v <= 0 on an observed cell gives -inf (a deliberate
 *           deviation: the reference's nansum would count the NaN as unobserved).  Needs the table
 *           (btf_set_likelihood_table: 1 <= G <= 128, finite shape > 0, scale > 0, weight >= 0, not all zero; else
 *           BTF_EINVAL) and L (btf_set_data_logsum, after btf_set_data_gaussian with the same Y: every observed y > 0,
 *           else BTF_EINVAL); btf_ess_eval / btf_ess_run / btf_gass_begin / btf_gass_run return BTF_ESTATE without them.
 *           L is allocated for this family only, in both layouts of S1.
 *
 * Host-driven form (rng="host": the uniforms come from the caller's generator, so a seeded chain walks the
 * reference's path): btf_ess_begin saves the current state x0 and draws nu (z: the normals of
 * sample_mvn_from_precision, W: sum_i min(i+1,K), V: (M, K*T) in the declared order; NULL = device Philox);
 * btf_ess_eval(theta, current=0) sets the state to x0 cos(theta) + nu sin(theta) and returns its log-likelihood
 * (current=1: of the state as it stands); when the caller stops, the state holds the last proposal, exactly what
 * elliptical_slice_ returns.  Synchronises.
 * link = BTF_ESS_HOST_LIKELIHOOD (-1): the likelihood is the CALLER's (the reference's Python callback
 * `loglikelihood(W, V, data)`, factor.py:567-612): btf_ess_begin draws nu as above (it needs no data on the device),
 * btf_ess_eval only forms the proposal in W (resp. V) - the caller reads it back (btf_get_W / btf_get_V), evaluates its
 * function and decides; *ll = 0.
 *
 * Device-driven form: btf_ess_run = begin + at most max_rounds proposal / likelihood / decision rounds queued on the
 * stream, uniforms from Philox, nothing read back.  mode 0: one slice over all of W (resp. V), as the reference;
 * mode 1: one slice per row of W (resp. per column of V) - the rows are conditionally independent given V - all
 * brackets shrinking in lockstep, one proposal per row per round.  btf_ess_info (synchronises): chains that used up
 * max_rounds (they keep the current state) and the log-likelihood the first chain ended on.                      */
#define BTF_ESS_HOST_LIKELIHOOD (-1)
int btf_set_likelihood_param(btf_ctx* ctx, int link, double parameter);   /* links 3 (1 / variance) and 4 (rate); > 0 */
int btf_set_likelihood_table(btf_ctx* ctx, int link, const double* shape, const double* scale, const double* prob, int G);   /* link 5 */
int btf_set_data_logsum(btf_ctx* ctx, const double* y_rows, const double* y_cols, int nreps);   /* link 5: L = sum_r log y */
int btf_ess_begin(btf_ctx* ctx, int what, const double* z, uint64_t seed, double eps0, int attempts);
int btf_ess_eval(btf_ctx* ctx, int what, double theta, int current, int link, double* ll);
int btf_ess_run(btf_ctx* ctx, int what, int link, int mode, const double* z, uint64_t seed, int max_rounds,
                double eps0, int attempts);
int btf_ess_info(btf_ctx* ctx, int32_t* unfinished, double* ll_first);

/* ---- generalized analytic slice sampling (gass.py:13-130) for the constrained non-conjugate model
 * (ConstrainedNonconjugateBayesianTensorFiltering._resample_W / _resample_V, factor.py:665-855): every row of W (what = 0)
 * or every column of V (what = 1) is one chain, all chains advance together.  Likelihood: the device likelihoods
 * of btf_ess_* (links 0..5) on the statistics of btf_set_data_gaussian (link 5: and btf_set_data_logsum).  Unsharded contexts.
 *
 * btf_gass_set_constraints: cons [J][T+1], row q = (Cons_q, bound_q): every curve tau_ij = (w_i . v_jt)_t must satisfy
 *   Cons_q . tau_ij >= bound_q (the reference's `Constraints`, factor.py:910); row_cons [nrc][K+1]: fixed constraints on
 *   every row of W (`Row_constraints`), or NULL.
 * btf_gass_begin: x0 <- current state, v <- prior draw (W: sigma z on the free entries; V: the banded sampler with the
 *   likelihood off - z / seed as btf_ess_begin), slice heights ll(x0) + log u (u: [nchains] uniforms, or NULL: Philox),
 *   and the constraint analysis: which of the 10000 grid angles of gass.py:68 are valid for every chain.
 *   pick_ngrid > 0: the device also draws the candidate angles (<= 128): all valid ones, or pick_ngrid of them
 *   without replacement; linspace(-pi, pi, pick_ngrid) when no constraint restricts the ellipse (gass.py:81-83).
 * btf_gass_grid: info [nchains][2] = {valid angles, 1 if unrestricted}; mask [nchains][10000] bytes, slice [nchains],
 *   cur_ll [nchains] (each optional).
 * btf_gass_eval: log-likelihood of every candidate, ll_out [nchains][128] (-inf beyond a chain's count).  thetas
 *   [nchains][128] + ntheta [nchains]: the caller's candidates (host-driven: the reference's np.random.choice), or NULL:
 *   the device's own.
 * btf_gass_commit: x = x0 cos(theta_c) + v sin(theta_c) for chains with keep[c] == 0 (host-driven selection).
 * btf_gass_select: one candidate above the slice per chain, uniformly (Philox); none: the state stays (gass.py:121-128).
 * btf_gass_run = begin(pick) + eval + select, nothing read back. */
int btf_gass_set_constraints(btf_ctx* ctx, const double* cons, int J, const double* row_cons, int nrc);
int btf_gass_begin(btf_ctx* ctx, int what, int link, const double* z, const double* u, uint64_t seed, double eps0, int attempts,
                   int pick_ngrid);
int btf_gass_grid(btf_ctx* ctx, int what, int32_t* info, uint8_t* mask, double* slice, double* cur_ll);
int btf_gass_eval(btf_ctx* ctx, int what, const double* thetas, const int32_t* ntheta, double* ll_out);
int btf_gass_commit(btf_ctx* ctx, int what, const double* theta, const int32_t* keep);
int btf_gass_select(btf_ctx* ctx, int what, uint64_t seed, int32_t* naccept_out);
int btf_gass_run(btf_ctx* ctx, int what, int link, uint64_t seed, int ngrid, double eps0, int attempts);
/* btf_gass_set_ep: EP-centred proposals (ep_approx, factor.py:677-688 and :771-793).  mu, sigma [N][M][T] (Mu_ep and
 * Sigma_ep, finite, sigma > 0; NULL, NULL clears).  While set, btf_gass_begin draws the proposal from N(0, Q^-1) with Q the
 * likelihood-weighted precision (rows: sum p v v' + I_d / sigma2; columns: kron(I_K, Delta' Lambda Delta) + X' Sigma X,
 * p = 1 / Sigma_ep^2; z in the same layouts as the plain update, columns in the twisted order), centres the ellipse
 * on mu = Q^-1 X' Sigma Mu_ep, and every likelihood it reports (cur_ll, slice, ll_out) is the corrected
 * ll - sum_cells log N(tau; Mu_ep, Sigma_ep) over every cell of the chain; commit and select write
 * x0 cos + v sin + mu.  The kernels are counted under BTF_K_ESS. */
int btf_gass_set_ep(btf_ctx* ctx, const double* mu, const double* sigma);
/* btf_gass_set_row_features: binary row features of the constrained model (doseresponse/fit.py:40-50, :102-145).  codes
 * [N][F]: 0, 1 or 2 (missing); U [F][K]: the feature embeddings (finite).  F = 0 clears.  While set,
 *   - the row chains (what = 0) add  sum_f x_if log(w_i . u_f) + (1 - x_if) log(1 - w_i . u_f)  (missing pairs and pairs
 *     outside [0, 1] add nothing) to cur_ll, the slice and every candidate's ll, for every likelihood family and with
 *     or without btf_gass_set_ep, and their constraints gain the 2F rows (u_f, 0), (-u_f, -1) behind row_cons, rebuilt
 *     from the current U at every btf_gass_begin;
 *   - what = 2 is accepted by btf_gass_begin / grid / eval / commit / select / run: one chain per feature, x0 = u_f,
 *     v = z ([F][K], or NULL: Philox), prior N(0, I_K), constraints 0 <= w_i . u <= 1 for every row, likelihood the same
 *     term summed over the rows; u, info, mask, slice, cur_ll, thetas, ll_out, theta, keep are indexed by feature; link,
 *     eps0 and attempts are ignored.  Without features what = 2 returns BTF_ESTATE.
 * btf_gass_set_U / btf_gass_get_U: U [F][K] (BTF_ESTATE without features).  Unsharded contexts, nembeds <= 10.  The
 * kernels are counted under BTF_K_ESS. */
int btf_gass_set_row_features(btf_ctx* ctx, int F, const uint8_t* codes, const double* U);
int btf_gass_set_U(btf_ctx* ctx, const double* U);
int btf_gass_get_U(btf_ctx* ctx, double* U);

/* ---- posterior summaries (stateless) --------------------------------
 * Mean and percentiles over the kept samples of f(w_s[i] . v_s[j,t]) for every cell: what the
 * reference's example scripts compute on the host as einsum('znk,zmtk->znmt', Ws, Vs).mean(0) /
 * np.percentile(., q, axis=0) (examples/gaussian_tensor_filtering.py:82-85), without materialising
 * the (S,N,M,T) tensor.  Ws (S,N,K), Vs (S,M,T,K) as run_gibbs returns them; transform 0 identity,
 * 1 ilogit, 2 square; q in [0,100], numpy's default linear interpolation; mean_out (N,M,T),
 * q_out (nq,N,M,T).  nsamples <= 16384.                                                      */
int btf_posterior_summary(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds,
                          const double* Ws, const double* Vs, int transform, const double* q, int nq,
                          double* mean_out, double* q_out);

/* ---- posterior curve functionals (csrc/btf_functionals.h; replaces doseresponse/feature_importance.py:40) ---------------
 * Per kept sample s and curve (i,j), m_t = f(w_i^s . v_jt^s) over the depth coordinates x (T, strictly increasing) is
 * reduced to one number per requested functional, and the S numbers of a curve to mean, variance (ddof 1; nan below two
 * values), percentiles (numpy's linear rule), and the share above `exceed`.  Functional codes (which[], distinct):
 *   0 auc: trapezoid rule  1 max  2 min  3 argmax  4 argmin: x at the first occurrence  5 rise: sum of the positive steps
 *   6 crossing: where m first crosses `level` (linear interpolation; x[0] if m_0 == level; undefined when it never does).
 * An undefined crossing is left out of mean / var / prob, counts as +inf in the percentiles (right-censored), and a
 * percentile that touches a non-finite order statistic is nan; defined_out (N,M) = share of samples with a crossing.
 * Outputs, each NULL or, with nw = nwhich in the order of which[]: mean_out, var_out, prob_out (nw,N,M); q_out (nw,nq,N,M);
 * curves_out (nw,ncurves,S): the raw values of the curves[] = (i,j) pairs in sample order (nan = undefined);
 * pointwise_out (nw,S,N,M).  transform as btf_posterior_summary.  ndepth >= 2, nsamples <= 8192 (BTF_EINVAL beyond).
 * fp64, no floating-point atomics, every sum in a fixed order: two calls return identical bits, whatever the launch
 * geometry and wherever the states come from.  btf_collect_functionals reads the first nsamples collected slots without
 * an upload and touches none of the sampler's state; its launches are counted under BTF_K_CRITERIA.  Synchronous.      */
int btf_posterior_functionals(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                              const double* Vs, int transform, const int* which, int nwhich, const double* x, double level,
                              double exceed, const double* q, int nq, const int* curves, int ncurves, double* mean_out,
                              double* var_out, double* q_out, double* defined_out, double* prob_out, double* curves_out,
                              double* pointwise_out);
int btf_collect_functionals(btf_ctx* ctx, int nsamples, int transform, const int* which, int nwhich, const double* x,
                            double level, double exceed, const double* q, int nq, const int* curves, int ncurves,
                            double* mean_out, double* var_out, double* q_out, double* defined_out, double* prob_out,
                            double* curves_out, double* pointwise_out);

/* ---- simultaneous credible bands per curve (csrc/btf_bands.h) -------------------------------------------------------------
 * A band that holds the WHOLE curve m_s(t) = f(w_i^s . v_jt^s) over the used depths with probability level / 100 among the
 * kept samples, where the percentiles of btf_posterior_summary hold each cell alone.  need = ceil(level / 100 * nsamples);
 * depths: ndepth flags (non-zero: the band is simultaneous over this depth; at least one) or NULL for all.
 * method 0 (supt): center_out, scale_out (N,M,T) = mean and sd (ddof 1) over the samples; D_s = max over the used depths with
 *   scale > 0 of |m_s - center| / scale (0 without one); crit_out (N,M) = the need-th smallest D_s (an order statistic, not
 *   interpolated); lower_out, upper_out (N,M,T) = center -+ crit * scale at every depth; inside_out (N,M) = #{s : D_s <= crit}
 *   / S >= need / S.  pointwise_inside_out is not written.  nsamples <= 8192.
 * method 1 (rank): per cell lo_s = #{s' : m_s' < m_s} and hi_s with >; depth_s = min over the used depths of min(lo_s, hi_s);
 *   crit_out (N,M) = k, the largest integer with #{s : depth_s >= k} >= need; lower_out, upper_out = the k-th and the
 *   (S-1-k)-th order statistic (0-based) of every cell; inside_out = #{s : depth_s >= k} / S; pointwise_inside_out (N,M) the
 *   same with k_pw = floor((1 - level / 100) / 2 * S): the share of kept curves wholly inside the pointwise band of the same
 *   level.  center_out and scale_out are not written.  nsamples <= 4096.
 * stat_out (ncurves,S): the raw D_s or depth_s of the curves[] = (i,j) pairs in sample order.  Outputs may be NULL.
 * transform as btf_posterior_summary; nsamples >= 2, ndepth >= 1, level in (0, 100), nembeds 1..10 (BTF_EINVAL otherwise).
 * scratch_bytes: the cap of the staging buffer, which holds whole columns (0: the default of the functionals; at least
 * one column is staged).  fp64, no floating-point atomics, every sum in a fixed order: two calls return
 * identical bits, whatever the chunking and wherever the states come from.  btf_collect_bands reads the first nsamples
 * collected slots without an upload and touches none of the sampler's state; its launches are counted under
 * BTF_K_CRITERIA.  Synchronous.                                                                                          */
int btf_posterior_bands(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                        const double* Vs, int transform, int method, double level, const int* depths, const int* curves,
                        int ncurves, double* center_out, double* scale_out, double* lower_out, double* upper_out,
                        double* crit_out, double* inside_out, double* pointwise_inside_out, double* stat_out,
                        long long scratch_bytes);
int btf_collect_bands(btf_ctx* ctx, int nsamples, int transform, int method, double level, const int* depths,
                      const int* curves, int ncurves, double* center_out, double* scale_out, double* lower_out,
                      double* upper_out, double* crit_out, double* inside_out, double* pointwise_inside_out, double* stat_out,
                      long long scratch_bytes);

/* ---- posterior ranking (csrc/btf_ranking.h) ----------------------------------------------------------------------------
 * The rank of every curve within its row (along 0: the ncols columns of a row are one group) or its column (along 1: the
 * nrows rows of a column), per kept sample, by the value of ONE functional `which` (the codes above; x, level, transform as
 * btf_posterior_functionals): rank = 1 + the number of members of the group before it in the order (value, index),
 * ascending or (descending 1) descending in the value; ties go to the smaller index, an undefined value (nan) ranks after
 * every defined one in both orders.  Over the samples, per curve, all in integers: A = sum r, B = sum r^2,
 * C_k = #{s : r <= top[k]} (top: ntop = 1..8 distinct integers >= 1), then one fp64 division each:
 *   expected_out (N,M) = A / S;  var_out (N,M) = (S B - A A) / (S (S - 1)), 0 when S = 1;  ptop_out (ntop,N,M) = C_k / S.
 * ranks_out (S,N,M) int32 or NULL: the ranks themselves.  pairs: npairs (i,j,i2,j2) rows, curves anywhere in the tensor:
 * prob_less_out (npairs) = #{s : f_s(i,j) < f_s(i2,j2)} / S and prob_defined_out = #{s : both defined} / S (a sample with an
 * undefined value counts for neither).  The values are those of btf_posterior_functionals bit for bit, and everything
 * after them is integer: two calls return identical bits whatever the geometry.  Groups of at most 4096 members and
 * nsamples <= 8192 (BTF_EINVAL beyond), ndepth >= 2.  scratch_bytes: the cap of the staging buffer, which holds whole
 * samples (0: the default of the functionals; at least one sample is staged).  btf_collect_ranking reads the first nsamples
 * collected slots without an upload and touches none of the sampler's state; its launches are counted under
 * BTF_K_CRITERIA.  Synchronous.                                                                                          */
int btf_posterior_ranking(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                          const double* Vs, int transform, int which, const double* x, double level, int along, int descending,
                          const int* top, int ntop, const int* pairs, int npairs, double* expected_out, double* var_out,
                          double* ptop_out, int* ranks_out, double* prob_less_out, double* prob_defined_out,
                          long long scratch_bytes);
int btf_collect_ranking(btf_ctx* ctx, int nsamples, int transform, int which, const double* x, double level, int along,
                        int descending, const int* top, int ntop, const int* pairs, int npairs, double* expected_out,
                        double* var_out, double* ptop_out, int* ranks_out, double* prob_less_out, double* prob_defined_out,
                        long long scratch_bytes);

/* ---- posterior similarity (csrc/btf_similarity.h) ------------------------------------------------------------------------
 * The distance between the fitted surfaces mu = W V' of two rows (along 0: E = nrows entities, each compared over the
 * columns `over` and every depth) or two columns (along 1: E = ncols, over the rows `over`), per kept sample, and every
 * entity's neighbours.  over: nover distinct indices, or NULL with nover 0 for all; n = (members of over) x ndepth cells.
 * metric 0 (rms): d = sqrt(d2), n d2(e,f) = sum_t delta_t' Q delta_t with Q the K x K sum of the members' outer products
 * and delta the difference of the entities' embeddings - the difference first, so identical embeddings give exactly 0, and
 * d2 is clamped at 0.  metric 1 (cosine): d = 1 - <e,f> / sqrt(|e|^2 |f|^2), the ratio clamped to [-1, 1] and taken as 0
 * where the product of the squared norms is 0.  d(e,f) and d(f,e) are the same bits and d(e,e) = 0 with both metrics.
 * Over the samples: mean_out, var_out (E,E; ddof 1, nan when nsamples = 1) and q_out (nq,E,E), numpy's linear percentiles,
 * of d.  Neighbours: within every (sample, e) the E entities are ranked by ascending key - d2 for rms, d for cosine - ties
 * to the smaller index, e itself last; expected_out, rank_var_out (E,E) and pnear_out (nnearest,E,E) are the integer
 * summaries of btf_posterior_ranking with nearest (1..8 distinct integers >= 1) in the place of top.  pairs: npairs (e,f)
 * rows; pair_out (nsamples,npairs) their distances.  dist_out (nsamples,E,E) or NULL: every distance.  nembeds 1..10,
 * E <= 4096 and nsamples <= 8192 (BTF_EINVAL beyond).  scratch_bytes: the cap of the staging buffer, which holds whole
 * entities with all samples and partners (0: the default of the functionals; at least one entity is staged); the tiling
 * cannot change a bit.  fp64, no floating-point atomics, every sum in a fixed order.  btf_collect_similarity reads the
 * first nsamples collected slots without an upload and touches none of the sampler's state; its launches are counted under
 * BTF_K_CRITERIA.  Synchronous.                                                                                          */
int btf_posterior_similarity(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                             const double* Vs, int along, int metric, const int* over, int nover, const double* q, int nq,
                             const int* nearest, int nnearest, const int* pairs, int npairs, double* mean_out, double* var_out,
                             double* q_out, double* expected_out, double* rank_var_out, double* pnear_out, double* pair_out,
                             double* dist_out, long long scratch_bytes);
int btf_collect_similarity(btf_ctx* ctx, int nsamples, int along, int metric, const int* over, int nover, const double* q,
                           int nq, const int* nearest, int nnearest, const int* pairs, int npairs, double* mean_out,
                           double* var_out, double* q_out, double* expected_out, double* rank_var_out, double* pnear_out,
                           double* pair_out, double* dist_out, long long scratch_bytes);

/* ---- posterior feature association (csrc/btf_assoc.h) -------------------------------------------------------------------
 * The association between a row feature's probability and ONE curve functional across the rows, per kept sample: what
 * doseresponse/feature_importance.py:39-54 computes on posterior means only.  For kept sample s, feature f (Us (S,F,K):
 * the feature embeddings u_f^s) and column j, with y_i = the functional `which` of curve (i,j) (codes, x, level, transform
 * as btf_posterior_functionals; the same values bit for bit), x_i = w_i^s . u_f^s, I = {i : y_i defined}, n = |I| and the
 * centred sums Sxx, Syy, Sxy over I:   r = Sxy / sqrt(Sxx Syy),  slope = Sxy / Sxx,  defined iff n >= 3, Sxx > 0, Syy > 0.
 * x is linear in w, so the sums follow from per-(sample, column) moments of W (3 + 2K + K(K+1)/2 doubles each, kept on the
 * device for the call) and the (S,F,M,N) product is never formed.  stats: nstats = 1..2 distinct codes, 0 r, 1 slope.
 * Outputs over the DEFINED samples, each NULL or, with ns = nstats in the order of stats[]: mean_out, var_out (ddof 1; 0 with
 * one defined sample), prob_out = share of defined samples with a value > 0 (ns,F,M), nan where no sample is defined;
 * q_out (ns,nq,F,M): numpy's linear percentiles of the defined samples; defined_out (F,M) = defined samples / S;
 * nmean_out (M) = mean_s n; values_out (ns,npairs,S): the raw statistics of the pairs[] = (f,j) rows, nan where undefined.
 * of_means_out (5,F,M) or NULL: the plug-in table r, slope, intercept, stderr = sqrt((1 - r^2) Syy / Sxx / (n - 2)), n of the
 * regression of gbar(:,j) = mean over the defined samples of y on Pbar(:,f) = mean_s W_s U_s' over the rows with a defined
 * gbar (scipy.stats.linregress's numbers), with sdx_out (F) and sdy_out (M), the ddof-0 standard deviations of Pbar(:,f)
 * over all rows and of gbar(:,j) over its defined rows.
 * fp64, no floating-point atomics, every sum in a fixed order: two calls return identical bits, whatever scratch_bytes
 * (the cap of the staging buffer, which holds whole samples; 0: the default of the functionals).  nsamples <= 8192
 * (BTF_EINVAL beyond), ndepth >= 2.  btf_collect_association reads W and V from the first nsamples collected slots without
 * an upload (Us alone is uploaded) and touches none of the sampler's state; its launches are counted under
 * BTF_K_CRITERIA.  Synchronous.                                                                                          */
int btf_posterior_association(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, int nfeatures,
                              const double* Ws, const double* Vs, const double* Us, int transform, int which, const double* x,
                              double level, const int* stats, int nstats, const double* q, int nq, const int* pairs, int npairs,
                              double* mean_out, double* var_out, double* q_out, double* prob_out, double* defined_out,
                              double* nmean_out, double* values_out, double* of_means_out, double* sdx_out, double* sdy_out,
                              long long scratch_bytes);
int btf_collect_association(btf_ctx* ctx, int nsamples, int nfeatures, const double* Us, int transform, int which, const double* x,
                            double level, const int* stats, int nstats, const double* q, int nq, const int* pairs, int npairs,
                            double* mean_out, double* var_out, double* q_out, double* prob_out, double* defined_out,
                            double* nmean_out, double* values_out, double* of_means_out, double* sdx_out, double* sdy_out,
                            long long scratch_bytes);

/* ---- monotone projection of the posterior (csrc/btf_monotone.h) ---------------------------------------------------------
 * What doseresponse/fit.py:365-374 does on the host before it reports anything: for kept sample s and column j,
 * V'_s[j] = factor_pav(W_s, V_s[j]) (btf_nmf_pav; functionalmf/utils.py:218-252) - the left-to-right pool-adjacent-
 * violators sweep under which no row's curve w_i . v'_jt increases with t - for all S x M blocks in one launch, equal to
 * btf_nmf_pav per sample bit for bit.  increasing != 0: -factor_pav(W_s, -V_s[j]) (no curve decreases).  W is not changed.
 * Outputs, each NULL (skipped) or: V_out (S,M,T,K) the projected samples; pools_out (S,M) = T minus the merges this call
 * made in that block (T: it was monotone already); mean_out (N,M,T) and q_out (nq,N,M,T): btf_posterior_summary of the
 * projected states, run where they lie (mean_out NULL: no summary, and nq must be 0; nsamples <= 16384 with one).
 * Limits: 8 T K + 4 T <= 65536 (the column in LDS: the bound of btf_nmf_pav), nembeds 1..10; BTF_EINVAL beyond.
 * btf_collect_monotone: Ws = Vs = NULL reads the first nsamples collected states where they lie (BTF_EINVAL beyond the
 * collected count) and projects into scratch - or, with in_place != 0, overwrites the collected V samples, so that every
 * later btf_collect_* / btf_crit_* call on them sees the projected posterior; that cannot be undone short of collecting
 * again.  Ws, Vs given: those states are uploaded instead (in_place is then BTF_EINVAL).  The sampler's state is not
 * touched.  fp64, no atomics: two calls return identical bits.  Launches are counted under BTF_K_CRITERIA.  Synchronous. */
int btf_posterior_monotone(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                           const double* Vs, int increasing, int transform, const double* q, int nq, double* V_out,
                           int* pools_out, double* mean_out, double* q_out);
int btf_collect_monotone(btf_ctx* ctx, int nsamples, const double* Ws, const double* Vs, int increasing, int in_place,
                         int transform, const double* q, int nq, double* V_out, int* pools_out, double* mean_out, double* q_out);

/* ---- folding new rows into a fitted posterior (csrc/btf_fold_in.h) ---------------------------------------------------
 * Given V the rows of W are conditionally independent (factor.py:333) with prior N(0, sigma2 I), so a row that was not in
 * the fitted tensor has, under kept sample s, the conditional _resample_W draws from (factor.py:333-362):
 *   Q_s = sum_jt count_jt v_jt^s v_jt^s' / nu2_s + I / sigma2_s,  b_s = sum_jt ysum_jt v_jt^s / nu2_s,  Q_s = L L',
 *   W_out[s][r] = Q_s^-1 b_s + L^-T z  (factor.py:357-362),  Wmean_out[s][r] = Q_s^-1 b_s  (NULL: not wanted).
 * family 0 Gaussian: count / ysum (R,M,T) = observed replicates of the cell and their sum (0, 0: missing), noise = nu2 and
 * sigma2 one value per sample; z (S,R,K) standard normals or NULL: Philox keyed (seed, sample0 + s, r).  family 1 Binomial
 * (factor.py:437-460): trials / ysum (R,M,T) = trials and successes of the observed cells (integers up to 32; 0: missing),
 * inner_sweeps >= 1 rounds per (s, r) from w = 0 of omega_jt ~ PG(trials_jt, w . v_jt) (exact sampler) and the draw with
 * weights omega and kappa = ysum - trials / 2; z must be NULL, noise is ignored.  A row without observations draws from
 * the prior.  sample0: the global index of sample 0 (generator keys only), so that a call over a slice of the samples
 * returns the bits of the whole call.  mean_out (R,M,T) non-NULL adds the summary stage on the device-resident W_out and
 * V: mean and percentiles q of f(w_r^s . v_jt^s) exactly as btf_posterior_summary (transform, q, nq, q_out (nq,R,M,T)
 * as there; nsamples <= 16384 then).  fp64, no floating-point atomics, every sum in a fixed order: two calls return
 * identical bits whatever the launch geometry and wherever the states come from.  A non-positive pivot: BTF_ENOTPD, and
 * btf_fail_index (ctx, or NULL after the stateless call) = (sample0 + s) * nrows_new + r of the first such pair.
 * btf_collect_fold_in reads V, nu2_s and sigma2_s of the first nsamples collected slots without an upload and touches none
 * of the sampler's state; its launches are counted under BTF_K_CRITERIA.  Synchronous.                                  */
int btf_fold_in_rows(int device, int family, int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs,
                     const double* noise, const double* sigma2, const double* count, const double* ysum, const double* trials,
                     const double* z, unsigned long long seed, int inner_sweeps, long long sample0, double* W_out,
                     double* Wmean_out, int transform, const double* q, int nq, double* mean_out, double* q_out);
int btf_collect_fold_in(btf_ctx* ctx, int family, int nsamples, int nrows_new, const double* count, const double* ysum,
                        const double* trials, const double* z, unsigned long long seed, int inner_sweeps, long long sample0,
                        double* W_out, double* Wmean_out, int transform, const double* q, int nq, double* mean_out,
                        double* q_out);

/* ---- folding new rows into a slice-sampled fit (csrc/btf_slice_fold.h) -----------------------------------------------
 * The row prior of the slice-sampled models is N(0, sigma2 I) (factor.py:685-686) and, given V_s (and U_s), every
 * restriction on a row is linear in w, so elliptical slice sampling (elliptical_slice.py:59-124, mu = 0) with the
 * restrictions as a likelihood of minus infinity samples p(w_new | y_new, V_s, U_s): `sweeps` updates per (sample, row),
 * each with at most max_rounds proposals (a sweep that uses them all keeps its state and is counted in unfinished_out),
 * all of them in ONE launch.  family: the codes of btf_ess_* (0..5); param: the parameter of families 3 (1 / variance) and
 * 4 (rate) as btf_set_likelihood_param takes it; shape / scale / prob (G): the gamma-grid table of family 5 as
 * btf_set_likelihood_table takes it (NULL otherwise).  S1 / cnt (R,M,T): sum and number of the observed replicates of the
 * cell (0, 0: missing), logsum (R,M,T): their sum of logs (family 5, NULL otherwise).  The chain of (s, r) starts at
 * start[s][r] ((S,R,K), non-NULL) or at the mean of the nrows_fit rows of Ws[s] ((S,nrows_fit,K); start NULL).
 * constraints (ncons, T+1): sum_t A[c,t] (w . v_jt) >= A[c,T] for every column j; row_constraints (nrow_cons, K+1):
 * a . w >= a[K]; Us (S,F,K) with codes (R,F) of 0, 1, 2 = missing: 0 <= w . u_f <= 1 and the term
 * sum_f x log(w . u_f) + (1 - x) log(1 - w . u_f) beside the likelihood (nfeatures 0: none).  draws
 * (S,R,sweeps,K+1+max_rounds): per sweep the K normals, u_h, u_a and the shrink uniforms, or NULL: Philox keyed (seed,
 * (sample0 + s) << 32 | r, sweep * (K+1+max_rounds) + position).  W_out (S,R,K): the last state of every chain;
 * Wstart_out (S,R,K): its start; rounds_out (S,R): likelihood evaluations of proposals; unfinished_out (S,R).  mean_out
 * non-NULL adds the summary stage as in btf_fold_in_rows.  A start that is infeasible or has a non-finite likelihood: that
 * chain's W_out is nan, the call returns BTF_ESTATE, and btf_fail_index (ctx, or NULL after the stateless call) =
 * (sample0 + s) * nrows_new + r of the first such pair.  fp64, no floating-point atomics, every sum in a fixed order: two
 * calls return identical bits whatever the launch geometry and wherever the states come from.  btf_collect_slice_fold
 * reads W, V and sigma2_s of the first nsamples collected slots without an upload, takes param / the table from the
 * context (btf_set_likelihood_param / btf_set_likelihood_table) and touches none of the sampler's state.  Launches are
 * counted under BTF_K_CRITERIA.  Synchronous.                                                                          */
int btf_slice_fold_rows(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                        int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs, const double* Ws,
                        int nrows_fit, const double* start, const double* sigma2, const double* S1, const double* cnt,
                        const double* logsum, const double* constraints, int ncons, const double* row_constraints, int nrow_cons,
                        const double* Us, int nfeatures, const unsigned char* codes, const double* draws, unsigned long long seed,
                        int sweeps, int max_rounds, long long sample0, double* W_out, double* Wstart_out, int* rounds_out,
                        int* unfinished_out, int transform, const double* q, int nq, double* mean_out, double* q_out);
int btf_collect_slice_fold(btf_ctx* ctx, int family, int nsamples, int nrows_new, const double* start, const double* S1,
                           const double* cnt, const double* logsum, const double* constraints, int ncons,
                           const double* row_constraints, int nrow_cons, const double* Us, int nfeatures,
                           const unsigned char* codes, const double* draws, unsigned long long seed, int sweeps, int max_rounds,
                           long long sample0, double* W_out, double* Wstart_out, int* rounds_out, int* unfinished_out,
                           int transform, const double* q, int nq, double* mean_out, double* q_out);

/* ---- folding new columns into a fitted posterior (csrc/btf_fold_in_cols.h) --------------------------------------------
 * The curves of ncols_new columns the chain never saw, one short Gibbs chain per (kept sample s, new column c) over the
 * column's curve v (T,K) and its horseshoe+ levels, given W_s, nu2_s and lam2_s: `sweeps` rounds of the conditionals of
 * _resample_V for one column (factor.py:378-409) and of _resample_Tau2 for one column (factor.py:136-141) from the prior
 * draw of the levels; functionalmf_amd/fold_in_cols.py (`chain`) is the definition.  family 0 (Gaussian: count, ysum
 * (C,N,T) = observed replicates and their sum, noise (S,) = nu2_s) or 1 (Binomial: trials, ysum = successes (C,N,T),
 * integer counts up to 32, 0 = missing; Polya-Gamma rounds from v = 0 as in btf_fold_in_rows).  Ws (S,N,K), lam2 (S,).
 * draws (S,C,4 nD + sweeps (T K + 4 nD)), Gaussian only: every variate of every chain - the start's unit Gamma(1/2)
 * variates (4,nD), then per sweep T K standard normals and (4,nD) unit gammas - or NULL: Philox keyed (seed,
 * (sample0 + s) << 32 | c, slot, element), so splitting the samples over calls or folding columns one at a time returns
 * identical bits.  stability: the clip of the level updates.  V_out, Vmean_out (S,C,T,K): the last state and the last
 * conditional mean; Tau2_out (S,C,nD).  mean_out non-NULL adds the summary stage on the device-resident W and new V:
 * mean (N,C,T) and q_out (nq,N,C,T) of f(w_i^s . v_ct^s) exactly as btf_posterior_summary (nsamples <= 16384 then).  The
 * band of a column and its side arrays must fit one workgroup's LDS: BTF_EINVAL otherwise, before any device call.  A
 * non-positive pivot: that chain's outputs are nan, the call returns BTF_ESTATE, and btf_fail_index (ctx, or NULL after
 * the stateless call) = (sample0 + s) * ncols_new + c of the first such chain.  fp64, no floating-point atomics, every sum
 * in a fixed order.  btf_collect_fold_in_cols reads W, nu2_s and lam2_s of the first nsamples collected slots without an
 * upload and touches none of the sampler's state; its launches are counted under BTF_K_CRITERIA.  Synchronous.          */
int btf_fold_in_cols(int device, int family, int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order,
                     const double* Ws, const double* noise, const double* lam2, const double* count, const double* ysum,
                     const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                     double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q, int nq,
                     double* mean_out, double* q_out);
int btf_collect_fold_in_cols(btf_ctx* ctx, int family, int nsamples, int ncols_new, const double* count, const double* ysum,
                             const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                             double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                             int nq, double* mean_out, double* q_out);

/* ---- folding new depth slices into a fitted posterior (csrc/btf_fold_in_depth.h) ---------------------------------------
 * The curves of every fitted column at `horizon` depths the chain never saw, one short Gibbs chain per (kept sample s,
 * fitted column j) over the new depths v (H,K) and the horseshoe+ levels of the nR rows of the penalty on ndepth + horizon
 * points that touch a new depth, given W_s, the last min(ndepth, tf_order + 1) depths of V_s[j], nu2_s and lam2_s;
 * functionalmf_amd/fold_in_depth.py (`chain`) is the definition.  family 0 (Gaussian: count, ysum = observed replicates and
 * their sum, noise (S,) = nu2_s) or 1 (Binomial: trials, ysum = successes, integer counts up to 32, 0 = missing;
 * Polya-Gamma rounds from v_t = V_s[j, ndepth - 1]).  The new data lies [column][depth][row]: (M,H,N); a slice of all
 * zeros is the model's forecast.  Ws (S,N,K); Vtail (S,M,min(ndepth, tf_order + 1),K): the last kept depths; lam2 (S,).
 * draws (S,M,4 nR + sweeps (H K + 4 nR)), Gaussian only: every variate of every chain - the start's unit Gamma(1/2)
 * variates (4,nR), then per sweep H K standard normals and (4,nR) unit gammas - or NULL: Philox keyed (seed,
 * (sample0 + s) << 32 | j, slot, element), so splitting the samples over calls returns identical bits.  stability: the
 * clip of the level updates.  V_out, Vmean_out (S,M,H,K): the last state and the last conditional mean; Tau2_out
 * (S,M,nR).  mean_out non-NULL adds the summary stage on the device-resident W and new V: mean (N,M,H) and q_out
 * (nq,N,M,H) of f(w_i^s . v_jt^s) exactly as btf_posterior_summary (nsamples <= 16384 then).  The band of the H K wide
 * system and its side arrays must fit one workgroup's LDS: BTF_EINVAL otherwise, before any device call.  A non-positive
 * pivot: that chain's outputs are nan, the call returns BTF_ESTATE, and btf_fail_index (ctx, or NULL after the stateless
 * call) = (sample0 + s) * ncols + j of the first such chain.  fp64, no floating-point atomics, every sum in a fixed order.
 * btf_collect_fold_in_depth reads W, the tail of V, nu2_s and lam2_s of the first nsamples collected slots without an
 * upload and touches none of the sampler's state; its launches are counted under BTF_K_CRITERIA.  Synchronous.          */
int btf_fold_in_depth(int device, int family, int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds,
                      int tf_order, const double* Ws, const double* Vtail, const double* noise, const double* lam2,
                      const double* count, const double* ysum, const double* trials, const double* draws, unsigned long long seed,
                      int sweeps, long long sample0, double stability, double* V_out, double* Vmean_out, double* Tau2_out,
                      int transform, const double* q, int nq, double* mean_out, double* q_out);
int btf_collect_fold_in_depth(btf_ctx* ctx, int family, int nsamples, int horizon, const double* count, const double* ysum,
                              const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                              double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                              int nq, double* mean_out, double* q_out);

/* ---- folding new columns and depth slices into a Negative-Binomial fit (csrc/btf_fold_chain.h) ------------------------
 * btf_fold_in_cols / btf_fold_in_depth for the Negative-Binomial model, whose cells depend on the sampled rate: a cell
 * with count = c observed replicates, their sum ysum and rate r is the Binomial cell with omega ~ PG(ysum + c r, w_i . v_t)
 * and kappa = (ysum - c r) / 2 (factor.py:506-511, 553); everything else is the chain of the Binomial family, from the same
 * start.  functionalmf_amd/negbin_fold_in.py (`chain_cols`, `chain_depth`) is the definition.  Stateless only (the model
 * keeps its samples on the host); the argument lists are their siblings' without family, noise and trials.  count, ysum:
 * (C,N,T) for columns, (M,H,N) for depths; counts of any size (0: missing).  rate: the rate of (sample s, column c, row i,
 * depth t) lies at rate[s rs_sample + c rs_col + i rs_row + t rs_depth]: a compact array over those four axes in that
 * order, every axis full or shared (stride 0); finite and positive, ysum + count * rate below 1e15.  The Polya-Gamma
 * weights come from the sampler of the Negative-Binomial sweeps (the sum-of-gammas series below 200, the moment-matched
 * normal from there on) on a generator keyed by the cell as in the Binomial family, so splitting the samples over calls
 * (sample0) returns identical bits; the chain's stream holds the column's INDEX IN THE CALL, so a column folded alone has
 * the bits it has as column 0 of a larger call, not those of a later position.  omega (S,C,sweeps,T,N) / (S,M,sweeps,H,N), or NULL: weights in
 * the place of every Polya-Gamma draw; draws (as in the siblings) needs omega beside it, and the two together make a chain
 * a deterministic function of its inputs.  A cell with count 0 draws nothing and adds exact zeros: a column or slice
 * without data runs the Gaussian family's chain on the prior with the same generator keys.  LDS: the sibling's count plus
 * 8 nrows bytes for the weights of one depth (btf_negbin_fold_lds_bytes; horizon 0: a column; -1: sizes no call takes);
 * beyond the limit BTF_EINVAL with the byte count.  Outputs, the summary stage, failures and btf_fail_index as in the
 * siblings.  Launches are counted under BTF_K_CRITERIA.  Synchronous.                                                    */
int btf_negbin_fold_in_cols(int device, int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order,
                            const double* Ws, const double* lam2, const double* count, const double* ysum, const double* rate,
                            long long rs_sample, long long rs_col, long long rs_row, long long rs_depth, const double* omega,
                            const double* draws, unsigned long long seed, int sweeps, long long sample0, double stability,
                            double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q, int nq,
                            double* mean_out, double* q_out);
int btf_negbin_fold_in_depth(int device, int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds, int tf_order,
                             const double* Ws, const double* Vtail, const double* lam2, const double* count, const double* ysum,
                             const double* rate, long long rs_sample, long long rs_col, long long rs_row, long long rs_depth,
                             const double* omega, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                             double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                             int nq, double* mean_out, double* q_out);
long long btf_negbin_fold_lds_bytes(int nrows, int ndepth, int horizon, int nembeds, int tf_order);

/* ---- folding new rows into a Negative-Binomial fit, with a fixed or a sampled rate (csrc/btf_negbin_fold_rows.h) ------
 * One chain per (kept sample s, new row) from w = 0 with the prior N(0, sigma2_s I): the chain of btf_fold_in_rows' Binomial
 * family on the pseudo-data above (omega ~ PG(ysum + c r, w . v_jt), kappa = (ysum - c r) / 2), `sweeps` sweeps.
 * functionalmf_amd/negbin_fold_in.py (`chain_rows`) is the definition.  Stateless only.  Vs (S,M,T,K), sigma2 (S,);
 * count, ysum (R,M,T): the observed replicates of a cell and their sum (0: missing), counts of any size.
 * rate != NULL - a FIXED rate: the rate of (sample s, new row r, column j, depth t) lies at rate[s rs_sample + r rs_row +
 *   j rs_col + t rs_depth], a compact array over those four axes in that order, every axis full or shared (stride 0);
 *   finite and positive, ysum + count * rate below 1e15.  rate_init, hist_y, hist_n, R_out, accept_out are not read.
 * rate == NULL - a SAMPLED rate: every (sample, row) has one scalar rate, started at rate_init (S,R) and updated in front
 *   of every sweep by nmetropolis random-walk Metropolis steps on log r (the model's own: proposal N(log r, rpropstdev),
 *   prior N(0, rstdev) on log r, accepted only above 1), whose count terms run over the row's histogram: hist_y (R,nbins)
 *   the distinct counts of a row, hist_n (R,nbins) how often each was observed (0: padding).  R_out (S,R): the rate at
 *   the last sweep; accept_out (S,R): the accepted share of the chain's steps.
 * Generators: keyed (seed, (sample0 + s) << 32 | row) - splitting the samples over calls (sample0) or the rows' first 64 k
 * over calls returns identical bits.  Replay: omega (S,sweeps,M*T,R) replaces every Polya-Gamma draw; z (S,R,sweeps,K) the
 * normals of the draws of w and mh (S,R,sweeps,2,nmetropolis) the normals, then the uniforms of the Metropolis steps - z
 * and mh need omega beside them, and mh goes with z when the rate is sampled.  W_out, Wmean_out (S,R,K): the last draw and
 * its conditional mean.  The summary stage (mean_out (R,M,T), q_out (nq,R,M,T); transform as btf_posterior_summary) runs on
 * the device-resident draws.  A non-positive pivot - also what a sigma2, V or w . v that is not finite ends in - returns
 * BTF_ENOTPD with btf_fail_index(NULL) = (sample0 + s) * nrows_new + row of the smallest failing pair, whose outputs are
 * nan.  Launches are counted under BTF_K_CRITERIA.  Synchronous.                                                         */
int btf_negbin_fold_in_rows(int device, int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs,
                            const double* sigma2, const double* count, const double* ysum, const double* rate, long long rs_sample,
                            long long rs_row, long long rs_col, long long rs_depth, const double* rate_init, const double* hist_y,
                            const double* hist_n, int nbins, int nmetropolis, double rpropstdev, double rstdev, const double* omega,
                            const double* z, const double* mh, unsigned long long seed, int sweeps, long long sample0, double* W_out,
                            double* Wmean_out, double* R_out, double* accept_out, int transform, const double* q, int nq,
                            double* mean_out, double* q_out);

/* ---- folding new columns into a slice-sampled fit (csrc/btf_slice_fold_cols.h) ---------------------------------------
 * The same for the slice-sampled models: one chain per (kept sample s, new column c) over the column's curve v (T,K) and
 * its horseshoe+ levels given W_s and lam2_s, the curve updated by elliptical slice sampling on an ellipse centred on a
 * per-cell Gaussian fit of the likelihood; functionalmf_amd/slice_fold_in_cols.py (`chain`) is the definition.  family and
 * param / the table as btf_slice_fold_rows.  Ws (S,N,K), lam2 (S,); start (S,C,T,K), or NULL: the mean over the nfit_cols
 * fitted columns of Vs (S,nfit_cols,T,K).  S1, cnt, logsum (C,N,T): the per-cell statistics of the new columns
 * (cnt = 0: missing; logsum: gamma grid only); fit_a, fit_b (C,N,T): 1 / Sigma_fit^2 and Mu_fit / Sigma_fit^2 (0, 0: the
 * cell carries no fit; the fit changes the mixing, never the target).  constraints (ncons, T + 1): sum_t A[q,t] (w_i . v_t)
 * >= C[q] for every fitted row i.  tau2 (S,C,nD) holds the local scales fixed (NULL: sampled).  draws
 * (S,C,4 nD + sweeps (T K + 1 + max_rounds + 4 nD)): the start's (4,nD) unit Gamma(1/2) variates, then per sweep T K
 * normals, u_h, u_a, max_rounds - 1 shrink uniforms and (4,nD) unit gammas - or NULL: Philox keyed (seed,
 * (sample0 + s) << 32 | c, slot, element).  V_out, Vstart_out (S,C,T,K), Tau2_out (S,C,nD), rounds_out, unfinished_out
 * (S,C); mean_out non-NULL adds the summary stage as in btf_fold_in_cols.  The band of a column, its side arrays and the
 * likelihood tables must fit one workgroup's LDS: BTF_EINVAL otherwise, before any device call.  A start that is infeasible
 * or has a non-finite likelihood, or a non-positive pivot: that chain's outputs are nan, the call returns BTF_ESTATE and
 * btf_fail_index (ctx, or NULL after the stateless call) = (sample0 + s) * ncols_new + c of the first such chain.  fp64,
 * no floating-point atomics, every sum in a fixed order.  btf_collect_slice_fold_cols reads W, V and lam2_s of the first
 * nsamples collected slots without an upload, takes param / the table from the context and touches none of the sampler's
 * state.  Launches are counted under BTF_K_CRITERIA.  Synchronous.                                                      */
int btf_slice_fold_cols(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                        int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order, const double* Ws,
                        const double* Vs, int nfit_cols, const double* lam2, const double* start, const double* S1,
                        const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                        const double* constraints, int ncons, const double* tau2, const double* draws, unsigned long long seed,
                        int sweeps, int max_rounds, long long sample0, double stability, double* V_out, double* Vstart_out,
                        double* Tau2_out, int* rounds_out, int* unfinished_out, int transform, const double* q, int nq,
                        double* mean_out, double* q_out);
int btf_collect_slice_fold_cols(btf_ctx* ctx, int family, int nsamples, int ncols_new, const double* start, const double* S1,
                                const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                                const double* constraints, int ncons, const double* tau2, const double* draws,
                                unsigned long long seed, int sweeps, int max_rounds, long long sample0, double stability,
                                double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out, int* unfinished_out,
                                int transform, const double* q, int nq, double* mean_out, double* q_out);

/* ---- folding new depth slices into a slice-sampled fit (csrc/btf_slice_fold_depth.h) --------------------------------
 * btf_fold_in_depth for the slice-sampled models: one chain per (kept sample s, fitted column j) over the `horizon` new
 * depths v (H,K) and the horseshoe+ levels of the nR new penalty rows, given W_s, the kept tail of V_s[j] and lam2_s - the
 * prior side of btf_fold_in_depth (new rows, offsets from the kept tail, fresh levels) with the curve update of
 * btf_slice_fold_cols (one elliptical slice update on an ellipse centred on a per-cell Gaussian fit);
 * functionalmf_amd/slice_fold_in_depth.py (`chain`) is the definition.  family and param / the table as
 * btf_slice_fold_rows.  Ws (S,N,K), lam2 (S,).  constraints (ncons, nback + H + 1): the rows of the constraints on the
 * extended grid that touch a new depth, cut to the nback trailing kept depths they reach, the H new depths and the bound
 * (slice_fold_in_depth.reduce_constraints): sum_t A[q,t] (w_i . V_s[j, T - nback + t]) + sum_h A[q,nback + h] (w_i . v_h) >=
 * c[q] for every fitted row i; kept and new terms go through one dot product in ascending depth order, so a new depth that
 * repeats the bits of the last kept depth ties exactly.  Vtail (S,M,Lt,K): the last Lt = max(min(ndepth, tf_order + 1),
 * nback) kept depths.  start (S,M,H,K), or NULL: every new depth starts at V_s[j, ndepth - 1].  S1, cnt, logsum, fit_a,
 * fit_b (M,N,H): the per-cell statistics and the fit of the new slices as in btf_slice_fold_cols (all zeros: the
 * constrained forecast).  tau2 (S,M,nR) holds the scales fixed.  draws (S,M,4 nR + sweeps (H K + 1 + max_rounds + 4 nR)):
 * the layout of btf_slice_fold_cols with nR and H K - or NULL: Philox keyed (seed, (sample0 + s) << 32 | j, slot, element).
 * V_out, Vstart_out (S,M,H,K), Tau2_out (S,M,nR), rounds_out, unfinished_out (S,M); mean_out non-NULL adds the summary
 * stage: mean (N,M,H), q_out (nq,N,M,H).  The band of the H K wide system, its side arrays, the tail and the likelihood
 * tables must fit one workgroup's LDS, and (tf_order + 1) nembeds < 64: BTF_EINVAL otherwise, before any device call.  A
 * start that is infeasible or has a non-finite likelihood, or a non-positive pivot: that chain's outputs are nan, the call
 * returns BTF_ESTATE and btf_fail_index (ctx, or NULL after the stateless call) = (sample0 + s) * ncols + j of the first
 * such chain.  fp64, no floating-point atomics, every sum in a fixed order.  btf_collect_slice_fold_depth reads W, the tail
 * of V and lam2_s of the first nsamples collected slots without an upload, takes param / the table from the context and
 * touches none of the sampler's state.  Launches are counted under BTF_K_CRITERIA.  Synchronous.                        */
int btf_slice_fold_depth(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                         int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds, int tf_order, const double* Ws,
                         const double* Vtail, const double* lam2, const double* start, const double* S1, const double* cnt,
                         const double* logsum, const double* fit_a, const double* fit_b, const double* constraints, int ncons,
                         int nback, const double* tau2, const double* draws, unsigned long long seed, int sweeps, int max_rounds,
                         long long sample0, double stability, double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out,
                         int* unfinished_out, int transform, const double* q, int nq, double* mean_out, double* q_out);
int btf_collect_slice_fold_depth(btf_ctx* ctx, int family, int nsamples, int horizon, const double* start, const double* S1,
                                 const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                                 const double* constraints, int ncons, int nback, const double* tau2, const double* draws,
                                 unsigned long long seed, int sweeps, int max_rounds, long long sample0, double stability,
                                 double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out, int* unfinished_out,
                                 int transform, const double* q, int nq, double* mean_out, double* q_out);

/* ---- convergence diagnostics (csrc/btf_diag.h) ----------------------------------------------------------------------
 * Split R-hat (rank-normalised, max of bulk and folded), bulk ESS, tail ESS (min over the 5 % / 95 % indicators), MCSE of
 * the mean and the mean, per cell of f(W V') over nchains chains of nsamples draws (Vehtari et al. 2021; one chain: its
 * two halves).  Chain c is ctxs[c]'s first nsamples collected samples (btf_collect_*, read where they lie, same device and
 * shape, unsharded) when ctxs && ctxs[c], else the host arrays Ws[c] (S,N,K) / Vs[c] (S,M,T,K), uploaded.  transform as
 * btf_posterior_summary; out (5,N,M,T): rhat, ess_bulk, ess_tail, mcse_mean, mean - nan for a cell whose draws are all
 * equal or hold a non-finite value.  nsamples >= 4, nchains <= 64, nchains * nsamples <= 4096.  Synchronous.          */
int btf_diag_eval(int device, int nchains, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* const* Ws,
                  const double* const* Vs, btf_ctx* const* ctxs, int transform, double* out);

/* ---- on-device sample collection (rng="device"; replaces the per-sample copies of
 * genlasso.py:51-65) ---------------------------------------------------------------------
 * btf_collect_begin allocates nsamples slots for W, V, Tau2 and the device-resident scalars;
 * btf_collect(slot) queues one copy kernel for the current state (no synchronisation);
 * btf_collect_end downloads the first nsamples slots (W (S,N,K), V (S,M,T,K), Tau2 (S,M,nD),
 * scalars (S,8): nu2, sigma2, lam2, lam2_a, ...; any may be NULL) and synchronises;
 * btf_collect_summary is btf_posterior_summary on the collected samples, without an upload.   */
int btf_collect_begin(btf_ctx* ctx, int nsamples);
int btf_collect(btf_ctx* ctx, int slot);
/* Let btf_gibbs_sweeps keep states by itself: after `countdown` more sweeps the state goes to slot first_slot, then every
 * `every`-th sweep to the next slot, until the slots of btf_collect_begin are full (genlasso.py:52-60: the samples kept
 * after burn-in, every nthin-th sweep).  every = 0 switches the schedule off.  One C call per block of sweeps instead of
 * one per kept sample.                                                                                               */
int btf_collect_schedule(btf_ctx* ctx, int every, int first_slot, int countdown);
int btf_collect_end(btf_ctx* ctx, int nsamples, double* W, double* V, double* Tau2, double* scalars8);
int btf_collect_summary(btf_ctx* ctx, int nsamples, int transform, const double* q, int nq, double* mean_out, double* q_out);

/* ---- model-selection criteria (replaces _BayesianModel.select_hyperparams_DIC's scoring, genlasso.py:69-136, on
 * logprob, factor.py:262-264 / :610-612 / :1002-1005, and the hand-made DIC of doseresponse/select_btf.py:9-23) ----------
 * The normalised log-likelihood ll_s(i,j) of every curve (i,j) - all its observed y_ijtr over depth and replicates -
 * under every kept sample s, reduced on the device to what WAIC, DIC and held-out scoring need (csrc/btf_criteria.h).
 * Touches none of the sampler's state (partials, caches, draw counters, status word): a chain continued after a
 * criteria call walks the same path.  Unsharded contexts.
 *
 * btf_crit_set_data: the criteria's own statistics for slot 0 (the bound data) or 1 (held-out data), in the kernel's
 *   layout: S1 [M][T][N] = sum_r y, cnt [M][T][N] = observed replicates (Binomial: trials), curve_c0 / curve_c1 [N][M]
 *   the curve's constant (family 3: sum y^2 and the observation count; otherwise the state-independent log-likelihood
 *   terms: - sum lgamma(y+1), sum log C(n,y), ...; curve_c1 unused).  16 B per cell + 16 B per curve on the device.
 *   All four NULL frees the slot.  Synchronises.
 * btf_crit_eval: families 0..4 as the ESS links (link 3: param = the VARIANCE here, not its inverse; link 4: the rate):
 *   0 Poisson log, 1 Poisson identity (-inf where w.v <= 0), 2 logit (Binomial / Bernoulli), 3 Gaussian, 4 NB logit.
 *   States: Ws (S,N,K) and Vs (S,M,T,K) uploaded from the host; or Ws = Vs = NULL: the first nsamples slots of
 *   btf_collect_begin (no upload); or flags & BTF_CRIT_CURRENT: the context's current W, V (nsamples = 1).
 *   flags & BTF_CRIT_NOISE_PER_SAMPLE (family 3): the variance of sample s is noise[s] (host), or with collected states
 *   and noise = NULL the collected nu2; otherwise every sample has variance `param`.
 *   curve_out [5][N][M]: per curve, over the samples in ascending order, the max-shifted sum of exp(ll_s), the max, the
 *   mean, Welford's M2, and ll at the plug-in (mean_s w.v per cell, mean variance); total_out (S,): sum_ij ll_s;
 *   pointwise_out (S,N,M) or NULL.  No floating-point atomics: two calls return identical bits.  Synchronises.
 * Family 5, the gamma grid (link 5 of btf_ess_*; csrc/btf_gg_criteria.h), in btf_crit_eval and btf_crit_loo alike: the
 *   table is the context's (btf_set_likelihood_table) and the slot carries a third per-cell statistic,
 *   btf_crit_set_logsum: L [M][T][N] = sum_r log y over the observed replicates, after btf_crit_set_data on that slot
 *   (with zero curve_c0 / curve_c1), else BTF_ESTATE; NULL frees it; btf_crit_set_data on the slot, or freeing the slot,
 *   drops it.  8 B per cell more on the device.  Without the table or L the calls return BTF_ESTATE and launch nothing;
 *   `param` is ignored, BTF_CRIT_NOISE_PER_SAMPLE is BTF_EINVAL.  A cell without observations inside an observed curve
 *   contributes log sum_g p_g, an observed cell with w.v <= 0 gives -inf, a curve without any observation counts 0.  */
enum { BTF_CRIT_NOISE_PER_SAMPLE = 1, BTF_CRIT_CURRENT = 2 };
int btf_crit_set_data(btf_ctx* ctx, int slot, const double* S1, const double* cnt, const double* curve_c0, const double* curve_c1);
int btf_crit_set_logsum(btf_ctx* ctx, int slot, const double* L);
int btf_crit_eval(btf_ctx* ctx, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
                  const double* noise, int flags, double* curve_out, double* total_out, double* pointwise_out);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-curve-out (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson,
 * Gelman, Yao, Gabry 2024), csrc/btf_loo.h; the written definition is functionalmf_amd/criteria.py: psis_curve --------
 * btf_crit_loo: slot, family, param, states, noise and flags as btf_crit_eval (without BTF_CRIT_CURRENT).  The pointwise
 *   log-likelihoods ll_s(i,j) stay on the device: per curve the log importance ratios -ll are sorted, the largest
 *   Mt = min(floor(0.2 S), ceil(3 sqrt(S / r_eff))) are replaced by the order statistics of the generalised Pareto
 *   distribution fitted to them (Zhang and Stephens 2009), every log weight is truncated at the raw maximum and
 *   elpd_loo = logsumexp_s(lw_s + ll_s) with normalised lw.  r_eff [N][M] (finite, > 0) or NULL: 1 for every curve.
 *   loo_out [4][N][M]: elpd_loo; the Pareto shape k-hat (inf: no fit - fewer than 5 tail samples, that is S < 25, or
 *   all ratios equal - and the unsmoothed estimate); then the two accumulators of lppd exactly as curve_out[0], [1] of
 *   btf_crit_eval (max-shifted sum of exp(ll_s), max), so that the caller forms lppd as it does there, bit for bit.
 *   A curve with a -inf sample: elpd_loo = -inf, k = inf; with a nan sample: nan; their log weights are nan.
 *   mean_out (N,M,T) or NULL: the leave-curve-out fitted curve sum_s exp(lw_s(i,j)) f(w_i^s . v_jt^s), f = `transform`
 *   as btf_posterior_summary (0 identity, 1 ilogit, 2 square); logw_out (S,N,M) or NULL: the normalised log weights.
 *   nsamples <= 4096.  Device scratch for the call's duration: 8 S N M bytes (1.05 GB at (512,256,64), S = 1000), and
 *   8 N M T with mean_out.  Touches none of the sampler's state.  No floating-point atomics: two calls return identical
 *   bits.  Unsharded contexts.  Synchronises.                                                                        */
int btf_crit_loo(btf_ctx* ctx, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
                 const double* noise, int flags, const double* r_eff, int transform, double* loo_out, double* mean_out,
                 double* logw_out);

/* ---- the same two for the conjugate Negative-Binomial model, whose rate R is SAMPLED (csrc/btf_nb_criteria.h) ------------
 * Family 4 of btf_crit_eval has one known rate; here every kept sample s has a rate tensor R_s that is full or shared
 * along each of rows, columns and depth, so lgamma(y + R_s) - lgamma(R_s) is summed per (sample, curve) by a kernel of its
 * own from the raw counts.  Not a family of btf_crit_eval (family 6 there stays BTF_EINVAL).
 * btf_crit_set_counts: the raw counts Y [N][M][T][nreps] (NaN = missing, otherwise finite and >= 0: BTF_EINVAL) of a
 *   slot, after btf_crit_set_data on it (S1, cnt as there; curve_c0 = - sum lgamma(y+1), curve_c1 unused), else BTF_ESTATE.
 *   NULL frees them; btf_crit_set_data on the slot, or freeing the slot, drops them.  8 nreps bytes per cell more on the
 *   device.  Synchronises.
 * btf_nb_crit_eval / btf_nb_crit_loo: slot, states and outputs as btf_crit_eval / btf_crit_loo (flags: BTF_CRIT_CURRENT
 *   or 0).  rates: (nsamples + 1, extent) on the host, rate tensor nsamples being the plug-in's R-bar (the mean over the
 *   samples); aux_flags: the BTF_PRED_AUX_ROWS / _COLS / _DEPTH bits of btf_predict_eval say along which axes the tensor
 *   is full (extent = the product of those axes' lengths, C order; BTF_PRED_AUX_PER_SAMPLE is accepted and implied).
 *   ll_s(i,j) = sum over observed (t,r) of lgamma(y+R) - lgamma(R) - lgamma(y+1) + y eta - (y+R) softplus(eta), eta not
 *   clipped; a curve without observations counts exactly 0.  BTF_ESTATE without counts on the slot; BTF_EINVAL for a rate
 *   that is not finite and > 0, and (btf_nb_crit_loo) nsamples > 4096.  Device scratch for the call's duration, beside
 *   what btf_crit_eval / btf_crit_loo take: 8 (nsamples + 1) N M bytes (the per-sample curve constants) and the rates.
 *   Counted under BTF_K_CRITERIA.  No floating-point atomics: two calls return identical bits.  Touches none of the
 *   sampler's state.  Unsharded contexts.  Synchronises.                                                              */
int btf_crit_set_counts(btf_ctx* ctx, int slot, const double* Y, int nreps);
int btf_nb_crit_eval(btf_ctx* ctx, int slot, int nsamples, const double* Ws, const double* Vs, const double* rates, int aux_flags,
                     int flags, double* curve_out, double* total_out, double* pointwise_out);
int btf_nb_crit_loo(btf_ctx* ctx, int slot, int nsamples, const double* Ws, const double* Vs, const double* rates, int aux_flags,
                    const double* r_eff, int transform, double* loo_out, double* mean_out, double* logw_out);

/* ---- posterior predictive of the observations (flutrends/benchmark.py:60-75, :129-134; politics/benchmark.py:147-172) ----
 * Replicated observations y_rep ~ p(y | theta_s) for every cell and kept sample, reduced on the device to moments, order
 * statistics and comparisons with data (csrc/btf_predict.h); the (S,N,M,T) draws never leave the chip.  Touches none of
 * the sampler's state: a chain continued after a predictive call walks the same path.  Unsharded contexts.
 *
 * btf_predict_batch (stateless, for validating the samplers): out[i] ~ family(eta[i], aux[i]); draw i uses global draw
 *   index i.  Families as btf_crit_eval: 0 Poisson log, 1 Poisson identity (nan where eta <= 0), 2 logit: aux = trials,
 *   3 Gaussian: aux = variance, 4 Negative-Binomial logit: aux = rate r (mean r p / (1 - p), p = ilogit(eta)).
 * btf_predict_eval: states as btf_crit_eval - Ws (S,N,K), Vs (S,M,T,K) uploaded, or both NULL: the first nsamples
 *   collected slots.  param: the Gaussian variance / the Negative-Binomial rate of every sample, unless aux_flags &
 *   BTF_PRED_AUX_PER_SAMPLE: sample s has aux_sample[s] (Gaussian; NULL with collected states: the collected nu2) or the
 *   rate tensor aux_sample[s][...] whose extent along rows / columns / depth is N / M / T where the BTF_PRED_AUX_ROWS /
 *   _COLS / _DEPTH bit is set and 1 (shared) otherwise.  trials (N,M,T) or NULL (one trial): the logit family's counts; a
 *   nan count gives nan draws.  Y (N,M,T,nreps) or NULL: observations, nan = missing.  Draw (s, r) of flat cell c has
 *   global draw index (c S + s) draws_per_sample + r: the draws do not depend on the launch geometry, on `cells` or on
 *   where the states come from.  nsamples * draws_per_sample <= 16384 (BTF_EINVAL beyond).
 *   Outputs, each may be NULL: mean (N,M,T) = mean_s E[y | theta_s] (no draws involved); y_mean, y_var (ddof 1) of the n =
 *   S * draws_per_sample draws; q_out (nq,N,M,T) their percentiles q (numpy's linear interpolation); with Y: pit_lo /
 *   pit_hi = mean over the cell's observed replicates of the fraction of draws < y / <= y (nan without observations),
 *   inside = observed replicates within [q_out[0], q_out[nq-1]] (nq >= 2, else nan), nobs = observed replicates,
 *   rmse / mae (S,) of y - E[y | theta_s] over all observed y (nan without any); draws_out (ncells, n): the raw draws of
 *   the listed flat cells, in draw order.  A cell with a nan draw has nan in every draw-based output.  No floating-point
 *   atomics: two calls with the same seed return identical bits.  Synchronises.                                    */
enum { BTF_PRED_AUX_PER_SAMPLE = 1, BTF_PRED_AUX_ROWS = 2, BTF_PRED_AUX_COLS = 4, BTF_PRED_AUX_DEPTH = 8 };
int btf_predict_batch(int device, int family, int64_t n, const double* eta, const double* aux, uint64_t seed, double* out);
int btf_predict_eval(btf_ctx* ctx, int family, double param, int nsamples, const double* Ws, const double* Vs,
                     const double* aux_sample, int aux_flags, const double* trials, const double* Y, int nreps,
                     int draws_per_sample, uint64_t seed, const double* q, int nq, const int32_t* cells, int ncells,
                     double* mean_out, double* ymean_out, double* yvar_out, double* q_out, double* pit_lo_out,
                     double* pit_hi_out, double* inside_out, double* nobs_out, double* rmse_out, double* mae_out,
                     double* draws_out);

/* ---- posterior predictive checks: predictive p-values of whole-curve discrepancies (csrc/btf_checks.h; the written
 * definition is functionalmf_amd/checks.py) ----
 * btf_predict_check: family, param, states, aux_sample / aux_flags, trials and their refusals as btf_predict_eval; Y
 *   (N,M,T,nreps) is required.  For every kept sample s and rho < reps a replicated data set is drawn at the observed
 *   slots of Y: slot (i,j,t,rep) of set e = s reps + rho is draw number cell n + s Rr + rho nreps + rep of the family's
 *   sampler, Rr = reps nreps, n = nsamples Rr - the draw btf_predict_eval returns for that cell with draws_per_sample = Rr
 *   and the same seed.  There is no 16384 limit (nothing is sorted); BTF_EINVAL where the 64-bit draw index overflows.
 *   which: nwhich distinct discrepancy codes, 0 chisq, 1 max, 2 lag1, 3 total, 4 zeros, each T(y, theta_s) of a curve
 *   (i,j) over its observed slots, t ascending then rep ascending: sum (y - mu)^2 / v; max |y - mu| / sqrt(v);
 *   sum_{t,t+1 defined} e_t e_{t+1} / sum_t e_t^2 with e_t = sum_rep (y - mu_t) / sqrt(v_t m_t), m_t the observed
 *   replicates at t (nan without an adjacent pair or with a zero denominator); sum y; #{y == 0}.  mu = E[y | theta_s],
 *   v = Var[y | theta_s]; slots with v == 0 are left out of codes 0..2.
 *   curve_out (5, nwhich, N, M): the number of sets with T(y_rep) >= T(y), with >, with both defined, and the sums of
 *   T(y) and of T(y_rep) over those sets; nobs_out (N,M): observed slots.  A curve without observations, and a bad curve
 *   (an observed slot nothing can be drawn at in some sample: eta <= 0 under the identity link, a missing trial count), is
 *   nan in both.  pool_obs_out (nwhich, nsamples), pool_rep_out (nwhich, nsamples reps): the discrepancies pooled over all
 *   other curves per sample / per set - chisq, total, zeros add, max is the maximum, lag1 pools numerator and denominator
 *   - the curves in row-major order in tiles of 8 columns, the tiles added in index order.  curves: ncurves flat curve
 *   indices i M + j whose raw values come back as tobs_out (ncurves, nwhich, nsamples) and trep_out (ncurves, nwhich,
 *   nsamples reps).  chunk_rows: rows per launch (0: what 192 MiB of pooled partials hold); no bit depends on it, on
 *   `which` or on where the states come from.  No floating-point atomics.  Touches none of the sampler's state.
 *   Unsharded contexts.  Synchronises.                                                                              */
int btf_predict_check(btf_ctx* ctx, int family, double param, int nsamples, const double* Ws, const double* Vs,
                      const double* aux_sample, int aux_flags, const double* trials, const double* Y, int nreps, int reps,
                      uint64_t seed, const int32_t* which, int nwhich, const int32_t* curves, int ncurves, int chunk_rows,
                      double* curve_out, double* nobs_out, double* pool_obs_out, double* pool_rep_out, double* tobs_out,
                      double* trep_out);

/* ---- the same for the gamma-grid likelihood (doseresponse/fit.py:475-478: likelihood.sample and the 5 / 95 percentiles
 * per curve), csrc/btf_gg_predict.h ----
 * The draw: y | eta = eta s_g Gamma(a_g, 1) with the component g chosen by the weights w_g = p_g / sum_h p_h of the table
 *   (the reference's sample picks it uniformly, whatever mean_probs says; a table with equal weights gives that).  The
 *   cumulative weights c_g = sum_{h<=g} w_h are summed once on the host in ascending g; draw number i uses the generator
 *   of family 5 at global draw index i, whose first uniform u takes the smallest g with u < c_g (never a component of
 *   weight 0; the last one with p_g > 0 where round-off leaves none), and the Gamma draw goes on with the same generator.
 *   eta <= 0 or nan gives nan.  E[y | eta] = eta mbar, mbar = sum_g w_g a_g s_g.  One component per replicated
 *   observation: the marginal predictive of one new observation.
 * btf_predict_gg_eval: btf_predict_eval for the table the context holds (btf_set_likelihood_table; without one BTF_ESTATE,
 *   nothing is launched): states, Y, draws_per_sample, seed, q, cells, every output, the global draw index, the limits
 *   and the refusals as there.  A cell with eta <= 0 in a sample has nan in mean and in every draw-based output, and
 *   every sample with such an observed cell a nan rmse / mae, as under family 1.  No floating-point atomics.  Synchronises.
 * btf_predict_gg_batch (stateless, for validating the sampler): out[i] = draw number i at eta[i] from the table shape,
 *   scale, prob (G entries each; 1 <= G <= 128, finite shape > 0, scale > 0, weight >= 0, not all zero, else BTF_EINVAL);
 *   comp_out[i] (or NULL): its component, -1 where eta[i] gives no draw.                                             */
int btf_predict_gg_eval(btf_ctx* ctx, int nsamples, const double* Ws, const double* Vs, const double* Y, int nreps,
                        int draws_per_sample, uint64_t seed, const double* q, int nq, const int32_t* cells, int ncells,
                        double* mean_out, double* ymean_out, double* yvar_out, double* q_out, double* pit_lo_out,
                        double* pit_hi_out, double* inside_out, double* nobs_out, double* rmse_out, double* mae_out,
                        double* draws_out);
int btf_predict_gg_batch(int device, int64_t n, const double* eta, int G, const double* shape, const double* scale,
                         const double* prob, uint64_t seed, double* out, int32_t* comp_out);

/* ---- non-negative tensor factorisation (replaces functionalmf.utils.tensor_nmf, utils.py:276-420, its max_entry
 * projection and row_features included) and the factor PAV projection (factor_pav, utils.py:218-252) ------------------
 * Context-free: a btf_nmf handle holds its own statistics, factors and a small device state on a stream of its own; no
 * btf_ctx is touched (csrc/btf_nmf.h).
 * btf_nmf_create: uploads the statistics of Y (N,M,T,R): S [N][M*T] = sum of the observed replicates per cell, counts
 *   [N][M*T] = their number as bytes, or NULL when every cell has all R; ssw = the within-cell sum of squares about the
 *   cell means.  K = nembeds in 1..10.  Synchronises.
 * btf_nmf_run: up to max_steps ALS steps from W (N,K) / V (M,T,K), both overwritten with the result.  Per step: if fit_W,
 *   each row i's first d = min(K, i+1) entries = max(NNLS, 1e-3) over its observed entries (utils.py:299-329); if fit_V,
 *   each (j,t) = max(NNLS, 1e-3) (utils.py:332-355) and, if monotone, factor_pav on every column (utils.py:357-359); then
 *   rmse = sqrt(residual sum of squares) and the step stops the run when (prev - rmse) / rmse <= tol (utils.py:381-390).
 *   All steps are queued without a host synchronisation; the decision is taken on the device.  rmse_out[max_steps]: the
 *   rmse of each step run; steps_out: the number run; device_ms (or NULL): device time of the queued steps.  verbose
 *   synchronises per step and prints "Step n" / "delta: x".  A Lawson-Hanson NNLS that reaches its cap of 3 x unknowns
 *   (scipy's default) returns BTF_EINVAL.  No floating-point atomics: two identical runs return identical bits.
 * btf_nmf_set_bounds: max_entry > 0 for the later runs of this handle (0: none, the default).  After its NNLS solve a row
 *   i (leading d entries), a cell (j,t) or a feature row R[f] whose fitted entries exceed max_entry, max_q c_q.x >
 *   max_entry over the shared rows c_q (all M*T vectors V[j,t,:d] for a row, all N rows of W otherwise), is replaced by
 *   the minimiser of 1/2 |b - A x|^2 subject to 0 <= c_q.x <= max_entry for every q and x >= 1e-6 (utils.py:338-347,
 *   369-377, 398-407: SLSQP there, an exact dual active-set method on the normal equations here, one wave per system).
 *   A projection that reaches its cap of 50 (K + 1) steps, has no feasible point or a singular A'A returns BTF_EINVAL.
 * btf_nmf_set_row_features: X [N][nfeatures] with 0 where missing, observed [N][nfeatures] bytes or NULL when nothing
 *   is missing; nfeatures = 0 removes them.  With features every observed x_if joins row i's system as the design row
 *   R[f] (its bound constraints stay those of V), and after the V step and PAV every R[f] = max(NNLS(W[obs], X[obs,f]),
 *   1e-3) with the same projection against W; a feature nobody observed keeps its value.  rmse and the stopping rule
 *   use Y only.  Synchronises.
 * btf_nmf_run_bounded: btf_nmf_run with R (nfeatures,K) read and overwritten (NULL exactly when no features are set;
 *   btf_nmf_run refuses a handle with features).  projected_out (or NULL) [N + M*T + nfeatures] bytes: 1 for every row,
 *   cell and feature projected in the last step run; nprojected_out (or NULL) [max_steps]: the systems projected per
 *   step.  Without bounds and features it queues the kernels of btf_nmf_run and returns the same bits.
 * btf_nmf_pav: factor_pav of every column of V (M,T,K) against W (N,K), in place; T (8 K + 4) <= 65536.  Synchronises. */
typedef struct btf_nmf btf_nmf;
int btf_nmf_create(btf_nmf** out, int device, int nrows, int ncols, int ndepth, int nreps, int nembeds, const double* S,
                   const unsigned char* counts, double ssw);
int btf_nmf_run(btf_nmf* h, double* W, double* V, int fit_W, int fit_V, int monotone, int max_steps, double tol, int verbose,
                int* steps_out, double* rmse_out, double* device_ms);
int btf_nmf_set_bounds(btf_nmf* h, double max_entry);
int btf_nmf_set_row_features(btf_nmf* h, int nfeatures, const double* X, const unsigned char* observed);
int btf_nmf_run_bounded(btf_nmf* h, double* W, double* V, double* R, int fit_W, int fit_V, int monotone, int max_steps,
                        double tol, int verbose, int* steps_out, double* rmse_out, double* device_ms,
                        unsigned char* projected_out, int* nprojected_out);
void btf_nmf_destroy(btf_nmf* h);
int btf_nmf_pav(int device, int nrows, int ncols, int ndepth, int nembeds, const double* W, double* V);

/* ---- measurement ----------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by hipEvents on the ctx
 * stream; btf_kernel_times drains them: total milliseconds and launch count per
 * BTF_K_* id (arrays of BTF_K_COUNT).                                         */
int btf_set_profiling(btf_ctx* ctx, int on);
int btf_kernel_times(btf_ctx* ctx, double* ms_total, int64_t* launches);
/* Launch geometry of the streaming kernels: rows per workgroup (0 = default).   */
int btf_set_tuning(btf_ctx* ctx, int rows_per_block_w, int rows_per_block_v);

#ifdef __cplusplus
}
#endif
#endif /* BTF_H_ */
