// The context behind the C ABI (include/btf.h) and the host plumbing that every unit with entry points shares: error
// reporting, device allocation, counted launches, the dispatch macros.  Host code only - never included by a kernel header.
#pragma once
#include "../../include/btf.h"
#include "btf_device.h"         // ESS_FAM_COUNT, HYP_*
#include "btf_pg_exact.h"       // PG_MODE_*
#include "btf_gamma_grid.h"     // GgComp
#include "btf_scratch.h"        // Scratch, report_error
#include <hip/hip_ext.h>

#include <algorithm>
#include <string>
#include <vector>

typedef struct ncclComm* ncclComm_t;      // as rccl.h has it; btf_comm.h, the peer transport and its kernel are btf_abi.hip's alone
namespace btf {
struct PeerMailbox; struct PeerTable;
constexpr int MAX_K = 10;
struct EvPair { hipEvent_t a, b; int kid; };
}  // namespace btf

struct btf_ctx {
  int N = 0, M = 0, T = 0, K = 0, TF = 0, nD = 0, KK = 0;
  int dev = 0;
  int ncu = 256;                     // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int row0 = 0, nl = 0, col0 = 0, ml = 0;
  int hrow = -1, hcol = -1;  // btf_set_shard_halo: global index of the ONE stale-weight source row / column outside the blocks (-1: none);
                             // its statistics sit at local index nl / ml of the slabs (never updated, never summed - only its weights are read)
  int ldw = 0, ldv = 0;      // padded leading dimensions of A_wT / A_v
  int R = 1;
  bool have_data = false, binomial = false, weighted = false;
  double* A_wT = nullptr; double* C_wT = nullptr; double* A_v = nullptr; double* C_v = nullptr;
  double* B_wT = nullptr; double* B_v = nullptr;   // binomial: trials (0 where missing)
  unsigned char* C8_wT = nullptr; unsigned char* C8_v = nullptr;   // Gaussian data with missing replicates: counts as bytes (C_* freed)
  signed char* A8_wT = nullptr; signed char* A8_v = nullptr;       // Binomial data with integer counts: 2 (Y - N/2) as bytes
  double* W = nullptr; double* V = nullptr;
  double* Tau2 = nullptr;
  double lam2 = 1.0, sigma2 = 1.0, nu2 = 1.0;
  bool have_W = false, have_V = false, have_hyper = false;
  double* part = nullptr; size_t part_elems = 0;
  double* gpart = nullptr; int ngp_gram = 16;      // partial Grams of the last gram_kernel launch
  double* zbuf = nullptr; size_t z_elems = 0;
  double* bsum = nullptr; size_t bsum_elems = 0;
  double* gband = nullptr; size_t gband_stride = 0;
  int* status = nullptr;   // [0] flag [1] index
  int* tries = nullptr;
  int* st_ptr = nullptr; int* st_row = nullptr; double* st_coef = nullptr;
  int* st_drow = nullptr; double* st_dcoef = nullptr; bool st_dense_ok = false;   // VS_MAXE slots per (t,d) (spectral sampler)
  int* srcmap_w = nullptr; int* srcmap_v = nullptr;   // per-output source index of the cached weights
  bool stale_w = false, stale_v = false;
  int v_part_mode = 0;               // accumulation mode of the V half-sweep's partials in c->part (2: Gram blocks at the source columns)
  double ssw = 0.0, nobs = 0.0, sa2 = 0.0;      // within-cell SS, observation count, sum S1^2/cnt (Gaussian data)
  double nobs_global = -1.0;                    // sharded runs: observation count over all ranks (btf_set_global_nobs)
  bool w_part_valid = false; int w_part_mode = 0, w_part_nch = 0, w_part_rpb = 0; bool w_part_gv = false;   // W-step partials current?
  int rpb_w = 0, rpb_v = 0;
  int sampler = BTF_SAMPLER_BANDED;   // BTF_OPT_SAMPLER
  double* eig = nullptr;              // gram_eig_kernel output (spectral sampler): K eigenvalues, K*K vectors, sweeps
  // elliptical slice sampling (btf_ess_*): current state, prior draw, per-chain {hh, lo, hi, theta, ll}, partial sums
  double* essX0 = nullptr; double* essNu = nullptr; double* ess_st = nullptr; double* ess_theta = nullptr; int* ess_done = nullptr;
  double* ess_part = nullptr; size_t ess_part_elems = 0; int ess_last_chains = 0;
  // generalized analytic slice sampling (btf_gass_*): constraints, per-chain grids / candidates / likelihoods
  double* gs_cons = nullptr; double* gs_cc = nullptr; double* gs_rc = nullptr; int gs_J = 0, gs_nrc = 0;
  int* gs_cptr = nullptr; int* gs_cidx = nullptr; double* gs_cval = nullptr; int gs_cnnz = 0;     // the constraint matrix by its non-zeros
  double* gs_av = nullptr; unsigned char* gs_mask = nullptr; int* gs_info = nullptr;
  double* gs_thetas = nullptr; int* gs_ntheta = nullptr; double* gs_ll = nullptr; double* gs_llp = nullptr; size_t gs_llp_elems = 0; double* gs_hh = nullptr; double* gs_cur = nullptr;
  int* gs_nacc = nullptr; double* gs_u = nullptr;
  int gs_chains = 0, gs_what = -1, gs_link = 0;
  // binary row features (btf_gass_set_row_features, btf_gass_features.h): the codes in both orientations, U, the user's
  // row constraints on the host (gs_rc holds them followed by the 2F derived rows), the rows' side term of the current
  // state, and the feature chains' own grids / candidates / likelihoods (what = 2)
  int ft_F = 0; unsigned char* ft_rows = nullptr; unsigned char* ft_cols = nullptr; double* ft_U = nullptr;
  std::vector<double> gs_rc_host; double* ft_side = nullptr;
  double* ft_X0 = nullptr; double* ft_Nu = nullptr; double* ft_z = nullptr; unsigned char* ft_mask = nullptr; int* ft_info = nullptr;
  double* ft_thetas = nullptr; int* ft_ntheta = nullptr; double* ft_ll = nullptr; double* ft_hh = nullptr; double* ft_cur = nullptr;
  double* ft_part = nullptr; int* ft_nacc = nullptr; double* ft_u = nullptr; double* ft_theta = nullptr; int* ft_keep = nullptr;
  // EP-centred GASS (btf_gass_set_ep): per-cell (Mu, p) in the row and the column layout, per-chain constants, the centre
  // and the current state's correction of the last begin, the twisted envelope of the column systems
  double2* ep_rows = nullptr; double2* ep_cols = nullptr; double* ep_crow = nullptr; double* ep_ccol = nullptr;
  double* ep_mu = nullptr; double* ep_corr = nullptr; double* ep_pband = nullptr; double* ep_envg = nullptr;
  int* ep_f = nullptr; int* ep_off = nullptr; int ep_env = 0, ep_bwe = 0; bool ep_on = false, gs_ep = false;
  double lik_par[btf::ESS_FAM_COUNT] = {0, 0, 0, 1.0, 1.0, 0};     // parameter per likelihood family (btf_set_likelihood_param)
  // the gamma-grid family (btf_gamma_grid.h): component table, log sum p, and L = sum_r log y in both layouts of S1
  btf::GgComp* gg_tab = nullptr; int gg_G = 0; double gg_lsp = 0.0;
  std::vector<double> gg_pred; double gg_mbar = 0.0;      // the same table for the predictive draw (gg_pred_table), on the host
  double* gg_Lw = nullptr; double* gg_Lv = nullptr; bool gg_have_L = false;
  long long* dbg = nullptr;
  double* vc_scratch = nullptr; size_t vc_scratch_elems = 0;     // factor records of the chunked chain sampler
#ifdef BTF_ACC_STAMPS
  long long* acc_stamps = nullptr;
#endif
  double* pband = nullptr;
  double* pimg = nullptr; unsigned long long pimg_version = 0;       // the band as LDS images [P | Pm] (dataflow tails of the fused V launch)
  // what the precomputed prior band (fused V launch, btf_fused.h) was formed from: every change of Tau2 / lam2 / the shard
  // moves prior_version on; the band is rebuilt (prior_band_kernel) when pband_version lags behind
  unsigned long long prior_version = 1, pband_version = 0, last_v_prior_version = 0;
  double* Ta = nullptr; double* Tb = nullptr; double* Tc = nullptr; double* lsum = nullptr;   // horseshoe+ chain (device mode)
  int* dr_ptr = nullptr; int* dr_col = nullptr; double* dr_val = nullptr;                   // Delta, CSR by row
  bool have_chain = false;
  double* pin = nullptr; size_t pin_elems = 0;   // pinned host staging (async SSE partials + W)
  size_t sse_nb = 0; bool sse_pending = false;
  double* pin_lsum = nullptr;
  // Negative-Binomial counts: raw replicates, per-cell sums / counts, rate buffers
  double* nb_data = nullptr; double* nb_S = nullptr; double* nb_cnt = nullptr;
  double* nb_R = nullptr; double* nb_C = nullptr; size_t nb_relems = 0;
  double* nb_tmp = nullptr; size_t nb_tmp_elems = 0;
  double* nb_out = nullptr; size_t nb_out_elems = 0;
  int nb_Rr = 0; bool counts = false; bool nb_bwt_written = false;
  unsigned int* nb_H = nullptr; double* nb_Hd = nullptr; double* nb_Hs = nullptr;   // per-row count histograms (u32, f64) and their sum over rows
  double* nb_L = nullptr;            // [N + 1]: per-row sum cnt*log(1-p), then the total
  int* fill_tab = nullptr; int fill_n = 0; int fill_key = -1;   // band assembly program of the twisted kernel
  int* nb_optr = nullptr; double* nb_oval = nullptr; int nb_nout = 0;   // per-row outlier lists (CSR)
  int nb_ymax = 0;                   // largest tabulated count present (histogram bins above it are empty)
  double* nb_G = nullptr;            // suffix sums of the histogram of all counts: nb_G[k] = #{observations > k}, k < NB_TAB
  bool nb_tabulable = false;        // every observed count is an integer in [0, NB_TAB)
  bool nb_L_valid = false;          // nb_L matches the current W, V
  bool nb_hist = true;              // BTF_OPT_NB_HISTOGRAMS
  int pg_mode = btf::PG_MODE_DEFAULT;    // BTF_OPT_PG_EXACT: PG_MODE_DEFAULT / PG_MODE_EXACT_ALL / PG_MODE_SERIES_ALL
  // trial counts below the normal range: any integer up to PG_AUTO_EXACT_MAX / any larger integer / any non-integer
  bool pg_has_small = true, pg_has_big = true, pg_has_frac = true;
  // on-device sample collection (run_gibbs, rng="device"): [nsamp] slots of W, V, Tau2 and the scalars
  double* smp_W = nullptr; double* smp_V = nullptr; double* smp_T = nullptr; double* smp_s = nullptr; int smp_n = 0;
  // model-selection criteria (btf_crit_*): the compact statistics of slot 0 (bound data) / 1 (held-out data)
  double* crit_S1[2] = {nullptr, nullptr}; double* crit_cnt[2] = {nullptr, nullptr};
  double* crit_c0[2] = {nullptr, nullptr}; double* crit_c1[2] = {nullptr, nullptr};
  double* crit_L[2] = {nullptr, nullptr};        // family 5: sum_r log y per cell (btf_crit_set_logsum)
  double* crit_Y[2] = {nullptr, nullptr}; int crit_nreps[2] = {0, 0};   // Negative-Binomial: raw counts [M][T * nreps][N] (btf_crit_set_counts)
  int col_every = 0, col_slot = 0, col_count = 0;       // btf_collect_schedule: btf_gibbs_sweeps keeps every col_every-th state
  double* hyp = nullptr;        // device-resident scalars [HYP_COUNT] (nu2, sigma2, lam2, lam2_a, ...)
  bool dev_scalars = false;     // kernels read nu2 / sigma2 / lam2 from hyp instead of the host copies
  double* pin_hyp = nullptr;
  double* gsum_v = nullptr; bool w_part_gsum = false;   // V'V summed by a side workgroup of the W accumulation launch (GramSide.sum_*): w_solve reads KK doubles
  double* gpart_w = nullptr; int ngp_w = 0;   // W'W partials written by w_solve (valid until W changes otherwise)
  double* gpart_v = nullptr; int ngp_v = 0;   // V'V partials written by the fast banded sampler
  // BTF_OPT_GRAM_ASIDE: the fused V launch left the columns' shares unformed (ngp_v stands for them all the same): the next W
  // accumulation launch forms them beside its stream, or pay_gram_shares (btf_abi.hip) before anything else reads gpart_v.
  // Meaningful only while ngp_v > 0.
  bool gv_owed = false; int gram_aside = 1;
  int share_cpw = 8;                 // columns per share side workgroup of the W accumulation launch (BTF_SHARE_CPW at creation: A/B aid)
  unsigned gv_cnt_total = 0;         // arrivals of the share side workgroups (fz_words + FZ_GSUM): a running total, never reset
  bool fuse_gram = true;
  // curve-structured replicate counts (btf_kernels.h, CurveLists): counts constant along the depth axis
  bool curve = false, curve_opt = true;
  std::vector<unsigned char> cv_cij;                                  // host copy of c_ij [N][M] (stale-source test)
  int* cv_cptr = nullptr; int* cv_crow = nullptr; double* cv_cdef = nullptr;   // by column: deficient rows
  int* cv_rptr = nullptr; int* cv_rcol = nullptr; double* cv_rdef = nullptr;   // by row: deficient columns
  double* eig_cols = nullptr;                                         // [M][K + K*K + 8] per-column eigen-systems
  int* cv_dcols = nullptr; int cv_ndef = 0;                           // the columns that have deficient rows
  bool w_part_curve = false;                                          // the W-step partials were made in curve mode
  // sharded runs, BTF_OPT_SPLIT_ACCUM: the chunks of the rank's own block of the fixed factor are accumulated right
  // behind the kernel that drew it (no exchange needed), the rest behind the all-gather
  bool split_accum = false;
  bool w_local_done = false, v_local_done = false;                    // own-block chunks of the next W / V accumulation are in c->part
  int w_local_rpb = 0, w_local_mode = 0, v_local_rpb = 0, v_local_mode = 0;
  hipEvent_t ev_draw = nullptr, ev_join = nullptr;                    // behind the last draw kernel / the comm stream's tail
  // the ctx-owned communicator (btf_comm_init; btf_comm.h).  comm_rank / comm_world are the communicator's; gather_rank /
  // gather_world the block decomposition the all-gathers reassemble - the same, except in a rehearsal (btf_comm_rehearse:
  // a one-rank communicator moving the messages of rank gather_rank of gather_world through scratch buffers)
  ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 1, gather_rank = 0, gather_world = 1;
  bool comm_rehearse = false;
  hipStream_t comm_stream = nullptr;                                  // the overlapped exchange runs its gathers here
  double* comm_scr = nullptr; size_t comm_scr_elems = 0;              // rehearsal: [send | recv] of the larger message
  double* comm_words = nullptr;                                       // 16 device doubles: btf_allreduce_sum's staging
  // the peer-window transport (btf_comm.h): this rank's mailbox, the table of where every rank's buffers are mapped
  // here, the mappings to close, the collective counter
  btf::PeerMailbox* peer_box = nullptr;
  btf::PeerTable* peer_tab = nullptr;
  unsigned* peer_counters = nullptr;
  std::vector<void*> peer_opened;
  bool peer_on = false;
  unsigned long long peer_epoch = 0;
  long long peer_timeout_ticks = 0;
  bool tau_pending = false; unsigned long long tau_seed = 0; double tau_stability = 1e-6;   // btf_queue_Tau2
  // the four-launch sweep (BTF_OPT_FUSED_SWEEP): per-column residual parts left by the spectral V sampler, and a queued
  // nu2 / sigma2 draw that the next W accumulation launch carries as a side workgroup (btf_queue_scalars)
  bool fused_sweep = true;
  double* sse_cols = nullptr; bool sse_cols_valid = false;
  double* vs_rec = nullptr; size_t vs_rec_elems = 0;       // HBM scratch of the spectral sampler's pivot records (long depth axes)
  bool nu2_drawn_since_v = false;      // a device nu2 draw happened since the last V half-sweep: the caller runs full sweeps
  bool sc_pending = false; unsigned long long sc_seed = 0; int sc_which = 0; double sc_prior[4] = {0, 0, 0, 0};
  bool lam_pending = false; unsigned long long lam_seed = 0; int lam_exact = 0;            // btf_queue_lam2
  bool band_in_wsolve = true;                                         // (A/B aid: BTF_BAND_IN_WSOLVE=0: the band's own launch)
  bool v_wants_band = false, band_img = false; int band_PB = 0;       // the last fused V launch loaded the precomputed prior band (and its LDS image)
  bool lam_in_wsolve = true;                                          // (A/B aid: BTF_LAM_IN_WSOLVE=0 leaves the draw to the V launch)
  unsigned long long sweep_w = 0, sweep_v = 0;
  // the two-launch W+V step (BTF_OPT_FUSED_STEP, btf_fused.h): tickets / flags (zeroed once; 32 words = one 128-byte line
  // per flag), the write-through copies the tails read, the epoch of the hand-offs (one per fused launch, never reused)
  int fused_dataflow = 1;            // BTF_OPT_FUSED_DATAFLOW: 1 (default) the fused V launch runs the barrier-free tail where it applies
  int fused_step = 1;                // BTF_OPT_FUSED_STEP: 0 four launches, 1 (default) the V launch carries its sampler, 2 the W launch its solve too
  unsigned* fz_words = nullptr; int fz_tiles_w = 0, fz_tiles_v = 0;
  double* fz_pub = nullptr;
  unsigned fz_epoch = 0, fz_gram_total = 0, fz_w_total = 0;
  bool profiling = false;
  std::vector<btf::EvPair> ev_pool;
  size_t ev_used = 0;
  double ms_total[BTF_K_COUNT] = {0};
  int64_t launches[BTF_K_COUNT] = {0};
  std::string err;
  int fail_index = -1;
};

namespace btf {
// records msg as the text btf_last_error(c) returns (c may be null: the context-free entry points) and hands code back
inline int fail(btf_ctx* c, int code, const std::string& msg) { return report_error(c, code, msg); }

#define HIPCHK(ctx, call)                                                                  \
  do {                                                                                     \
    hipError_t e__ = (call);                                                               \
    if (e__ != hipSuccess)                                                                 \
      return fail(ctx, BTF_EHIP, std::string(#call) + ": " + hipGetErrorString(e__));      \
  } while (0)

template <typename T>
inline int dev_alloc(btf_ctx* c, T** p, size_t n) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (n == 0) n = 1;
  HIPCHK(c, hipMalloc((void**)p, n * sizeof(T)));
  return BTF_OK;
}

void launch_summary(Scratch& s, const double* W, const double* V, int S, int rows, int MT, int K, int transform, const double* dq,
                    int nq, double* mean, double* quant);      // (btf_abi.hip, beside the kernel)
// Delta (nD,T) dense, rebuilt from its definition, and the CSR of the Delta' Delta stencil per (t, d), d = 0..tf+1 (btf_abi.hip)
void penalty_stencil(int T, int tf, std::vector<double>& Delta, int& nD, std::vector<int>& ptr, std::vector<int>& row,
                     std::vector<double>& coef);
// btf_fail_index(NULL): the failing (sample, row) of this thread's last stateless fold-in (btf_analysis.hip)
int fold_fail_index();
// the device of a stateless entry point
inline int use_device(int device) {
  const hipError_t e = hipSetDevice(device);
  return e == hipSuccess ? BTF_OK : fail(nullptr, BTF_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
}

// One kernel launch, counted per BTF_K_* id.  With profiling on the launch goes through
// hipExtLaunchKernelGGL so that the two events bracket exactly this dispatch (its start
// and completion timestamps), not the gaps around it.
struct Prof {
  btf_ctx* c; int kid; EvPair* ev = nullptr;
  Prof(btf_ctx* c_, int kid_) : c(c_), kid(kid_) {
    c->launches[kid]++;
    if (c->profiling && c->ev_used < c->ev_pool.size()) {
      ev = &c->ev_pool[c->ev_used++];
      ev->kid = kid;
    }
  }
  template <typename F, typename... Args>
  void launch(F kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    launch_on(c->stream, kernel, grid, block, lds, args...);
  }
  template <typename F, typename... Args>
  void launch_on(hipStream_t st, F kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, ev->a, ev->b, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, args...);
  }
};

// One launch of an analysis entry point on its scratch's stream: counted under kid when the call has a context, and not
// made at all once an allocation or copy of the scratch has failed.
template <typename F, typename... Args>
void launch_counted(Scratch& s, int kid, F kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
  if (!s.ctx()) return s.launch(kernel, grid, block, lds, args...);
  if (s.rc()) return;
  { Prof p(s.ctx(), kid); p.launch_on(s.stream(), kernel, grid, block, lds, args...); }
  s.check(hipGetLastError(), "hipGetLastError (kernel launch)");
}
// dynamic LDS beyond the default 64 KiB has to be allowed per kernel
template <typename F>
void allow_lds(Scratch& s, F kernel, size_t lds) {
  s.check(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute");
}

// LDS geometry of the kernels that sort the n values of a cell in a row of P doubles: P the power of two >= n (and >= 2),
// as many cells per workgroup as `budget` bytes hold, at least one (a row over the budget still gets its workgroup) and at
// most `cap`.
struct SortGeom { int P, cells; size_t lds; };
inline SortGeom sort_geom(int n, size_t budget, int cap) {
  SortGeom g;
  g.P = 2;
  while (g.P < n) g.P <<= 1;
  g.cells = std::max(1, std::min(cap, (int)(budget / ((size_t)g.P * sizeof(double)))));
  g.lds = (size_t)g.cells * g.P * sizeof(double);
  return g;
}
constexpr size_t SUMMARY_SORT_LDS = 128 * 1024, PRED_SORT_LDS = 64 * 1024;
constexpr int SUMMARY_SORT_CELLS = 16, PRED_SORT_CELLS = 16;

#define K_SWITCH(K, CALL)                                          \
  switch (K) {                                                     \
    case 1: { constexpr int KT = 1; CALL; } break;                 \
    case 2: { constexpr int KT = 2; CALL; } break;                 \
    case 3: { constexpr int KT = 3; CALL; } break;                 \
    case 4: { constexpr int KT = 4; CALL; } break;                 \
    case 5: { constexpr int KT = 5; CALL; } break;                 \
    case 6: { constexpr int KT = 6; CALL; } break;                 \
    case 7: { constexpr int KT = 7; CALL; } break;                 \
    case 8: { constexpr int KT = 8; CALL; } break;                 \
    case 9: { constexpr int KT = 9; CALL; } break;                 \
    case 10: { constexpr int KT = 10; CALL; } break;               \
    default: break;                                                \
  }
// the same over the five likelihood families of the criteria and predictive kernels (CRIT_FAM_* / PRED_FAM_*), as FT
#define FAM_SWITCH(F, CALL)                                        \
  switch (F) {                                                     \
    case 0: { constexpr int FT = 0; CALL; } break;                 \
    case 1: { constexpr int FT = 1; CALL; } break;                 \
    case 2: { constexpr int FT = 2; CALL; } break;                 \
    case 3: { constexpr int FT = 3; CALL; } break;                 \
    case 4: { constexpr int FT = 4; CALL; } break;                 \
    default: break;                                                \
  }

}  // namespace btf
