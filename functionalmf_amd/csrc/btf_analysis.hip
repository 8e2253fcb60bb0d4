// The posterior analyses behind the C ABI (include/btf.h): summaries, criteria, PSIS-LOO, predictive, functionals, bands, ranking,
// similarity, association, monotone projection, fold-in (rows and columns: conjugate and slice-sampled), diagnostics.  Host code over kernels in units of their own.  gfx950 only.
#include "btf_ctx.h"            // struct btf_ctx, fail, Scratch, launch_counted, K_SWITCH / FAM_SWITCH
#include "btf_diag.h"           // convergence diagnostics (instances in btf_diag.hip)
#include "btf_criteria.h"       // model-selection criteria (instances in btf_criteria.hip)
#include "btf_gg_criteria.h"    // the same for the gamma-grid likelihood (kernels in btf_gg_criteria.hip)
#include "btf_nb_criteria.h"    // the same for the Negative-Binomial model's sampled rate (kernels in btf_nb_criteria.hip)
#include "btf_loo.h"            // PSIS-LOO (instances in btf_loo.hip)
#include "btf_predict.h"        // posterior predictive (instances in btf_predict.hip)
#include "btf_checks.h"         // posterior predictive checks (instances in btf_predict.hip)
#include "btf_gg_predict.h"     // the same for the gamma-grid likelihood (kernels in btf_gg_predict.hip)
#include "btf_functionals.h"    // posterior curve functionals (kernels in btf_functionals.hip)
#include "btf_bands.h"          // simultaneous credible bands (kernels in btf_functionals.hip)
#include "btf_ranking.h"        // posterior ranking (kernels in btf_ranking.hip)
#include "btf_similarity.h"     // posterior similarity (kernels in btf_similarity.hip)
#include "btf_assoc.h"          // posterior feature association (kernels in btf_assoc.hip)
#include "btf_monotone.h"       // monotone projection of the posterior (kernel in btf_monotone.hip)
#include "btf_fold_in.h"        // folding new rows in (kernel in btf_fold_in.hip)
#include "btf_negbin_fold_rows.h"  // the same for a Negative-Binomial fit, with a fixed or a sampled rate (kernel in btf_fold_in.hip)
#include "btf_slice_fold.h"     // the same for the slice-sampled models (kernels in btf_slice_fold.hip)
#include "btf_fold_in_cols.h"   // folding new columns in (kernel in btf_fold_in_cols.hip)
#include "btf_fold_in_depth.h"  // folding new depth slices in (kernel in btf_fold_in_depth.hip)
#include "btf_slice_fold_cols.h"   // the same for the slice-sampled models (kernels in btf_slice_fold_cols.hip)
#include "btf_slice_fold_depth.h"  // new depth slices for the slice-sampled models (kernels in btf_slice_fold_depth.hip)

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace btf;
static_assert(CRIT_FAM_COUNT == 5 && PRED_FAM_COUNT == 5, "FAM_SWITCH covers families 0..4");
// Cells per workgroup of the predictive launch: the rows of a workgroup get what half the 160 KiB of a CU leaves beside
// the family's static table (the gamma grid's 3 KiB; none for the other five), at most PRED_SORT_LDS - so two workgroups
// fit a CU with or without a table, and while the table stays under 16 KiB all six families have one geometry.
constexpr size_t PRED_CU_LDS = 160 * 1024;
constexpr size_t pred_row_budget(size_t table_bytes) { return std::min(PRED_SORT_LDS, PRED_CU_LDS / 2 - table_bytes); }
static_assert(pred_row_budget(GGP_TAB_DOUBLES * sizeof(double)) == PRED_SORT_LDS, "the gamma-grid table costs the rows nothing");

extern "C" {
namespace {
// the summary of btf_*_summary, the monotone projection and fold-in: its buffers, the launch (btf_abi.hip), the downloads
void summary_stage(Scratch& s, const double* W, const double* V, int S, int rows, int MT, int K, int transform, const double* q,
                   int nq, double* mean_out, double* q_out) {
  const size_t n = (size_t)rows * MT;
  double* dm = s.alloc<double>(n);
  const double* dq = nq ? s.upload(q, (size_t)nq) : s.alloc<double>(1);
  double* dqo = s.alloc<double>((size_t)nq * n);
  launch_summary(s, W, V, S, rows, MT, K, transform, dq, nq, dm, dqo);
  s.download(mean_out, dm, n);
  if (nq) s.download(q_out, dqo, (size_t)nq * n);
}

struct States { double *W, *V; const double* noise; long long noise_stride; };
// W, V on the device: the uploaded host arrays (Ws null: the call reads no W), else the context's current state
// (`current`), else its collected ones, where they lie
States states_of(btf_ctx* c, Scratch& s, int S, int N, int MT, int K, const double* Ws, const double* Vs, bool current) {
  if (Vs) return {Ws ? s.upload(Ws, (size_t)S * N * K) : nullptr, s.upload(Vs, (size_t)S * MT * K), nullptr, 1};
  return current ? States{c->W, c->V, nullptr, 1} : States{c->smp_W, c->smp_V, nullptr, 1};
}
// The same for criteria and predictive, with their per-sample noise: the uploaded `noise` (`per` values a sample), else
// the collected nu2 of every kept state.  The callers have refused what they do not take.
States resolve_states(btf_ctx* c, Scratch& s, int S, const double* Ws, const double* Vs, bool current, bool per_sample,
                      const double* noise, size_t per) {
  States r = states_of(c, s, S, c->N, c->M * c->T, c->K, Ws, Vs, current);
  if (per_sample && noise) { r.noise = s.upload(noise, (size_t)S * per); r.noise_stride = (long long)per; }
  else if (per_sample) { r.noise = c->smp_s + HYP_NU2; r.noise_stride = HYP_COUNT; }
  return r;
}

// the first S collected states of c are there (btf_collect_begin allocates the slot arrays together), and the refusal
bool has_collected(const btf_ctx* c, int S) { return c->smp_W && c->smp_V && c->smp_s && S <= c->smp_n; }
int no_collected(btf_ctx* c, int code, const std::string& who) { return fail(c, code, who + ": not that many collected samples"); }

// The states of one call of a pair btf_posterior_X / btf_collect_X, after its checks: selects the device (the scratch's
// context's, else `device`), resolves W, V; collected states that are not there are refused with `code` under `who`.
int resolve_pair(Scratch& s, int device, const char* who, int code, int S, int N, int MT, int K, const double* Ws, const double* Vs,
                 States& st) {
  btf_ctx* c = s.ctx();
  if (c && !Vs && !has_collected(c, S)) return no_collected(c, code, who);
  if (c) HIPCHK(c, hipSetDevice(c->dev));
  else if (int rc = use_device(device)) return rc;
  st = states_of(c, s, S, N, MT, K, Ws, Vs, false);
  return BTF_OK;
}

int check_percentiles(btf_ctx* c, const double* q, int nq) {
  for (int k = 0; k < nq; ++k)
    if (!(q[k] >= 0.0 && q[k] <= 100.0)) return fail(c, BTF_EINVAL, "percentiles must lie in [0, 100]");
  return BTF_OK;
}

// The curve axis x (T depths) and the functional codes of a request, refused under the feature's name `who` in the order
// every feature refuses them.  (Ranking and association hand in their one code, already range-checked.)
int check_curve_axis(btf_ctx* c, const std::string& who, int T, const double* x, const int* which, int nwhich, double level) {
  if (T < 2) return fail(c, BTF_EINVAL, who + ": a curve needs ndepth >= 2");
  bool seen[FUNC_COUNT] = {false};
  for (int k = 0; k < nwhich; ++k) {
    if (which[k] < 0 || which[k] >= FUNC_COUNT || seen[which[k]]) return fail(c, BTF_EINVAL, who + ": functional codes must be distinct and in 0..6");
    seen[which[k]] = true;
  }
  if (seen[FUNC_CROSSING] && !(level == level)) return fail(c, BTF_EINVAL, who + ": crossing needs a level");
  for (int t = 1; t < T; ++t)
    if (!(x[t] > x[t - 1])) return fail(c, BTF_EINVAL, who + ": x must be strictly increasing");
  return BTF_OK;
}

// sample slices of a func_sweep launch: enough workgroups to fill the chip when rows x columns alone do not (geometry only)
int func_sweep_slices(int S, int rowblocks, int jc) {
  return std::max(1, std::min((S + FUNC_WAVES - 1) / FUNC_WAVES, (2048 + rowblocks * jc - 1) / (rowblocks * jc)));
}

// One curve functional of the device states dW (S,N,K), dV (S,M,T,K), swept a chunk of samples at a time into the scratch
// vals[column][sample of the chunk][row]; scratch_bytes caps it (0: FUNC_SCRATCH_BYTES; one sample is the least).
struct FuncSweep { Scratch* s; FuncKernel kern; FuncArgs f; const double *dW, *dV; double* vals; int K, sc_max; };
// false, before anything is allocated: no kernel for this nembeds / transform
bool func_sweep_init(FuncSweep& w, Scratch& s, const double* dW, const double* dV, int S, int N, int M, int T, int K, int transform,
                     int which, const double* x, double level, long long scratch_bytes) {
  w = FuncSweep{&s, func_sweep_fn(K, transform), {}, dW, dV, nullptr, K, 1};
  if (!w.kern) return false;
  const size_t NM = (size_t)N * M, cap = scratch_bytes > 0 ? (size_t)scratch_bytes : FUNC_SCRATCH_BYTES;
  w.sc_max = (int)std::max<size_t>(1, std::min<size_t>(S, cap / (NM * sizeof(double))));
  FuncArgs& f = w.f;
  f.level = level; f.exceed = std::nan(""); f.N = N; f.M = M; f.T = T; f.nslots = 1;
  for (int k = 0; k < FUNC_COUNT; ++k) f.slot[k] = -1;
  f.slot[which] = 0; f.code[0] = which;
  f.x = s.upload(x, (size_t)T);
  w.vals = s.alloc<double>(NM * w.sc_max);
  return true;
}
// the sc samples from s0 on
void sweep_chunk(FuncSweep& w, int s0, int sc) {
  FuncArgs& f = w.f;
  const int rowblocks = (f.N + WAVE - 1) / WAVE, JMAX = 65535;   // (a grid's y extent)
  f.W = w.dW + (size_t)s0 * f.N * w.K; f.V = w.dV + (size_t)s0 * f.M * f.T * w.K; f.S = sc;
  for (int j0 = 0; j0 < f.M; j0 += JMAX) {
    f.j0 = j0; f.jc = std::min(JMAX, f.M - j0); f.vals = w.vals + (size_t)j0 * sc * f.N;
    launch_counted(*w.s, BTF_K_CRITERIA, w.kern, dim3(rowblocks, f.jc, func_sweep_slices(sc, rowblocks, f.jc)), dim3(FUNC_WAVES * WAVE), 0, f);
  }
}
}  // namespace

// posterior summaries straight from the collected samples (no upload); see btf_posterior_summary
int btf_collect_summary(btf_ctx* c, int nsamples, int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (!c || nsamples < 1 || nsamples > c->smp_n || nsamples > 16384 || !mean_out || nq < 0 || (nq > 0 && (!q || !q_out)) ||
      transform < 0 || transform > 2)
    return fail(c, BTF_EINVAL, "bad collect_summary arguments");
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_summary", BTF_EINVAL, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  summary_stage(s, st.W, st.V, nsamples, c->N, c->M * c->T, c->K, transform, q, nq, mean_out, q_out);
  return s.finish();
}

// ---------------------------------------------------------- model-selection criteria (btf_criteria.h)
int btf_crit_set_data(btf_ctx* c, int slot, const double* S1, const double* cnt, const double* curve_c0, const double* curve_c1) {
  if (!c || slot < 0 || slot > 1) return fail(c, BTF_EINVAL, "criteria slot must be 0 or 1");
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));        // (a criteria call still reading the old statistics)
  double** bufs[4] = {&c->crit_S1[slot], &c->crit_cnt[slot], &c->crit_c0[slot], &c->crit_c1[slot]};
  if (c->crit_L[slot]) { (void)hipFree(c->crit_L[slot]); c->crit_L[slot] = nullptr; }      // (the old data's log sums)
  if (c->crit_Y[slot]) { (void)hipFree(c->crit_Y[slot]); c->crit_Y[slot] = nullptr; c->crit_nreps[slot] = 0; }   // (and raw counts)
  if (!S1 && !cnt && !curve_c0 && !curve_c1) {       // free the slot
    for (double** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
    return BTF_OK;
  }
  if (!S1 || !cnt || !curve_c0 || !curve_c1) return fail(c, BTF_EINVAL, "btf_crit_set_data: all four arrays, or none");
  const size_t cells = (size_t)c->M * c->T * c->N, curves = (size_t)c->N * c->M;
  const double* src[4] = {S1, cnt, curve_c0, curve_c1};
  const size_t n[4] = {cells, cells, curves, curves};
  for (int q = 0; q < 4; ++q) {
    int rc;
    if ((rc = dev_alloc(c, bufs[q], n[q]))) return rc;
    HIPCHK(c, hipMemcpyAsync(*bufs[q], src[q], n[q] * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BTF_OK;
}

int btf_crit_set_logsum(btf_ctx* c, int slot, const double* L) {
  if (!c || slot < 0 || slot > 1) return fail(c, BTF_EINVAL, "criteria slot must be 0 or 1");
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));        // (a criteria call still reading the old statistic)
  if (!L) {
    if (c->crit_L[slot]) (void)hipFree(c->crit_L[slot]);
    c->crit_L[slot] = nullptr;
    return BTF_OK;
  }
  if (!c->crit_S1[slot]) return fail(c, BTF_ESTATE, "btf_crit_set_logsum: no statistics in this slot (btf_crit_set_data first)");
  const size_t cells = (size_t)c->M * c->T * c->N;
  int rc;
  if ((rc = dev_alloc(c, &c->crit_L[slot], cells))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->crit_L[slot], L, cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BTF_OK;
}

int btf_crit_set_counts(btf_ctx* c, int slot, const double* Y, int nreps) {
  if (!c || slot < 0 || slot > 1) return fail(c, BTF_EINVAL, "criteria slot must be 0 or 1");
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));        // (a criteria call still reading the old counts)
  if (!Y) {
    if (c->crit_Y[slot]) (void)hipFree(c->crit_Y[slot]);
    c->crit_Y[slot] = nullptr; c->crit_nreps[slot] = 0;
    return BTF_OK;
  }
  if (nreps < 1) return fail(c, BTF_EINVAL, "btf_crit_set_counts: nreps >= 1");
  if (!c->crit_S1[slot]) return fail(c, BTF_ESTATE, "btf_crit_set_counts: no statistics in this slot (btf_crit_set_data first)");
  // [N][M][T][nreps] -> [M][T * nreps][N]: one lane per row, so that the kernel's loads coalesce
  const size_t N = (size_t)c->N, MF = (size_t)c->M * c->T * nreps;
  std::vector<double> yt(N * MF);
  for (size_t i = 0; i < N; ++i)
    for (size_t f = 0; f < MF; ++f) {
      const double y = Y[i * MF + f];
      if (y < 0.0 || std::isinf(y)) return fail(c, BTF_EINVAL, "btf_crit_set_counts: an observed count must be finite and >= 0");
      yt[f * N + i] = y;
    }
  int rc;
  if ((rc = dev_alloc(c, &c->crit_Y[slot], yt.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->crit_Y[slot], yt.data(), yt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->crit_nreps[slot] = nreps;
  return BTF_OK;
}

namespace {
// the rates of a Negative-Binomial criteria call (btf_nb_crit_eval / btf_nb_crit_loo): (S + 1, extent) on the host
struct NbIn { const double* rates; int aux_flags; };

// families 0..4 of FAM_SWITCH, or the gamma-grid family of btf_gg_criteria.h
bool crit_family_ok(int family) { return (family >= 0 && family < CRIT_FAM_COUNT) || family == CRIT_FAM_GAMMA_GRID; }

// the device side of a criteria call: its scratch (the uploaded states, crit_kernel's outputs) and the kernels' arguments
struct CritRun {
  Scratch s;
  CritArgs a{};
  double* tot = nullptr;      // [S] per-sample totals (crit_total_kernel)
  explicit CritRun(btf_ctx* c) : s(c, c->stream) {}
};

// Checks the arguments that btf_crit_eval and btf_crit_loo share, uploads the states and queues crit_kernel (with
// `reduce` also the plug-in and per-sample-total kernels) on the context's stream.  `who` names the caller in messages.
// nb: the Negative-Binomial model's sampled rates (btf_nb_criteria.h) - family 4's term with the rate of every sample, the
// constant kernel ahead of it; family / param / noise are then unused.
int crit_run(btf_ctx* c, const std::string& who, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
             const double* noise, int flags, bool pointwise, bool reduce, CritRun& r, const NbIn* nb = nullptr) {
  if (!c->crit_S1[slot]) return fail(c, BTF_ESTATE, who + ": no statistics in this slot (btf_crit_set_data)");
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, who + " needs an unsharded context");
  const bool current = (flags & BTF_CRIT_CURRENT) != 0, per_sample = (flags & BTF_CRIT_NOISE_PER_SAMPLE) != 0;
  if (current && (Ws || nsamples != 1 || !c->have_W || !c->have_V))
    return fail(c, BTF_EINVAL, "BTF_CRIT_CURRENT scores the context's own W, V: one sample, Ws = Vs = NULL");
  if (!Ws && !current && !has_collected(c, nsamples)) return no_collected(c, BTF_ESTATE, who);
  if (per_sample && family != CRIT_FAM_GAUSSIAN) return fail(c, BTF_EINVAL, "per-sample noise is the Gaussian family's");
  if (per_sample && !noise && (Ws || current)) return fail(c, BTF_EINVAL, "per-sample noise of uploaded / current states: pass `noise`");
  if (!nb && !per_sample && (family == CRIT_FAM_GAUSSIAN || family == CRIT_FAM_NEGBIN) && !(param > 0.0))
    return fail(c, BTF_EINVAL, "the Gaussian (variance) and Negative-Binomial (rate) families need param > 0");
  const bool gamma_grid = !nb && family == CRIT_FAM_GAMMA_GRID;
  NbRate rt{};
  if (nb) {
    if (!c->crit_Y[slot]) return fail(c, BTF_ESTATE, who + ": no counts in this slot (btf_crit_set_counts)");
    const long long n0 = (nb->aux_flags & BTF_PRED_AUX_ROWS) ? c->N : 1, n1 = (nb->aux_flags & BTF_PRED_AUX_COLS) ? c->M : 1,
                    n2 = (nb->aux_flags & BTF_PRED_AUX_DEPTH) ? c->T : 1;
    rt.ext = n0 * n1 * n2; rt.sr2 = n2 > 1 ? 1 : 0; rt.sr1 = n1 > 1 ? n2 : 0; rt.sr0 = n0 > 1 ? n1 * n2 : 0;
    const size_t nr = (size_t)(nsamples + 1) * (size_t)rt.ext;
    for (size_t q = 0; q < nr; ++q)
      if (!(nb->rates[q] > 0.0) || !std::isfinite(nb->rates[q]))
        return fail(c, BTF_EINVAL, who + ": every rate must be finite and > 0 (sample " + std::to_string(q / (size_t)rt.ext) + ")");
  }
  if (gamma_grid && (!c->gg_tab || !c->crit_L[slot]))
    return fail(c, BTF_ESTATE, who + ": the gamma-grid family needs its table (btf_set_likelihood_table) and the slot's L (btf_crit_set_logsum)");
  HIPCHK(c, hipSetDevice(c->dev));
  const int S = nsamples, N = c->N, M = c->M, T = c->T, K = c->K;
  const dim3 grid((N + WAVE - 1) / WAVE, M);
  const int nwg = (int)(grid.x * grid.y);
  const size_t NM = (size_t)N * M;
  Scratch& s = r.s;
  CritArgs& a = r.a;
  a.S1 = c->crit_S1[slot]; a.cnt = c->crit_cnt[slot]; a.c0 = c->crit_c0[slot]; a.c1 = c->crit_c1[slot];
  const States st = resolve_states(c, s, S, Ws, Vs, current, per_sample, noise, 1);
  a.W = st.W; a.V = st.V; a.noise = st.noise; a.noise_stride = st.noise_stride;
  a.par = param; a.S = S; a.N = N; a.M = M; a.T = T;
  a.mu = s.alloc<double>((size_t)M * T * N); a.curve = s.alloc<double>(CRIT_OUT * NM);
  a.tot_part = s.alloc<double>((size_t)S * nwg); r.tot = s.alloc<double>((size_t)S);
  if (pointwise) a.pw = s.alloc<double>((size_t)S * NM);
  const GgTab gt{c->crit_L[slot], c->gg_tab, c->gg_G, c->gg_lsp};
  const double* nbC = nullptr;      // [S + 1][M][N]: the per-sample curve constants
  const bool nb_rows = rt.sr0 != 0;
  if (nb) {
    rt.R = s.upload(nb->rates, (size_t)(S + 1) * (size_t)rt.ext);
    NbConstArgs ca{c->crit_Y[slot], c->crit_nreps[slot], S + 1, N, M, T, rt, s.alloc<double>((size_t)(S + 1) * NM)};
    nbC = ca.C;
    // one rate per (sample, column): the table form (an A/B switch for measurements: BTF_NB_CRIT_TABLE=0)
    static const bool tab_ok = [] { const char* e = std::getenv("BTF_NB_CRIT_TABLE"); return !e || std::atoi(e) != 0; }();
    const bool tabbed = tab_ok && rt.sr0 == 0 && rt.sr2 == 0;
    launch_counted(s, BTF_K_CRITERIA, tabbed ? nb_crit_const_tab_fn() : nb_crit_const_fn(nb_rows), grid, dim3(CRIT_WAVES * WAVE), 0, ca);
    launch_counted(s, BTF_K_CRITERIA, nb_crit_fn(K, nb_rows), grid, dim3(CRIT_WAVES * WAVE), 0, a, rt, nbC);
  }
  else if (gamma_grid) launch_counted(s, BTF_K_CRITERIA, gg_crit_fn(K), grid, dim3(GGC_WAVES * WAVE), 0, a, gt);
  else K_SWITCH(K, FAM_SWITCH(family, launch_counted(s, BTF_K_CRITERIA, crit_kernel<KT, FT>, grid, dim3(CRIT_WAVES * WAVE), 0, a)));
  if (reduce) {
    if (nb) launch_counted(s, BTF_K_CRITERIA, nb_crit_plugin_fn(nb_rows), grid, dim3(WAVE), 0, a, rt, nbC);
    else if (gamma_grid) launch_counted(s, BTF_K_CRITERIA, gg_crit_plugin_fn(), grid, dim3(WAVE), 0, a, gt);
    else FAM_SWITCH(family, launch_counted(s, BTF_K_CRITERIA, crit_plugin_kernel<FT>, grid, dim3(WAVE), 0, a));
    launch_counted(s, BTF_K_CRITERIA, crit_total_kernel, dim3((S + 255) / 256), dim3(256), 0, (const double*)a.tot_part, S, nwg, r.tot);
  }
  return s.rc();
}
}  // namespace

namespace {
// btf_crit_eval and btf_nb_crit_eval (nb: its rates) after their argument checks
int crit_eval_run(btf_ctx* c, const char* who, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
                  const double* noise, int flags, double* curve_out, double* total_out, double* pointwise_out, const NbIn* nb) {
  CritRun r(c);
  int rc = crit_run(c, who, slot, family, param, nsamples, Ws, Vs, noise, flags, pointwise_out != nullptr, true, r, nb);
  if (rc) return rc;
  const size_t S = (size_t)nsamples, NM = (size_t)c->N * c->M;
  r.s.download(curve_out, r.a.curve, CRIT_OUT * NM);
  r.s.download(total_out, r.tot, S);
  r.s.download(pointwise_out, r.a.pw, S * NM);
  return r.s.finish();        // (not check_status: the sampler's status word is not this call's)
}
bool nb_flags_ok(int aux_flags) {
  return !(aux_flags & ~(BTF_PRED_AUX_PER_SAMPLE | BTF_PRED_AUX_ROWS | BTF_PRED_AUX_COLS | BTF_PRED_AUX_DEPTH));
}
}  // namespace

int btf_crit_eval(btf_ctx* c, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
                  const double* noise, int flags, double* curve_out, double* total_out, double* pointwise_out) {
  if (!c || slot < 0 || slot > 1 || !crit_family_ok(family) || nsamples < 1 || !curve_out || !total_out ||
      (flags & ~(BTF_CRIT_NOISE_PER_SAMPLE | BTF_CRIT_CURRENT)) || (!Ws) != (!Vs))
    return fail(c, BTF_EINVAL, "bad btf_crit_eval arguments");
  return crit_eval_run(c, "btf_crit_eval", slot, family, param, nsamples, Ws, Vs, noise, flags, curve_out, total_out, pointwise_out, nullptr);
}

int btf_nb_crit_eval(btf_ctx* c, int slot, int nsamples, const double* Ws, const double* Vs, const double* rates, int aux_flags,
                     int flags, double* curve_out, double* total_out, double* pointwise_out) {
  if (!c || slot < 0 || slot > 1 || nsamples < 1 || !curve_out || !total_out || !rates || !nb_flags_ok(aux_flags) ||
      (flags & ~BTF_CRIT_CURRENT) || (!Ws) != (!Vs))
    return fail(c, BTF_EINVAL, "bad btf_nb_crit_eval arguments");
  const NbIn nb{rates, aux_flags};
  return crit_eval_run(c, "btf_nb_crit_eval", slot, CRIT_FAM_NEGBIN, 0.0, nsamples, Ws, Vs, nullptr, flags, curve_out, total_out,
                       pointwise_out, &nb);
}

// ---------------------------------------------------------- PSIS-LOO (btf_loo.h)
namespace {
// btf_crit_loo and btf_nb_crit_loo (nb: its rates) after their argument checks, under the name `who`
int crit_loo_run(btf_ctx* c, const std::string& who, int slot, int family, double param, int nsamples, const double* Ws,
                 const double* Vs, const double* noise, int flags, const double* r_eff, int transform, double* loo_out,
                 double* mean_out, double* logw_out, const NbIn* nb) {
  if (nsamples > LOO_MAX_S)
    return fail(c, BTF_EINVAL, who + ": " + std::to_string(nsamples) + " samples, at most " + std::to_string(LOO_MAX_S));
  const int S = nsamples, N = c->N, M = c->M, T = c->T;
  const size_t NM = (size_t)N * M;
  // the tail length Mt = min(floor(0.2 S), ceil(3 sqrt(S / r_eff))) of every curve, on the host: IEEE sqrt and division
  auto tail = [S](double re) { return (int)std::min((double)(S / 5), std::ceil(3.0 * std::sqrt((double)S / re))); };
  std::vector<int> mt;
  if (r_eff) {
    mt.resize(NM);
    for (size_t o = 0; o < NM; ++o) {
      if (!(r_eff[o] > 0.0) || !std::isfinite(r_eff[o]))
        return fail(c, BTF_EINVAL, who + ": r_eff must be finite and > 0 (curve " + std::to_string(o) + ")");
      mt[o] = tail(r_eff[o]);
    }
  }
  CritRun r(c);
  int rc = crit_run(c, who, slot, family, param, nsamples, Ws, Vs, noise, flags, true, false, r, nb);
  if (rc) return rc;
  Scratch& s = r.s;
  double* dloo = s.alloc<double>(2 * NM);
  LooArgs a{};
  a.pw = r.a.pw; a.mt = r_eff ? s.upload(mt.data(), NM) : nullptr; a.mt_all = tail(1.0); a.S = S; a.NM = (int)NM; a.out = dloo;
  a.P = 64; while (a.P < S) a.P <<= 1;
  a.per_xcd = (int)((NM + 7) / 8);
  const size_t lds = (size_t)a.P * (2 * sizeof(double) + sizeof(unsigned short));
  void (*const psis)(LooArgs) = (mean_out || logw_out) ? loo_psis_kernel<1> : loo_psis_kernel<0>;      // <1> keeps the log weights
  allow_lds(s, psis, lds);
  launch_counted(s, BTF_K_CRITERIA, psis, dim3(8 * a.per_xcd), dim3(WAVE), lds, a);
  if (mean_out) {
    LooMeanArgs ma{};
    ma.lw = r.a.pw; ma.W = r.a.W; ma.V = r.a.V; ma.S = S; ma.N = N; ma.M = M; ma.T = T; ma.transform = transform;
    ma.mean = s.alloc<double>(NM * T);
    K_SWITCH(c->K, launch_counted(s, BTF_K_CRITERIA, loo_mean_kernel<KT>, dim3((N + WAVE - 1) / WAVE, M), dim3(LOO_WAVES * WAVE), 0, ma));
    s.download(mean_out, ma.mean, NM * T);
  }
  // loo_out: elpd_loo, pareto_k, then crit_kernel's two accumulators of lppd (curve_out[0], [1] of btf_crit_eval)
  s.download(loo_out, dloo, 2 * NM);
  s.download(loo_out + 2 * NM, r.a.curve, 2 * NM);
  s.download(logw_out, r.a.pw, (size_t)S * NM);
  return s.finish();
}
}  // namespace

int btf_crit_loo(btf_ctx* c, int slot, int family, double param, int nsamples, const double* Ws, const double* Vs,
                 const double* noise, int flags, const double* r_eff, int transform, double* loo_out, double* mean_out,
                 double* logw_out) {
  if (!c || slot < 0 || slot > 1 || !crit_family_ok(family) || nsamples < 1 || !loo_out ||
      (flags & ~BTF_CRIT_NOISE_PER_SAMPLE) || (!Ws) != (!Vs) || transform < 0 || transform > 2)
    return fail(c, BTF_EINVAL, "bad btf_crit_loo arguments");
  return crit_loo_run(c, "btf_crit_loo", slot, family, param, nsamples, Ws, Vs, noise, flags, r_eff, transform, loo_out, mean_out,
                      logw_out, nullptr);
}

int btf_nb_crit_loo(btf_ctx* c, int slot, int nsamples, const double* Ws, const double* Vs, const double* rates, int aux_flags,
                    const double* r_eff, int transform, double* loo_out, double* mean_out, double* logw_out) {
  if (!c || slot < 0 || slot > 1 || nsamples < 1 || !loo_out || !rates || !nb_flags_ok(aux_flags) || (!Ws) != (!Vs) ||
      transform < 0 || transform > 2)
    return fail(c, BTF_EINVAL, "bad btf_nb_crit_loo arguments");
  const NbIn nb{rates, aux_flags};
  return crit_loo_run(c, "btf_nb_crit_loo", slot, CRIT_FAM_NEGBIN, 0.0, nsamples, Ws, Vs, nullptr, 0, r_eff, transform, loo_out,
                      mean_out, logw_out, &nb);
}

// ---------------------------------------------------------- posterior predictive (btf_predict.h)
int btf_predict_batch(int device, int family, int64_t n, const double* eta, const double* aux, uint64_t seed, double* out) {
  if (family < 0 || family >= PRED_FAM_COUNT || n < 1 || !eta || !aux || !out) return fail(nullptr, BTF_EINVAL, "bad predict_batch arguments");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double *de = s.upload(eta, (size_t)n), *da = s.upload(aux, (size_t)n);
  double* dout = s.alloc<double>((size_t)n);
  const dim3 grid((unsigned)((n + PRED_THREADS - 1) / PRED_THREADS)), block(PRED_THREADS);
  FAM_SWITCH(family, s.launch(pred_batch_kernel<FT>, grid, block, 0, de, da, (long long)n, (unsigned long long)seed, dout));
  s.download(out, dout, (size_t)n);
  return s.finish();
}

namespace {
// where the outputs of btf_predict_eval / btf_predict_gg_eval go on the host, in the order of their arguments
struct PredOut { double *mean, *ymean, *yvar, *q, *pit_lo, *pit_hi, *inside, *nobs, *rmse, *mae, *draws; };
struct PredKernels { void (*draw)(PredArgs); void (*score)(PredArgs); };
PredKernels pred_kernels(int family) {
  PredKernels k{nullptr, nullptr};
  if (family == PRED_FAM_GAMMA_GRID) { k.draw = gg_pred_fn(); k.score = gg_pred_score_fn(); }
  else FAM_SWITCH(family, { k.draw = pred_kernel<FT>; k.score = pred_score_kernel<FT>; });
  return k;
}

// What btf_predict_eval, btf_predict_gg_eval and btf_predict_check decide alike, under the name `who`.
// the arguments every one of them takes the same way
bool pred_head_bad(int nsamples, const double* Ws, const double* Vs, int aux_flags) {
  return nsamples < 1 || (!Ws) != (!Vs) ||
         (aux_flags & ~(BTF_PRED_AUX_PER_SAMPLE | BTF_PRED_AUX_ROWS | BTF_PRED_AUX_COLS | BTF_PRED_AUX_DEPTH));
}
// the context, the states and the family's parameter: refused here, in this order
int pred_states_ok(btf_ctx* c, const std::string& who, int family, double param, int nsamples, const double* Ws, const double* aux_sample,
                   int aux_flags) {
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, who + " needs an unsharded context");
  if (!Ws && !has_collected(c, nsamples)) return no_collected(c, BTF_ESTATE, who);
  const bool per_sample = (aux_flags & BTF_PRED_AUX_PER_SAMPLE) != 0;
  const bool needs_par = family == PRED_FAM_GAUSSIAN || family == PRED_FAM_NEGBIN;
  if (per_sample && !needs_par) return fail(c, BTF_EINVAL, "per-sample parameters are the Gaussian (variance) and Negative-Binomial (rate) families'");
  if (per_sample && !aux_sample && (Ws || family != PRED_FAM_GAUSSIAN))
    return fail(c, BTF_EINVAL, "per-sample parameters of uploaded states (and every Negative-Binomial rate): pass aux_sample");
  if (!per_sample && needs_par && !(param > 0.0))
    return fail(c, BTF_EINVAL, "the Gaussian (variance) and Negative-Binomial (rate) families need param > 0");
  return BTF_OK;
}
// the extent of the per-sample parameter along rows / columns / depth into `a`; returns its size per sample
size_t pred_aux_layout(PredArgs& a, int family, int aux_flags, int N, int M, int T) {
  a.aux_n0 = a.aux_n1 = a.aux_n2 = 1;
  if ((aux_flags & BTF_PRED_AUX_PER_SAMPLE) && family == PRED_FAM_NEGBIN) {
    a.aux_n0 = (aux_flags & BTF_PRED_AUX_ROWS) ? N : 1; a.aux_n1 = (aux_flags & BTF_PRED_AUX_COLS) ? M : 1; a.aux_n2 = (aux_flags & BTF_PRED_AUX_DEPTH) ? T : 1;
  }
  return (size_t)a.aux_n0 * a.aux_n1 * a.aux_n2;
}
// the states, the per-sample parameter, the trials and the observations on the device, into `a`
void pred_upload(btf_ctx* c, Scratch& s, PredArgs& a, int S, const double* Ws, const double* Vs, bool per_sample, const double* aux_sample,
                 size_t naux, const double* trials, const double* Y, int nreps, size_t ncell) {
  const States st = resolve_states(c, s, S, Ws, Vs, false, per_sample, aux_sample, naux);
  a.W = st.W; a.V = st.V; a.aux = st.noise; a.aux_stride = st.noise_stride;
  if (trials) a.trials = s.upload(trials, ncell);
  if (Y) { a.Y = s.upload(Y, ncell * (size_t)nreps); a.nreps = nreps; }
}

// btf_predict_eval (families 0..4) and btf_predict_gg_eval (family 5: the context's table, param = its mbar) under the
// name `who`: one set of limits and refusals, one launch geometry
int predict_run(btf_ctx* c, const std::string& who, int family, double param, int nsamples, const double* Ws, const double* Vs,
                const double* aux_sample, int aux_flags, const double* trials, const double* Y, int nreps, int draws_per_sample,
                uint64_t seed, const double* q, int nq, const int32_t* cells, int ncells, const PredOut& o) {
  double *const mean_out = o.mean, *const ymean_out = o.ymean, *const yvar_out = o.yvar, *const q_out = o.q, *const pit_lo_out = o.pit_lo,
         *const pit_hi_out = o.pit_hi, *const inside_out = o.inside, *const nobs_out = o.nobs, *const rmse_out = o.rmse,
         *const mae_out = o.mae, *const draws_out = o.draws;
  const bool gamma_grid = family == PRED_FAM_GAMMA_GRID;
  if (!c || (!gamma_grid && (family < 0 || family >= PRED_FAM_COUNT)) || pred_head_bad(nsamples, Ws, Vs, aux_flags) || draws_per_sample < 1 ||
      nq < 0 || (nq > 0 && !q) || (q_out && nq < 1) || ncells < 0 || (ncells > 0 && (!cells || !draws_out)) || (Y && nreps < 1))
    return fail(c, BTF_EINVAL, "bad " + who + " arguments");
  if (gamma_grid && c->gg_pred.empty())
    return fail(c, BTF_ESTATE, who + ": the gamma-grid family needs its table (btf_set_likelihood_table)");
  if (!Y && (pit_lo_out || pit_hi_out || inside_out || nobs_out || rmse_out || mae_out))
    return fail(c, BTF_EINVAL, who + ": pit / inside / nobs / rmse / mae compare with observations: pass Y");
  if ((long long)nsamples * draws_per_sample > PRED_MAX_DRAWS)
    return fail(c, BTF_EINVAL, who + ": nsamples * draws_per_sample = " + std::to_string((long long)nsamples * draws_per_sample) +
                " exceeds 16384 (the draws of a cell are sorted in LDS)");
  if (int rc = pred_states_ok(c, who, family, param, nsamples, Ws, aux_sample, aux_flags)) return rc;
  const bool per_sample = (aux_flags & BTF_PRED_AUX_PER_SAMPLE) != 0;
  if (int rc = check_percentiles(c, q, nq)) return rc;
  const int S = nsamples, R = draws_per_sample, N = c->N, M = c->M, T = c->T, K = c->K, MT = M * T, n = S * R;
  const size_t ncell = (size_t)N * MT;
  if (ncell > 0x7fffffffULL) return fail(c, BTF_EINVAL, who + ": more than 2^31 - 1 cells");
  for (int k = 0; k < ncells; ++k)
    if (cells[k] < 0 || (size_t)cells[k] >= ncell) return fail(c, BTF_EINVAL, who + ": cell index out of range");
  HIPCHK(c, hipSetDevice(c->dev));
  PredArgs a{};
  const size_t naux = pred_aux_layout(a, family, aux_flags, N, M, T);
  const SortGeom g = sort_geom(n, pred_row_budget(gamma_grid ? GGP_TAB_DOUBLES * sizeof(double) : 0), PRED_SORT_CELLS);
  const size_t nblk = (size_t)N * ((MT + g.cells - 1) / g.cells);
  if (nblk > 0x7fffffffULL) return fail(c, BTF_EINVAL, who + ": too many workgroups for one launch");
  const int chunks = (int)((ncell + PRED_SCORE_CELLS - 1) / PRED_SCORE_CELLS);
  const bool score = rmse_out || mae_out;
  Scratch s(c, c->stream);
  pred_upload(c, s, a, S, Ws, Vs, per_sample, aux_sample, naux, trials, Y, nreps, ncell);
  if (nq) a.q = s.upload(q, (size_t)nq);
  a.nq = nq;
  if (ncells) { a.list = s.upload(cells, (size_t)ncells); a.nlist = ncells; a.draws = s.alloc<double>((size_t)ncells * n); }
  if (mean_out) a.mean = s.alloc<double>(ncell);
  if (ymean_out) a.y_mean = s.alloc<double>(ncell);
  if (yvar_out) a.y_var = s.alloc<double>(ncell);
  if (q_out) a.quant = s.alloc<double>((size_t)nq * ncell);
  if (pit_lo_out) a.pit_lo = s.alloc<double>(ncell);
  if (pit_hi_out) a.pit_hi = s.alloc<double>(ncell);
  if (inside_out) a.inside = s.alloc<double>(ncell);
  if (nobs_out) a.nobs = s.alloc<double>(ncell);
  double* dsc = nullptr;      // [rmse | mae] per sample
  if (score) { a.score_part = s.alloc<double>((size_t)3 * S * chunks); dsc = s.alloc<double>((size_t)2 * S); }
  a.par = param; a.S = S; a.R = R; a.N = N; a.M = M; a.T = T; a.K = K; a.P = g.P; a.cells = g.cells; a.seed = seed; a.chunks = chunks;
  if (gamma_grid) { a.gg_G = (int)(c->gg_pred.size() / 3); a.gg = s.upload(c->gg_pred.data(), c->gg_pred.size()); }
  const PredKernels k = pred_kernels(family);
  allow_lds(s, k.draw, g.lds);
  s.launch(k.draw, dim3((unsigned)nblk), dim3(PRED_THREADS), g.lds, a);
  if (score) s.launch(k.score, dim3(chunks, S), dim3(PRED_THREADS), 0, a);
  if (score) s.launch(pred_score_total_kernel, dim3((S + 255) / 256), dim3(256), 0, (const double*)a.score_part, S, chunks, dsc);
  s.download(mean_out, a.mean, ncell); s.download(ymean_out, a.y_mean, ncell); s.download(yvar_out, a.y_var, ncell);
  s.download(q_out, a.quant, (size_t)nq * ncell);
  s.download(pit_lo_out, a.pit_lo, ncell); s.download(pit_hi_out, a.pit_hi, ncell); s.download(inside_out, a.inside, ncell);
  s.download(nobs_out, a.nobs, ncell);
  if (score && !s.rc()) { s.download(rmse_out, dsc, (size_t)S); s.download(mae_out, dsc + S, (size_t)S); }
  if (ncells) s.download(draws_out, a.draws, (size_t)ncells * n);
  return s.finish();        // (not check_status: the sampler's status word is not this call's)
}
}  // namespace

int btf_predict_eval(btf_ctx* c, int family, double param, int nsamples, const double* Ws, const double* Vs,
                     const double* aux_sample, int aux_flags, const double* trials, const double* Y, int nreps,
                     int draws_per_sample, uint64_t seed, const double* q, int nq, const int32_t* cells, int ncells,
                     double* mean_out, double* ymean_out, double* yvar_out, double* q_out, double* pit_lo_out, double* pit_hi_out,
                     double* inside_out, double* nobs_out, double* rmse_out, double* mae_out, double* draws_out) {
  if (family == PRED_FAM_GAMMA_GRID) family = -1;       // (its own entry point: btf_predict_gg_eval)
  return predict_run(c, "btf_predict_eval", family, param, nsamples, Ws, Vs, aux_sample, aux_flags, trials, Y, nreps, draws_per_sample, seed,
                     q, nq, cells, ncells, PredOut{mean_out, ymean_out, yvar_out, q_out, pit_lo_out, pit_hi_out, inside_out, nobs_out,
                                                   rmse_out, mae_out, draws_out});
}

// ---------------------------------------------------------- the same for the gamma-grid likelihood (btf_gg_predict.h)
int btf_predict_gg_eval(btf_ctx* c, int nsamples, const double* Ws, const double* Vs, const double* Y, int nreps, int draws_per_sample,
                        uint64_t seed, const double* q, int nq, const int32_t* cells, int ncells,
                        double* mean_out, double* ymean_out, double* yvar_out, double* q_out, double* pit_lo_out, double* pit_hi_out,
                        double* inside_out, double* nobs_out, double* rmse_out, double* mae_out, double* draws_out) {
  return predict_run(c, "btf_predict_gg_eval", PRED_FAM_GAMMA_GRID, c ? c->gg_mbar : 0.0, nsamples, Ws, Vs, nullptr, 0, nullptr, Y, nreps,
                     draws_per_sample, seed, q, nq, cells, ncells, PredOut{mean_out, ymean_out, yvar_out, q_out, pit_lo_out, pit_hi_out,
                                                                           inside_out, nobs_out, rmse_out, mae_out, draws_out});
}

// ---------------------------------------------------------- posterior predictive checks (btf_checks.h)
int btf_predict_check(btf_ctx* c, int family, double param, int nsamples, const double* Ws, const double* Vs, const double* aux_sample,
                      int aux_flags, const double* trials, const double* Y, int nreps, int reps, uint64_t seed, const int32_t* which,
                      int nwhich, const int32_t* curves, int ncurves, int chunk_rows, double* curve_out, double* nobs_out,
                      double* pool_obs_out, double* pool_rep_out, double* tobs_out, double* trep_out) {
  const std::string who = "btf_predict_check";
  if (!c || family < 0 || family >= PRED_FAM_COUNT || pred_head_bad(nsamples, Ws, Vs, aux_flags) || !Y || nreps < 1 || !which || nwhich < 1 ||
      nwhich > CHK_COUNT || ncurves < 0 || (ncurves > 0 && (!curves || !tobs_out || !trep_out)) || chunk_rows < 0)
    return fail(c, BTF_EINVAL, "bad " + who + " arguments");
  if (reps < 1) return fail(c, BTF_EINVAL, who + ": reps must be >= 1");
  bool seen[CHK_COUNT] = {false};
  for (int k = 0; k < nwhich; ++k) {
    if (which[k] < 0 || which[k] >= CHK_COUNT || seen[which[k]]) return fail(c, BTF_EINVAL, who + ": discrepancy codes must be distinct and in 0..4");
    seen[which[k]] = true;
  }
  if (int rc = pred_states_ok(c, who, family, param, nsamples, Ws, aux_sample, aux_flags)) return rc;
  const bool per_sample = (aux_flags & BTF_PRED_AUX_PER_SAMPLE) != 0;
  const int S = nsamples, N = c->N, M = c->M, T = c->T, K = c->K;
  static_assert(CHK_MAX_K == MAX_K, "chk_kernel keeps w in MAX_K registers");
  const size_t NM = (size_t)N * M, ncell = NM * T;
  if (ncell > 0x7fffffffULL) return fail(c, BTF_EINVAL, who + ": more than 2^31 - 1 cells");
  const long long nsets_ll = (long long)S * reps, Rr_ll = (long long)reps * nreps;
  // the draw index g = cell n + d owns PRED_BLOCKS generator blocks: g PRED_BLOCKS stays below 2^64
  if (nsets_ll > 0x7fffffffLL || Rr_ll > 0x7fffffffLL || (double)ncell * (double)nsets_ll * (double)nreps >= 18446744073709551616.0 / PRED_BLOCKS)
    return fail(c, BTF_EINVAL, who + ": nsamples * reps * nreps = " + std::to_string(nsets_ll * nreps) + " draws a cell overflow the 64-bit draw index");
  for (int k = 0; k < ncurves; ++k)
    if (curves[k] < 0 || (size_t)curves[k] >= NM) return fail(c, BTF_EINVAL, who + ": curve index out of range");
  const int nsets = (int)nsets_ll, tiles = (M + CHK_TILE - 1) / CHK_TILE;
  // rows per launch: what CHK_PART_BYTES of pooled partials hold (one row is the least), or the caller's chunk
  const size_t row_bytes = (size_t)tiles * 2 * CHK_SLOTS * nsets * sizeof(double);
  long long rows_max = std::max<long long>(1, (long long)(CHK_PART_BYTES / row_bytes));
  if (chunk_rows > 0) rows_max = std::min<long long>(rows_max, chunk_rows);
  rows_max = std::min<long long>(rows_max, N);
  if ((unsigned long long)rows_max * tiles > 0x7fffffffULL) return fail(c, BTF_EINVAL, who + ": too many workgroups for one launch");
  HIPCHK(c, hipSetDevice(c->dev));
  ChkArgs a{};
  const size_t naux = pred_aux_layout(a.p, family, aux_flags, N, M, T);
  Scratch s(c, c->stream);
  pred_upload(c, s, a.p, S, Ws, Vs, per_sample, aux_sample, naux, trials, Y, nreps, ncell);
  a.p.par = param; a.p.S = S; a.p.R = (int)Rr_ll; a.p.N = N; a.p.M = M; a.p.T = T; a.p.K = K; a.p.seed = seed;
  a.reps = reps; a.nsets = nsets; a.tiles = tiles;
  // listed curves: each distinct one gets a slot of the device arrays; the host copies slots to the rows of the list
  std::vector<int> slot_of, list_slot(ncurves);
  int nslots = 0;
  if (ncurves) {
    slot_of.assign(NM, -1);
    for (int k = 0; k < ncurves; ++k) {
      if (slot_of[curves[k]] < 0) slot_of[curves[k]] = nslots++;
      list_slot[k] = slot_of[curves[k]];
    }
    a.listed = s.upload(slot_of.data(), NM);
    a.t_obs = s.alloc<double>((size_t)nslots * CHK_COUNT * nsets);
    a.t_rep = s.alloc<double>((size_t)nslots * CHK_COUNT * nsets);
  }
  a.cur = s.alloc<double>((size_t)CHK_OUTS * CHK_COUNT * NM);
  a.nobs = s.alloc<double>(NM);
  a.part = s.alloc<double>((size_t)rows_max * row_bytes / sizeof(double));
  const size_t npool = (size_t)2 * CHK_SLOTS * nsets;
  double* tot = s.alloc<double>(npool);
  void (*kern)(ChkArgs) = nullptr;
  FAM_SWITCH(family, kern = chk_kernel<FT>);
  for (int row0 = 0; row0 < N; row0 += (int)rows_max) {
    a.row0 = row0; a.rows = std::min<int>((int)rows_max, N - row0);
    s.launch(kern, dim3((unsigned)((size_t)a.rows * tiles)), dim3(CHK_THREADS), 0, a);
    s.launch(chk_pool_kernel, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, (const double*)a.part, (long long)a.rows * tiles, nsets,
             row0 == 0 ? 1 : 0, tot);
  }
  std::vector<double> htot(npool), hto, htr;
  s.download(htot.data(), (const double*)tot, npool);
  for (int o = 0; o < CHK_OUTS; ++o)
    for (int k = 0; k < nwhich; ++k)
      s.download(curve_out ? curve_out + ((size_t)o * nwhich + k) * NM : nullptr, (const double*)a.cur + ((size_t)o * CHK_COUNT + which[k]) * NM, NM);
  s.download(nobs_out, (const double*)a.nobs, NM);
  if (ncurves) {
    hto.resize((size_t)nslots * CHK_COUNT * nsets); htr.resize(hto.size());
    s.download(hto.data(), (const double*)a.t_obs, hto.size());
    s.download(htr.data(), (const double*)a.t_rep, htr.size());
  }
  if (int rc = s.finish()) return rc;
  // the pooled discrepancies of every set from their slots (lag1 = num / den); T_obs of sample s from its first set
  const auto pooled = [&](int side, int code, int e) {
    const auto at = [&](int slot) { return htot[((size_t)side * CHK_SLOTS + slot) * nsets + e]; };
    switch (code) {
      case CHK_CHISQ: return at(CHK_S_CHISQ);
      case CHK_MAX: return at(CHK_S_MAX);
      case CHK_LAG1: return (at(CHK_S_PAIR) != 0.0 && at(CHK_S_DEN) != 0.0) ? at(CHK_S_NUM) / at(CHK_S_DEN) : std::nan("");
      case CHK_TOTAL: return at(CHK_S_TOTAL);
      default: return at(CHK_S_ZEROS);
    }
  };
  for (int k = 0; k < nwhich; ++k) {
    if (pool_rep_out) for (int e = 0; e < nsets; ++e) pool_rep_out[(size_t)k * nsets + e] = pooled(0, which[k], e);
    if (pool_obs_out) for (int sm = 0; sm < S; ++sm) pool_obs_out[(size_t)k * S + sm] = pooled(1, which[k], sm * reps);
    for (int l = 0; l < ncurves; ++l) {
      const size_t src = ((size_t)list_slot[l] * CHK_COUNT + which[k]) * nsets;
      for (int e = 0; e < nsets; ++e) trep_out[((size_t)l * nwhich + k) * nsets + e] = htr[src + e];
      for (int sm = 0; sm < S; ++sm) tobs_out[((size_t)l * nwhich + k) * S + sm] = hto[src + (size_t)sm * reps];
    }
  }
  return BTF_OK;
}

int btf_predict_gg_batch(int device, int64_t n, const double* eta, int G, const double* shape, const double* scale, const double* prob,
                         uint64_t seed, double* out, int32_t* comp_out) {
  if (n < 1 || !eta || !out) return fail(nullptr, BTF_EINVAL, "bad predict_gg_batch arguments");
  std::vector<double> tab;
  double mbar;
  if (!gg_pred_table(shape, scale, prob, G, tab, mbar))
    return fail(nullptr, BTF_EINVAL, "btf_predict_gg_batch: the gamma grid has 1..128 components with finite shape > 0, scale > 0 and "
                                     "weight >= 0, not all zero");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double *de = s.upload(eta, (size_t)n), *dt = s.upload(tab.data(), tab.size());
  double* dout = s.alloc<double>((size_t)n);
  int* dcomp = comp_out ? s.alloc<int>((size_t)n) : nullptr;
  s.launch(gg_pred_batch_fn(), dim3((unsigned)((n + PRED_THREADS - 1) / PRED_THREADS)), dim3(PRED_THREADS), 0, de, dt, G, (long long)n,
           (unsigned long long)seed, dout, dcomp);
  s.download(out, dout, (size_t)n);
  s.download((int*)comp_out, (const int*)dcomp, (size_t)n);
  return s.finish();
}

// ---------------------------------------------------------------- posterior summaries
int btf_posterior_summary(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws,
                          const double* Vs, int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (nsamples < 1 || nsamples > 16384 || nrows < 1 || ncols < 1 || ndepth < 1 || nembeds < 1 || nembeds > MAX_K || !Ws || !Vs ||
      !mean_out || nq < 0 || (nq > 0 && (!q || !q_out)) || transform < 0 || transform > 2)
    return fail(nullptr, BTF_EINVAL, "bad posterior_summary arguments");
  if (int rc = check_percentiles(nullptr, q, nq)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  summary_stage(s, st.W, st.V, nsamples, nrows, ncols * ndepth, nembeds, transform, q, nq, mean_out, q_out);
  return s.finish();
}

// ---------------------------------------------------------------- posterior curve functionals (btf_functionals.h)
namespace {
struct FuncOut { double *mean, *var, *quant, *defined, *prob, *curves, *pw; };

// The whole evaluation on device states dW (S,N,K), dV (S,M,T,K): scratch, the launches chunk by chunk, the downloads.
// The scratch's context may be null (the stateless form: default stream, launches not counted).
int functionals_run(Scratch& s, const double* dW, const double* dV, int S, int N, int M, int T, int K, int transform,
                    const int* which, int nwhich, const double* x, double level, double exceed, const double* q, int nq,
                    const int* curves, int ncurves, const FuncOut& o) {
  FuncArgs a = {};
  a.W = dW; a.V = dV; a.level = level; a.exceed = exceed;
  a.S = S; a.N = N; a.M = M; a.T = T; a.nslots = nwhich; a.nq = nq;
  for (int f = 0; f < FUNC_COUNT; ++f) a.slot[f] = -1;
  for (int k = 0; k < nwhich; ++k) { a.slot[which[k]] = k; a.code[k] = which[k]; }
  const SortGeom g = sort_geom(S, FUNC_SORT_LDS, FUNC_SORT_CELLS);
  a.P = g.P; a.cells = g.cells;
  const size_t NM = (size_t)N * M, per_col = (size_t)nwhich * S * N;      // doubles of scratch a column takes
  const int jc_max = (int)std::max<size_t>(1, std::min<size_t>(std::min(M, 65535), FUNC_SCRATCH_BYTES / (per_col * sizeof(double))));   // (a grid's y extent)
  FuncKernel sweep = func_sweep_fn(K, transform), sort = func_sort_fn();
  if (!sweep) return fail(s.ctx(), BTF_EINVAL, "posterior functionals: nembeds must be 1..10 and transform 0..2");
  a.x = s.upload(x, (size_t)T);
  a.vals = s.alloc<double>(per_col * jc_max);
  if (o.mean) a.mean = s.alloc<double>(nwhich * NM);
  if (o.var) a.var = s.alloc<double>(nwhich * NM);
  if (o.prob) a.prob = s.alloc<double>(nwhich * NM);
  if (o.defined) a.defined = s.alloc<double>(NM);
  if (nq) { a.q = s.upload(q, (size_t)nq); a.quant = s.alloc<double>((size_t)nq * nwhich * NM); }
  const int* dcv = nullptr;
  double* dcur = nullptr;
  if (ncurves) { dcv = s.upload(curves, (size_t)2 * ncurves); dcur = s.alloc<double>((size_t)nwhich * ncurves * S); }
  if (o.pw) a.pw = s.alloc<double>((size_t)nwhich * S * NM);
  allow_lds(s, sort, g.lds);
  const int rowblocks = (N + WAVE - 1) / WAVE;
  const bool reduce = o.mean || o.var || o.prob || o.defined || nq;
  for (int j0 = 0; j0 < M; j0 += jc_max) {
    a.j0 = j0; a.jc = std::min(jc_max, M - j0);
    launch_counted(s, BTF_K_CRITERIA, sweep, dim3(rowblocks, a.jc, func_sweep_slices(S, rowblocks, a.jc)), dim3(FUNC_WAVES * WAVE), 0, a);
    if (ncurves) launch_counted(s, BTF_K_CRITERIA, func_gather_fn(), dim3(ncurves, nwhich), dim3(256), 0, a, dcv, ncurves, dcur);
    if (reduce) launch_counted(s, BTF_K_CRITERIA, sort, dim3((N + a.cells - 1) / a.cells, a.jc, nwhich), dim3(256), g.lds, a);
  }
  s.download(o.mean, a.mean, nwhich * NM);
  s.download(o.var, a.var, nwhich * NM);
  s.download(o.prob, a.prob, nwhich * NM);
  if (o.defined) {
    if (a.slot[FUNC_CROSSING] < 0) s.zero(a.defined, NM * sizeof(double));
    s.download(o.defined, a.defined, NM);
  }
  if (nq) s.download(o.quant, a.quant, (size_t)nq * nwhich * NM);
  if (ncurves) s.download(o.curves, dcur, (size_t)nwhich * ncurves * S);
  s.download(o.pw, a.pw, (size_t)nwhich * S * NM);
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int functionals_check(btf_ctx* c, int S, int N, int M, int T, int K, int transform, const int* which, int nwhich, const double* x,
                      double level, const double* q, int nq, const int* curves, int ncurves, const FuncOut& o) {
  if (S < 1 || N < 1 || M < 1 || K < 1 || K > MAX_K || transform < 0 || transform > 2 || !which || nwhich < 1 || nwhich > FUNC_COUNT ||
      !x || nq < 0 || (nq > 0 && (!q || !o.quant)) || ncurves < 0 || (ncurves > 0 && (!curves || !o.curves)))
    return fail(c, BTF_EINVAL, "bad posterior functionals arguments");
  if (S > FUNC_MAX_S) return fail(c, BTF_EINVAL, "posterior functionals: at most " + std::to_string(FUNC_MAX_S) + " samples (one curve's values are sorted in LDS)");
  if (int rc = check_curve_axis(c, "posterior functionals", T, x, which, nwhich, level)) return rc;
  if (int rc = check_percentiles(c, q, nq)) return rc;
  for (int k = 0; k < ncurves; ++k)
    if (curves[2 * k] < 0 || curves[2 * k] >= N || curves[2 * k + 1] < 0 || curves[2 * k + 1] >= M)
      return fail(c, BTF_EINVAL, "posterior functionals: curve index out of range");
  return BTF_OK;
}
}  // namespace

int btf_posterior_functionals(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws, const double* Vs,
                              int transform, const int* which, int nwhich, const double* x, double level, double exceed,
                              const double* q, int nq, const int* curves, int ncurves, double* mean_out, double* var_out,
                              double* q_out, double* defined_out, double* prob_out, double* curves_out, double* pointwise_out) {
  const FuncOut o = {mean_out, var_out, q_out, defined_out, prob_out, curves_out, pointwise_out};
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior functionals arguments");
  if (int rc = functionals_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, transform, which, nwhich, x, level, q, nq, curves, ncurves, o)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  return functionals_run(s, st.W, st.V, nsamples, nrows, ncols, ndepth, nembeds, transform, which, nwhich, x, level, exceed, q, nq,
                         curves, ncurves, o);
}

// the same on the first nsamples collected states, read where they lie (no upload)
int btf_collect_functionals(btf_ctx* c, int nsamples, int transform, const int* which, int nwhich, const double* x, double level,
                            double exceed, const double* q, int nq, const int* curves, int ncurves, double* mean_out, double* var_out,
                            double* q_out, double* defined_out, double* prob_out, double* curves_out, double* pointwise_out) {
  if (!c) return fail(c, BTF_EINVAL, "bad posterior functionals arguments");
  const FuncOut o = {mean_out, var_out, q_out, defined_out, prob_out, curves_out, pointwise_out};
  if (int rc = functionals_check(c, nsamples, c->N, c->M, c->T, c->K, transform, which, nwhich, x, level, q, nq, curves, ncurves, o)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_functionals", BTF_ESTATE, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return functionals_run(s, st.W, st.V, nsamples, c->N, c->M, c->T, c->K, transform, which, nwhich, x, level, exceed,
                         q, nq, curves, ncurves, o);
}

// ---------------------------------------------------------------- simultaneous credible bands (btf_bands.h)
namespace {
struct BandOut { double *center, *scale, *lower, *upper, *crit, *inside, *pw_inside, *stat; };

// The whole evaluation on device states dW (S,N,K), dV (S,M,T,K): scratch, the launches, the downloads.  Both methods go
// chunk by chunk of columns through a stage that scratch_bytes caps (0: FUNC_SCRATCH_BYTES; one column is the least a
// chunk holds).  The scratch's context may be null (the stateless form).
int bands_run(Scratch& s, const double* dW, const double* dV, int S, int N, int M, int T, int K, int transform, int method,
              double level, const int* depths, const int* curves, int ncurves, const BandOut& o, long long scratch_bytes) {
  BandArgs a = {};
  a.W = dW; a.V = dV; a.S = S; a.N = N; a.M = M; a.T = T; a.ncurves = ncurves;
  a.need = (int)std::ceil(level / 100.0 * S);
  a.kpw = (int)std::floor((1.0 - level / 100.0) / 2.0 * S);
  BandKernel moments = band_moments_fn(K, transform), sweep = band_sweep_fn(K, transform);
  BandKernel depth = band_rank_depth_fn(K, transform), write = band_rank_write_fn(K, transform);
  if (!moments || !sweep || !depth || !write) return fail(s.ctx(), BTF_EINVAL, "posterior bands: nembeds must be 1..10 and transform 0..2");
  std::vector<int> use(T, 1);                            // (alive until finish())
  if (depths) for (int t = 0; t < T; ++t) use[t] = depths[t] != 0;
  a.use = s.upload(use.data(), (size_t)T);
  const size_t NM = (size_t)N * M, NMT = NM * T;
  a.lower = s.alloc<double>(NMT); a.upper = s.alloc<double>(NMT);
  a.crit = s.alloc<double>(NM); a.inside = s.alloc<double>(NM);
  double* dstat = nullptr;
  if (ncurves) { a.curves = s.upload(curves, (size_t)2 * ncurves); dstat = s.alloc<double>((size_t)ncurves * S); }
  const int rowblocks = (N + WAVE - 1) / WAVE, JMAX = 65535;   // (a grid's y extent)
  if (method == BAND_SUPT) {
    const SortGeom g = sort_geom(S, FUNC_SORT_LDS, BAND_CELLS);
    a.P = g.P; a.cells = g.cells;
    const size_t per_col = ((size_t)S + 2 * (size_t)T) * N, cap = scratch_bytes > 0 ? (size_t)scratch_bytes : FUNC_SCRATCH_BYTES;
    const int jc_max = (int)std::max<size_t>(1, std::min<size_t>(std::min(M, JMAX), cap / (per_col * sizeof(double))));
    a.vals = s.alloc<double>((size_t)S * N * jc_max);
    a.cen = s.alloc<double>((size_t)T * N * jc_max); a.scl = s.alloc<double>((size_t)T * N * jc_max);
    a.center = s.alloc<double>(NMT); a.scale = s.alloc<double>(NMT);
    FuncArgs ga = {};                                    // the gather of the functionals reads the same stage
    ga.S = S; ga.N = N; ga.nslots = 1; ga.vals = a.vals;
    allow_lds(s, band_supt_fn(), g.lds);
    for (int j0 = 0; j0 < M; j0 += jc_max) {
      a.j0 = ga.j0 = j0; a.jc = ga.jc = std::min(jc_max, M - j0);
      launch_counted(s, BTF_K_CRITERIA, moments, dim3(rowblocks, a.jc, (T + BAND_TB - 1) / BAND_TB), dim3(BAND_PARTS * WAVE), 0, a);
      launch_counted(s, BTF_K_CRITERIA, sweep, dim3(rowblocks, a.jc, func_sweep_slices(S, rowblocks, a.jc)), dim3(FUNC_WAVES * WAVE), 0, a);
      if (ncurves) launch_counted(s, BTF_K_CRITERIA, func_gather_fn(), dim3(ncurves, 1), dim3(256), 0, ga, a.curves, ncurves, dstat);
      launch_counted(s, BTF_K_CRITERIA, band_supt_fn(), dim3((N + a.cells - 1) / a.cells, a.jc), dim3(256), g.lds, a);
    }
  } else {
    a.P = 2;
    while (a.P < S) a.P <<= 1;
    a.cells = std::max(1, std::min(BAND_CELLS, BAND_RANK_LDS / (a.P * BAND_RANK_BYTES)));
    const size_t lds = (size_t)a.cells * a.P * BAND_RANK_BYTES, lds_keys = (size_t)a.cells * a.P * sizeof(double);
    const int tiles = (N + a.cells - 1) / a.cells;
    // slices of the depth axis: enough workgroups to fill the chip when rows x columns alone do not (geometry only)
    const long long curves_wg = (long long)tiles * std::min(M, JMAX);
    a.zb = (int)std::max<long long>(1, std::min<long long>(T, (2048 + curves_wg - 1) / curves_wg));
    const size_t per_col = (size_t)a.zb * N * S, cap = scratch_bytes > 0 ? (size_t)scratch_bytes : FUNC_SCRATCH_BYTES;
    const int jc_max = (int)std::max<size_t>(1, std::min<size_t>(std::min(M, JMAX), cap / (per_col * sizeof(int))));
    a.dep = s.alloc<int>(per_col * jc_max);
    a.pw_inside = s.alloc<double>(NM);
    a.stat = dstat;
    allow_lds(s, depth, lds);
    allow_lds(s, write, lds_keys);
    allow_lds(s, band_rank_k_fn(), lds_keys);
    for (int j0 = 0; j0 < M; j0 += jc_max) {
      a.j0 = j0; a.jc = std::min(jc_max, M - j0);
      launch_counted(s, BTF_K_CRITERIA, depth, dim3(tiles, a.jc, a.zb), dim3(256), lds, a);
      launch_counted(s, BTF_K_CRITERIA, band_rank_k_fn(), dim3(tiles, a.jc), dim3(256), lds_keys, a);
      launch_counted(s, BTF_K_CRITERIA, write, dim3(tiles, a.jc, a.zb), dim3(256), lds_keys, a);
    }
  }
  if (a.center) { s.download(o.center, a.center, NMT); s.download(o.scale, a.scale, NMT); }
  s.download(o.lower, a.lower, NMT);
  s.download(o.upper, a.upper, NMT);
  s.download(o.crit, a.crit, NM);
  s.download(o.inside, a.inside, NM);
  if (a.pw_inside) s.download(o.pw_inside, a.pw_inside, NM);
  if (ncurves) s.download(o.stat, dstat, (size_t)ncurves * S);
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int bands_check(btf_ctx* c, int S, int N, int M, int T, int K, int transform, int method, double level, const int* depths,
                const int* curves, int ncurves, const BandOut& o, long long scratch_bytes) {
  if (N < 1 || M < 1 || K < 1 || K > MAX_K || transform < 0 || transform > 2 || ncurves < 0 || (ncurves > 0 && (!curves || !o.stat)) ||
      scratch_bytes < 0)
    return fail(c, BTF_EINVAL, "bad posterior bands arguments");
  if (method != BAND_SUPT && method != BAND_RANK) return fail(c, BTF_EINVAL, "posterior bands: method must be 0 (supt) or 1 (rank)");
  if (S < 2) return fail(c, BTF_EINVAL, "posterior bands: at least two samples");
  if (T < 1) return fail(c, BTF_EINVAL, "posterior bands: ndepth >= 1");
  if (!(level > 0.0 && level < 100.0)) return fail(c, BTF_EINVAL, "posterior bands: level must lie in (0, 100)");
  const int max_s = method == BAND_SUPT ? FUNC_MAX_S : BAND_RANK_MAX_S;
  if (S > max_s) return fail(c, BTF_EINVAL, "posterior bands: at most " + std::to_string(max_s) + " samples with this method (one curve's values are sorted in LDS)");
  if (depths) {
    bool any = false;
    for (int t = 0; t < T; ++t) any = any || depths[t] != 0;
    if (!any) return fail(c, BTF_EINVAL, "posterior bands: depths selects no depth");
  }
  for (int k = 0; k < ncurves; ++k)
    if (curves[2 * k] < 0 || curves[2 * k] >= N || curves[2 * k + 1] < 0 || curves[2 * k + 1] >= M)
      return fail(c, BTF_EINVAL, "posterior bands: curve index out of range");
  return BTF_OK;
}
}  // namespace

int btf_posterior_bands(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws, const double* Vs,
                        int transform, int method, double level, const int* depths, const int* curves, int ncurves,
                        double* center_out, double* scale_out, double* lower_out, double* upper_out, double* crit_out,
                        double* inside_out, double* pointwise_inside_out, double* stat_out, long long scratch_bytes) {
  const BandOut o = {center_out, scale_out, lower_out, upper_out, crit_out, inside_out, pointwise_inside_out, stat_out};
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior bands arguments");
  if (int rc = bands_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, transform, method, level, depths, curves, ncurves, o, scratch_bytes)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  return bands_run(s, st.W, st.V, nsamples, nrows, ncols, ndepth, nembeds, transform, method, level, depths, curves, ncurves, o, scratch_bytes);
}

// the same on the first nsamples collected states, read where they lie (no upload)
int btf_collect_bands(btf_ctx* c, int nsamples, int transform, int method, double level, const int* depths, const int* curves,
                      int ncurves, double* center_out, double* scale_out, double* lower_out, double* upper_out, double* crit_out,
                      double* inside_out, double* pointwise_inside_out, double* stat_out, long long scratch_bytes) {
  if (!c) return fail(c, BTF_EINVAL, "bad posterior bands arguments");
  const BandOut o = {center_out, scale_out, lower_out, upper_out, crit_out, inside_out, pointwise_inside_out, stat_out};
  if (int rc = bands_check(c, nsamples, c->N, c->M, c->T, c->K, transform, method, level, depths, curves, ncurves, o, scratch_bytes)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_bands", BTF_ESTATE, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return bands_run(s, st.W, st.V, nsamples, c->N, c->M, c->T, c->K, transform, method, level, depths, curves, ncurves, o, scratch_bytes);
}

// ---------------------------------------------------------------- posterior ranking (btf_ranking.h)
namespace {
struct RankOut { double *expected, *var, *ptop; int* ranks; double *prob_less, *prob_defined; };

// The whole evaluation on device states dW (S,N,K), dV (S,M,T,K): per chunk of samples the functionals' sweep into the
// scratch, the gather and count of the pairs, the rank kernel; then the finish kernel and the downloads.  scratch_bytes
// caps the chunk's scratch (0: FUNC_SCRATCH_BYTES; one sample is the least a chunk holds).
int ranking_run(Scratch& s, const double* dW, const double* dV, int S, int N, int M, int T, int K, int transform, int which,
                const double* x, double level, int along, int descending, const int* top, int ntop, const int* pairs, int npairs,
                const RankOut& o, long long scratch_bytes) {
  FuncSweep w;
  if (!func_sweep_init(w, s, dW, dV, S, N, M, T, K, transform, which, x, level, scratch_bytes))
    return fail(s.ctx(), BTF_EINVAL, "posterior ranking: nembeds must be 1..10 and transform 0..2");
  const size_t NM = (size_t)N * M;
  RankArgs r = {};
  r.vals = w.vals; r.S = S; r.N = N; r.M = M; r.along = along; r.ntop = ntop; r.P = npairs;
  for (int k = 0; k < ntop; ++k) r.top[k] = std::min(top[k], RANK_MAX_L + 1);      // (a rank never exceeds RANK_MAX_L)
  r.L = along ? N : M;
  while ((1 << r.lshift) < r.L) ++r.lshift;
  r.Lp = 1 << r.lshift;
  const int ngroups = along ? M : N;
  r.G = std::max(1, std::min(ngroups, std::min(RANK_MAX_L / r.Lp, RANK_MAX_GROUPS)));
  const size_t lds = rank_lds_bytes(r.G, r.Lp);
  const int tiles = (ngroups + r.G - 1) / r.G;
  r.A = s.alloc<unsigned long long>(NM);
  r.B = s.alloc<unsigned long long>(NM);
  r.C = s.alloc<unsigned int>((size_t)ntop * NM);
  if (o.ranks) r.ranks = s.alloc<int>((size_t)S * NM);
  r.expected = s.alloc<double>(NM); r.var = s.alloc<double>(NM); r.ptop = s.alloc<double>((size_t)ntop * NM);
  const int* dpairs = nullptr; double* dpv = nullptr;
  if (npairs) {
    dpairs = s.upload(pairs, (size_t)4 * npairs);             // (i,j,i2,j2) rows = 2 npairs (i,j) curves for the gather
    dpv = s.alloc<double>((size_t)2 * npairs * w.sc_max);
    r.pvals = dpv;
    r.pless = s.alloc<unsigned int>(npairs); r.pdef = s.alloc<unsigned int>(npairs);
    r.prob_less = s.alloc<double>(npairs); r.prob_defined = s.alloc<double>(npairs);
  }
  s.zero(r.A, NM * sizeof(unsigned long long)); s.zero(r.B, NM * sizeof(unsigned long long)); s.zero(r.C, (size_t)ntop * NM * sizeof(unsigned int));
  if (npairs) { s.zero(r.pless, npairs * sizeof(unsigned int)); s.zero(r.pdef, npairs * sizeof(unsigned int)); }
  RankKernel rank = rank_fn(descending != 0);
  for (int s0 = 0; s0 < S; s0 += w.sc_max) {
    const int sc = std::min(w.sc_max, S - s0);
    sweep_chunk(w, s0, sc);
    r.s0 = s0; r.sc = sc;
    if (npairs) {
      w.f.j0 = 0; w.f.jc = M; w.f.vals = w.vals;                // (the gather reads the chunk's scratch over every column)
      launch_counted(s, BTF_K_CRITERIA, func_gather_fn(), dim3(2 * npairs, 1), dim3(256), 0, w.f, dpairs, 2 * npairs, dpv);
      launch_counted(s, BTF_K_CRITERIA, rank_pairs_fn(), dim3(npairs), dim3(256), 0, r);
    }
    // sample slices: enough workgroups for two per CU when the tiles alone are fewer (geometry only)
    const int ys = std::max(1, std::min(sc, (1024 + tiles - 1) / tiles));
    launch_counted(s, BTF_K_CRITERIA, rank, dim3(tiles, ys), dim3(RANK_THREADS), lds, r);
  }
  launch_counted(s, BTF_K_CRITERIA, rank_finish_fn(), dim3((unsigned)((NM + npairs + 255) / 256)), dim3(256), 0, r);
  s.download(o.expected, r.expected, NM);
  s.download(o.var, r.var, NM);
  s.download(o.ptop, r.ptop, (size_t)ntop * NM);
  s.download(o.ranks, r.ranks, (size_t)S * NM);
  if (npairs) { s.download(o.prob_less, r.prob_less, (size_t)npairs); s.download(o.prob_defined, r.prob_defined, (size_t)npairs); }
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int ranking_check(btf_ctx* c, int S, int N, int M, int T, int K, int transform, int which, const double* x, double level, int along,
                  int descending, const int* top, int ntop, const int* pairs, int npairs, const RankOut& o, long long scratch_bytes) {
  if (S < 1 || N < 1 || M < 1 || K < 1 || K > MAX_K || transform < 0 || transform > 2 || which < 0 || which >= FUNC_COUNT || !x ||
      along < 0 || along > 1 || descending < 0 || descending > 1 || !top || ntop < 1 || ntop > RANK_MAX_TOP || npairs < 0 ||
      (npairs > 0 && (!pairs || !o.prob_less || !o.prob_defined)) || scratch_bytes < 0)
    return fail(c, BTF_EINVAL, "bad posterior ranking arguments");
  if (S > FUNC_MAX_S) return fail(c, BTF_EINVAL, "posterior ranking: at most " + std::to_string(FUNC_MAX_S) + " samples");
  if ((along ? N : M) > RANK_MAX_L)
    return fail(c, BTF_EINVAL, "posterior ranking: at most " + std::to_string(RANK_MAX_L) + " members in a group (it is sorted in LDS)");
  if (int rc = check_curve_axis(c, "posterior ranking", T, x, &which, 1, level)) return rc;
  for (int k = 0; k < ntop; ++k) {
    if (top[k] < 1) return fail(c, BTF_EINVAL, "posterior ranking: top must hold integers >= 1");
    for (int l = 0; l < k; ++l)
      if (top[l] == top[k]) return fail(c, BTF_EINVAL, "posterior ranking: top must hold distinct integers");
  }
  for (int k = 0; k < 2 * npairs; ++k)
    if (pairs[2 * k] < 0 || pairs[2 * k] >= N || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= M)
      return fail(c, BTF_EINVAL, "posterior ranking: pair index out of range");
  return BTF_OK;
}
}  // namespace

int btf_posterior_ranking(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws, const double* Vs,
                          int transform, int which, const double* x, double level, int along, int descending, const int* top, int ntop,
                          const int* pairs, int npairs, double* expected_out, double* var_out, double* ptop_out, int* ranks_out,
                          double* prob_less_out, double* prob_defined_out, long long scratch_bytes) {
  const RankOut o = {expected_out, var_out, ptop_out, ranks_out, prob_less_out, prob_defined_out};
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior ranking arguments");
  if (int rc = ranking_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, transform, which, x, level, along, descending, top, ntop,
                             pairs, npairs, o, scratch_bytes)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  return ranking_run(s, st.W, st.V, nsamples, nrows, ncols, ndepth, nembeds, transform, which, x, level, along, descending, top, ntop,
                     pairs, npairs, o, scratch_bytes);
}

// the same on the first nsamples collected states, read where they lie (no upload)
int btf_collect_ranking(btf_ctx* c, int nsamples, int transform, int which, const double* x, double level, int along, int descending,
                        const int* top, int ntop, const int* pairs, int npairs, double* expected_out, double* var_out,
                        double* ptop_out, int* ranks_out, double* prob_less_out, double* prob_defined_out, long long scratch_bytes) {
  if (!c) return fail(c, BTF_EINVAL, "bad posterior ranking arguments");
  const RankOut o = {expected_out, var_out, ptop_out, ranks_out, prob_less_out, prob_defined_out};
  if (int rc = ranking_check(c, nsamples, c->N, c->M, c->T, c->K, transform, which, x, level, along, descending, top, ntop, pairs, npairs,
                             o, scratch_bytes)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_ranking", BTF_ESTATE, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return ranking_run(s, st.W, st.V, nsamples, c->N, c->M, c->T, c->K, transform, which, x, level, along, descending, top, ntop,
                     pairs, npairs, o, scratch_bytes);
}

// ---------------------------------------------------------------- posterior similarity (btf_similarity.h)
namespace {
struct SimOut { double *mean, *var, *quant, *expected, *rank_var, *pnear, *pair_values, *dist; };

// The whole evaluation on device states dW (S,N,K), dV (S,M,T,K): the metric of every sample, then per tile of entities
// the keys of every (partner, sample, entity) into the stage, the unchanged rank kernel on them, the keys to distances in
// place, the unchanged sort kernel's reductions over the samples, and the tile's rows of the outputs.  scratch_bytes caps
// the stage (0: FUNC_SCRATCH_BYTES; one entity is the least a tile holds).
int sim_run(Scratch& s, const double* dW, const double* dV, int S, int N, int M, int T, int K, int along, int metric, const int* over,
            int nover, const double* q, int nq, const int* nearest, int nnearest, const int* pairs, int npairs, const SimOut& o,
            long long scratch_bytes) {
  const bool cols = along == 1, cosine = metric == 1;
  const int E = cols ? M : N, YN = cols ? N : M;
  std::vector<int> all;
  if (!over) { all.resize(YN); for (int k = 0; k < YN; ++k) all[k] = k; over = all.data(); nover = YN; }
  SimKernel metric_k = sim_metric_fn(K), dist_k = sim_dist_fn(K, cosine);
  if (!metric_k || !dist_k) return fail(s.ctx(), BTF_EINVAL, "posterior similarity: nembeds must be 1..10");
  const size_t EE = (size_t)E * E, cap = scratch_bytes > 0 ? (size_t)scratch_bytes : FUNC_SCRATCH_BYTES;
  const int ne_max = (int)std::max<size_t>(1, std::min<size_t>(E, cap / ((size_t)S * E * sizeof(double))));
  const size_t tile_max = (size_t)ne_max * E;
  SimArgs a = {};
  a.X = cols ? dV : dW; a.Y = cols ? dW : dV; a.over = s.upload(over, (size_t)nover);
  a.S = S; a.E = E; a.TT = cols ? T : 1; a.YN = YN; a.mt = cols ? 1 : T; a.nmem = nover * a.mt;
  a.ncells = (double)nover * T; a.rms = cosine ? 0 : 1; a.ntop = nnearest; a.nq = nq; a.P = npairs;
  a.metric = s.alloc<double>((size_t)S * K * K);
  if (cosine) a.norms = s.alloc<double>((size_t)S * E);
  a.stage = s.alloc<double>((size_t)S * tile_max);
  if (o.dist) a.dist = s.alloc<double>((size_t)S * EE);
  if (npairs) { a.pairs = s.upload(pairs, (size_t)2 * npairs); a.pair_values = s.alloc<double>((size_t)S * npairs); }
  unsigned long long* dA = s.alloc<unsigned long long>(tile_max);
  unsigned long long* dB = s.alloc<unsigned long long>(tile_max);
  unsigned int* dC = s.alloc<unsigned int>((size_t)nnearest * tile_max);
  double* dqt = s.alloc<double>((size_t)nq * tile_max);
  a.A = dA; a.B = dB; a.C = dC; a.qtmp = dqt;
  a.expected = s.alloc<double>(EE); a.rank_var = s.alloc<double>(EE); a.pnear = s.alloc<double>((size_t)nnearest * EE);
  a.quant = s.alloc<double>((size_t)nq * EE);
  double* dmean = s.alloc<double>(EE);
  double* dvar = s.alloc<double>(EE);
  // the two borrowed kernels: the sort reduces column = partner, row = local entity; the rank kernel ranks the E partners
  // (along 0: the "columns") of every (sample, local entity)
  FuncArgs f = {};
  f.S = S; f.M = E; f.j0 = 0; f.jc = E; f.nslots = 1; f.nq = nq; f.exceed = std::nan("");
  for (int k = 0; k < FUNC_COUNT; ++k) f.slot[k] = -1;
  f.slot[FUNC_AUC] = 0; f.code[0] = FUNC_AUC;            // (any functional but the crossing: no value is censored)
  f.q = nq ? s.upload(q, (size_t)nq) : nullptr;
  const SortGeom g = sort_geom(S, FUNC_SORT_LDS, FUNC_SORT_CELLS);
  f.P = g.P; f.cells = g.cells;
  FuncKernel sort = func_sort_fn();
  allow_lds(s, sort, g.lds);
  RankArgs r = {};
  r.S = S; r.M = E; r.along = 0; r.ntop = nnearest; r.s0 = 0; r.sc = S; r.L = E;
  for (int k = 0; k < nnearest; ++k) r.top[k] = std::min(nearest[k], RANK_MAX_L + 1);      // (a rank never exceeds RANK_MAX_L)
  while ((1 << r.lshift) < r.L) ++r.lshift;
  r.Lp = 1 << r.lshift;
  r.A = dA; r.B = dB; r.C = dC;
  RankKernel rank = rank_fn(false);
  launch_counted(s, BTF_K_CRITERIA, metric_k, dim3(S), dim3(SIM_THREADS), 0, a);
  const int fblocks = (E + SIM_FBLK - 1) / SIM_FBLK;
  for (int e0 = 0; e0 < E; e0 += ne_max) {
    const int ne = std::min(ne_max, E - e0);
    const size_t tile = (size_t)ne * E;
    a.e0 = e0; a.ne = ne;
    // sample slices: enough workgroups to fill the chip when entity blocks x partner blocks alone do not (geometry only)
    const int eblocks = (ne + WAVE - 1) / WAVE;
    const int zs = std::max(1, std::min(S, (2048 + eblocks * fblocks - 1) / (eblocks * fblocks)));
    launch_counted(s, BTF_K_CRITERIA, dist_k, dim3(eblocks, fblocks, zs), dim3(SIM_THREADS), sim_dist_lds_bytes(K), a);
    // ---- neighbours: the ranks of the E partners of every (sample, entity) on the keys; the entity itself (nan) last
    s.zero(dA, tile * sizeof(unsigned long long)); s.zero(dB, tile * sizeof(unsigned long long));
    s.zero(dC, (size_t)nnearest * tile * sizeof(unsigned int));
    r.vals = a.stage; r.N = ne;
    r.G = std::max(1, std::min(ne, std::min(RANK_MAX_L / r.Lp, RANK_MAX_GROUPS)));
    const int rtiles = (ne + r.G - 1) / r.G;
    launch_counted(s, BTF_K_CRITERIA, rank, dim3(rtiles, std::max(1, std::min(S, (1024 + rtiles - 1) / rtiles))), dim3(RANK_THREADS),
                   rank_lds_bytes(r.G, r.Lp), r);
    // ---- keys to distances, the pointwise output and the pairs
    launch_counted(s, BTF_K_CRITERIA, sim_root_fn(), dim3((unsigned)(((size_t)S * tile + 255) / 256)), dim3(256), 0, a);
    if (npairs) launch_counted(s, BTF_K_CRITERIA, sim_pairs_fn(), dim3(npairs), dim3(256), 0, a);
    // ---- mean, variance and percentiles over the samples; mean and variance land in their rows directly
    f.vals = a.stage; f.N = ne; f.mean = dmean + (size_t)e0 * E; f.var = dvar + (size_t)e0 * E; f.quant = dqt;
    launch_counted(s, BTF_K_CRITERIA, sort, dim3((ne + f.cells - 1) / f.cells, E, 1), dim3(256), g.lds, f);
    launch_counted(s, BTF_K_CRITERIA, sim_finish_fn(), dim3((unsigned)((tile + 255) / 256)), dim3(256), 0, a);
  }
  s.download(o.mean, dmean, EE);
  s.download(o.var, dvar, EE);
  if (nq) s.download(o.quant, a.quant, (size_t)nq * EE);
  s.download(o.expected, a.expected, EE);
  s.download(o.rank_var, a.rank_var, EE);
  s.download(o.pnear, a.pnear, (size_t)nnearest * EE);
  if (npairs) s.download(o.pair_values, a.pair_values, (size_t)S * npairs);
  s.download(o.dist, a.dist, (size_t)S * EE);
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int sim_check(btf_ctx* c, int S, int N, int M, int T, int K, int along, int metric, const int* over, int nover, const double* q, int nq,
              const int* nearest, int nnearest, const int* pairs, int npairs, const SimOut& o, long long scratch_bytes) {
  if (S < 1 || N < 1 || M < 1 || T < 1 || K < 1 || K > MAX_K || along < 0 || along > 1 || metric < 0 || metric > 1 || nover < 0 ||
      (over && nover < 1) || (!over && nover > 0) || nq < 0 || (nq > 0 && (!q || !o.quant)) || !nearest || nnearest < 1 ||
      nnearest > SIM_MAX_NEAREST || npairs < 0 || (npairs > 0 && (!pairs || !o.pair_values)) || scratch_bytes < 0)
    return fail(c, BTF_EINVAL, "bad posterior similarity arguments");
  if (S > FUNC_MAX_S) return fail(c, BTF_EINVAL, "posterior similarity: at most " + std::to_string(FUNC_MAX_S) + " samples");
  const int E = along ? M : N, YN = along ? N : M;
  if (E > SIM_MAX_E)
    return fail(c, BTF_EINVAL, "posterior similarity: at most " + std::to_string(SIM_MAX_E) + " entities (a neighbour group is sorted in LDS)");
  if (int rc = check_percentiles(c, q, nq)) return rc;
  for (int k = 0; k < nnearest; ++k) {
    if (nearest[k] < 1) return fail(c, BTF_EINVAL, "posterior similarity: nearest must hold integers >= 1");
    for (int l = 0; l < k; ++l)
      if (nearest[l] == nearest[k]) return fail(c, BTF_EINVAL, "posterior similarity: nearest must hold distinct integers");
  }
  if (over) {
    std::vector<char> seen((size_t)YN, 0);
    for (int k = 0; k < nover; ++k) {
      if (over[k] < 0 || over[k] >= YN || seen[over[k]]) return fail(c, BTF_EINVAL, "posterior similarity: over must hold distinct indices in range");
      seen[over[k]] = 1;
    }
  }
  for (int k = 0; k < 2 * npairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= E) return fail(c, BTF_EINVAL, "posterior similarity: pair index out of range");
  return BTF_OK;
}
}  // namespace

int btf_posterior_similarity(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws, const double* Vs,
                             int along, int metric, const int* over, int nover, const double* q, int nq, const int* nearest,
                             int nnearest, const int* pairs, int npairs, double* mean_out, double* var_out, double* q_out,
                             double* expected_out, double* rank_var_out, double* pnear_out, double* pair_out, double* dist_out,
                             long long scratch_bytes) {
  const SimOut o = {mean_out, var_out, q_out, expected_out, rank_var_out, pnear_out, pair_out, dist_out};
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior similarity arguments");
  if (int rc = sim_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, along, metric, over, nover, q, nq, nearest, nnearest, pairs,
                         npairs, o, scratch_bytes)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  return sim_run(s, st.W, st.V, nsamples, nrows, ncols, ndepth, nembeds, along, metric, over, nover, q, nq, nearest, nnearest, pairs,
                 npairs, o, scratch_bytes);
}

// the same on the first nsamples collected states, read where they lie (no upload)
int btf_collect_similarity(btf_ctx* c, int nsamples, int along, int metric, const int* over, int nover, const double* q, int nq,
                           const int* nearest, int nnearest, const int* pairs, int npairs, double* mean_out, double* var_out,
                           double* q_out, double* expected_out, double* rank_var_out, double* pnear_out, double* pair_out,
                           double* dist_out, long long scratch_bytes) {
  if (!c) return fail(c, BTF_EINVAL, "bad posterior similarity arguments");
  const SimOut o = {mean_out, var_out, q_out, expected_out, rank_var_out, pnear_out, pair_out, dist_out};
  if (int rc = sim_check(c, nsamples, c->N, c->M, c->T, c->K, along, metric, over, nover, q, nq, nearest, nnearest, pairs, npairs, o,
                         scratch_bytes)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_similarity", BTF_ESTATE, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return sim_run(s, st.W, st.V, nsamples, c->N, c->M, c->T, c->K, along, metric, over, nover, q, nq, nearest, nnearest, pairs, npairs, o,
                 scratch_bytes);
}

// ---------------------------------------------------------------- posterior feature association (btf_assoc.h)
namespace {
struct AssocOut { double *mean, *var, *quant, *prob, *defined, *nmean, *values, *of_means, *sdx, *sdy; };

// The whole evaluation on device states dW (S,N,K), dV (S,M,T,K), dU (S,F,K): per chunk of samples the functionals' sweep
// into the scratch, the moments of every (sample, column) and the running curve means; then the reduction over the samples
// per (feature, column), the raw values of the requested pairs, the plug-in table, and the downloads.  scratch_bytes caps
// the chunk's scratch (0: FUNC_SCRATCH_BYTES; one sample is the least a chunk holds).
int assoc_run(Scratch& s, const double* dW, const double* dV, const double* dU, int S, int N, int M, int T, int K, int F, int transform,
              int which, const double* x, double level, const int* stats, int nstats, const double* q, int nq, const int* pairs,
              int npairs, const AssocOut& o, long long scratch_bytes) {
  AssocKernel moments = assoc_moments_fn(K), reduce = assoc_reduce_fn(K);
  FuncSweep w;
  if (!moments || !reduce || !func_sweep_init(w, s, dW, dV, S, N, M, T, K, transform, which, x, level, scratch_bytes))
    return fail(s.ctx(), BTF_EINVAL, "posterior association: nembeds must be 1..10 and transform 0..2");
  const size_t NM = (size_t)N * M, FM = (size_t)F * M;
  AssocArgs a = {};
  a.vals = w.vals; a.W = dW; a.U = dU; a.S = S; a.N = N; a.M = M; a.F = F;
  a.mom = s.alloc<double>((size_t)S * M * assoc_nmom(K));
  a.nst = nstats;
  for (int k = 0; k < nstats; ++k) a.st[k] = stats[k];
  const SortGeom g = sort_geom(S, ASSOC_SORT_LDS, ASSOC_ROWS);      // rows of P doubles; a pair takes one per statistic
  a.P = g.P;
  while ((1 << a.pshift) < a.P) ++a.pshift;
  a.cells = std::max(1, std::min(g.cells / nstats, F));
  const size_t lds = (size_t)a.cells * nstats * a.P * sizeof(double);
  a.nq = nq;
  if (nq) { a.q = s.upload(q, (size_t)nq); a.quant = s.alloc<double>((size_t)nstats * nq * FM); }
  a.mean = s.alloc<double>(nstats * FM); a.var = s.alloc<double>(nstats * FM); a.prob = s.alloc<double>(nstats * FM);
  a.defined = s.alloc<double>(FM); a.nmean = s.alloc<double>(M);
  if (npairs) { a.npairs = npairs; a.pairs = s.upload(pairs, (size_t)2 * npairs); a.values = s.alloc<double>((size_t)nstats * npairs * S); }
  const bool plug = o.of_means != nullptr;
  if (plug) {
    a.pbar = s.alloc<double>((size_t)F * N); a.gbar = s.alloc<double>(NM); a.gcnt = s.alloc<int>(NM);
    a.om = s.alloc<double>(ASSOC_OM * FM); a.sdx = s.alloc<double>(F); a.sdy = s.alloc<double>(M);
    s.zero(a.gbar, NM * sizeof(double)); s.zero(a.gcnt, NM * sizeof(int));
  }
  allow_lds(s, reduce, lds);
  const unsigned rb = (unsigned)((N + ASSOC_THREADS - 1) / ASSOC_THREADS);
  for (int s0 = 0; s0 < S; s0 += w.sc_max) {
    const int sc = std::min(w.sc_max, S - s0);
    sweep_chunk(w, s0, sc);
    a.s0 = s0; a.sc = sc;
    launch_counted(s, BTF_K_CRITERIA, moments, dim3(M, sc), dim3(WAVE), 0, a);
    if (plug) launch_counted(s, BTF_K_CRITERIA, assoc_gbar_fn(), dim3(rb * M), dim3(ASSOC_THREADS), 0, a);
  }
  const unsigned ftiles = (unsigned)((F + a.cells - 1) / a.cells);
  launch_counted(s, BTF_K_CRITERIA, reduce, dim3(ftiles * M), dim3(ASSOC_THREADS), lds, a);
  if (npairs) launch_counted(s, BTF_K_CRITERIA, assoc_values_fn(K), dim3(npairs), dim3(ASSOC_THREADS), 0, a);
  if (plug) {
    launch_counted(s, BTF_K_CRITERIA, assoc_pbar_fn(K), dim3(rb * ((F + ASSOC_FT - 1) / ASSOC_FT)), dim3(ASSOC_THREADS), 0, a);
    launch_counted(s, BTF_K_CRITERIA, assoc_gbar_finish_fn(), dim3((unsigned)((NM + ASSOC_THREADS - 1) / ASSOC_THREADS)), dim3(ASSOC_THREADS), 0, a);
    launch_counted(s, BTF_K_CRITERIA, assoc_cross_fn(), dim3((unsigned)F * ((M + 3) / 4)), dim3(ASSOC_THREADS), 0, a);
  }
  s.download(o.mean, a.mean, nstats * FM);
  s.download(o.var, a.var, nstats * FM);
  s.download(o.prob, a.prob, nstats * FM);
  if (nq) s.download(o.quant, a.quant, (size_t)nstats * nq * FM);
  s.download(o.defined, a.defined, FM);
  s.download(o.nmean, a.nmean, (size_t)M);
  if (npairs) s.download(o.values, a.values, (size_t)nstats * npairs * S);
  if (plug) { s.download(o.of_means, a.om, ASSOC_OM * FM); s.download(o.sdx, a.sdx, (size_t)F); s.download(o.sdy, a.sdy, (size_t)M); }
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int assoc_check(btf_ctx* c, int S, int N, int M, int T, int K, int F, const double* Us, int transform, int which, const double* x,
                double level, const int* stats, int nstats, const double* q, int nq, const int* pairs, int npairs, const AssocOut& o,
                long long scratch_bytes) {
  if (S < 1 || N < 1 || M < 1 || F < 1 || K < 1 || K > MAX_K || !Us || transform < 0 || transform > 2 || which < 0 || which >= FUNC_COUNT ||
      !x || !stats || nstats < 1 || nstats > ASSOC_NSTATS || nq < 0 || (nq > 0 && (!q || !o.quant)) || npairs < 0 ||
      (npairs > 0 && (!pairs || !o.values)) || (o.of_means && (!o.sdx || !o.sdy)) || scratch_bytes < 0)
    return fail(c, BTF_EINVAL, "bad posterior association arguments");
  if (S > FUNC_MAX_S) return fail(c, BTF_EINVAL, "posterior association: at most " + std::to_string(FUNC_MAX_S) + " samples (the values of a pair are sorted in LDS)");
  if ((long long)F * M > 0x7fffffffLL || (long long)N * M > 0x7fffffffLL * (long long)ASSOC_THREADS)
    return fail(c, BTF_EINVAL, "posterior association: too many (feature, column) pairs or curves for one launch");
  if (int rc = check_curve_axis(c, "posterior association", T, x, &which, 1, level)) return rc;
  for (int k = 0; k < nstats; ++k)
    if (stats[k] < 0 || stats[k] >= ASSOC_NSTATS || (k > 0 && stats[k] == stats[0]))
      return fail(c, BTF_EINVAL, "posterior association: statistic codes must be distinct and in 0..1");
  if (int rc = check_percentiles(c, q, nq)) return rc;
  for (int k = 0; k < npairs; ++k)
    if (pairs[2 * k] < 0 || pairs[2 * k] >= F || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= M)
      return fail(c, BTF_EINVAL, "posterior association: pair index out of range");
  return BTF_OK;
}
}  // namespace

int btf_posterior_association(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, int nfeatures, const double* Ws,
                              const double* Vs, const double* Us, int transform, int which, const double* x, double level,
                              const int* stats, int nstats, const double* q, int nq, const int* pairs, int npairs, double* mean_out,
                              double* var_out, double* q_out, double* prob_out, double* defined_out, double* nmean_out,
                              double* values_out, double* of_means_out, double* sdx_out, double* sdy_out, long long scratch_bytes) {
  const AssocOut o = {mean_out, var_out, q_out, prob_out, defined_out, nmean_out, values_out, of_means_out, sdx_out, sdy_out};
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior association arguments");
  if (int rc = assoc_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, nfeatures, Us, transform, which, x, level, stats, nstats, q, nq,
                           pairs, npairs, o, scratch_bytes)) return rc;
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  const double* dU = s.upload(Us, (size_t)nsamples * nfeatures * nembeds);
  return assoc_run(s, st.W, st.V, dU, nsamples, nrows, ncols, ndepth, nembeds, nfeatures, transform, which, x, level, stats, nstats, q, nq,
                   pairs, npairs, o, scratch_bytes);
}

// the same on the first nsamples collected states, read where they lie; only Us (the host keeps U) is uploaded
int btf_collect_association(btf_ctx* c, int nsamples, int nfeatures, const double* Us, int transform, int which, const double* x,
                            double level, const int* stats, int nstats, const double* q, int nq, const int* pairs, int npairs,
                            double* mean_out, double* var_out, double* q_out, double* prob_out, double* defined_out, double* nmean_out,
                            double* values_out, double* of_means_out, double* sdx_out, double* sdy_out, long long scratch_bytes) {
  if (!c) return fail(c, BTF_EINVAL, "bad posterior association arguments");
  const AssocOut o = {mean_out, var_out, q_out, prob_out, defined_out, nmean_out, values_out, of_means_out, sdx_out, sdy_out};
  if (int rc = assoc_check(c, nsamples, c->N, c->M, c->T, c->K, nfeatures, Us, transform, which, x, level, stats, nstats, q, nq, pairs, npairs,
                           o, scratch_bytes)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_association", BTF_ESTATE, nsamples, c->N, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  const double* dU = s.upload(Us, (size_t)nsamples * nfeatures * c->K);
  return assoc_run(s, st.W, st.V, dU, nsamples, c->N, c->M, c->T, c->K, nfeatures, transform, which, x, level, stats, nstats, q, nq,
                   pairs, npairs, o, scratch_bytes);
}

// ---------------------------------------------------------------- monotone projection of the posterior (btf_monotone.h)
namespace {
// The projection of the device states dW (S,N,K), dVin (S,M,T,K) into dVout (dVin itself: in place), the summary of the
// projected states where they lie, and the downloads.  Null outputs are skipped; mean_out null: no summary.
int mono_run(Scratch& s, const double* dW, const double* dVin, double* dVout, int S, int N, int M, int T, int K, int increasing,
             int transform, const double* q, int nq, double* V_out, int* pools_out, double* mean_out, double* q_out) {
  MonoKernel project = mono_project_fn(K);
  if (!project) return fail(s.ctx(), BTF_EINVAL, "posterior monotone: nembeds must be 1..10");
  const size_t nW = (size_t)N * K, nV = (size_t)M * T * K, YMAX = 65535;   // (a grid's y extent)
  int* dpools = s.alloc<int>((size_t)S * M);
  MonoArgs a = {};
  a.N = N; a.M = M; a.T = T; a.increasing = increasing ? 1 : 0;
  for (size_t s0 = 0; s0 < (size_t)S; s0 += YMAX) {
    const unsigned sc = (unsigned)std::min<size_t>(YMAX, (size_t)S - s0);
    a.W = dW + s0 * nW; a.Vin = dVin + s0 * nV; a.Vout = dVout + s0 * nV; a.pools = dpools + s0 * M;
    launch_counted(s, BTF_K_CRITERIA, project, dim3((unsigned)M, sc), dim3(MONO_THREADS), mono_lds(T, K), a);
  }
  if (mean_out) summary_stage(s, dW, dVout, S, N, M * T, K, transform, q, nq, mean_out, q_out);
  s.download(V_out, (const double*)dVout, (size_t)S * nV);
  s.download(pools_out, (const int*)dpools, (size_t)S * M);
  return s.finish();
}

// argument checks shared by the two entry points; everything here runs before any device call
int mono_check(btf_ctx* c, int S, int N, int M, int T, int K, int transform, const double* q, int nq, const double* mean_out,
               const double* q_out) {
  if (S < 1 || N < 1 || M < 1 || T < 1 || K < 1 || K > MAX_K || nq < 0 || (nq > 0 && (!q || !q_out || !mean_out)) ||
      (mean_out && (transform < 0 || transform > 2)))
    return fail(c, BTF_EINVAL, "bad posterior monotone arguments");
  if (mean_out && S > 16384) return fail(c, BTF_EINVAL, "posterior monotone: at most 16384 samples with a summary (its values are sorted in LDS)");
  if (!mono_fits(T, K))
    return fail(c, BTF_EINVAL, "posterior monotone: ndepth * nembeds too large for the PAV kernels (pav_fits: 8 T K + 4 T <= 65536 bytes of LDS)");
  if ((long long)M * T > 0x7fffffffLL) return fail(c, BTF_EINVAL, "posterior monotone: too many cells for one launch");
  if (int rc = check_percentiles(c, q, nq)) return rc;
  return BTF_OK;
}
}  // namespace

int btf_posterior_monotone(int device, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* Ws, const double* Vs,
                           int increasing, int transform, const double* q, int nq, double* V_out, int* pools_out, double* mean_out,
                           double* q_out) {
  if (!Ws || !Vs) return fail(nullptr, BTF_EINVAL, "bad posterior monotone arguments");
  if (int rc = mono_check(nullptr, nsamples, nrows, ncols, ndepth, nembeds, transform, q, nq, mean_out, q_out)) return rc;
  Scratch s(nullptr, nullptr); States st;      // (V: the scratch's own copy, projected where it lies)
  if (int rc = resolve_pair(s, device, "", 0, nsamples, nrows, ncols * ndepth, nembeds, Ws, Vs, st)) return rc;
  return mono_run(s, st.W, st.V, st.V, nsamples, nrows, ncols, ndepth, nembeds, increasing, transform, q, nq, V_out, pools_out, mean_out, q_out);
}

// the same on the first nsamples collected states, read where they lie (Ws = Vs = NULL), or on uploaded states on the
// context's device and stream; in_place overwrites the collected V samples and needs no second copy of them
int btf_collect_monotone(btf_ctx* c, int nsamples, const double* Ws, const double* Vs, int increasing, int in_place, int transform,
                         const double* q, int nq, double* V_out, int* pools_out, double* mean_out, double* q_out) {
  if (!c || (Ws == nullptr) != (Vs == nullptr)) return fail(c, BTF_EINVAL, "bad posterior monotone arguments");
  if (int rc = mono_check(c, nsamples, c->N, c->M, c->T, c->K, transform, q, nq, mean_out, q_out)) return rc;
  if (in_place && Ws) return fail(c, BTF_EINVAL, "btf_collect_monotone: in_place projects the collected samples, not uploaded states");
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_monotone", BTF_EINVAL, nsamples, c->N, c->M * c->T, c->K, Ws, Vs, st)) return rc;
  if (Ws) return mono_run(s, st.W, st.V, st.V, nsamples, c->N, c->M, c->T, c->K, increasing, transform, q, nq, V_out, pools_out, mean_out, q_out);
  double* dVout = in_place ? st.V : s.alloc<double>((size_t)nsamples * c->M * c->T * c->K);
  return mono_run(s, st.W, st.V, dVout, nsamples, c->N, c->M, c->T, c->K, increasing, transform, q, nq, V_out, pools_out, mean_out, q_out);
}

// ---------------------------------------------------------------- folding new rows in (btf_fold_in.h)
namespace {
thread_local int g_fold_fail_index = -1;      // btf_fail_index(NULL): the failing (sample, row) of the last stateless call

struct FoldIn {
  int family, S, R, M, T, K;
  const double *count, *ysum, *trials, *z;
  unsigned long long seed;
  int inner_sweeps;
  long long sample0;
  double *W_out, *Wmean_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
};

// everything that can be refused without a device
int fold_in_check(btf_ctx* c, const FoldIn& f) {
  if (f.family < FOLD_GAUSSIAN || f.family > FOLD_BINOMIAL || f.S < 1 || f.R < 1 || f.M < 1 || f.T < 1 || f.K < 1 || f.K > MAX_K ||
      !f.ysum || !f.W_out || f.sample0 < 0 || f.nq < 0 || (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2)
    return fail(c, BTF_EINVAL, "bad fold_in arguments");
  if (f.family == FOLD_GAUSSIAN && !f.count) return fail(c, BTF_EINVAL, "fold_in: the Gaussian family needs count");
  if (f.family == FOLD_BINOMIAL && (!f.trials || f.z || f.inner_sweeps < 1))
    return fail(c, BTF_EINVAL, "fold_in: the Binomial family needs trials and inner_sweeps >= 1, and takes no z");
  if (f.mean_out && f.S > 16384) return fail(c, BTF_EINVAL, "fold_in: the summary stage takes at most 16384 samples");
  if ((double)(f.sample0 + f.S) * f.R >= 2147483647.0 || (double)f.R * f.M * f.T >= 2147483647.0)
    return fail(c, BTF_EINVAL, "fold_in: (sample0 + nsamples) * nrows_new and nrows_new * ncols * ndepth must stay below 2^31");
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  const size_t n = (size_t)f.R * f.M * f.T;
  const double* cw = f.family == FOLD_GAUSSIAN ? f.count : f.trials;
  for (size_t e = 0; e < n; ++e) {
    if (!(cw[e] >= 0.0 && cw[e] < 1e15) || !(std::fabs(f.ysum[e]) < INFINITY))
      return fail(c, BTF_EINVAL, "fold_in: counts must be finite and non-negative, sums finite (0 where nothing was observed)");
    if (f.family == FOLD_BINOMIAL && (cw[e] != std::floor(cw[e]) || cw[e] > (double)FOLD_MAX_TRIALS))
      return fail(c, BTF_EINVAL, "fold_in: Binomial trial counts must be integers up to " + std::to_string(FOLD_MAX_TRIALS));
  }
  return BTF_OK;
}

// The launches on device states dV (S,M,T,K) and per-sample scalars on the device (noise may be null: 1).  The scratch's
// context may be null (the stateless form: default stream, launches not counted).  W stays on the device between the draw
// and the summary.
int fold_in_run(Scratch& s, const double* dV, const double* dnoise, int nstride, const double* dsig, int sstride, const FoldIn& f) {
  btf_ctx* c = s.ctx();
  const int S = f.S, R = f.R, MT = f.M * f.T, K = f.K;
  FoldKernel kern = fold_in_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, "fold_in: nembeds must be 1..10 and family 0..1");
  // row statistics in the kernel's [cell][row] layout; Binomial: kappa = successes - trials / 2
  std::vector<double> hc((size_t)MT * R), hy((size_t)MT * R);
  const double* cw = f.family == FOLD_GAUSSIAN ? f.count : f.trials;
  for (int r = 0; r < R; ++r)
    for (int jt = 0; jt < MT; ++jt) {
      const double cv = cw[(size_t)r * MT + jt], yv = f.ysum[(size_t)r * MT + jt];
      hc[(size_t)jt * R + r] = cv;
      hy[(size_t)jt * R + r] = f.family == FOLD_BINOMIAL ? (cv > 0.0 ? yv - 0.5 * cv : 0.0) : (cv > 0.0 ? yv : 0.0);
    }
  const size_t nW = (size_t)S * R * K, cellsN = (size_t)R * MT;
  const int stat0[2] = {0, INT_MAX};
  FoldArgs a = {};
  a.V = dV; a.noise = dnoise; a.sigma2 = dsig; a.nstride = nstride; a.sstride = sstride;
  a.cnt = s.upload(hc.data(), cellsN); a.ysum = s.upload(hy.data(), cellsN);
  a.W = s.alloc<double>(nW); a.status = s.upload(stat0, 2);
  if (f.Wmean_out) a.Wmean = s.alloc<double>(nW);
  if (f.z) a.z = s.upload(f.z, nW);
  a.seed = f.seed; a.sample0 = f.sample0; a.S = S; a.R = R; a.MT = MT; a.sweeps = f.inner_sweeps;
  launch_counted(s, BTF_K_CRITERIA, kern, dim3(S, (R + WAVE - 1) / WAVE), dim3(FOLD_PARTS * WAVE), 0, a);
  // the summary stage reads the device-resident W (S,R,K) and V
  if (f.mean_out) summary_stage(s, a.W, dV, S, R, MT, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[2] = {0, INT_MAX};
  s.download(stat, a.status, 2);
  s.download(f.W_out, a.W, nW);
  s.download(f.Wmean_out, a.Wmean, nW);
  const int rc = s.finish();
  if (rc) return rc;
  if (stat[0]) {
    if (c) c->fail_index = stat[1];
    g_fold_fail_index = stat[1];
    return fail(c, BTF_ENOTPD, "fold_in: the precision of (sample, row) index " + std::to_string(stat[1]) +
                                   " = sample * nrows_new + row is not positive definite (or nu2 / sigma2 / V not finite)");
  }
  return BTF_OK;
}
}  // namespace

int btf_fold_in_rows(int device, int family, int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs,
                     const double* noise, const double* sigma2, const double* count, const double* ysum, const double* trials,
                     const double* z, unsigned long long seed, int inner_sweeps, long long sample0, double* W_out, double* Wmean_out,
                     int transform, const double* q, int nq, double* mean_out, double* q_out) {
  const FoldIn f = {family, nsamples, nrows_new, ncols, ndepth, nembeds, count, ysum, trials, z, seed, inner_sweeps, sample0,
                    W_out, Wmean_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Vs || !sigma2 || (family == FOLD_GAUSSIAN && !noise)) return fail(nullptr, BTF_EINVAL, "bad fold_in arguments");
  if (int rc = fold_in_check(nullptr, f)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(sigma2[s] > 0.0 && sigma2[s] < INFINITY) || (family == FOLD_GAUSSIAN && !(noise[s] > 0.0 && noise[s] < INFINITY)))
      return fail(nullptr, BTF_EINVAL, "fold_in: nu2 and sigma2 must be finite and positive");
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, 0, ncols * ndepth, nembeds, nullptr, Vs, st)) return rc;
  const double* ds = s.upload(sigma2, (size_t)nsamples);
  const double* dn = family == FOLD_GAUSSIAN ? s.upload(noise, (size_t)nsamples) : nullptr;
  return fold_in_run(s, st.V, dn, 1, ds, 1, f);
}

// the same on the first nsamples collected states, read where they lie (no upload): V from the sample slots, nu2_s and
// sigma2_s from the collected scalars
int btf_collect_fold_in(btf_ctx* c, int family, int nsamples, int nrows_new, const double* count, const double* ysum,
                        const double* trials, const double* z, unsigned long long seed, int inner_sweeps, long long sample0,
                        double* W_out, double* Wmean_out, int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (!c) return fail(c, BTF_EINVAL, "bad fold_in arguments");
  const FoldIn f = {family, nsamples, nrows_new, c->M, c->T, c->K, count, ysum, trials, z, seed, inner_sweeps, sample0,
                    W_out, Wmean_out, transform, q, nq, mean_out, q_out};
  if (int rc = fold_in_check(c, f)) return rc;
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_fold_in", BTF_ESTATE, nsamples, 0, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return fold_in_run(s, st.V, family == FOLD_GAUSSIAN ? c->smp_s + HYP_NU2 : nullptr, (int)HYP_COUNT,
                     c->smp_s + HYP_SIGMA2, (int)HYP_COUNT, f);
}

// ---------------------------------------------------------------- folding new rows into a slice-sampled fit (btf_slice_fold.h)
namespace {
struct SliceFold {
  int family; double param;
  int S, R, M, T, K;
  const double *start, *S1, *cnt, *L;
  const double* cons; int J;
  const double* rcons; int nrc;
  const double* Us; int F; const unsigned char* codes;
  const double* draws;
  unsigned long long seed;
  int sweeps, max_rounds;
  long long sample0;
  double *W_out, *Wstart_out; int *rounds_out, *unf_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
};

bool all_finite(const double* p, size_t n) {
  for (size_t e = 0; e < n; ++e)
    if (!(std::fabs(p[e]) < INFINITY)) return false;
  return true;
}

// everything that can be refused without a device
int slice_fold_check(btf_ctx* c, const SliceFold& f) {
  if (f.family < 0 || f.family >= ESS_FAM_COUNT || f.S < 1 || f.R < 1 || f.M < 1 || f.T < 1 || f.K < 1 || f.K > MAX_K || !f.S1 || !f.cnt ||
      !f.W_out || !f.rounds_out || !f.unf_out || f.sample0 < 0 || f.nq < 0 || (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) ||
      f.transform < 0 || f.transform > 2 || f.J < 0 || (f.J > 0 && !f.cons) || f.nrc < 0 || (f.nrc > 0 && !f.rcons) || f.F < 0 ||
      (f.F > 0 && (!f.Us || !f.codes)))
    return fail(c, BTF_EINVAL, "bad slice_fold arguments");
  if (f.sweeps < 1 || f.max_rounds < 1 || f.max_rounds > 65536) return fail(c, BTF_EINVAL, "slice_fold: sweeps >= 1 and max_rounds in 1..65536");
  if (f.family == ESS_FAM_GAMMA_GRID && !f.L) return fail(c, BTF_EINVAL, "slice_fold: the gamma-grid family needs logsum");
  if (f.mean_out && f.S > 16384) return fail(c, BTF_EINVAL, "slice_fold: the summary stage takes at most 16384 samples");
  if ((double)(f.sample0 + f.S) * f.R >= 2147483647.0 || (double)f.R * f.M * f.T >= 2147483647.0 || (double)f.M * f.J >= 2147483647.0 ||
      (double)f.sweeps * (f.K + 1 + f.max_rounds) >= 2147483647.0)
    return fail(c, BTF_EINVAL, "slice_fold: (sample0 + nsamples) * nrows_new, nrows_new * ncols * ndepth, ncols * ncons and the draws of a chain must stay below 2^31");
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  const size_t n = (size_t)f.R * f.M * f.T;
  for (size_t e = 0; e < n; ++e)
    if (!(f.cnt[e] >= 0.0 && f.cnt[e] < 1e15) || !(std::fabs(f.S1[e]) < INFINITY) || (f.L && !(std::fabs(f.L[e]) < INFINITY)))
      return fail(c, BTF_EINVAL, "slice_fold: counts must be finite and non-negative, sums finite (0 where nothing was observed)");
  if (!all_finite(f.cons, (size_t)f.J * (f.T + 1)) || !all_finite(f.rcons, (size_t)f.nrc * (f.K + 1)))
    return fail(c, BTF_EINVAL, "slice_fold: constraints must be finite");
  for (size_t e = 0; e < (size_t)f.R * f.F; ++e)
    if (f.codes[e] > 2) return fail(c, BTF_EINVAL, "slice_fold: feature codes are 0, 1 or 2 (missing)");
  return BTF_OK;
}

// The launches on device states dV (S,M,T,K), dW (S,N,K; read when the call has no start) and per-sample sigma2 on the
// device; dgg: the gamma-grid table on the device (family 5).  The scratch's context may be null (the stateless form).
// W stays on the device between the chains and the summary.
int slice_fold_run(Scratch& s, const double* dV, const double* dW, int N, const double* dsig, int sstride, const GgComp* dgg, int G,
                   double lsp, const SliceFold& f) {
  btf_ctx* c = s.ctx();
  const int S = f.S, R = f.R, MT = f.M * f.T, K = f.K, T = f.T;
  SliceFoldKernel kern = slice_fold_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, "slice_fold: nembeds must be 1..10 and family 0..5");
  // Constraints_A by its non-zeros (CSR over the constraints), the bounds beside it
  std::vector<int> cptr(1, 0), cidx;
  std::vector<double> cval, cc;
  for (int q = 0; q < f.J; ++q) {
    for (int t = 0; t < T; ++t)
      if (f.cons[(size_t)q * (T + 1) + t] != 0.0) { cidx.push_back(t); cval.push_back(f.cons[(size_t)q * (T + 1) + t]); }
    cptr.push_back((int)cidx.size());
    cc.push_back(f.cons[(size_t)q * (T + 1) + T]);
  }
  const size_t nW = (size_t)S * R * K, cells = (size_t)R * MT, nch = (size_t)S * R;
  const int stat0[2] = {0, INT_MAX};
  SliceFoldArgs a = {};
  a.V = dV; a.sigma2 = dsig; a.sstride = sstride;
  a.S1 = s.upload(f.S1, cells); a.cnt = s.upload(f.cnt, cells);
  if (f.L) a.L = s.upload(f.L, cells);
  if (cidx.empty()) { cidx.push_back(0); cval.push_back(0.0); cc.push_back(0.0); }      // (never read: J = 0, or rows of zeros)
  a.cs_ptr = s.upload(cptr.data(), cptr.size()); a.cs_idx = s.upload(cidx.data(), cidx.size());
  a.cs_val = s.upload(cval.data(), cval.size()); a.Cc = s.upload(cc.data(), cc.size()); a.J = f.J;
  if (f.nrc) a.Rc = s.upload(f.rcons, (size_t)f.nrc * (K + 1));
  a.nrc = f.nrc;
  if (f.F) { a.U = s.upload(f.Us, (size_t)S * f.F * K); a.codes = s.upload(f.codes, (size_t)R * f.F); }
  a.F = f.F;
  const int rec = K + 1 + f.max_rounds;
  if (f.draws) a.draws = s.upload(f.draws, nch * f.sweeps * rec);
  a.gg = dgg; a.G = G; a.lsp = lsp; a.fam = f.family; a.par = f.param;
  double* dmean = nullptr;
  if (f.start) { a.start = s.upload(f.start, nW); a.st_s = (long long)R * K; a.st_r = K; }
  else {
    dmean = s.alloc<double>((size_t)S * K);
    const int nb = (int)(((size_t)S * K + 255) / 256);
    launch_counted(s, BTF_K_CRITERIA, slice_fold_mean_fn(), dim3(nb), dim3(256), 0, dW, S, N, K, dmean);
    a.start = dmean; a.st_s = K; a.st_r = 0;
  }
  double* dWout = s.alloc<double>(nW);
  a.W = dWout; a.rounds = s.alloc<int>(nch); a.unfinished = s.alloc<int>(nch); a.status = s.upload(stat0, 2);
  a.seed = f.seed; a.sample0 = f.sample0; a.S = S; a.R = R; a.M = f.M; a.T = T; a.sweeps = f.sweeps; a.max_rounds = f.max_rounds;
  launch_counted(s, BTF_K_CRITERIA, kern, dim3((unsigned)((nch + SF_CHAINS - 1) / SF_CHAINS)), dim3(SF_CHAINS * WAVE), 0, a);
  // the summary stage reads the device-resident W (S,R,K) and V
  if (f.mean_out) summary_stage(s, dWout, dV, S, R, MT, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[2] = {0, INT_MAX};
  std::vector<double> hmean(dmean ? (size_t)S * K : 0);
  s.download(stat, (const int*)a.status, 2);
  s.download(f.W_out, (const double*)dWout, nW);
  s.download(f.rounds_out, (const int*)a.rounds, nch);
  s.download(f.unf_out, (const int*)a.unfinished, nch);
  if (dmean && f.Wstart_out) s.download(hmean.data(), (const double*)dmean, hmean.size());
  const int rc = s.finish();
  if (rc) return rc;
  if (f.Wstart_out) {
    if (f.start) std::copy(f.start, f.start + nW, f.Wstart_out);
    else
      for (size_t e = 0; e < nW; ++e) f.Wstart_out[e] = hmean[(e / ((size_t)R * K)) * K + e % K];
  }
  if (stat[0]) {
    if (c) c->fail_index = stat[1];
    g_fold_fail_index = stat[1];
    const long long sg = stat[1] / R;
    return fail(c, BTF_ESTATE, "slice_fold: the start of (sample " + std::to_string(sg) + ", row " + std::to_string(stat[1] - sg * R) +
                                   ") is infeasible or has a non-finite likelihood (index " + std::to_string(stat[1]) +
                                   " = sample * nrows_new + row)");
  }
  return BTF_OK;
}
}  // namespace

int btf_slice_fold_rows(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                        int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs, const double* Ws,
                        int nrows_fit, const double* start, const double* sigma2, const double* S1, const double* cnt,
                        const double* logsum, const double* constraints, int ncons, const double* row_constraints, int nrow_cons,
                        const double* Us, int nfeatures, const unsigned char* codes, const double* draws, unsigned long long seed,
                        int sweeps, int max_rounds, long long sample0, double* W_out, double* Wstart_out, int* rounds_out,
                        int* unfinished_out, int transform, const double* q, int nq, double* mean_out, double* q_out) {
  const SliceFold f = {family, param, nsamples, nrows_new, ncols, ndepth, nembeds, start, S1, cnt, logsum, constraints, ncons,
                       row_constraints, nrow_cons, Us, nfeatures, codes, draws, seed, sweeps, max_rounds, sample0, W_out, Wstart_out,
                       rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Vs || !sigma2 || (!start && (!Ws || nrows_fit < 1))) return fail(nullptr, BTF_EINVAL, "bad slice_fold arguments");
  if (int rc = slice_fold_check(nullptr, f)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(sigma2[s] > 0.0 && sigma2[s] < INFINITY)) return fail(nullptr, BTF_EINVAL, "slice_fold: sigma2 must be finite and positive");
  if ((family == ESS_FAM_GAUSSIAN || family == ESS_FAM_NEGBIN_LOGIT) && !(param > 0.0 && param < INFINITY))
    return fail(nullptr, BTF_EINVAL, "slice_fold: the parameter must be positive");
  std::vector<GgComp> tab;
  double lsp = 0.0;
  if (family == ESS_FAM_GAMMA_GRID && gg_comp_table(shape, scale, prob, G, tab, lsp) != 0)
    return fail(nullptr, BTF_EINVAL, "slice_fold: the gamma grid has 1..128 components with finite shape > 0, scale > 0, weight >= 0, not all zero");
  Scratch s(nullptr, nullptr); States st;
  const bool mean_start = start == nullptr;
  if (int rc = resolve_pair(s, device, "", 0, nsamples, mean_start ? nrows_fit : 0, ncols * ndepth, nembeds, mean_start ? Ws : nullptr, Vs, st))
    return rc;
  const double* ds = s.upload(sigma2, (size_t)nsamples);
  const GgComp* dgg = tab.empty() ? nullptr : s.upload(tab.data(), tab.size());
  return slice_fold_run(s, st.V, st.W, nrows_fit, ds, 1, dgg, (int)tab.size(), lsp, f);
}

// the same on the first nsamples collected states, read where they lie (no upload): W and V from the sample slots,
// sigma2_s from the collected scalars, the likelihood's parameter or table from the context
int btf_collect_slice_fold(btf_ctx* c, int family, int nsamples, int nrows_new, const double* start, const double* S1,
                           const double* cnt, const double* logsum, const double* constraints, int ncons,
                           const double* row_constraints, int nrow_cons, const double* Us, int nfeatures,
                           const unsigned char* codes, const double* draws, unsigned long long seed, int sweeps, int max_rounds,
                           long long sample0, double* W_out, double* Wstart_out, int* rounds_out, int* unfinished_out,
                           int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (!c || family < 0 || family >= ESS_FAM_COUNT) return fail(c, BTF_EINVAL, "bad slice_fold arguments");
  const SliceFold f = {family, c->lik_par[family], nsamples, nrows_new, c->M, c->T, c->K, start, S1, cnt, logsum, constraints, ncons,
                       row_constraints, nrow_cons, Us, nfeatures, codes, draws, seed, sweeps, max_rounds, sample0, W_out, Wstart_out,
                       rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  if (int rc = slice_fold_check(c, f)) return rc;
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, "btf_collect_slice_fold needs an unsharded context");
  if (family == ESS_FAM_GAMMA_GRID && !c->gg_tab) return fail(c, BTF_ESTATE, "btf_collect_slice_fold: the gamma-grid family needs its table (btf_set_likelihood_table)");
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_slice_fold", BTF_ESTATE, nsamples, 0, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return slice_fold_run(s, st.V, st.W, c->N, c->smp_s + HYP_SIGMA2, (int)HYP_COUNT, c->gg_tab, c->gg_G, c->gg_lsp, f);
}

// ---------------------------------------------------------------- what the column and depth fold-ins share (btf_fold_chain.h)
namespace {
// first and last non-zero of a penalty row over T depths (hi < 0: none)
void penalty_row_window(const double* row, int T, int& lo, int& hi) {
  lo = T; hi = -1;
  for (int t = 0; t < T; ++t)
    if (row[t] != 0.0) { lo = std::min(lo, t); hi = std::max(hi, t); }
}
// its D1 = tf + 2 coefficients from lo on (0 past the row's end)
void penalty_row_coefs(const double* row, int lo, int hi, int D1, std::vector<double>& rcoef) {
  for (int e = 0; e < D1; ++e) rcoef.push_back(lo + e <= hi ? row[lo + e] : 0.0);
}

// the sweeps a chain's generator slots hold; `name` opens every message
bool fold_sweeps_ok(int sweeps) { return sweeps >= 1 && (unsigned long long)sweeps < FOLD_CHAIN_PG_SLOT; }
int fold_sweeps_check(btf_ctx* c, const std::string& name, int sweeps) {
  return fold_sweeps_ok(sweeps) ? BTF_OK : fail(c, BTF_EINVAL, name + ": sweeps must be in 1..2^20 - 2");
}
// the same with the proposals of a slice sweep
int slice_fold_sweeps_check(btf_ctx* c, const std::string& name, int sweeps, int max_rounds) {
  if (fold_sweeps_ok(sweeps) && max_rounds >= 1 && max_rounds <= 65536) return BTF_OK;
  return fail(c, BTF_EINVAL, name + ": sweeps in 1..2^20 - 2 and max_rounds in 1..65536");
}
// the sizes: S samples at sample0, C chains per sample (`cols`: their name), N rows, T depths (`depths`: their name) per chain;
// pg_cells: the Polya-Gamma cell indices of a chain (sweeps * N * T, 0 for a chain without them)
int fold_sizes_check(btf_ctx* c, const std::string& name, const char* cols, const char* depths, int S, int C, int N, int T, int K, int tf,
                     long long sample0, bool summary, double pg_cells) {
  if ((tf + 1) * K >= WAVE) return fail(c, BTF_EINVAL, name + ": the half bandwidth (tf_order + 1) nembeds must stay below 64");
  if (summary && S > 16384) return fail(c, BTF_EINVAL, name + ": the summary stage takes at most 16384 samples");
  if ((double)(sample0 + S) * C >= 2147483647.0 || (double)C * N * T >= 2147483647.0 || pg_cells >= 9.0e15)
    return fail(c, BTF_EINVAL, name + ": (sample0 + nsamples) * " + cols + " and " + cols + " * nrows * " + depths + " must stay below 2^31");
  return BTF_OK;
}
int fold_lds_check(btf_ctx* c, const std::string& name, const char* what, size_t lds) {
  if (lds <= FOLD_CHAIN_LDS_LIMIT) return BTF_OK;
  return fail(c, BTF_EINVAL, name + ": the band of " + what + " needs " + std::to_string(lds) + " bytes of LDS, beyond the limit of " +
                                 std::to_string(FOLD_CHAIN_LDS_LIMIT));
}
// the cells of a Gibbs fold-in: cw the counts (Gaussian) or the trials (Binomial)
int fold_cells_check(btf_ctx* c, const std::string& name, const double* cw, const double* ysum, size_t ncell, bool binomial) {
  for (size_t e = 0; e < ncell; ++e) {
    if (!(cw[e] >= 0.0 && cw[e] < 1e15) || !(std::fabs(ysum[e]) < INFINITY))
      return fail(c, BTF_EINVAL, name + ": counts must be finite and non-negative, sums finite (0 where nothing was observed)");
    if (binomial && (cw[e] != std::floor(cw[e]) || cw[e] > (double)FOLD_CHAIN_MAX_TRIALS))
      return fail(c, BTF_EINVAL, name + ": Binomial trial counts must be integers up to " + std::to_string(FOLD_CHAIN_MAX_TRIALS));
  }
  return BTF_OK;
}
// the cells of a slice-sampled fold-in: statistics and the fit (L: the gamma grid's, or null)
int slice_fold_cells_check(btf_ctx* c, const std::string& name, const double* cnt, const double* S1, const double* L, const double* fa,
                           const double* fb, size_t ncell) {
  for (size_t e = 0; e < ncell; ++e)
    if (!(cnt[e] >= 0.0 && cnt[e] < 1e15) || !(std::fabs(S1[e]) < INFINITY) || (L && !(std::fabs(L[e]) < INFINITY)) ||
        !(fa[e] >= 0.0 && fa[e] < INFINITY) || !(std::fabs(fb[e]) < INFINITY))
      return fail(c, BTF_EINVAL, name + ": counts and fit weights must be finite and non-negative, sums finite (0 where there is nothing)");
  return BTF_OK;
}
// The cells and the rate of a Negative-Binomial fold-in, in the place of fold_cells_check's "integers up to 32": counts and
// sums finite and non-negative; the rate a compact array over dims = (samples, chains, rows, depths) with every axis full or
// shared (stride 0), finite and positive; b = ysum + count * rate below 1e15, checked with the largest of each; the replay
// weights finite and non-negative.  nrate: the values the rate holds.
int negbin_fold_cells_check(btf_ctx* c, const std::string& name, const double* cnt, const double* ysum, size_t ncell, const double* rate,
                            const long long (&rs)[4], const int (&dims)[4], const double* omega, size_t nomega, size_t& nrate) {
  double cmax = 0.0, ymax = 0.0, rmax = 0.0;
  for (size_t e = 0; e < ncell; ++e) {
    if (!(cnt[e] >= 0.0 && cnt[e] < 1e15) || !(ysum[e] >= 0.0 && ysum[e] < 1e15))
      return fail(c, BTF_EINVAL, name + ": counts and their sums must be finite and non-negative (0 where nothing was observed)");
    cmax = std::max(cmax, cnt[e]); ymax = std::max(ymax, ysum[e]);
  }
  nrate = 1;
  for (int a = 3; a >= 0; --a) {
    if (rs[a] == 0) continue;
    if (rs[a] != (long long)nrate)
      return fail(c, BTF_EINVAL, name + ": the rate strides must be those of a compact (sample, column, row, depth) array, 0 on a shared axis");
    nrate *= (size_t)dims[a];
  }
  for (size_t e = 0; e < nrate; ++e) {
    if (!(rate[e] > 0.0 && rate[e] < INFINITY)) return fail(c, BTF_EINVAL, name + ": the rate must be finite and positive");
    rmax = std::max(rmax, rate[e]);
  }
  if (!(ymax + cmax * rmax < 1e15)) return fail(c, BTF_EINVAL, name + ": ysum + count * rate must stay below 1e15");
  for (size_t e = 0; omega && e < nomega; ++e)
    if (!(omega[e] >= 0.0 && omega[e] < INFINITY)) return fail(c, BTF_EINVAL, name + ": omega must be finite and non-negative");
  return BTF_OK;
}
// `draws` of nch chains: 4 nlev start gammas, then per sweep n normals, nu uniforms (0: a Gibbs chain) and 4 nlev gammas
int fold_draws_check(btf_ctx* c, const std::string& name, const double* draws, size_t nch, size_t n, size_t nu, size_t nlev, int sweeps) {
  if (!draws) return BTF_OK;
  const size_t head = 4 * nlev, per = n + nu + 4 * nlev, L = head + (size_t)sweeps * per;
  for (size_t ch = 0; ch < nch; ++ch) {
    const double* d = draws + ch * L;
    for (size_t e = 0; e < L; ++e) {
      const size_t pos = e < head ? per : (e - head) % per;         // (per: a start gamma)
      const bool normal = pos < n, uniform = pos >= n && pos < n + nu;
      if (!(std::fabs(d[e]) < INFINITY) || (!normal && !(d[e] > 0.0)) || (uniform && !(d[e] < 1.0)))
        return fail(c, BTF_EINVAL, name + (nu ? ": draws must be finite, its uniforms inside (0, 1), its gamma variates positive"
                                              : ": draws must be finite, its gamma variates positive"));
    }
  }
  return BTF_OK;
}
// a chain's failure, from the kernel's status pair: the index for btf_fail_index ...
void fold_fail_at(btf_ctx* c, int index) {
  if (c) c->fail_index = index;
  g_fold_fail_index = index;
}
// ... and the message.  `cols`: the name of the chains per sample; `inputs`: what a non-positive pivot may come from.
int fold_pivot_fail(btf_ctx* c, const std::string& name, int index, const char* cols, const char* inputs) {
  fold_fail_at(c, index);
  return fail(c, BTF_ESTATE, name + ": the precision of (sample, column) index " + std::to_string(index) + " = sample * " + cols +
                                 " + column is not positive definite (or " + inputs + " not finite); its outputs are nan");
}
int slice_fold_start_fail(btf_ctx* c, const std::string& name, int index, int C, const char* cols) {
  fold_fail_at(c, index);
  const long long sg = index / C;
  return fail(c, BTF_ESTATE, name + ": the start of (sample " + std::to_string(sg) + ", column " + std::to_string(index - sg * C) +
                                 ") is infeasible or has a non-finite likelihood (index " + std::to_string(index) + " = sample * " + cols +
                                 " + column)");
}
}  // namespace

// ---------------------------------------------------------------- folding new columns in (btf_fold_in_cols.h)
namespace {
struct FoldCols {
  int family, S, C, N, T, K, tf;
  const double *count, *ysum, *trials, *draws;
  unsigned long long seed;
  int sweeps;
  long long sample0;
  double stability;
  double *V_out, *Vmean_out, *Tau2_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
  // the Negative-Binomial family (FOLDC_NEGBIN) alone: the rate, its strides (sample, column, row, depth), the replay weights
  const double* rate; long long rs[4]; const double* omega;
  size_t nrate;
};

// the penalty rows on the host: Delta, its CSR stencil, and every row as (first depth, tf + 2 coefficients from there on)
struct FoldColsPenalty {
  int nD = 0;
  std::vector<double> Delta, coef, rcoef;
  std::vector<int> ptr, row, rcol0;
};

// fills the penalty of T depths (shared with slice_fold_cols_check); `name` opens the messages
int fold_cols_rows(btf_ctx* c, const char* name, int T, int tf, FoldColsPenalty& p) {
  const int D1 = tf + 2;
  p.rcol0.assign(p.nD, 0); p.rcoef.clear();
  for (int r = 0; r < p.nD; ++r) {
    int lo, hi;
    penalty_row_window(&p.Delta[(size_t)r * T], T, lo, hi);
    if (hi < 0 || hi - lo >= D1) return fail(c, BTF_EINVAL, std::string(name) + ": penalty row wider than the band");
    p.rcol0[r] = lo;
    penalty_row_coefs(&p.Delta[(size_t)r * T], lo, hi, D1, p.rcoef);
  }
  return BTF_OK;
}

// everything that can be refused without a device; fills the penalty
int fold_cols_check(btf_ctx* c, const FoldCols& f, FoldColsPenalty& p) {
  if (f.family < FOLDC_GAUSSIAN || f.family > FOLDC_BINOMIAL || f.S < 1 || f.C < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 ||
      f.T < 2 || !f.ysum || !f.V_out || !f.Vmean_out || !f.Tau2_out || f.sample0 < 0 || f.nq < 0 ||
      (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2 || !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad fold_in_cols arguments");
  if (f.family == FOLDC_GAUSSIAN && !f.count) return fail(c, BTF_EINVAL, "fold_in_cols: the Gaussian family needs count");
  if (f.family == FOLDC_BINOMIAL && (!f.trials || f.draws))
    return fail(c, BTF_EINVAL, "fold_in_cols: the Binomial family needs trials and takes no draws");
  if (int rc = fold_sweeps_check(c, "fold_in_cols", f.sweeps)) return rc;
  if (int rc = fold_sizes_check(c, "fold_in_cols", "ncols_new", "ndepth", f.S, f.C, f.N, f.T, f.K, f.tf, f.sample0, f.mean_out != nullptr,
                                (double)f.sweeps * f.N * f.T))
    return rc;
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  penalty_stencil(f.T, f.tf, p.Delta, p.nD, p.ptr, p.row, p.coef);
  if (int rc = fold_lds_check(c, "fold_in_cols", "a column", foldc_lds_bytes(f.T, f.K, f.tf, p.nD))) return rc;
  if (int rc = fold_cols_rows(c, "fold_in_cols", f.T, f.tf, p)) return rc;
  if (int rc = fold_cells_check(c, "fold_in_cols", f.family == FOLDC_GAUSSIAN ? f.count : f.trials, f.ysum, (size_t)f.C * f.N * f.T,
                                f.family == FOLDC_BINOMIAL))
    return rc;
  return fold_draws_check(c, "fold_in_cols", f.draws, (size_t)f.S * f.C, (size_t)f.T * f.K, 0, (size_t)p.nD, f.sweeps);
}

// the same for the Negative-Binomial family: the shared checks, the weight buffer in the LDS count, and a cell check of its own
int negbin_fold_cols_check(btf_ctx* c, FoldCols& f, FoldColsPenalty& p) {
  const std::string name = "negbin_fold_in_cols";
  if (f.family != FOLDC_NEGBIN || f.S < 1 || f.C < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 || f.T < 2 || !f.count || !f.ysum ||
      !f.rate || !f.V_out || !f.Vmean_out || !f.Tau2_out || f.sample0 < 0 || f.nq < 0 || (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) ||
      f.transform < 0 || f.transform > 2 || !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad " + name + " arguments");
  if (f.draws && !f.omega) return fail(c, BTF_EINVAL, name + ": draws needs omega beside it (the chain also draws Polya-Gamma variates)");
  if (int rc = fold_sweeps_check(c, name, f.sweeps)) return rc;
  if (int rc = fold_sizes_check(c, name, "ncols_new", "ndepth", f.S, f.C, f.N, f.T, f.K, f.tf, f.sample0, f.mean_out != nullptr,
                                (double)f.sweeps * f.N * f.T))
    return rc;
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  penalty_stencil(f.T, f.tf, p.Delta, p.nD, p.ptr, p.row, p.coef);
  if (int rc = fold_lds_check(c, name, "a column and the weights of a depth", foldc_negbin_lds_bytes(f.T, f.K, f.tf, p.nD, f.N))) return rc;
  if (int rc = fold_cols_rows(c, name.c_str(), f.T, f.tf, p)) return rc;
  const int dims[4] = {f.S, f.C, f.N, f.T};
  if (int rc = negbin_fold_cells_check(c, name, f.count, f.ysum, (size_t)f.C * f.N * f.T, f.rate, f.rs, dims, f.omega,
                                       (size_t)f.S * f.C * f.sweeps * f.T * f.N, f.nrate))
    return rc;
  return fold_draws_check(c, name, f.draws, (size_t)f.S * f.C, (size_t)f.T * f.K, 0, (size_t)p.nD, f.sweeps);
}

// The launches on device states dW (S,N,K) and per-sample scalars on the device (noise null: the Binomial family).  The
// scratch's context may be null (the stateless form).  The new V stays on the device between the chains and the summary.
int fold_cols_run(Scratch& s, const double* dW, const double* dnoise, int nstride, const double* dlam, int lstride, const FoldCols& f,
                  const FoldColsPenalty& p) {
  btf_ctx* c = s.ctx();
  const int S = f.S, C = f.C, N = f.N, T = f.T, K = f.K, nD = p.nD;
  const bool negbin = f.family == FOLDC_NEGBIN;
  const std::string name = negbin ? "negbin_fold_in_cols" : "fold_in_cols";
  FoldColsKernel kern = negbin ? fold_cols_negbin_fn(K) : fold_cols_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, name + (negbin ? ": nembeds must be 1..10" : ": nembeds must be 1..10 and family 0..1"));
  // column statistics in the kernel's [column][depth][row] layout; Binomial: kappa = successes - trials / 2
  const size_t ncell = (size_t)C * N * T;
  std::vector<double> hc(ncell), hy(ncell);
  const double* cw = f.family == FOLDC_BINOMIAL ? f.trials : f.count;
  for (int j = 0; j < C; ++j)
    for (int i = 0; i < N; ++i)
      for (int t = 0; t < T; ++t) {
        const size_t src = ((size_t)j * N + i) * T + t, dst = ((size_t)j * T + t) * N + i;
        const double cv = cw[src], yv = f.ysum[src];
        hc[dst] = cv;
        hy[dst] = f.family == FOLDC_BINOMIAL ? (cv > 0.0 ? yv - 0.5 * cv : 0.0) : (cv > 0.0 ? yv : 0.0);
      }
  const size_t nV = (size_t)S * C * T * K, nT = (size_t)S * C * nD;
  const size_t L = 4 * (size_t)nD + (size_t)f.sweeps * ((size_t)T * K + 4 * (size_t)nD);
  const int stat0[2] = {0, INT_MAX};
  FoldColsArgs a = {};
  a.W = dW; a.noise = dnoise; a.lam2 = dlam; a.nstride = nstride; a.lstride = lstride;
  a.cnt = s.upload(hc.data(), ncell); a.ysum = s.upload(hy.data(), ncell);
  if (f.draws) a.draws = s.upload(f.draws, (size_t)S * C * L);
  if (negbin) {
    a.rate = s.upload(f.rate, f.nrate);
    a.rs_s = f.rs[0]; a.rs_c = f.rs[1]; a.rs_i = f.rs[2]; a.rs_t = f.rs[3];
    if (f.omega) a.omega = s.upload(f.omega, (size_t)S * C * f.sweeps * T * N);
  }
  a.rcol0 = s.upload(p.rcol0.data(), p.rcol0.size()); a.rcoef = s.upload(p.rcoef.data(), p.rcoef.size());
  a.st_ptr = s.upload(p.ptr.data(), p.ptr.size());
  a.st_row = s.upload(p.row.data(), p.row.size()); a.st_coef = s.upload(p.coef.data(), p.coef.size());
  a.V = s.alloc<double>(nV); a.Vmean = s.alloc<double>(nV); a.Tau2 = s.alloc<double>(nT);
  a.status = s.upload(stat0, 2);
  a.seed = f.seed; a.sample0 = f.sample0; a.lo = f.stability; a.hi = 1.0 / f.stability;
  a.S = S; a.C = C; a.N = N; a.T = T; a.tf = f.tf; a.nD = nD; a.sweeps = f.sweeps;
  const size_t lds = negbin ? foldc_negbin_lds_bytes(T, K, f.tf, nD, N) : foldc_lds_bytes(T, K, f.tf, nD);
  allow_lds(s, kern, lds);
  launch_counted(s, BTF_K_CRITERIA, kern, dim3((unsigned)((size_t)S * C)), dim3(WAVE), lds, a);
  // the summary stage reads the device-resident W (S,N,K) and the new V (S,C*T,K)
  if (f.mean_out) summary_stage(s, dW, a.V, S, N, C * T, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[2] = {0, INT_MAX};
  s.download(stat, a.status, 2);
  s.download(f.V_out, a.V, nV);
  s.download(f.Vmean_out, a.Vmean, nV);
  s.download(f.Tau2_out, a.Tau2, nT);
  const int rc = s.finish();
  if (rc) return rc;
  return stat[0] ? fold_pivot_fail(c, name, stat[1], "ncols_new", negbin ? "W / lam2" : "W / nu2 / lam2") : BTF_OK;
}
}  // namespace

// the Negative-Binomial family under a name of its own: count and ysum (C,N,T) are the observed replicates of a cell and their
// sum; the rate of (sample, column, row, depth) lies at rate[s rs_sample + c rs_col + i rs_row + t rs_depth]
int btf_negbin_fold_in_cols(int device, int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order, const double* Ws,
                            const double* lam2, const double* count, const double* ysum, const double* rate, long long rs_sample,
                            long long rs_col, long long rs_row, long long rs_depth, const double* omega, const double* draws,
                            unsigned long long seed, int sweeps, long long sample0, double stability, double* V_out,
                            double* Vmean_out, double* Tau2_out, int transform, const double* q, int nq, double* mean_out,
                            double* q_out) {
  FoldCols f = {FOLDC_NEGBIN, nsamples, ncols_new, nrows, ndepth, nembeds, tf_order, count, ysum, nullptr, draws, seed, sweeps, sample0,
                stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out, rate,
                {rs_sample, rs_col, rs_row, rs_depth}, omega, 0};
  g_fold_fail_index = -1;
  if (!Ws || !lam2) return fail(nullptr, BTF_EINVAL, "bad negbin_fold_in_cols arguments");
  FoldColsPenalty p;
  if (int rc = negbin_fold_cols_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY)) return fail(nullptr, BTF_EINVAL, "negbin_fold_in_cols: lam2 must be finite and positive");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  return fold_cols_run(s, dW, nullptr, 1, dl, 1, f, p);
}

// ---------------------------------------------------------------- new rows for a Negative-Binomial fit (btf_negbin_fold_rows.h)
// rate: the fixed rate through its strides, or NULL: one sampled rate per (sample, row) from rate_init (S,R), the rows'
// histograms hist_y / hist_n (R,nbins) and nmetropolis steps per sweep.  Stateless: everything is uploaded.
int btf_negbin_fold_in_rows(int device, int nsamples, int nrows_new, int ncols, int ndepth, int nembeds, const double* Vs,
                            const double* sigma2, const double* count, const double* ysum, const double* rate, long long rs_sample,
                            long long rs_row, long long rs_col, long long rs_depth, const double* rate_init, const double* hist_y,
                            const double* hist_n, int nbins, int nmetropolis, double rpropstdev, double rstdev, const double* omega,
                            const double* z, const double* mh, unsigned long long seed, int sweeps, long long sample0, double* W_out,
                            double* Wmean_out, double* R_out, double* accept_out, int transform, const double* q, int nq,
                            double* mean_out, double* q_out) {
  const std::string name = "negbin_fold_in_rows";
  const int S = nsamples, R = nrows_new, M = ncols, T = ndepth, K = nembeds;
  const bool sampled = rate == nullptr;
  g_fold_fail_index = -1;
  if (S < 1 || R < 1 || M < 1 || T < 1 || K < 1 || K > MAX_K || !Vs || !sigma2 || !count || !ysum || !W_out || !Wmean_out || sample0 < 0 ||
      nq < 0 || (nq > 0 && (!q || !q_out || !mean_out)) || transform < 0 || transform > 2)
    return fail(nullptr, BTF_EINVAL, "bad " + name + " arguments");
  if (sampled && (!rate_init || !hist_y || !hist_n || nbins < 1 || !R_out || !accept_out || nmetropolis < 1 || nmetropolis > NBROWS_MAX_STEPS ||
                  !(rpropstdev > 0.0 && rpropstdev < INFINITY) || !(rstdev > 0.0 && rstdev < INFINITY)))
    return fail(nullptr, BTF_EINVAL, name + ": a sampled rate needs rate_init, the rows' histograms, the outputs R and accept, nmetropolis in 1.." +
                                         std::to_string(NBROWS_MAX_STEPS) + " and positive finite rpropstdev and rstdev");
  if (sweeps < 1 || sweeps > NBROWS_MAX_STEPS) return fail(nullptr, BTF_EINVAL, name + ": sweeps must lie in 1.." + std::to_string(NBROWS_MAX_STEPS));
  if ((z != nullptr || mh != nullptr) && !omega)
    return fail(nullptr, BTF_EINVAL, name + ": z and mh need omega beside them (the chain also draws Polya-Gamma variates)");
  if ((mh != nullptr) != (sampled && z != nullptr))
    return fail(nullptr, BTF_EINVAL, name + ": z replays a chain together with mh when the rate is sampled, and alone when it is fixed");
  if (mean_out && S > 16384) return fail(nullptr, BTF_EINVAL, name + ": the summary stage takes at most 16384 samples");
  if ((double)(sample0 + S) * R >= 2147483647.0 || (double)R * M * T >= 2147483647.0)
    return fail(nullptr, BTF_EINVAL, name + ": (sample0 + nsamples) * nrows_new and nrows_new * ncols * ndepth must stay below 2^31");
  if (int rc = check_percentiles(nullptr, q, nq)) return rc;
  const int MT = M * T;
  const size_t cellsN = (size_t)R * MT, nSR = (size_t)S * R, nW = nSR * K, nom = (size_t)S * sweeps * cellsN;
  double r0max = 0.0;
  for (size_t e = 0; sampled && e < nSR; ++e) {
    if (!(rate_init[e] > 0.0 && rate_init[e] < INFINITY)) return fail(nullptr, BTF_EINVAL, name + ": rate_init must be finite and positive");
    r0max = std::max(r0max, rate_init[e]);
  }
  const long long rs[4] = {sampled ? 0 : rs_sample, sampled ? 0 : rs_row, sampled ? 0 : rs_col, sampled ? 0 : rs_depth};
  const int dims[4] = {S, R, M, T};
  size_t nrate = 0;
  if (int rc = negbin_fold_cells_check(nullptr, name, count, ysum, cellsN, sampled ? &r0max : rate, rs, dims, omega, nom, nrate)) return rc;
  for (size_t e = 0; sampled && e < (size_t)R * nbins; ++e)
    if (!(hist_y[e] >= 0.0 && hist_y[e] < 1e15) || !(hist_n[e] >= 0.0 && hist_n[e] < 1e15))
      return fail(nullptr, BTF_EINVAL, name + ": the histograms must be finite and non-negative");
  for (size_t e = 0; z && e < nW * sweeps; ++e)
    if (!(std::fabs(z[e]) < INFINITY)) return fail(nullptr, BTF_EINVAL, name + ": z must be finite");
  for (size_t e = 0; mh && e < nSR * sweeps * 2 * nmetropolis; ++e) {
    const bool uniform = (e / nmetropolis) % 2 == 1;
    if (!(std::fabs(mh[e]) < INFINITY) || (uniform && !(mh[e] > 0.0 && mh[e] < 1.0)))
      return fail(nullptr, BTF_EINVAL, name + ": mh must be finite, its uniforms inside (0, 1)");
  }
  for (int s = 0; s < S; ++s)
    if (sigma2[s] <= 0.0) return fail(nullptr, BTF_EINVAL, name + ": sigma2 must be positive");      // (nan / inf: the kernel flags the sample)
  NegbinFoldRowsKernel kern = negbin_fold_rows_fn(K, sampled ? 1 : 0);
  if (!kern) return fail(nullptr, BTF_EINVAL, name + ": nembeds must be 1..10");
  Scratch s(nullptr, nullptr); States st;
  if (int rc = resolve_pair(s, device, "", 0, S, 0, MT, K, nullptr, Vs, st)) return rc;
  // row statistics and histograms in the kernel's [cell][row] / [bin][row] layouts
  std::vector<double> hc(cellsN), hy(cellsN), by, bn;
  for (int r = 0; r < R; ++r)
    for (int jt = 0; jt < MT; ++jt) {
      const double cv = count[(size_t)r * MT + jt];
      hc[(size_t)jt * R + r] = cv;
      hy[(size_t)jt * R + r] = cv > 0.0 ? ysum[(size_t)r * MT + jt] : 0.0;
    }
  const int stat0[2] = {0, INT_MAX};
  NegbinFoldRowsArgs a = {};
  a.V = st.V; a.sigma2 = s.upload(sigma2, (size_t)S);
  a.cnt = s.upload(hc.data(), cellsN); a.ysum = s.upload(hy.data(), cellsN);
  if (sampled) {
    by.resize((size_t)R * nbins); bn.resize((size_t)R * nbins);
    for (int r = 0; r < R; ++r)
      for (int b = 0; b < nbins; ++b) {
        by[(size_t)b * R + r] = hist_y[(size_t)r * nbins + b];
        bn[(size_t)b * R + r] = hist_n[(size_t)r * nbins + b];
      }
    a.rate0 = s.upload(rate_init, nSR);
    a.hy = s.upload(by.data(), by.size()); a.hn = s.upload(bn.data(), bn.size());
    a.Rout = s.alloc<double>(nSR); a.accept = s.alloc<double>(nSR);
    a.B = nbins; a.nm = nmetropolis; a.rprop = rpropstdev; a.rstdev = rstdev;
  } else {
    a.rate = s.upload(rate, nrate);
    a.rs_s = rs[0]; a.rs_r = rs[1]; a.rs_j = rs[2]; a.rs_t = rs[3];
  }
  if (omega) a.omega = s.upload(omega, nom);
  if (z) a.z = s.upload(z, nW * sweeps);
  if (mh) a.mh = s.upload(mh, nSR * sweeps * 2 * nmetropolis);
  a.W = s.alloc<double>(nW); a.Wmean = s.alloc<double>(nW); a.status = s.upload(stat0, 2);
  a.seed = seed; a.sample0 = sample0; a.S = S; a.R = R; a.T = T; a.MT = MT; a.sweeps = sweeps;
  launch_counted(s, BTF_K_CRITERIA, kern, dim3(S, (R + WAVE - 1) / WAVE), dim3(FOLD_PARTS * WAVE), 0, a);
  // the summary stage reads the device-resident W (S,R,K) and the uploaded V
  if (mean_out) summary_stage(s, a.W, st.V, S, R, MT, K, transform, q, nq, mean_out, q_out);
  int stat[2] = {0, INT_MAX};
  s.download(stat, a.status, 2);
  s.download(W_out, a.W, nW);
  s.download(Wmean_out, a.Wmean, nW);
  if (sampled) { s.download(R_out, a.Rout, nSR); s.download(accept_out, a.accept, nSR); }
  const int rc = s.finish();
  if (rc) return rc;
  if (stat[0]) {
    g_fold_fail_index = stat[1];
    return fail(nullptr, BTF_ENOTPD, name + ": the precision of (sample, row) index " + std::to_string(stat[1]) +
                                         " = sample * nrows_new + row is not positive definite (or sigma2 / V / w . v not finite); its outputs are nan");
  }
  return BTF_OK;
}

int btf_fold_in_cols(int device, int family, int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order,
                     const double* Ws, const double* noise, const double* lam2, const double* count, const double* ysum,
                     const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                     double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q, int nq,
                     double* mean_out, double* q_out) {
  const FoldCols f = {family, nsamples, ncols_new, nrows, ndepth, nembeds, tf_order, count, ysum, trials, draws, seed, sweeps, sample0,
                      stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Ws || !lam2 || (family == FOLDC_GAUSSIAN && !noise)) return fail(nullptr, BTF_EINVAL, "bad fold_in_cols arguments");
  FoldColsPenalty p;
  if (int rc = fold_cols_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY) || (family == FOLDC_GAUSSIAN && !(noise[s] > 0.0 && noise[s] < INFINITY)))
      return fail(nullptr, BTF_EINVAL, "fold_in_cols: nu2 and lam2 must be finite and positive");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  const double* dn = family == FOLDC_GAUSSIAN ? s.upload(noise, (size_t)nsamples) : nullptr;
  return fold_cols_run(s, dW, dn, 1, dl, 1, f, p);
}

// the same on the first nsamples collected states, read where they lie (no upload): W from the sample slots, nu2_s and
// lam2_s from the collected scalars
int btf_collect_fold_in_cols(btf_ctx* c, int family, int nsamples, int ncols_new, const double* count, const double* ysum,
                             const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                             double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                             int nq, double* mean_out, double* q_out) {
  if (!c) return fail(c, BTF_EINVAL, "bad fold_in_cols arguments");
  const FoldCols f = {family, nsamples, ncols_new, c->N, c->T, c->K, c->TF, count, ysum, trials, draws, seed, sweeps, sample0,
                      stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out};
  FoldColsPenalty p;
  if (int rc = fold_cols_check(c, f, p)) return rc;
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, "btf_collect_fold_in_cols needs an unsharded context");
  if (!has_collected(c, nsamples)) return no_collected(c, BTF_ESTATE, "btf_collect_fold_in_cols");
  HIPCHK(c, hipSetDevice(c->dev));
  Scratch s(c, c->stream);
  return fold_cols_run(s, c->smp_W, family == FOLDC_GAUSSIAN ? c->smp_s + HYP_NU2 : nullptr, (int)HYP_COUNT, c->smp_s + HYP_LAM2,
                       (int)HYP_COUNT, f, p);
}

// ---------------------------------------------------------------- folding new depth slices in (btf_fold_in_depth.h)
namespace {
struct FoldDepth {
  int family, S, N, M, T, H, K, tf;
  const double *count, *ysum, *trials, *draws;
  unsigned long long seed;
  int sweeps;
  long long sample0;
  double stability;
  double *V_out, *Vmean_out, *Tau2_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
  // the Negative-Binomial family (FOLDD_NEGBIN) alone: the rate, its strides (sample, column, row, depth), the replay weights
  const double* rate; long long rs[4]; const double* omega;
  size_t nrate;
};

// the new rows of the penalty on T + H points on the host: every row as (first depth counted from the first new one,
// tf + 2 coefficients from there on), and the D_n' D_n stencil per (t, d) as CSR over the new rows
struct FoldDepthPenalty {
  int nR = 0, L = 0;
  std::vector<double> rcoef, coef;
  std::vector<int> rcol0, ptr, row;
};

// fills the penalty of H new depths behind T kept ones (shared with slice_fold_depth_check); `name` opens the messages
int fold_depth_rows(btf_ctx* c, const char* name, int T, int H, int tf, FoldDepthPenalty& p) {
  const int TH = T + H, D1 = tf + 2;
  std::vector<double> Delta; std::vector<int> ptr0, row0; std::vector<double> coef0; int nD = 0;
  penalty_stencil(TH, tf, Delta, nD, ptr0, row0, coef0);
  p.L = std::min(T, tf + 1);
  p.rcol0.clear(); p.rcoef.clear();
  for (int r = 0; r < nD; ++r) {
    int lo, hi;
    penalty_row_window(&Delta[(size_t)r * TH], TH, lo, hi);
    if (hi < T) continue;                                        // a row on kept depths alone (or an empty one)
    if (hi - lo >= D1 || lo < T - p.L) return fail(c, BTF_EINVAL, std::string(name) + ": penalty row wider than the band");
    p.rcol0.push_back(lo - T);
    penalty_row_coefs(&Delta[(size_t)r * TH], lo, hi, D1, p.rcoef);
  }
  p.nR = (int)p.rcol0.size();
  if (p.nR < 1) return fail(c, BTF_EINVAL, std::string(name) + ": no penalty row touches the new depths");
  // D_n[r][t] = rcoef[r][t - rcol0[r]] inside the row's window
  auto dn = [&](int r, int t) {
    const int e = t - p.rcol0[r];
    return e >= 0 && e < D1 ? p.rcoef[(size_t)r * D1 + e] : 0.0;
  };
  p.ptr.assign((size_t)H * D1 + 1, 0); p.row.clear(); p.coef.clear();
  for (int t = 0; t < H; ++t)
    for (int d = 0; d < D1; ++d) {
      if (t + d < H)
        for (int r = 0; r < p.nR; ++r) {
          const double pr = dn(r, t) * dn(r, t + d);
          if (pr != 0.0) { p.row.push_back(r); p.coef.push_back(pr); }
        }
      p.ptr[(size_t)t * D1 + d + 1] = (int)p.row.size();
    }
  return BTF_OK;
}

// everything that can be refused without a device; fills the penalty
int fold_depth_check(btf_ctx* c, const FoldDepth& f, FoldDepthPenalty& p) {
  if (f.family < FOLDD_GAUSSIAN || f.family > FOLDD_BINOMIAL || f.S < 1 || f.M < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 ||
      f.T < 2 || f.H < 1 || !f.ysum || !f.V_out || !f.Vmean_out || !f.Tau2_out || f.sample0 < 0 || f.nq < 0 ||
      (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2 || !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad fold_in_depth arguments");
  if (f.family == FOLDD_GAUSSIAN && !f.count) return fail(c, BTF_EINVAL, "fold_in_depth: the Gaussian family needs count");
  if (f.family == FOLDD_BINOMIAL && (!f.trials || f.draws))
    return fail(c, BTF_EINVAL, "fold_in_depth: the Binomial family needs trials and takes no draws");
  if (int rc = fold_sweeps_check(c, "fold_in_depth", f.sweeps)) return rc;
  if (int rc = fold_sizes_check(c, "fold_in_depth", "ncols", "horizon", f.S, f.M, f.N, f.H, f.K, f.tf, f.sample0, f.mean_out != nullptr,
                                (double)f.sweeps * f.N * f.H))
    return rc;
  if ((double)f.T + f.H > (double)FOLDD_MAX_GRID)        // (the penalty on the extended grid is built dense on the host)
    return fail(c, BTF_EINVAL, "fold_in_depth: ndepth + horizon must stay within " + std::to_string(FOLDD_MAX_GRID));
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  // a band this wide is refused whatever the rows are (3 H + 2 bounds them from above only for tf <= 2: count them below)
  if (foldd_lds_bytes(f.H, f.K, f.tf, f.H, 1) > FOLDD_LDS_LIMIT)
    return fail(c, BTF_EINVAL, "fold_in_depth: the band of the new depths needs more than the LDS limit of " + std::to_string(FOLDD_LDS_LIMIT) + " bytes");
  if (int rc = fold_depth_rows(c, "fold_in_depth", f.T, f.H, f.tf, p)) return rc;
  if (int rc = fold_lds_check(c, "fold_in_depth", "the new depths", foldd_lds_bytes(f.H, f.K, f.tf, p.nR, p.L))) return rc;
  if (int rc = fold_cells_check(c, "fold_in_depth", f.family == FOLDD_GAUSSIAN ? f.count : f.trials, f.ysum, (size_t)f.M * f.H * f.N,
                                f.family == FOLDD_BINOMIAL))
    return rc;
  return fold_draws_check(c, "fold_in_depth", f.draws, (size_t)f.S * f.M, (size_t)f.H * f.K, 0, (size_t)p.nR, f.sweeps);
}

// the same for the Negative-Binomial family: the shared checks, the weight buffer in the LDS count, and a cell check of its own
int negbin_fold_depth_check(btf_ctx* c, FoldDepth& f, FoldDepthPenalty& p) {
  const std::string name = "negbin_fold_in_depth";
  if (f.family != FOLDD_NEGBIN || f.S < 1 || f.M < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 || f.T < 2 || f.H < 1 || !f.count ||
      !f.ysum || !f.rate || !f.V_out || !f.Vmean_out || !f.Tau2_out || f.sample0 < 0 || f.nq < 0 ||
      (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2 || !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad " + name + " arguments");
  if (f.draws && !f.omega) return fail(c, BTF_EINVAL, name + ": draws needs omega beside it (the chain also draws Polya-Gamma variates)");
  if (int rc = fold_sweeps_check(c, name, f.sweeps)) return rc;
  if (int rc = fold_sizes_check(c, name, "ncols", "horizon", f.S, f.M, f.N, f.H, f.K, f.tf, f.sample0, f.mean_out != nullptr,
                                (double)f.sweeps * f.N * f.H))
    return rc;
  if ((double)f.T + f.H > (double)FOLDD_MAX_GRID)
    return fail(c, BTF_EINVAL, name + ": ndepth + horizon must stay within " + std::to_string(FOLDD_MAX_GRID));
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  if (int rc = fold_lds_check(c, name, "the new depths and the weights of a depth", foldd_negbin_lds_bytes(f.H, f.K, f.tf, f.H, 1, f.N))) return rc;
  if (int rc = fold_depth_rows(c, name.c_str(), f.T, f.H, f.tf, p)) return rc;
  if (int rc = fold_lds_check(c, name, "the new depths and the weights of a depth", foldd_negbin_lds_bytes(f.H, f.K, f.tf, p.nR, p.L, f.N)))
    return rc;
  const int dims[4] = {f.S, f.M, f.N, f.H};
  if (int rc = negbin_fold_cells_check(c, name, f.count, f.ysum, (size_t)f.M * f.H * f.N, f.rate, f.rs, dims, f.omega,
                                       (size_t)f.S * f.M * f.sweeps * f.H * f.N, f.nrate))
    return rc;
  return fold_draws_check(c, name, f.draws, (size_t)f.S * f.M, (size_t)f.H * f.K, 0, (size_t)p.nR, f.sweeps);
}

// The launches on device states dW (S,N,K), the kept tails (tail of (s, j) at dVt[(s M + j) vstride], L x K) and per-sample
// scalars on the device (noise null: the Binomial family).  The scratch's context may be null (the stateless form).  The new
// V stays on the device between the chains and the summary.
int fold_depth_run(Scratch& s, const double* dW, const double* dVt, long long vstride, const double* dnoise, int nstride,
                   const double* dlam, int lstride, const FoldDepth& f, const FoldDepthPenalty& p) {
  btf_ctx* c = s.ctx();
  const int S = f.S, M = f.M, N = f.N, H = f.H, K = f.K, nR = p.nR;
  const bool negbin = f.family == FOLDD_NEGBIN;
  const std::string name = negbin ? "negbin_fold_in_depth" : "fold_in_depth";
  FoldDepthKernel kern = negbin ? fold_depth_negbin_fn(K) : fold_depth_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, name + (negbin ? ": nembeds must be 1..10" : ": nembeds must be 1..10 and family 0..1"));
  // the slice statistics lie [column][depth][row] as the kernel reads them; Binomial: kappa = successes - trials / 2
  const size_t ncell = (size_t)M * H * N;
  const double* cw = f.family == FOLDD_BINOMIAL ? f.trials : f.count;
  std::vector<double> hy(ncell);
  for (size_t e = 0; e < ncell; ++e)
    hy[e] = cw[e] > 0.0 ? (f.family == FOLDD_BINOMIAL ? f.ysum[e] - 0.5 * cw[e] : f.ysum[e]) : 0.0;
  const size_t nV = (size_t)S * M * H * K, nT = (size_t)S * M * nR;
  const size_t LD = 4 * (size_t)nR + (size_t)f.sweeps * ((size_t)H * K + 4 * (size_t)nR);
  const int stat0[2] = {0, INT_MAX};
  FoldDepthArgs a = {};
  a.W = dW; a.Vtail = dVt; a.vstride = vstride; a.noise = dnoise; a.lam2 = dlam; a.nstride = nstride; a.lstride = lstride;
  a.cnt = s.upload(cw, ncell); a.ysum = s.upload(hy.data(), ncell);
  if (f.draws) a.draws = s.upload(f.draws, (size_t)S * M * LD);
  if (negbin) {
    a.rate = s.upload(f.rate, f.nrate);
    a.rs_s = f.rs[0]; a.rs_c = f.rs[1]; a.rs_i = f.rs[2]; a.rs_t = f.rs[3];
    if (f.omega) a.omega = s.upload(f.omega, (size_t)S * M * f.sweeps * H * N);
  }
  a.rcol0 = s.upload(p.rcol0.data(), p.rcol0.size()); a.rcoef = s.upload(p.rcoef.data(), p.rcoef.size());
  a.st_ptr = s.upload(p.ptr.data(), p.ptr.size());
  // (a prior that couples nothing - H = 1 rows only - still has its diagonal entries: row and coef are never empty)
  a.st_row = s.upload(p.row.data(), p.row.size()); a.st_coef = s.upload(p.coef.data(), p.coef.size());
  a.V = s.alloc<double>(nV); a.Vmean = s.alloc<double>(nV); a.Tau2 = s.alloc<double>(nT);
  a.status = s.upload(stat0, 2);
  a.seed = f.seed; a.sample0 = f.sample0; a.lo = f.stability; a.hi = 1.0 / f.stability;
  a.S = S; a.M = M; a.N = N; a.H = H; a.L = p.L; a.tf = f.tf; a.nR = nR; a.sweeps = f.sweeps;
  const size_t lds = negbin ? foldd_negbin_lds_bytes(H, K, f.tf, nR, p.L, N) : foldd_lds_bytes(H, K, f.tf, nR, p.L);
  allow_lds(s, kern, lds);
  launch_counted(s, BTF_K_CRITERIA, kern, dim3((unsigned)((size_t)S * M)), dim3(WAVE), lds, a);
  // the summary stage reads the device-resident W (S,N,K) and the new V (S,M*H,K)
  if (f.mean_out) summary_stage(s, dW, a.V, S, N, M * H, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[2] = {0, INT_MAX};
  s.download(stat, a.status, 2);
  s.download(f.V_out, a.V, nV);
  s.download(f.Vmean_out, a.Vmean, nV);
  s.download(f.Tau2_out, a.Tau2, nT);
  const int rc = s.finish();
  if (rc) return rc;
  return stat[0] ? fold_pivot_fail(c, name, stat[1], "ncols", negbin ? "W / V / lam2" : "W / V / nu2 / lam2") : BTF_OK;
}
}  // namespace

// the Negative-Binomial family under a name of its own: count and ysum (M,H,N) are the observed replicates of a cell and their
// sum; the rate of (sample, column, row, new depth) lies at rate[s rs_sample + j rs_col + i rs_row + t rs_depth]
int btf_negbin_fold_in_depth(int device, int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds, int tf_order,
                             const double* Ws, const double* Vtail, const double* lam2, const double* count, const double* ysum,
                             const double* rate, long long rs_sample, long long rs_col, long long rs_row, long long rs_depth,
                             const double* omega, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                             double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                             int nq, double* mean_out, double* q_out) {
  FoldDepth f = {FOLDD_NEGBIN, nsamples, nrows, ncols, ndepth, horizon, nembeds, tf_order, count, ysum, nullptr, draws, seed, sweeps,
                 sample0, stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out, rate,
                 {rs_sample, rs_col, rs_row, rs_depth}, omega, 0};
  g_fold_fail_index = -1;
  if (!Ws || !Vtail || !lam2) return fail(nullptr, BTF_EINVAL, "bad negbin_fold_in_depth arguments");
  FoldDepthPenalty p;
  if (int rc = negbin_fold_depth_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY)) return fail(nullptr, BTF_EINVAL, "negbin_fold_in_depth: lam2 must be finite and positive");
  const size_t ntail = (size_t)nsamples * ncols * p.L * nembeds;
  if (!all_finite(Vtail, ntail)) return fail(nullptr, BTF_EINVAL, "negbin_fold_in_depth: the kept curves must be finite");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dVt = s.upload(Vtail, ntail);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  return fold_depth_run(s, dW, dVt, (long long)p.L * nembeds, nullptr, 1, dl, 1, f, p);
}

// LDS one chain's workgroup of the Negative-Binomial fold-ins needs: horizon 0: a new column (foldc_negbin_lds_bytes), else
// `horizon` new depths (foldd_negbin_lds_bytes); -1 on sizes no call takes
long long btf_negbin_fold_lds_bytes(int nrows, int ndepth, int horizon, int nembeds, int tf_order) {
  if (nrows < 1 || ndepth < 2 || horizon < 0 || nembeds < 1 || nembeds > MAX_K || tf_order < 0 || (double)ndepth + horizon > (double)FOLDD_MAX_GRID)
    return -1;
  if (horizon == 0) {
    FoldColsPenalty p;
    penalty_stencil(ndepth, tf_order, p.Delta, p.nD, p.ptr, p.row, p.coef);
    return (long long)foldc_negbin_lds_bytes(ndepth, nembeds, tf_order, p.nD, nrows);
  }
  FoldDepthPenalty p;
  if (fold_depth_rows(nullptr, "negbin_fold_in_depth", ndepth, horizon, tf_order, p)) return -1;
  return (long long)foldd_negbin_lds_bytes(horizon, nembeds, tf_order, p.nR, p.L, nrows);
}

int btf_fold_in_depth(int device, int family, int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds,
                      int tf_order, const double* Ws, const double* Vtail, const double* noise, const double* lam2,
                      const double* count, const double* ysum, const double* trials, const double* draws, unsigned long long seed,
                      int sweeps, long long sample0, double stability, double* V_out, double* Vmean_out, double* Tau2_out,
                      int transform, const double* q, int nq, double* mean_out, double* q_out) {
  const FoldDepth f = {family, nsamples, nrows, ncols, ndepth, horizon, nembeds, tf_order, count, ysum, trials, draws, seed, sweeps,
                       sample0, stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Ws || !Vtail || !lam2 || (family == FOLDD_GAUSSIAN && !noise)) return fail(nullptr, BTF_EINVAL, "bad fold_in_depth arguments");
  FoldDepthPenalty p;
  if (int rc = fold_depth_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY) || (family == FOLDD_GAUSSIAN && !(noise[s] > 0.0 && noise[s] < INFINITY)))
      return fail(nullptr, BTF_EINVAL, "fold_in_depth: nu2 and lam2 must be finite and positive");
  const size_t ntail = (size_t)nsamples * ncols * p.L * nembeds;
  if (!all_finite(Vtail, ntail)) return fail(nullptr, BTF_EINVAL, "fold_in_depth: the kept curves must be finite");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dVt = s.upload(Vtail, ntail);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  const double* dn = family == FOLDD_GAUSSIAN ? s.upload(noise, (size_t)nsamples) : nullptr;
  return fold_depth_run(s, dW, dVt, (long long)p.L * nembeds, dn, 1, dl, 1, f, p);
}

// the same on the first nsamples collected states, read where they lie (no upload): W and the last depths of V from the
// sample slots, nu2_s and lam2_s from the collected scalars
int btf_collect_fold_in_depth(btf_ctx* c, int family, int nsamples, int horizon, const double* count, const double* ysum,
                              const double* trials, const double* draws, unsigned long long seed, int sweeps, long long sample0,
                              double stability, double* V_out, double* Vmean_out, double* Tau2_out, int transform, const double* q,
                              int nq, double* mean_out, double* q_out) {
  if (!c) return fail(c, BTF_EINVAL, "bad fold_in_depth arguments");
  const FoldDepth f = {family, nsamples, c->N, c->M, c->T, horizon, c->K, c->TF, count, ysum, trials, draws, seed, sweeps, sample0,
                       stability, V_out, Vmean_out, Tau2_out, transform, q, nq, mean_out, q_out};
  FoldDepthPenalty p;
  if (int rc = fold_depth_check(c, f, p)) return rc;
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, "btf_collect_fold_in_depth needs an unsharded context");
  if (!has_collected(c, nsamples)) return no_collected(c, BTF_ESTATE, "btf_collect_fold_in_depth");
  HIPCHK(c, hipSetDevice(c->dev));
  Scratch s(c, c->stream);
  return fold_depth_run(s, c->smp_W, c->smp_V + (size_t)(c->T - p.L) * c->K, (long long)c->T * c->K,
                        family == FOLDD_GAUSSIAN ? c->smp_s + HYP_NU2 : nullptr, (int)HYP_COUNT, c->smp_s + HYP_LAM2, (int)HYP_COUNT, f, p);
}

// ---------------------------------------------------------------- convergence diagnostics (btf_diag.h)
// ---------------------------------------------------------------- folding new columns into a slice-sampled fit (btf_slice_fold_cols.h)
namespace {
struct SliceFoldCols {
  int family; double param;
  int S, C, N, T, K, tf;
  const double *start, *S1, *cnt, *L, *fa, *fb;
  const double* cons; int J;
  const double *tau2, *draws;
  unsigned long long seed;
  int sweeps, max_rounds;
  long long sample0;
  double stability;
  double *V_out, *Vstart_out, *Tau2_out; int *rounds_out, *unf_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
};

// everything that can be refused without a device; fills the penalty (its rows as fold_cols_check does)
int slice_fold_cols_check(btf_ctx* c, const SliceFoldCols& f, FoldColsPenalty& p) {
  if (f.family < 0 || f.family >= ESS_FAM_COUNT || f.S < 1 || f.C < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 || f.T < 2 ||
      !f.S1 || !f.cnt || !f.fa || !f.fb || !f.V_out || !f.Tau2_out || !f.rounds_out || !f.unf_out || f.sample0 < 0 || f.nq < 0 ||
      (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2 || f.J < 0 || (f.J > 0 && !f.cons) ||
      !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad slice_fold_cols arguments");
  if (int rc = slice_fold_sweeps_check(c, "slice_fold_cols", f.sweeps, f.max_rounds)) return rc;
  if (f.family == ESS_FAM_GAMMA_GRID && !f.L) return fail(c, BTF_EINVAL, "slice_fold_cols: the gamma-grid family needs logsum");
  if (int rc = fold_sizes_check(c, "slice_fold_cols", "ncols_new", "ndepth", f.S, f.C, f.N, f.T, f.K, f.tf, f.sample0, f.mean_out != nullptr, 0.0))
    return rc;
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  penalty_stencil(f.T, f.tf, p.Delta, p.nD, p.ptr, p.row, p.coef);
  if ((double)f.T * f.K + 1.0 + f.max_rounds + 4.0 * p.nD >= 2147483647.0)
    return fail(c, BTF_EINVAL, "slice_fold_cols: the record of a sweep must stay below 2^31 numbers");
  if (int rc = fold_lds_check(c, "slice_fold_cols", "a column", scols_lds_bytes(f.T, f.K, f.tf, p.nD))) return rc;
  if (int rc = fold_cols_rows(c, "slice_fold_cols", f.T, f.tf, p)) return rc;
  if (int rc = slice_fold_cells_check(c, "slice_fold_cols", f.cnt, f.S1, f.L, f.fa, f.fb, (size_t)f.C * f.N * f.T)) return rc;
  if (!all_finite(f.cons, (size_t)f.J * (f.T + 1))) return fail(c, BTF_EINVAL, "slice_fold_cols: constraints must be finite");
  if (f.start && !all_finite(f.start, (size_t)f.S * f.C * f.T * f.K)) return fail(c, BTF_EINVAL, "slice_fold_cols: start must be finite");
  if (f.tau2)
    for (size_t e = 0; e < (size_t)f.S * f.C * p.nD; ++e)
      if (!(f.tau2[e] > 0.0 && f.tau2[e] < INFINITY)) return fail(c, BTF_EINVAL, "slice_fold_cols: tau2 must be finite and positive");
  return fold_draws_check(c, "slice_fold_cols", f.draws, (size_t)f.S * f.C, (size_t)f.T * f.K, 1 + (size_t)f.max_rounds, (size_t)p.nD, f.sweeps);
}

// The launches on device states dW (S,N,K), dV (S,M,T,K; read when the call has no start) and per-sample lam2 on the
// device; dgg: the gamma-grid table on the device (family 5).  The scratch's context may be null (the stateless form).
// The new V stays on the device between the chains and the summary.
int slice_fold_cols_run(Scratch& s, const double* dW, const double* dV, int M, const double* dlam, int lstride, const GgComp* dgg,
                        int G, double lsp, const SliceFoldCols& f, const FoldColsPenalty& p) {
  btf_ctx* c = s.ctx();
  const int S = f.S, C = f.C, N = f.N, T = f.T, K = f.K, nD = p.nD;
  SliceFoldColsKernel kern = slice_fold_cols_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, "slice_fold_cols: nembeds must be 1..10 and family 0..5");
  // column statistics and the fit in the kernel's [column][depth][row] layout; per column the rows with any observed or
  // fitted cell, ascending
  const size_t ncell = (size_t)C * N * T;
  std::vector<double> h1(ncell), hc(ncell), hl(f.L ? ncell : 0), ha(ncell), hb(ncell);
  std::vector<int> rptr(1, 0), ridx;
  for (int j = 0; j < C; ++j) {
    for (int i = 0; i < N; ++i) {
      bool any = false;
      for (int t = 0; t < T; ++t) {
        const size_t src = ((size_t)j * N + i) * T + t, dst = ((size_t)j * T + t) * N + i;
        const double cv = f.cnt[src], av = f.fa[src];
        hc[dst] = cv; h1[dst] = cv > 0.0 ? f.S1[src] : 0.0;
        if (f.L) hl[dst] = cv > 0.0 ? f.L[src] : 0.0;
        ha[dst] = av; hb[dst] = av > 0.0 ? f.fb[src] : 0.0;
        any = any || cv > 0.0 || av > 0.0;
      }
      if (any) ridx.push_back(i);
    }
    rptr.push_back((int)ridx.size());
  }
  if (ridx.empty()) ridx.push_back(0);                       // (never read)
  // Constraints_A by its non-zeros (CSR over the constraints), the bounds beside it
  std::vector<int> cptr(1, 0), cidx;
  std::vector<double> cval, cc;
  for (int q = 0; q < f.J; ++q) {
    for (int t = 0; t < T; ++t)
      if (f.cons[(size_t)q * (T + 1) + t] != 0.0) { cidx.push_back(t); cval.push_back(f.cons[(size_t)q * (T + 1) + t]); }
    cptr.push_back((int)cidx.size());
    cc.push_back(f.cons[(size_t)q * (T + 1) + T]);
  }
  if (cidx.empty()) { cidx.push_back(0); cval.push_back(0.0); }
  if (cc.empty()) cc.push_back(0.0);
  const size_t n = (size_t)T * K, nV = (size_t)S * C * n, nT = (size_t)S * C * nD, nch = (size_t)S * C;
  const size_t LD = 4 * (size_t)nD + (size_t)f.sweeps * (n + 1 + (size_t)f.max_rounds + 4 * (size_t)nD);
  const int stat0[4] = {0, INT_MAX, 0, INT_MAX};
  SliceFoldColsArgs a = {};
  a.W = dW; a.lam2 = dlam; a.lstride = lstride;
  a.S1 = s.upload(h1.data(), ncell); a.cnt = s.upload(hc.data(), ncell);
  if (f.L) a.L = s.upload(hl.data(), ncell);
  a.fa = s.upload(ha.data(), ncell); a.fb = s.upload(hb.data(), ncell);
  a.rptr = s.upload(rptr.data(), rptr.size()); a.ridx = s.upload(ridx.data(), ridx.size());
  a.cs_ptr = s.upload(cptr.data(), cptr.size()); a.cs_idx = s.upload(cidx.data(), cidx.size());
  a.cs_val = s.upload(cval.data(), cval.size()); a.Cc = s.upload(cc.data(), cc.size()); a.J = f.J;
  if (f.tau2) a.tau2 = s.upload(f.tau2, nT);
  if (f.draws) a.draws = s.upload(f.draws, nch * LD);
  a.rcol0 = s.upload(p.rcol0.data(), p.rcol0.size()); a.rcoef = s.upload(p.rcoef.data(), p.rcoef.size());
  a.st_ptr = s.upload(p.ptr.data(), p.ptr.size());
  a.st_row = s.upload(p.row.data(), p.row.size()); a.st_coef = s.upload(p.coef.data(), p.coef.size());
  a.gg = dgg; a.G = G; a.lsp = lsp; a.fam = f.family; a.par = f.param;
  double* dmean = nullptr;
  if (f.start) { a.start = s.upload(f.start, nV); a.st_s = (long long)C * (long long)n; a.st_c = (long long)n; }
  else {
    dmean = s.alloc<double>((size_t)S * n);
    const int nb = (int)(((size_t)S * n + 255) / 256);
    launch_counted(s, BTF_K_CRITERIA, slice_fold_cols_mean_fn(), dim3(nb), dim3(256), 0, dV, S, M, (int)n, dmean);
    a.start = dmean; a.st_s = (long long)n; a.st_c = 0;
  }
  a.V = s.alloc<double>(nV); a.Tau2 = s.alloc<double>(nT);
  a.rounds = s.alloc<int>(nch); a.unfinished = s.alloc<int>(nch); a.status = s.upload(stat0, 4);
  a.seed = f.seed; a.sample0 = f.sample0; a.lo = f.stability; a.hi = 1.0 / f.stability;
  a.S = S; a.C = C; a.N = N; a.T = T; a.tf = f.tf; a.nD = nD; a.sweeps = f.sweeps; a.max_rounds = f.max_rounds;
  const size_t lds = scols_dyn_lds_bytes(T, K, f.tf, nD);
  allow_lds(s, kern, lds);
  launch_counted(s, BTF_K_CRITERIA, kern, dim3((unsigned)nch), dim3(WAVE), lds, a);
  // the summary stage reads the device-resident W (S,N,K) and the new V (S,C*T,K)
  if (f.mean_out) summary_stage(s, dW, a.V, S, N, C * T, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[4] = {0, INT_MAX, 0, INT_MAX};
  std::vector<double> hmean(dmean ? (size_t)S * n : 0);
  s.download(stat, (const int*)a.status, 4);
  s.download(f.V_out, (const double*)a.V, nV);
  s.download(f.Tau2_out, (const double*)a.Tau2, nT);
  s.download(f.rounds_out, (const int*)a.rounds, nch);
  s.download(f.unf_out, (const int*)a.unfinished, nch);
  if (dmean && f.Vstart_out) s.download(hmean.data(), (const double*)dmean, hmean.size());
  const int rc = s.finish();
  if (rc) return rc;
  if (f.Vstart_out) {
    if (f.start) std::copy(f.start, f.start + nV, f.Vstart_out);
    else
      for (size_t e = 0; e < nV; ++e) f.Vstart_out[e] = hmean[(e / ((size_t)C * n)) * n + e % n];
  }
  if (stat[0]) return slice_fold_start_fail(c, "slice_fold_cols", stat[1], C, "ncols_new");
  return stat[2] ? fold_pivot_fail(c, "slice_fold_cols", stat[3], "ncols_new", "W / lam2 / the fit") : BTF_OK;
}
}  // namespace

int btf_slice_fold_cols(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                        int nsamples, int ncols_new, int nrows, int ndepth, int nembeds, int tf_order, const double* Ws,
                        const double* Vs, int nfit_cols, const double* lam2, const double* start, const double* S1,
                        const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                        const double* constraints, int ncons, const double* tau2, const double* draws, unsigned long long seed,
                        int sweeps, int max_rounds, long long sample0, double stability, double* V_out, double* Vstart_out,
                        double* Tau2_out, int* rounds_out, int* unfinished_out, int transform, const double* q, int nq,
                        double* mean_out, double* q_out) {
  const SliceFoldCols f = {family, param, nsamples, ncols_new, nrows, ndepth, nembeds, tf_order, start, S1, cnt, logsum, fit_a, fit_b,
                           constraints, ncons, tau2, draws, seed, sweeps, max_rounds, sample0, stability, V_out, Vstart_out, Tau2_out,
                           rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Ws || !lam2 || (!start && (!Vs || nfit_cols < 1))) return fail(nullptr, BTF_EINVAL, "bad slice_fold_cols arguments");
  FoldColsPenalty p;
  if (int rc = slice_fold_cols_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY)) return fail(nullptr, BTF_EINVAL, "slice_fold_cols: lam2 must be finite and positive");
  if ((family == ESS_FAM_GAUSSIAN || family == ESS_FAM_NEGBIN_LOGIT) && !(param > 0.0 && param < INFINITY))
    return fail(nullptr, BTF_EINVAL, "slice_fold_cols: the parameter must be positive");
  std::vector<GgComp> tab;
  double lsp = 0.0;
  if (family == ESS_FAM_GAMMA_GRID && gg_comp_table(shape, scale, prob, G, tab, lsp) != 0)
    return fail(nullptr, BTF_EINVAL, "slice_fold_cols: the gamma grid has 1..128 components with finite shape > 0, scale > 0, weight >= 0, not all zero");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dV = start ? nullptr : s.upload(Vs, (size_t)nsamples * nfit_cols * ndepth * nembeds);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  const GgComp* dgg = tab.empty() ? nullptr : s.upload(tab.data(), tab.size());
  return slice_fold_cols_run(s, dW, dV, nfit_cols, dl, 1, dgg, (int)tab.size(), lsp, f, p);
}

// the same on the first nsamples collected states, read where they lie (no upload): W and V from the sample slots,
// lam2_s from the collected scalars, the likelihood's parameter or table from the context
int btf_collect_slice_fold_cols(btf_ctx* c, int family, int nsamples, int ncols_new, const double* start, const double* S1,
                                const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                                const double* constraints, int ncons, const double* tau2, const double* draws,
                                unsigned long long seed, int sweeps, int max_rounds, long long sample0, double stability,
                                double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out, int* unfinished_out,
                                int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (!c || family < 0 || family >= ESS_FAM_COUNT) return fail(c, BTF_EINVAL, "bad slice_fold_cols arguments");
  const SliceFoldCols f = {family, c->lik_par[family], nsamples, ncols_new, c->N, c->T, c->K, c->TF, start, S1, cnt, logsum, fit_a,
                           fit_b, constraints, ncons, tau2, draws, seed, sweeps, max_rounds, sample0, stability, V_out, Vstart_out,
                           Tau2_out, rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  FoldColsPenalty p;
  if (int rc = slice_fold_cols_check(c, f, p)) return rc;
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, "btf_collect_slice_fold_cols needs an unsharded context");
  if (family == ESS_FAM_GAMMA_GRID && !c->gg_tab)
    return fail(c, BTF_ESTATE, "btf_collect_slice_fold_cols: the gamma-grid family needs its table (btf_set_likelihood_table)");
  Scratch s(c, c->stream); States st;
  if (int rc = resolve_pair(s, 0, "btf_collect_slice_fold_cols", BTF_ESTATE, nsamples, 0, c->M * c->T, c->K, nullptr, nullptr, st)) return rc;
  return slice_fold_cols_run(s, st.W, st.V, c->M, c->smp_s + HYP_LAM2, (int)HYP_COUNT, c->gg_tab, c->gg_G, c->gg_lsp, f, p);
}

// ---------------------------------------------------------------- folding new depth slices into a slice-sampled fit (btf_slice_fold_depth.h)
namespace {
struct SliceFoldDepth {
  int family; double param;
  int S, N, M, T, H, K, tf;
  const double *start, *S1, *cnt, *L, *fa, *fb;
  const double* cons; int J, B;          // the reduced constraints (J, B + H + 1): B trailing kept depths, the H new ones, the bound
  const double *tau2, *draws;
  unsigned long long seed;
  int sweeps, max_rounds;
  long long sample0;
  double stability;
  double *V_out, *Vstart_out, *Tau2_out; int *rounds_out, *unf_out;
  int transform;
  const double* q; int nq;
  double *mean_out, *q_out;
};

// kept depths the chain reads: the prior's min(T, tf + 1), or the B the constraints reach back
int slice_fold_depth_tail(const SliceFoldDepth& f) { return std::max(std::min(f.T, f.tf + 1), f.B); }

// everything that can be refused without a device; fills the penalty
int slice_fold_depth_check(btf_ctx* c, const SliceFoldDepth& f, FoldDepthPenalty& p) {
  if (f.family < 0 || f.family >= ESS_FAM_COUNT || f.S < 1 || f.M < 1 || f.N < 1 || f.K < 1 || f.K > MAX_K || f.tf < 0 || f.T < 2 ||
      f.H < 1 || !f.S1 || !f.cnt || !f.fa || !f.fb || !f.V_out || !f.Tau2_out || !f.rounds_out || !f.unf_out || f.sample0 < 0 ||
      f.nq < 0 || (f.nq > 0 && (!f.q || !f.q_out || !f.mean_out)) || f.transform < 0 || f.transform > 2 || f.J < 0 ||
      (f.J > 0 && !f.cons) || f.B < 0 || f.B > f.T || (f.J == 0 && f.B != 0) || !(f.stability > 0.0 && f.stability <= 1.0))
    return fail(c, BTF_EINVAL, "bad slice_fold_depth arguments");
  if (int rc = slice_fold_sweeps_check(c, "slice_fold_depth", f.sweeps, f.max_rounds)) return rc;
  if (f.family == ESS_FAM_GAMMA_GRID && !f.L) return fail(c, BTF_EINVAL, "slice_fold_depth: the gamma-grid family needs logsum");
  if (int rc = fold_sizes_check(c, "slice_fold_depth", "ncols", "horizon", f.S, f.M, f.N, f.H, f.K, f.tf, f.sample0, f.mean_out != nullptr, 0.0))
    return rc;
  if ((double)f.T + f.H > (double)FOLDD_MAX_GRID)        // (the penalty on the extended grid is built dense on the host)
    return fail(c, BTF_EINVAL, "slice_fold_depth: ndepth + horizon must stay within " + std::to_string(FOLDD_MAX_GRID));
  if (int rc = check_percentiles(c, f.q, f.nq)) return rc;
  // a band this wide is refused whatever the rows are (count them below)
  if (sdepth_lds_bytes(f.H, f.K, f.tf, f.H, 1) > SDEPTH_LDS_LIMIT)
    return fail(c, BTF_EINVAL, "slice_fold_depth: the band of the new depths needs more than the LDS limit of " + std::to_string(SDEPTH_LDS_LIMIT) + " bytes");
  if (int rc = fold_depth_rows(c, "slice_fold_depth", f.T, f.H, f.tf, p)) return rc;
  if ((double)f.H * f.K + 1.0 + f.max_rounds + 4.0 * p.nR >= 2147483647.0)
    return fail(c, BTF_EINVAL, "slice_fold_depth: the record of a sweep must stay below 2^31 numbers");
  if (int rc = fold_lds_check(c, "slice_fold_depth", "the new depths", sdepth_lds_bytes(f.H, f.K, f.tf, p.nR, slice_fold_depth_tail(f)))) return rc;
  if (int rc = slice_fold_cells_check(c, "slice_fold_depth", f.cnt, f.S1, f.L, f.fa, f.fb, (size_t)f.M * f.N * f.H)) return rc;
  if (!all_finite(f.cons, (size_t)f.J * (f.B + f.H + 1))) return fail(c, BTF_EINVAL, "slice_fold_depth: constraints must be finite");
  const size_t n = (size_t)f.H * f.K;
  if (f.start && !all_finite(f.start, (size_t)f.S * f.M * n)) return fail(c, BTF_EINVAL, "slice_fold_depth: start must be finite");
  if (f.tau2)
    for (size_t e = 0; e < (size_t)f.S * f.M * p.nR; ++e)
      if (!(f.tau2[e] > 0.0 && f.tau2[e] < INFINITY)) return fail(c, BTF_EINVAL, "slice_fold_depth: tau2 must be finite and positive");
  return fold_draws_check(c, "slice_fold_depth", f.draws, (size_t)f.S * f.M, n, 1 + (size_t)f.max_rounds, (size_t)p.nR, f.sweeps);
}

// The launch on device states dW (S,N,K), the kept tails (tail of (s, j) at dVt[(s M + j) vstride], Lt x K) and per-sample
// lam2 on the device; dgg: the gamma-grid table on the device (family 5).  The scratch's context may be null (the
// stateless form).  The new V stays on the device between the chains and the summary.
int slice_fold_depth_run(Scratch& s, const double* dW, const double* dVt, long long vstride, const double* dlam, int lstride,
                         const GgComp* dgg, int G, double lsp, const SliceFoldDepth& f, const FoldDepthPenalty& p) {
  btf_ctx* c = s.ctx();
  const int S = f.S, M = f.M, N = f.N, H = f.H, K = f.K, nR = p.nR, Lt = slice_fold_depth_tail(f), BH = f.B + H;
  SliceFoldDepthKernel kern = slice_fold_depth_fn(K, f.family);
  if (!kern) return fail(c, BTF_EINVAL, "slice_fold_depth: nembeds must be 1..10 and family 0..5");
  // slice statistics and the fit, (M,N,H) as given, in the kernel's [column][depth][row] layout; per fitted column the rows
  // with any observed or fitted new cell, ascending
  const size_t ncell = (size_t)M * N * H;
  std::vector<double> h1(ncell), hc(ncell), hl(f.L ? ncell : 0), ha(ncell), hb(ncell);
  std::vector<int> rptr(1, 0), ridx;
  for (int j = 0; j < M; ++j) {
    for (int i = 0; i < N; ++i) {
      bool any = false;
      for (int h = 0; h < H; ++h) {
        const size_t src = ((size_t)j * N + i) * H + h, dst = ((size_t)j * H + h) * N + i;
        const double cv = f.cnt[src], av = f.fa[src];
        hc[dst] = cv; h1[dst] = cv > 0.0 ? f.S1[src] : 0.0;
        if (f.L) hl[dst] = cv > 0.0 ? f.L[src] : 0.0;
        ha[dst] = av; hb[dst] = av > 0.0 ? f.fb[src] : 0.0;
        any = any || cv > 0.0 || av > 0.0;
      }
      if (any) ridx.push_back(i);
    }
    rptr.push_back((int)ridx.size());
  }
  if (ridx.empty()) ridx.push_back(0);                       // (never read)
  // the reduced constraints by their non-zeros (CSR over the constraints, local depths ascending), the bounds beside them
  std::vector<int> cptr(1, 0), cidx;
  std::vector<double> cval, cc;
  for (int q = 0; q < f.J; ++q) {
    for (int l = 0; l < BH; ++l)
      if (f.cons[(size_t)q * (BH + 1) + l] != 0.0) { cidx.push_back(l); cval.push_back(f.cons[(size_t)q * (BH + 1) + l]); }
    cptr.push_back((int)cidx.size());
    cc.push_back(f.cons[(size_t)q * (BH + 1) + BH]);
  }
  if (cidx.empty()) { cidx.push_back(0); cval.push_back(0.0); }
  if (cc.empty()) cc.push_back(0.0);
  const size_t n = (size_t)H * K, nV = (size_t)S * M * n, nT = (size_t)S * M * nR, nch = (size_t)S * M;
  const size_t LD = 4 * (size_t)nR + (size_t)f.sweeps * (n + 1 + (size_t)f.max_rounds + 4 * (size_t)nR);
  const int stat0[4] = {0, INT_MAX, 0, INT_MAX};
  SliceFoldDepthArgs a = {};
  a.W = dW; a.Vtail = dVt; a.vstride = vstride; a.lam2 = dlam; a.lstride = lstride;
  if (f.start) a.start = s.upload(f.start, nV);
  a.S1 = s.upload(h1.data(), ncell); a.cnt = s.upload(hc.data(), ncell);
  if (f.L) a.L = s.upload(hl.data(), ncell);
  a.fa = s.upload(ha.data(), ncell); a.fb = s.upload(hb.data(), ncell);
  a.rptr = s.upload(rptr.data(), rptr.size()); a.ridx = s.upload(ridx.data(), ridx.size());
  a.cs_ptr = s.upload(cptr.data(), cptr.size()); a.cs_idx = s.upload(cidx.data(), cidx.size());
  a.cs_val = s.upload(cval.data(), cval.size()); a.Cc = s.upload(cc.data(), cc.size()); a.J = f.J;
  if (f.tau2) a.tau2 = s.upload(f.tau2, nT);
  if (f.draws) a.draws = s.upload(f.draws, nch * LD);
  a.rcol0 = s.upload(p.rcol0.data(), p.rcol0.size()); a.rcoef = s.upload(p.rcoef.data(), p.rcoef.size());
  a.st_ptr = s.upload(p.ptr.data(), p.ptr.size());
  a.st_row = s.upload(p.row.data(), p.row.size()); a.st_coef = s.upload(p.coef.data(), p.coef.size());
  a.gg = dgg; a.G = G; a.lsp = lsp; a.fam = f.family; a.par = f.param;
  a.V = s.alloc<double>(nV); a.Vstart = s.alloc<double>(nV); a.Tau2 = s.alloc<double>(nT);
  a.rounds = s.alloc<int>(nch); a.unfinished = s.alloc<int>(nch); a.status = s.upload(stat0, 4);
  a.seed = f.seed; a.sample0 = f.sample0; a.lo = f.stability; a.hi = 1.0 / f.stability;
  a.S = S; a.M = M; a.N = N; a.H = H; a.Lt = Lt; a.B = f.B; a.tf = f.tf; a.nR = nR; a.sweeps = f.sweeps; a.max_rounds = f.max_rounds;
  const size_t lds = sdepth_dyn_lds_bytes(H, K, f.tf, nR, Lt);
  allow_lds(s, kern, lds);
  launch_counted(s, BTF_K_CRITERIA, kern, dim3((unsigned)nch), dim3(WAVE), lds, a);
  // the summary stage reads the device-resident W (S,N,K) and the new V (S,M*H,K)
  if (f.mean_out) summary_stage(s, dW, a.V, S, N, M * H, K, f.transform, f.q, f.nq, f.mean_out, f.q_out);
  int stat[4] = {0, INT_MAX, 0, INT_MAX};
  s.download(stat, (const int*)a.status, 4);
  s.download(f.V_out, (const double*)a.V, nV);
  if (f.Vstart_out) s.download(f.Vstart_out, (const double*)a.Vstart, nV);
  s.download(f.Tau2_out, (const double*)a.Tau2, nT);
  s.download(f.rounds_out, (const int*)a.rounds, nch);
  s.download(f.unf_out, (const int*)a.unfinished, nch);
  const int rc = s.finish();
  if (rc) return rc;
  if (stat[0]) return slice_fold_start_fail(c, "slice_fold_depth", stat[1], M, "ncols");
  return stat[2] ? fold_pivot_fail(c, "slice_fold_depth", stat[3], "ncols", "W / V / lam2 / the fit") : BTF_OK;
}
}  // namespace

int btf_slice_fold_depth(int device, int family, double param, const double* shape, const double* scale, const double* prob, int G,
                         int nsamples, int nrows, int ncols, int ndepth, int horizon, int nembeds, int tf_order, const double* Ws,
                         const double* Vtail, const double* lam2, const double* start, const double* S1, const double* cnt,
                         const double* logsum, const double* fit_a, const double* fit_b, const double* constraints, int ncons,
                         int nback, const double* tau2, const double* draws, unsigned long long seed, int sweeps, int max_rounds,
                         long long sample0, double stability, double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out,
                         int* unfinished_out, int transform, const double* q, int nq, double* mean_out, double* q_out) {
  const SliceFoldDepth f = {family, param, nsamples, nrows, ncols, ndepth, horizon, nembeds, tf_order, start, S1, cnt, logsum, fit_a,
                            fit_b, constraints, ncons, nback, tau2, draws, seed, sweeps, max_rounds, sample0, stability, V_out,
                            Vstart_out, Tau2_out, rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  g_fold_fail_index = -1;
  if (!Ws || !Vtail || !lam2) return fail(nullptr, BTF_EINVAL, "bad slice_fold_depth arguments");
  FoldDepthPenalty p;
  if (int rc = slice_fold_depth_check(nullptr, f, p)) return rc;
  for (int s = 0; s < nsamples; ++s)
    if (!(lam2[s] > 0.0 && lam2[s] < INFINITY)) return fail(nullptr, BTF_EINVAL, "slice_fold_depth: lam2 must be finite and positive");
  if ((family == ESS_FAM_GAUSSIAN || family == ESS_FAM_NEGBIN_LOGIT) && !(param > 0.0 && param < INFINITY))
    return fail(nullptr, BTF_EINVAL, "slice_fold_depth: the parameter must be positive");
  const int Lt = slice_fold_depth_tail(f);
  const size_t ntail = (size_t)nsamples * ncols * Lt * nembeds;
  if (!all_finite(Vtail, ntail)) return fail(nullptr, BTF_EINVAL, "slice_fold_depth: the kept curves must be finite");
  std::vector<GgComp> tab;
  double lsp = 0.0;
  if (family == ESS_FAM_GAMMA_GRID && gg_comp_table(shape, scale, prob, G, tab, lsp) != 0)
    return fail(nullptr, BTF_EINVAL, "slice_fold_depth: the gamma grid has 1..128 components with finite shape > 0, scale > 0, weight >= 0, not all zero");
  if (int rc = use_device(device)) return rc;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(Ws, (size_t)nsamples * nrows * nembeds);
  const double* dVt = s.upload(Vtail, ntail);
  const double* dl = s.upload(lam2, (size_t)nsamples);
  const GgComp* dgg = tab.empty() ? nullptr : s.upload(tab.data(), tab.size());
  return slice_fold_depth_run(s, dW, dVt, (long long)Lt * nembeds, dl, 1, dgg, (int)tab.size(), lsp, f, p);
}

// the same on the first nsamples collected states, read where they lie (no upload): W and the last depths of V from the
// sample slots, lam2_s from the collected scalars, the likelihood's parameter or table from the context
int btf_collect_slice_fold_depth(btf_ctx* c, int family, int nsamples, int horizon, const double* start, const double* S1,
                                 const double* cnt, const double* logsum, const double* fit_a, const double* fit_b,
                                 const double* constraints, int ncons, int nback, const double* tau2, const double* draws,
                                 unsigned long long seed, int sweeps, int max_rounds, long long sample0, double stability,
                                 double* V_out, double* Vstart_out, double* Tau2_out, int* rounds_out, int* unfinished_out,
                                 int transform, const double* q, int nq, double* mean_out, double* q_out) {
  if (!c || family < 0 || family >= ESS_FAM_COUNT) return fail(c, BTF_EINVAL, "bad slice_fold_depth arguments");
  const SliceFoldDepth f = {family, c->lik_par[family], nsamples, c->N, c->M, c->T, horizon, c->K, c->TF, start, S1, cnt, logsum,
                            fit_a, fit_b, constraints, ncons, nback, tau2, draws, seed, sweeps, max_rounds, sample0, stability, V_out,
                            Vstart_out, Tau2_out, rounds_out, unfinished_out, transform, q, nq, mean_out, q_out};
  FoldDepthPenalty p;
  if (int rc = slice_fold_depth_check(c, f, p)) return rc;
  if (c->nl != c->N || c->ml != c->M) return fail(c, BTF_ESTATE, "btf_collect_slice_fold_depth needs an unsharded context");
  if (family == ESS_FAM_GAMMA_GRID && !c->gg_tab)
    return fail(c, BTF_ESTATE, "btf_collect_slice_fold_depth: the gamma-grid family needs its table (btf_set_likelihood_table)");
  if (!has_collected(c, nsamples)) return no_collected(c, BTF_ESTATE, "btf_collect_slice_fold_depth");
  HIPCHK(c, hipSetDevice(c->dev));
  Scratch s(c, c->stream);
  const int Lt = slice_fold_depth_tail(f);
  return slice_fold_depth_run(s, c->smp_W, c->smp_V + (size_t)(c->T - Lt) * c->K, (long long)c->T * c->K, c->smp_s + HYP_LAM2,
                              (int)HYP_COUNT, c->gg_tab, c->gg_G, c->gg_lsp, f, p);
}

int btf_diag_eval(int device, int nchains, int nsamples, int nrows, int ncols, int ndepth, int nembeds, const double* const* Ws,
                  const double* const* Vs, btf_ctx* const* ctxs, int transform, double* out) {
  if (nchains < 1 || nchains > DIAG_MAX_CHAINS || nsamples < 4 || (long long)nchains * nsamples > DIAG_MAX_DRAWS || nrows < 1 ||
      ncols < 1 || ndepth < 1 || nembeds < 1 || nembeds > MAX_K || transform < 0 || transform > 2 || !out ||
      (long long)nrows * ncols * ndepth > 0x7fffffffLL)
    return fail(nullptr, BTF_EINVAL, "bad btf_diag_eval arguments");
  for (int c = 0; c < nchains; ++c) {
    const btf_ctx* x = ctxs ? ctxs[c] : nullptr;
    if (x) {
      if (x->dev != device || x->N != nrows || x->M != ncols || x->T != ndepth || x->K != nembeds)
        return fail(nullptr, BTF_EINVAL, "btf_diag_eval: a context of another device or shape");
      if (x->nl != x->N || x->ml != x->M) return fail(nullptr, BTF_ESTATE, "btf_diag_eval needs unsharded contexts");
      if (!has_collected(x, nsamples)) return no_collected(nullptr, BTF_ESTATE, "btf_diag_eval");
    } else if (!Ws || !Vs || !Ws[c] || !Vs[c]) {
      return fail(nullptr, BTF_EINVAL, "btf_diag_eval: chain without host arrays or a context");
    }
  }
  if (int rc = use_device(device)) return rc;
  const int MT = ncols * ndepth;
  const size_t cells = (size_t)nrows * MT;
  const size_t nW = (size_t)nsamples * nrows * nembeds, nV = (size_t)nsamples * MT * nembeds;
  Scratch s(nullptr, nullptr);
  std::vector<const double*> pw(nchains), pv(nchains);
  for (int c = 0; c < nchains; ++c) {
    const btf_ctx* x = ctxs ? ctxs[c] : nullptr;
    if (x) {                                               // the collection copies may still be in flight on its stream
      s.check(hipStreamSynchronize(x->stream), "hipStreamSynchronize");
      pw[c] = x->smp_W; pv[c] = x->smp_V;
    } else {
      pw[c] = s.upload(Ws[c], nW); pv[c] = s.upload(Vs[c], nV);
    }
  }
  double* dout = s.alloc<double>(DIAG_OUT * cells);
  int P = 2;
  while (P < nchains * nsamples) P <<= 1;
  DiagArgs a{s.upload(pw.data(), (size_t)nchains), s.upload(pv.data(), (size_t)nchains), nchains, nsamples, nrows, MT, P, transform, dout};
  const size_t lds = (size_t)(nchains * nsamples + P) * sizeof(double);
  K_SWITCH(nembeds, {
    allow_lds(s, diag_kernel<KT>, lds);
    s.launch(diag_kernel<KT>, dim3((unsigned)cells), dim3(DIAG_THREADS), lds, a);
  });
  s.download(out, dout, DIAG_OUT * cells);
  return s.finish();
}

}  // extern "C"
int btf::fold_fail_index() { return g_fold_fail_index; }
