// Subgroup audit of a fold (mmskin.subgroup.SubgroupAudit): the bootstrap of bootstrap.hip scored per group of rows -- for whom is
// the model good?  The weights of replicate b are those of mmskin_bootstrap_weights on the WHOLE fold (phase 1 is the code of
// bootstrap_core.h), so a group's replicate, another group's and the fold's are one resample and their differences are paired.
// The contract is in include/mmskin.h; tests/subgroup_oracle.py restates all of it in numpy.
//
//   replicates  one workgroup per replicate.  Phase 1: w_b in LDS (build_weights).  Phase 2: the confusion cells [G][K][K] and
//               pos[G][K] by integer LDS atomic adds of w_b[i] into the cells of row i's group; a row in no group adds nothing.
//               Phase 3, per class c: the caller's order table walks the rows in ascending order of (group, s[.][c]), so group g
//               owns the positions [start_g, start_{g+1}) and a tie group never crosses a group boundary.  v_q = w of the row at
//               position q if it is a negative of c, else 0; P = the exclusive prefix sum of v over ALL positions: one scan, the
//               one of bootstrap.hip, whatever G is.  The negatives of group g before position x weigh P[x] - P[start_g], so a
//               positive of group g at position q with tie group [lo, hi) adds w_q (P[lo] + P[hi] - 2 P[start_g]) = 2 less + equal
//               to wins2[g][c]: an int64 LDS atomic add.  Every row is a positive of one class only, so these atomics number at
//               most N per replicate, as the confusion atomics do.
//   metrics     one thread per (group, replicate): the bootstrap columns by metric_columns of bootstrap_core.h on the group's
//               integers, then the false-positive and predicted rates per class; all NaN below min_rows.
//   summary     one workgroup per (group, column): summarize_column of column_summary.h.
//   gaps        one workgroup per (column, quantity): lowest, highest and gap over the groups defined in a replicate, the count of
//               replicates in which each group is the lowest (integer LDS atomics), then summarize_column.
#include "../../include/mmskin.h"
#include "bootstrap_core.h"
#include "column_summary.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SG_MAX_N = MMSKIN_SUBGROUP_MAX_ROWS;        // 8192
constexpr int SG_MAX_G = MMSKIN_SUBGROUP_MAX_GROUPS;      // 64
constexpr int SG_MAX_CELLS = MMSKIN_SUBGROUP_MAX_CELLS;   // 16384 = G K K
constexpr int SG_MAX_GK = 1024;                           // G K at most: G <= 64 and G K K <= 16384 give G K <= min(64 K, 16384 / K) <= 1024
constexpr int NO_GROUP = 0xFF;
static_assert(SG_MAX_G < NO_GROUP, "a group id must fit a byte beside NO_GROUP");
static_assert(SG_MAX_G * 16 <= SG_MAX_GK && SG_MAX_CELLS / 16 <= SG_MAX_GK, "G K peaks at K = 16");

// Dynamic LDS of the replicates kernel, in bytes, for N rows (Np = N rounded up to 4):
//   w      int32 [Np]                      the replicate's weights
//   P      int32 [max(Np, G K K)]          phase 2: the confusion cells; phase 3: the prefix within the segment
//   lab    uint8 [Np]                      the rows' labels (gathered at random in phase 3)
//   grp    uint8 [Np]                      the rows' groups (NO_GROUP outside [0, G))
//   pos    int32 [G K]                     the groups' weighted class counts (G K <= 1024)
// and statically start[K + 1] + gstart[G + 1] + base[G] + seg_total[16] int32 and wins[G] int64: (65 + 65 + 64 + 16) 4 + 512 = 1352
// bytes.  At the limits N = 8192, G K K = 16384 (G K <= 1024): 32768 + 65536 + 8192 + 8192 + 4096 + 1352 = 120136 bytes = 117.3 KiB
// of the 160 KiB a workgroup may declare.  (N = 8192, G = 16, K = 8): 1024 cells, P holds 8192: 32768 + 32768 + 16384 + 512 + 1352 =
// 83784 bytes.  (N = 8192, G = 4, K = 64): 16384 cells, 32768 + 65536 + 16384 + 1024 + 1352 = 117064 bytes.
// pos is dynamic so that a fold of 5000 rows keeps THREE workgroups on a CU as the bootstrap's kernel does (N = 5000, G = 16,
// K = 8: 50000 + 512 + 1352 = 51864 bytes, 3 x 51864 <= 163840; 4 KiB more would leave two).
inline size_t sg_np(int N) { return (size_t)((N + 3) & ~3); }
inline size_t sg_p_cells(int N, int G, int K) { return sg_np(N) > (size_t)G * K * K ? sg_np(N) : (size_t)G * K * K; }
inline size_t sg_lds_bytes(int N, int G, int K) { return (sg_np(N) + sg_p_cells(N, G, K) + (size_t)G * K) * 4 + 2 * sg_np(N); }
static_assert(((size_t)SG_MAX_N + SG_MAX_CELLS + SG_MAX_GK) * 4 + 2 * SG_MAX_N + 1352 <= 160 * 1024, "the limits must fit one workgroup's LDS");
static_assert(SG_MAX_CELLS >= SG_MAX_N, "the LDS bound above takes the cells as the larger use of P");

// ------------------------------------------------------------------------------------------------ replicates
__global__ __launch_bounds__(1024) void subgroup_replicates_kernel(uint64_t key, int mode, int N, int K, int G, const int64_t* __restrict__ labels,
                                                                   const int64_t* __restrict__ preds, const int32_t* __restrict__ groups,
                                                                   const int32_t* __restrict__ members, const int32_t* __restrict__ class_start,
                                                                   const int32_t* __restrict__ order, const int32_t* __restrict__ lo,
                                                                   const int32_t* __restrict__ hi, const int32_t* __restrict__ group_start, int b0,
                                                                   int seg, int32_t* __restrict__ confusion, int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int32_t s_start[MAX_K + 1];
  __shared__ int32_t s_gstart[SG_MAX_G + 1];
  __shared__ int32_t s_base[SG_MAX_G];
  __shared__ int32_t s_seg[MAX_WAVES];
  __shared__ unsigned long long s_wins[SG_MAX_G];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = nt >> 6;
  const int Np = (N + 3) & ~3, cells = G * K * K;
  int32_t* s_w = reinterpret_cast<int32_t*>(lds);
  int32_t* s_P = s_w + Np;                                          // max(Np, G K K) cells
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_P + max(Np, cells));
  uint8_t* s_grp = s_lab + Np;
  int32_t* s_pos = reinterpret_cast<int32_t*>(s_grp + Np);           // Np is a multiple of 4: aligned; G K cells
  const int64_t b = (int64_t)b0 + blockIdx.x;

  for (int i = tid; i < N; i += nt) {
    const int32_t g = groups[i];
    s_grp[i] = (uint8_t)((g >= 0 && g < G) ? g : NO_GROUP);
  }
  for (int g = tid; g <= G; g += nt) s_gstart[g] = group_start[g];
  stage_labels(labels, class_start, N, K, mode, s_lab, s_start);    // ends with a barrier
  build_weights(key, (uint64_t)b, mode, N, members, s_lab, s_start, s_w);

  // phase 2: the confusion cells live where P will; pos[g][c] = the weight of group g's rows with label c, whatever their prediction
  for (int e = tid; e < cells; e += nt) s_P[e] = 0;
  for (int e = tid; e < G * K; e += nt) s_pos[e] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += nt) {
    const int y = s_lab[i], g = s_grp[i], w = s_w[i];
    if (!w || y == NO_LABEL || g == NO_GROUP) continue;
    const int64_t p = preds[i];
    atomicAdd(&s_pos[g * K + y], w);
    if (p >= 0 && p < K) atomicAdd(&s_P[(g * K + y) * K + (int)p], w);
  }
  __syncthreads();
  int32_t* conf = confusion + b * cells;
  for (int e = tid; e < cells; e += nt) conf[e] = s_P[e];
  int64_t* cnt = counts + b * G * 3 * K;                            // [G][3 K]
  for (int e = tid; e < G * K; e += nt) {
    const int g = e / K, c = e - g * K;
    int32_t rows = 0;                                               // the weight of the group's rows that count
    for (int k = 0; k < K; ++k) rows += s_pos[g * K + k];
    cnt[g * 3 * K + c] = s_pos[e];
    cnt[g * 3 * K + K + c] = rows - s_pos[e];
  }
  __syncthreads();                                                  // the cells are out: P may be written

  // phase 3
  const int q_beg = min(wave * seg, N), q_end = min(q_beg + seg, N);   // seg is a multiple of 64 and waves * seg >= N
  for (int c = 0; c < K; ++c) {
    const int32_t* ord = order + (int64_t)c * N;
    int32_t carry = 0;
    for (int q0 = q_beg; q0 < q_end; q0 += 64) {
      const int q = q0 + lane;
      int32_t v = 0;
      if (q < q_end) {
        const int row = ord[q];
        if ((unsigned)row < (unsigned)N) {
          const int y = s_lab[row];
          v = (y != NO_LABEL && y != c) ? s_w[row] : 0;
        }
      }
      int32_t incl = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (q < q_end) s_P[q] = carry + incl - v;                     // q < N <= the cells of P
      carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) s_seg[wave] = carry;
    if (tid < G) s_wins[tid] = 0ull;                                // G <= 64 <= nt; last read by this same thread (below)
    __syncthreads();
    int32_t total = 0;
    for (int k = 0; k < waves; ++k) total += s_seg[k];
    // P at position x of the whole order: x <= 0 -> 0, x >= N -> every negative
    auto prefix_at = [&](int x) -> int32_t {
      if (x <= 0) return 0;
      if (x >= N) return total;
      int32_t p = s_P[x];
      for (int k = 0; k < x / seg; ++k) p += s_seg[k];
      return p;
    };
    if (tid < G) s_base[tid] = prefix_at(s_gstart[tid]);
    __syncthreads();
    for (int q = tid; q < N; q += nt) {
      const int row = ord[q];
      if ((unsigned)row >= (unsigned)N || s_lab[row] != c) continue;
      const int g = s_grp[row];
      const int32_t w = s_w[row];
      if (!w || g == NO_GROUP) continue;
      const int32_t below = prefix_at(lo[(int64_t)c * N + q]), upto = prefix_at(hi[(int64_t)c * N + q]);
      // w <= N, below + upto - 2 base within +-2 N: below 2^28 in magnitude; two's complement carries a negative term of bad tables
      atomicAdd(&s_wins[g], (unsigned long long)((int64_t)w * (int64_t)(below + upto - 2 * s_base[g])));
    }
    __syncthreads();                                                // the reads of P, the segment totals and base are done
    if (tid < G) cnt[tid * 3 * K + 2 * K + c] = (int64_t)s_wins[tid];
  }
}

// ------------------------------------------------------------------------------------------------ metrics
__global__ __launch_bounds__(256) void subgroup_metrics_kernel(const int32_t* __restrict__ confusion, const int64_t* __restrict__ counts, int B,
                                                               int G, int K, int64_t min_rows, double* __restrict__ metrics) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;       // = g B + b
  if (e >= (int64_t)G * B) return;
  const int g = (int)(e / B), b = (int)(e - (int64_t)g * B);
  const int M = 7 + 4 * K;
  const int32_t* cm = confusion + ((int64_t)b * G + g) * K * K;
  const int64_t* cnt = counts + ((int64_t)b * G + g) * 3 * K;
  double* col = metrics + (int64_t)g * M * B + b;                  // column m of (g, b): col[m B]
  const double nan = nan64();
  int64_t rows = 0;
  for (int c = 0; c < K; ++c) rows += cnt[c];
  if (rows < min_rows) {
    for (int m = 0; m < M; ++m) col[(int64_t)m * B] = nan;
    return;
  }
  metric_columns(cm, cnt, K, col, B);
  for (int c = 0; c < K; ++c) {
    int64_t pred_n = 0;
    for (int k = 0; k < K; ++k) pred_n += cm[k * K + c];
    const int64_t others = rows - cnt[c];
    col[(int64_t)(7 + 2 * K + c) * B] = others > 0 ? (double)(pred_n - cm[c * K + c]) / (double)others : nan;
    col[(int64_t)(7 + 3 * K + c) * B] = rows > 0 ? (double)pred_n / (double)rows : nan;
  }
}

__global__ __launch_bounds__(NT_COL) void subgroup_summary_kernel(const double* __restrict__ metrics, int B, int n, int M, double q_lo, double q_hi,
                                                                  double* __restrict__ summary) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x, g = blockIdx.y;
  for (int i = threadIdx.x; i < B; i += NT_COL) s_val[i] = metrics[((int64_t)g * M + m) * B + i];
  __syncthreads();
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary + (int64_t)g * 5 * M);
}

// ------------------------------------------------------------------------------------------------ gaps
// blockIdx.y = 0 lowest, 1 highest, 2 gap: each workgroup forms its own quantity of column m (G B reads) and summarises it.
__global__ __launch_bounds__(NT_COL) void subgroup_gaps_kernel(const double* __restrict__ metrics, int B, int n, int G, int M, double q_lo,
                                                               double q_hi, double* __restrict__ lowest, double* __restrict__ highest,
                                                               double* __restrict__ gap, int64_t* __restrict__ lowest_group,
                                                               double* __restrict__ summary) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int32_t s_low[SG_MAX_G];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x, which = blockIdx.y;
  if (threadIdx.x < G) s_low[threadIdx.x] = 0;
  __syncthreads();
  double* out = which == 0 ? lowest : (which == 1 ? highest : gap);
  for (int i = threadIdx.x; i < B; i += NT_COL) {
    double lo_v = 0.0, hi_v = 0.0;
    int defined = 0, lo_g = 0;
    for (int g = 0; g < G; ++g) {
      const double v = metrics[((int64_t)g * M + m) * B + i];
      if (v != v) continue;
      if (!defined || v < lo_v) { lo_v = v; lo_g = g; }             // strict: a tie stays with the smallest id
      if (!defined || v > hi_v) hi_v = v;
      ++defined;
    }
    const double r = which == 0 ? (defined ? lo_v : nan64()) : (which == 1 ? (defined ? hi_v : nan64()) : (defined >= 2 ? hi_v - lo_v : nan64()));
    out[(int64_t)m * B + i] = r;
    s_val[i] = r;
    if (which == 0 && defined) atomicAdd(&s_low[lo_g], 1);
  }
  __syncthreads();
  if (which == 0 && threadIdx.x < G) lowest_group[(int64_t)m * G + threadIdx.x] = s_low[threadIdx.x];
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary + (int64_t)which * 5 * M);
}

// ------------------------------------------------------------------------------------------------ host
int group_limits(const char* what, int G, int K) {
  if (G < 1 || G > SG_MAX_G) {
    mmskin_set_error("%s: %d groups; a row's group is a byte in LDS, which holds 1 .. MMSKIN_SUBGROUP_MAX_GROUPS = %d", what, G, SG_MAX_G);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if ((int64_t)G * K * K > SG_MAX_CELLS) {
    mmskin_set_error("%s: %d groups of %d classes are %lld confusion cells; LDS holds G K K <= MMSKIN_SUBGROUP_MAX_CELLS = %d", what, G, K,
                     (long long)G * K * K, SG_MAX_CELLS);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_subgroup_metric_columns(int K) { return (K < 2 || K > MAX_K) ? -1 : 7 + 4 * K; }

extern "C" int mmskin_subgroup_replicates(uint64_t seed, int mode, int N, int K, int G, int B, const int64_t* labels, const int64_t* preds,
                                          const int32_t* groups, const int32_t* members, const int32_t* class_start, const int32_t* order,
                                          const int32_t* lo, const int32_t* hi, const int32_t* group_start, int b0, int b1, int32_t* confusion,
                                          int64_t* counts, void* stream) {
  if (int rc = study_limits("subgroup_replicates", N, K, B, SG_MAX_N, "MMSKIN_SUBGROUP_MAX_ROWS")) return rc;
  if (int rc = group_limits("subgroup_replicates", G, K)) return rc;
  if (int rc = mode_ok("subgroup_replicates", mode)) return rc;
  if (int rc = range_ok("subgroup_replicates", B, b0, b1)) return rc;
  ARG_CHECK(labels && preds && groups && order && lo && hi && group_start && confusion && counts, "subgroup_replicates: null argument");
  ARG_CHECK(mode != MMSKIN_BOOTSTRAP_STRATIFIED || (members && class_start), "subgroup_replicates: stratified resampling needs members and class_start");
  if (b0 == b1) return MMSKIN_OK;
  const int nt = replicate_threads(N), waves = nt / 64;
  const int seg = scan_segment(N, waves);
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)subgroup_replicates_kernel, (int)(((size_t)SG_MAX_N + SG_MAX_CELLS + SG_MAX_GK) * 4 + 2 * SG_MAX_N)));
  hipLaunchKernelGGL(subgroup_replicates_kernel, dim3((unsigned)(b1 - b0)), dim3(nt), sg_lds_bytes(N, G, K), ST(stream), mix64(seed), mode, N, K, G,
                     labels, preds, groups, members, class_start, order, lo, hi, group_start, b0, seg, confusion, counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_subgroup_finalize(const int32_t* confusion, const int64_t* counts, int B, int G, int K, int64_t min_rows, double q_lo,
                                        double q_hi, double* metrics, double* summary, void* stream) {
  if (int rc = study_limits("subgroup_finalize", 1, K, B)) return rc;
  if (int rc = group_limits("subgroup_finalize", G, K)) return rc;
  if (int rc = quantiles_ok("subgroup_finalize", q_lo, q_hi)) return rc;
  ARG_CHECK(min_rows >= 1, "subgroup_finalize: min_rows must be >= 1, got %lld", (long long)min_rows);
  ARG_CHECK(confusion && counts && metrics && summary, "subgroup_finalize: null argument");
  const int M = 7 + 4 * K;
  hipLaunchKernelGGL(subgroup_metrics_kernel, dim3((unsigned)(((int64_t)G * B + 255) / 256)), dim3(256), 0, ST(stream), confusion, counts, B, G, K,
                     min_rows, metrics);
  HIP_CHECK_RET(hipGetLastError());
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)subgroup_summary_kernel, (int)column_lds_bytes(MAX_B)));
  hipLaunchKernelGGL(subgroup_summary_kernel, dim3(M, G), dim3(NT_COL), column_lds_bytes(B), ST(stream), metrics, B, pow2_at_least(B), M, q_lo, q_hi,
                     summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_subgroup_gaps(const double* metrics, int B, int G, int M, double q_lo, double q_hi, double* lowest, double* highest,
                                    double* gap, int64_t* lowest_group, double* summary, void* stream) {
  if (int rc = study_limits("subgroup_gaps", 1, 2, B)) return rc;
  if (G < 1 || G > SG_MAX_G) {
    mmskin_set_error("subgroup_gaps: %d groups; the kernels hold 1 .. MMSKIN_SUBGROUP_MAX_GROUPS = %d", G, SG_MAX_G);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (int rc = quantiles_ok("subgroup_gaps", q_lo, q_hi)) return rc;
  ARG_CHECK(M >= 1 && M <= 7 + 4 * MAX_K, "subgroup_gaps: %d metric columns are outside 1 .. %d", M, 7 + 4 * MAX_K);
  ARG_CHECK(metrics && lowest && highest && gap && lowest_group && summary, "subgroup_gaps: null argument");
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)subgroup_gaps_kernel, (int)column_lds_bytes(MAX_B)));
  hipLaunchKernelGGL(subgroup_gaps_kernel, dim3(M, 3), dim3(NT_COL), column_lds_bytes(B), ST(stream), metrics, B, pow2_at_least(B), G, M, q_lo, q_hi,
                     lowest, highest, gap, lowest_group, summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
