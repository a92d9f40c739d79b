// Bootstrap confidence intervals of a fold's metrics (mmskin.bootstrap.BootstrapMetrics): the non-parametric bootstrap over the
// fold's N rows, B replicates, every replicate scored as exact integers on the device.  The contract is in include/mmskin.h;
// tests/bootstrap_oracle.py restates all of it in numpy.
//
// The generator (counter based, no state): key = mix64(seed); replicate b, draw t: h = mix64(key ^ (b << 32 | t)), u = h >> 32.
// Plain: draw t hits row (u N) >> 32.  Stratified: with c the label of row t, draw t hits the ((u n_c) >> 32)-th row of class c
// (members / class_start).  w_b[i] = the number of draws of replicate b that hit row i.  Point: w = 1, the fold itself.
//
//   replicates  one workgroup per replicate.  Phase 1: w_b in LDS by integer LDS atomic adds (order-free, so deterministic).
//               Phase 2: the confusion cells by integer LDS atomic adds of w_b[i] into cell [y_i][p_i], and of pos[y_i] beside them.
//               Phase 3, per class c: walk the rows in ascending order of s[.][c] (the prep's table), v_q = w of the row at
//               position q if it is a negative of c, else 0; P = the exclusive prefix sum of v.  A positive at position q whose
//               tie group is [lo, hi) has P[lo] of negative weight strictly below and P[hi] at or below, so
//               wins2[c] = sum over positives of w_q (P[lo_q] + P[hi_q]) = 2 less + equal, in int64.
//               The scan: wave k owns the contiguous segment [k seg, (k + 1) seg) of positions (seg a multiple of 64), scans it
//               64 positions at a time with a running carry and leaves the prefix WITHIN the segment in LDS; the segment totals
//               are summed after one barrier, P[x] = within[x] + (sum of the totals of the segments before x's).
//               Every sum has one owner or is an integer LDS atomic; nothing floats, nothing is added in global memory.
//   weights     phase 1 alone, w_b written out: for tests and for users who want the resamples themselves.
//   metrics     one thread per replicate: the metric columns in fp64 (layout: mmskin.h).
//   summary     one workgroup per metric column: the B values in LDS; n_valid, mean and deviation (ddof = 1) summed in replicate
//               order by one thread; then a bitonic sort of order-preserving 64-bit keys, NaN last, and numpy's linear percentile.
//   compare     the same on d = a - b of two metric tables, plus the counts of d <= 0 and d >= 0 (integer LDS atomics).
#include "../../include/mmskin.h"
#include "auc_pairs.h"
#include "bootstrap_core.h"
#include "column_summary.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_N = MMSKIN_BOOTSTRAP_MAX_ROWS;         // 16384; MAX_K, MAX_B, MAX_WAVES, NO_LABEL: bootstrap_core.h

// Dynamic LDS of the replicates kernel, in bytes, for N rows (Np = N rounded up to 4):
//   w      int32 [Np]                      the replicate's weights
//   P      int32 [max(Np, K K)]            phase 2: the confusion cells; phase 3: the prefix within the segment
//   lab    uint8 [Np]                      the rows' labels (gathered at random in phase 3)
// and statically start[K + 1] + pos[K] + seg_total[16] int32 and red[16] int64: (65 + 64 + 16) 4 + 128 = 708 bytes.
// At the limits N = 16384, K = 64: 65536 + 65536 + 16384 + 708 = 148164 bytes = 144.7 KiB of the 160 KiB a workgroup may declare.
inline size_t p_cells(int N, int K) { return (size_t)(((N + 3) & ~3) > K * K ? ((N + 3) & ~3) : K * K); }
inline size_t replicate_lds_bytes(int N, int K) { return ((size_t)((N + 3) & ~3) + p_cells(N, K)) * 4 + (size_t)((N + 3) & ~3); }
static_assert(((size_t)MAX_N + MAX_N) * 4 + MAX_N + 708 <= 160 * 1024, "the limits must fit one workgroup's LDS");

// The generator, stage_labels and build_weights (phase 1), wave_sum_i64 and metric_columns: bootstrap_core.h, shared with subgroup.hip.

// ------------------------------------------------------------------------------------------------ weights
__global__ __launch_bounds__(1024) void bootstrap_weights_kernel(uint64_t key, int mode, int N, int K, const int64_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ members, const int32_t* __restrict__ class_start,
                                                                 int b0, int32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int32_t s_start[MAX_K + 1];
  const int Np = (N + 3) & ~3;
  int32_t* s_w = reinterpret_cast<int32_t*>(lds);
  uint8_t* s_lab = lds + (size_t)Np * 4;
  if (mode == MMSKIN_BOOTSTRAP_STRATIFIED) stage_labels(labels, class_start, N, K, mode, s_lab, s_start);
  build_weights(key, (uint64_t)(b0 + blockIdx.x), mode, N, members, s_lab, s_start, s_w);
  int32_t* dst = out + (int64_t)blockIdx.x * N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = s_w[i];
}

// ------------------------------------------------------------------------------------------------ replicates
__global__ __launch_bounds__(1024) void bootstrap_replicates_kernel(uint64_t key, int mode, int N, int K, const int64_t* __restrict__ labels,
                                                                    const int64_t* __restrict__ preds, const int32_t* __restrict__ members,
                                                                    const int32_t* __restrict__ class_start, const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int b0,
                                                                    int seg, int32_t* __restrict__ confusion, int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int32_t s_start[MAX_K + 1];
  __shared__ int32_t s_pos[MAX_K];
  __shared__ int32_t s_seg[MAX_WAVES];
  __shared__ int64_t s_red[MAX_WAVES];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = nt >> 6;
  const int Np = (N + 3) & ~3;
  int32_t* s_w = reinterpret_cast<int32_t*>(lds);
  int32_t* s_P = s_w + Np;                                          // max(Np, K K) cells
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_P + max(Np, K * K));
  const int64_t b = (int64_t)b0 + blockIdx.x;

  stage_labels(labels, class_start, N, K, mode, s_lab, s_start);
  build_weights(key, (uint64_t)b, mode, N, members, s_lab, s_start, s_w);

  // phase 2: the confusion cells live where P will; pos[c] = the weight of the rows with label c, whatever their prediction
  for (int e = tid; e < K * K; e += nt) s_P[e] = 0;
  if (tid < K) s_pos[tid] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += nt) {
    const int y = s_lab[i], w = s_w[i];
    if (!w || y == NO_LABEL) continue;
    const int64_t p = preds[i];
    atomicAdd(&s_pos[y], w);
    if (p >= 0 && p < K) atomicAdd(&s_P[y * K + (int)p], w);
  }
  __syncthreads();
  int32_t* conf = confusion + b * K * K;
  for (int e = tid; e < K * K; e += nt) conf[e] = s_P[e];
  int32_t valid = 0;                                                // the weight of the rows that count: N unless a label is out of range
  for (int c = 0; c < K; ++c) valid += s_pos[c];
  int64_t* cnt = counts + b * 3 * K;
  if (tid < K) {
    cnt[tid] = s_pos[tid];
    cnt[K + tid] = valid - s_pos[tid];
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
    __syncthreads();
    int32_t total = 0;
    for (int k = 0; k < waves; ++k) total += s_seg[k];
    int64_t acc = 0;
    for (int q = tid; q < N; q += nt) {
      const int row = ord[q];
      if ((unsigned)row >= (unsigned)N || s_lab[row] != c) continue;
      const int32_t w = s_w[row];
      if (!w) continue;
      const int l = lo[(int64_t)c * N + q], h = hi[(int64_t)c * N + q];
      int32_t below = 0, upto = total;                              // position N: every negative lies before it
      if ((unsigned)l < (unsigned)N) {
        below = s_P[l];
        for (int k = 0; k < l / seg; ++k) below += s_seg[k];
      } else if (l < 0) {
        below = 0;
      } else {
        below = total;
      }
      if ((unsigned)h < (unsigned)N) {
        upto = s_P[h];
        for (int k = 0; k < h / seg; ++k) upto += s_seg[k];
      } else if (h < 0) {
        upto = 0;
      }
      acc += (int64_t)w * (int64_t)(below + upto);                  // w <= N, below + upto <= 2 N: below 2^30
    }
    acc = wave_sum_i64(acc);
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();                                                // the reads of P and of the segment totals are done
    if (tid == 0) {
      int64_t wins = 0;
      for (int k = 0; k < waves; ++k) wins += s_red[k];
      cnt[2 * K + c] = wins;
    }
  }
}

// ------------------------------------------------------------------------------------------------ metrics
__global__ __launch_bounds__(256) void bootstrap_metrics_kernel(const int32_t* __restrict__ confusion, const int64_t* __restrict__ counts,
                                                                int B, int K, double* __restrict__ metrics) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  metric_columns(confusion + (int64_t)b * K * K, counts + (int64_t)b * 3 * K, K, metrics + b, B);   // column m of replicate b: metrics[m B + b]
}

// ------------------------------------------------------------------------------------------------ summary
// n_valid, mean, deviation, the sort and the percentiles of a column: summarize_column of column_summary.h.  Dynamic LDS of a column
// workgroup: the B values (fp64) and n >= B sort keys (n a power of two, >= 2): at B = 8192, 128 KiB (asserted in bootstrap_core.h).

__global__ __launch_bounds__(NT_COL) void bootstrap_summary_kernel(const double* __restrict__ metrics, int B, int n, int M, double q_lo,
                                                                   double q_hi, double* __restrict__ summary) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x;
  for (int i = threadIdx.x; i < B; i += NT_COL) s_val[i] = metrics[(int64_t)m * B + i];
  __syncthreads();
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary);
}

__global__ __launch_bounds__(NT_COL) void bootstrap_compare_kernel(const double* __restrict__ a, const double* __restrict__ b, int B, int n,
                                                                   int M, double q_lo, double q_hi, double* __restrict__ delta,
                                                                   double* __restrict__ summary, int64_t* __restrict__ sign_counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int32_t s_sign[2];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x;
  if (threadIdx.x < 2) s_sign[threadIdx.x] = 0;
  __syncthreads();
  int32_t le = 0, ge = 0;
  for (int i = threadIdx.x; i < B; i += NT_COL) {
    const double d = a[(int64_t)m * B + i] - b[(int64_t)m * B + i];      // NaN if either side is
    delta[(int64_t)m * B + i] = d;
    s_val[i] = d;
    le += d <= 0.0;
    ge += d >= 0.0;
  }
  if (le) atomicAdd(&s_sign[0], le);
  if (ge) atomicAdd(&s_sign[1], ge);
  __syncthreads();
  if (threadIdx.x < 2) sign_counts[2 * m + threadIdx.x] = s_sign[threadIdx.x];
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary);
}

// ------------------------------------------------------------------------------------------------ host
// study_limits, range_ok, mode_ok, quantiles_ok, replicate_threads, scan_segment: bootstrap_core.h

}  // namespace

extern "C" int mmskin_bootstrap_metric_columns(int K) { return (K < 2 || K > MAX_K) ? -1 : 7 + 2 * K; }

extern "C" int mmskin_bootstrap_weights(uint64_t seed, int mode, int N, int K, int B, const int64_t* labels, const int32_t* members,
                                        const int32_t* class_start, int b0, int b1, int32_t* w, void* stream) {
  if (int rc = study_limits("bootstrap_weights", N, K, B)) return rc;
  if (int rc = mode_ok("bootstrap_weights", mode)) return rc;
  if (int rc = range_ok("bootstrap_weights", B, b0, b1)) return rc;
  ARG_CHECK(mode != MMSKIN_BOOTSTRAP_STRATIFIED || (labels && members && class_start), "bootstrap_weights: stratified resampling needs labels, members and class_start");
  ARG_CHECK(w || b0 == b1, "bootstrap_weights: null argument");
  if (b0 == b1) return MMSKIN_OK;
  const int bytes = (int)(((size_t)((N + 3) & ~3)) * 5);
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)bootstrap_weights_kernel, (MAX_N * 5)));
  hipLaunchKernelGGL(bootstrap_weights_kernel, dim3((unsigned)(b1 - b0)), dim3(replicate_threads(N)), bytes, ST(stream), mix64(seed), mode, N, K,
                     labels, members, class_start, b0, w);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_bootstrap_replicates(uint64_t seed, int mode, int N, int K, int B, const int64_t* labels, const int64_t* preds,
                                           const int32_t* members, const int32_t* class_start, const int32_t* order, const int32_t* lo,
                                           const int32_t* hi, int b0, int b1, int32_t* confusion, int64_t* counts, void* stream) {
  if (int rc = study_limits("bootstrap_replicates", N, K, B)) return rc;
  if (int rc = mode_ok("bootstrap_replicates", mode)) return rc;
  if (int rc = range_ok("bootstrap_replicates", B, b0, b1)) return rc;
  ARG_CHECK(labels && preds && order && lo && hi && confusion && counts, "bootstrap_replicates: null argument");
  ARG_CHECK(mode != MMSKIN_BOOTSTRAP_STRATIFIED || (members && class_start), "bootstrap_replicates: stratified resampling needs members and class_start");
  if (b0 == b1) return MMSKIN_OK;
  const int nt = replicate_threads(N), waves = nt / 64;
  const int seg = scan_segment(N, waves);
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)bootstrap_replicates_kernel, (int)replicate_lds_bytes(MAX_N, MAX_K)));
  hipLaunchKernelGGL(bootstrap_replicates_kernel, dim3((unsigned)(b1 - b0)), dim3(nt), replicate_lds_bytes(N, K), ST(stream), mix64(seed), mode, N,
                     K, labels, preds, members, class_start, order, lo, hi, b0, seg, confusion, counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_bootstrap_finalize(const int32_t* confusion, const int64_t* counts, int B, int K, double q_lo, double q_hi,
                                         double* metrics, double* summary, void* stream) {
  if (int rc = study_limits("bootstrap_finalize", 1, K, B)) return rc;
  if (int rc = quantiles_ok("bootstrap_finalize", q_lo, q_hi)) return rc;
  ARG_CHECK(confusion && counts && metrics && summary, "bootstrap_finalize: null argument");
  const int M = 7 + 2 * K;
  hipLaunchKernelGGL(bootstrap_metrics_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, ST(stream), confusion, counts, B, K, metrics);
  HIP_CHECK_RET(hipGetLastError());
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)bootstrap_summary_kernel, (int)column_lds_bytes(MAX_B)));
  hipLaunchKernelGGL(bootstrap_summary_kernel, dim3(M), dim3(NT_COL), column_lds_bytes(B), ST(stream), metrics, B, pow2_at_least(B), M, q_lo, q_hi,
                     summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_bootstrap_compare(const double* metrics_a, const double* metrics_b, int B, int M, double q_lo, double q_hi, double* delta,
                                        double* summary, int64_t* sign_counts, void* stream) {
  if (int rc = study_limits("bootstrap_compare", 1, 2, B)) return rc;
  if (int rc = quantiles_ok("bootstrap_compare", q_lo, q_hi)) return rc;
  ARG_CHECK(M >= 1 && M <= 7 + 2 * MAX_K, "bootstrap_compare: %d metric columns are outside 1 .. %d", M, 7 + 2 * MAX_K);
  ARG_CHECK(metrics_a && metrics_b && delta && summary && sign_counts, "bootstrap_compare: null argument");
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)bootstrap_compare_kernel, (int)column_lds_bytes(MAX_B)));
  hipLaunchKernelGGL(bootstrap_compare_kernel, dim3(M), dim3(NT_COL), column_lds_bytes(B), ST(stream), metrics_a, metrics_b, B, pow2_at_least(B), M,
                     q_lo, q_hi, delta, summary, sign_counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
