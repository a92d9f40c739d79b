// What bootstrap.hip and subgroup.hip share, stated once: the counter-based generator and phase 1 of a replicate (the weights w_b in
// LDS), the 64-bit wave sum, the metric columns of one replicate's integers, and the host-side checks of a study's extents.  The
// contract is in include/mmskin.h (the bootstrap section); tests/bootstrap_oracle.py restates it in numpy.
#pragma once
#include "../../include/mmskin.h"
#include "column_summary.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_K = MMSKIN_BOOTSTRAP_MAX_CLASSES;      // 64
constexpr int MAX_B = MMSKIN_BOOTSTRAP_MAX_RESAMPLES;    // 8192
constexpr int MAX_WAVES = 16;                            // 1024 threads
constexpr int NO_LABEL = 0xFF;

__device__ __forceinline__ uint32_t draw_u(uint64_t key, uint64_t b, int t) { return (uint32_t)(mix64(key ^ ((b << 32) | (uint64_t)(uint32_t)t)) >> 32); }

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)((uint64_t)v >> 32), o, 64);
    v += (int64_t)(((uint64_t)hi << 32) | lo);
  }
  return v;
}

// labels -> LDS bytes (NO_LABEL outside [0, K)), class_start -> LDS; ends with a barrier
__device__ __forceinline__ void stage_labels(const int64_t* __restrict__ labels, const int32_t* __restrict__ class_start, int N, int K,
                                             int mode, uint8_t* s_lab, int32_t* s_start) {
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int64_t y = labels[i];
    s_lab[i] = (uint8_t)((y >= 0 && y < K) ? (int)y : NO_LABEL);
  }
  if (mode == MMSKIN_BOOTSTRAP_STRATIFIED)
    for (int c = threadIdx.x; c <= K; c += blockDim.x) s_start[c] = class_start[c];
  __syncthreads();
}

// phase 1: w[0 .. N) of replicate b; ends with a barrier.  Every index into w is checked: a table entry out of range draws nothing.
__device__ __forceinline__ void build_weights(uint64_t key, uint64_t b, int mode, int N, const int32_t* __restrict__ members,
                                              const uint8_t* s_lab, const int32_t* s_start, int32_t* s_w) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < N; i += nt) s_w[i] = mode == MMSKIN_BOOTSTRAP_POINT ? 1 : 0;
  __syncthreads();
  if (mode == MMSKIN_BOOTSTRAP_PLAIN) {
    for (int t = tid; t < N; t += nt) {
      const int row = (int)(((uint64_t)draw_u(key, b, t) * (uint64_t)N) >> 32);       // < N
      atomicAdd(&s_w[row], 1);
    }
  } else if (mode == MMSKIN_BOOTSTRAP_STRATIFIED) {
    for (int t = tid; t < N; t += nt) {
      const int c = s_lab[t];
      if (c == NO_LABEL) continue;
      const int s = s_start[c], n = s_start[c + 1] - s;
      if (s < 0 || n < 1 || s + n > N) continue;
      const int row = members[s + (int)(((uint64_t)draw_u(key, b, t) * (uint64_t)n) >> 32)];
      if ((unsigned)row < (unsigned)N) atomicAdd(&s_w[row], 1);
    }
  }
  __syncthreads();
}

// The 7 + 2 K metric columns (layout: mmskin.h) of one set of integers: cm int32 [K][K], cnt int64 [3 K] (pos, neg, wins2).
// Column m goes to col[m stride].
__device__ __forceinline__ void metric_columns(const int32_t* __restrict__ cm, const int64_t* __restrict__ cnt, int K, double* __restrict__ col,
                                               int64_t stride) {
  const double nan = nan64();
  int64_t n = 0, hits = 0;
  for (int e = 0; e < K * K; ++e) n += cm[e];
  double recall_sum = 0.0, wp = 0.0, wr = 0.0, wf = 0.0, p1 = 0.0, r1 = 0.0, f1 = 0.0;
  int present = 0;
  for (int c = 0; c < K; ++c) {
    int64_t true_n = 0, pred_n = 0;
    for (int k = 0; k < K; ++k) { true_n += cm[c * K + k]; pred_n += cm[k * K + c]; }
    const double tp = (double)cm[c * K + c];
    hits += cm[c * K + c];
    const double prec = pred_n > 0 ? tp / (double)pred_n : 0.0, rec = true_n > 0 ? tp / (double)true_n : 0.0;
    const double f = true_n + pred_n > 0 ? 2.0 * tp / (double)(true_n + pred_n) : 0.0;
    if (true_n > 0) { recall_sum += rec; ++present; }
    wp += prec * (double)true_n; wr += rec * (double)true_n; wf += f * (double)true_n;
    if (c == 1) { p1 = prec; r1 = rec; f1 = f; }
    col[(int64_t)(7 + c) * stride] = true_n > 0 ? rec : nan;
  }
  col[0] = n > 0 ? (double)hits / (double)n : nan;
  col[(int64_t)1 * stride] = present > 0 ? recall_sum / (double)present : nan;
  if (K == 2) {
    col[(int64_t)2 * stride] = p1; col[(int64_t)3 * stride] = r1; col[(int64_t)4 * stride] = f1;
  } else {
    col[(int64_t)2 * stride] = n > 0 ? wp / (double)n : 0.0;
    col[(int64_t)3 * stride] = n > 0 ? wr / (double)n : 0.0;
    col[(int64_t)4 * stride] = n > 0 ? wf / (double)n : 0.0;
  }
  double weighted = 0.0, weight = 0.0, plain = 0.0, auc1 = nan;
  int ranked = 0;
  for (int c = 0; c < K; ++c) {
    const double pos = (double)cnt[c], pairs = 2.0 * pos * (double)cnt[K + c];
    double auc = nan;
    if (pairs > 0.0) {
      auc = (double)cnt[2 * K + c] / pairs;
      weighted += auc * pos; weight += pos; plain += auc; ++ranked;
    }
    if (c == 1) auc1 = auc;
    col[(int64_t)(7 + K + c) * stride] = auc;
  }
  col[(int64_t)5 * stride] = K == 2 ? auc1 : (ranked > 0 ? weighted / weight : nan);
  col[(int64_t)6 * stride] = ranked > 0 ? plain / (double)ranked : nan;
}

// a metric column must fit one summary workgroup's LDS: the B values (fp64) and n >= B sort keys: at B = 8192, 128 KiB
static_assert(((size_t)MAX_B + MAX_B) * 8 + 64 <= 160 * 1024, "a column must fit one workgroup's LDS");

// ------------------------------------------------------------------------------------------------ host
// max_rows / rows_name: the row limit of the caller's replicate kernel and the macro that states it
inline int study_limits(const char* what, int N, int K, int B, int max_rows = MMSKIN_BOOTSTRAP_MAX_ROWS,
                        const char* rows_name = "MMSKIN_BOOTSTRAP_MAX_ROWS") {
  if (N < 1 || N > max_rows) {
    mmskin_set_error("%s: %d rows; a replicate's weights live in LDS, which holds 1 .. %s = %d", what, N, rows_name, max_rows);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (K < 2 || K > MAX_K) {
    mmskin_set_error("%s: %d classes; the kernels hold 2 .. MMSKIN_BOOTSTRAP_MAX_CLASSES = %d", what, K, MAX_K);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (B < 1 || B > MAX_B) {
    mmskin_set_error("%s: %d replicates; a metric column is sorted in LDS, which holds 1 .. MMSKIN_BOOTSTRAP_MAX_RESAMPLES = %d", what, B,
                     MAX_B);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

inline int range_ok(const char* what, int B, int b0, int b1) {
  ARG_CHECK(b0 >= 0 && b0 <= b1 && b1 <= B, "%s: replicates [%d, %d) are not a range of the study's %d", what, b0, b1, B);
  return MMSKIN_OK;
}

inline int mode_ok(const char* what, int mode) {
  ARG_CHECK(mode == MMSKIN_BOOTSTRAP_PLAIN || mode == MMSKIN_BOOTSTRAP_STRATIFIED || mode == MMSKIN_BOOTSTRAP_POINT, "%s: unknown mode %d", what,
            mode);
  return MMSKIN_OK;
}

inline int quantiles_ok(const char* what, double q_lo, double q_hi) {
  ARG_CHECK(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "%s: the quantiles (%g, %g) must satisfy 0 <= low <= high <= 1", what, q_lo, q_hi);
  return MMSKIN_OK;
}

// threads of a replicate's workgroup: more waves where one workgroup fills the CU's LDS alone
inline int replicate_threads(int N) { return N <= 4096 ? 256 : (N <= 8192 ? 512 : 1024); }
// positions per wave in the scan: a multiple of 64, waves * seg >= N
inline int scan_segment(int N, int waves) { return ((N + waves - 1) / waves + 63) / 64 * 64; }

}  // namespace
