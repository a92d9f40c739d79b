// The criterion of the training step: weighted cross-entropy (torch nn.CrossEntropyLoss(weight=w), train_pad_20.py:52), the
// reference's focal loss (models/focalLoss.py:13-26, gamma a run-time float) and its soft-target cross-entropy
// (models/softtargetsCrossEntropy.py:10-22), each as ONE forward launch and ONE backward launch on logits [B][C], fp32 or bf16.
// All arithmetic is fp32.
//
//   geometry   one wavefront per row; lane l holds classes l, l + 64, ... in registers (KPL = 1 for C <= 64, 16 up to 1024).  A
//              workgroup of 16 waves serves 64 consecutive rows, four per wave.  Row max, sum of exponentials and arg-max go
//              through wave shuffles.
//   per row    m = max z, ls = ln sum exp(z - m) = log1p(sum over the classes other than the arg-max), ce = ls - (z[y] - m): the
//              order of torch's log_softmax, exact in (z[y] - m) where the rounded sum m + ls would lose ulp(m).  For that
//              reason the side buffer [B][2] keeps the log-sum-exp in its two parts (m, ls); the backward re-reads the logits once and forms p = exp((z - m) - ls) from them.
//              Focal: 1 - pt = -expm1(-ce), never 1 - exp(-ce); gamma == 0 skips the modulating factor, so it IS cross-entropy.
//   reduction  every workgroup adds its 64 row values in a fixed order and publishes one partial (loss, weight, valid rows);
//              the workgroup that draws the last ticket sums the partials in an order that depends on the grid alone.  The
//              only atomics on the loss path are the integer ticket and the agent-scope stores / loads of the partials: the
//              result is bitwise repeatable.  The ticket word is zero between launches (the last workgroup re-zeroes it).
//   meter      with an accumulator block the same launch adds the batch's loss sum and valid-row count (one thread, after the
//              reduction: one add per launch, in stream order) and counts [label][first arg-max of the logits] into an int32
//              confusion matrix with integer atomics; probs_out receives the soft-max.
//
// tests/criterion_oracle.py restates the formulas in float64 and is pinned to values recorded from the reference's own classes.
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 1024;                 // threads per workgroup
constexpr int WAVES = NT / 64;
constexpr int ROWS_PER_WG = 64;          // four rows per wave
constexpr int MAX_C = 1024;              // 16 classes per lane
constexpr int MAX_B = 1 << 20;

struct MeterBlock {                      // mmskin.h: the accumulator block's layout
  double loss_sum;
  int64_t rows;
  int32_t confusion[1];                  // [C][C]
};

// The one place that lays the scratch buffer out: run on a null base it sizes it (mmskin_criterion_scratch_floats).
struct Scratch {
  float* side;          // [B][2]  row max, ln sum exp(z - max)
  float* part_loss;     // [workgroups]
  float* part_weight;   // [workgroups]
  int32_t* part_rows;   // [workgroups]
  float* denom;         // [1]     what `mean` divided by
  size_t floats;
};
Scratch carve_scratch(float* base, int B) {
  Carver c(base);
  const size_t wgs = (size_t)ceil_div(B, ROWS_PER_WG);
  Scratch s;
  s.side = c.take<float>(2 * (size_t)B);
  s.part_loss = c.take<float>(wgs);
  s.part_weight = c.take<float>(wgs);
  s.part_rows = c.take<int32_t>(wgs);
  s.denom = c.take<float>(1);
  s.floats = c.cur / sizeof(float);
  return s;
}

__device__ __forceinline__ void publish(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void publish(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float fetch(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t fetch(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, int KPL>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int C, int lane, float (&z)[KPL]) {
#pragma unroll
  for (int k = 0; k < KPL; ++k) {
    const int c = lane + 64 * k;
    z[k] = c < C ? to_f32(row[c]) : -INFINITY;     // exp(-inf - m) = 0: the padding drops out of every sum
  }
}

// (1 - pt)^gamma and d/dce [(1 - pt)^gamma ce] for pt = exp(-ce); gamma is 0 or >= 1 (checked on the host)
__device__ __forceinline__ float focal_factor(float ce, float gamma) {
  if (gamma == 0.f) return 1.f;
  return powf(fmaxf(-expm1f(-ce), 0.f), gamma);
}
__device__ __forceinline__ float focal_slope(float ce, float gamma) {
  if (gamma == 0.f) return 1.f;
  const float omp = fmaxf(-expm1f(-ce), 0.f), pt = expf(-ce);
  return gamma * powf(omp, gamma - 1.f) * pt * ce + powf(omp, gamma);
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int KPL>
__global__ __launch_bounds__(NT) void criterion_forward_kernel(const T* __restrict__ logits, const void* __restrict__ targets,
                                                               const float* __restrict__ weight, int kind, int reduction,
                                                               float gamma, int B, int C, float* __restrict__ loss, Scratch sc,
                                                               int32_t* ticket, MeterBlock* meter, float* __restrict__ probs_out) {
  __shared__ float s_loss[WAVES], s_weight[WAVES];
  __shared__ int32_t s_rows[WAVES];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * ROWS_PER_WG, r1 = min(r0 + ROWS_PER_WG, B);
  const bool soft = kind == MMSKIN_CRITERION_SOFT;

  float acc_loss = 0.f, acc_weight = 0.f;
  int32_t acc_rows = 0;
  for (int r = r0 + wave; r < r1; r += WAVES) {                   // uniform per wave: the shuffles see all 64 lanes
    const T* zrow = logits + (int64_t)r * C;
    float z[KPL];
    load_row<T, KPL>(zrow, C, lane, z);
    float top = z[0];
    int arg = lane;
#pragma unroll
    for (int k = 1; k < KPL; ++k)
      if (z[k] > top) { top = z[k]; arg = lane + 64 * k; }        // ascending classes: the first maximum stays
    wave_argmax(top, arg);
    const float m = top;
    float e = 0.f;                                                 // every class but the arg-max, whose term is exactly 1:
#pragma unroll
    for (int k = 0; k < KPL; ++k) e += lane + 64 * k == arg ? 0.f : expf(z[k] - m);
    const float rest = wave_sum(e);                                // ln(1 + rest) keeps a confident row's tiny ce, which
    const float ls = log1pf(rest), sum = 1.f + rest;               // ln(fl(1 + rest)) rounds away

    float value, w;
    bool valid;
    int64_t y = 0;
    if (soft) {
      const float* trow = (const float*)targets + (int64_t)r * C;
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        const int c = lane + 64 * k;
        if (c < C) a += trow[c] * ((z[k] - m) - ls) * (weight ? weight[c] : 1.f);
      }
      value = -wave_sum(a);
      w = 1.f;
      valid = true;
    } else {
      y = ((const int64_t*)targets)[r];
      valid = y >= 0 && y < C;                                     // any other label (torch's ignore_index -100 included): no loss
      w = valid ? (weight ? weight[y] : 1.f) : 0.f;
      const float ce = valid ? ls - (to_f32(zrow[valid ? y : 0]) - m) : 0.f;
      value = valid ? w * ce : 0.f;
      if (kind == MMSKIN_CRITERION_FOCAL && gamma != 0.f) value = focal_factor(ce, gamma) * value;
    }
    if (probs_out) {
      const float inv = 1.f / sum;
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        const int c = lane + 64 * k;
        if (c < C) probs_out[(int64_t)r * C + c] = expf(z[k] - m) * inv;
      }
    }
    if (lane == 0) {
      sc.side[2 * (int64_t)r] = m;
      sc.side[2 * (int64_t)r + 1] = ls;
      if (reduction == MMSKIN_REDUCE_NONE) loss[r] = value;
      if (meter && !soft && valid) atomicAdd(&meter->confusion[y * C + arg], 1);
    }
    acc_loss += value;
    acc_weight += w;
    acc_rows += valid ? 1 : 0;
  }
  if (lane == 0) { s_loss[wave] = acc_loss; s_weight[wave] = acc_weight; s_rows[wave] = acc_rows; }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f, w = 0.f;
    int32_t n = 0;
    for (int i = 0; i < WAVES; ++i) { a += s_loss[i]; w += s_weight[i]; n += s_rows[i]; }
    publish(sc.part_loss + blockIdx.x, a);
    publish(sc.part_weight + blockIdx.x, w);
    publish(sc.part_rows + blockIdx.x, n);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");            // the partials are out before the ticket is drawn
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == (int)gridDim.x - 1;
    if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!s_last) return;

  // last workgroup: thread t takes partials t, t + NT, ...; waves by butterfly; the 16 wave sums in order
  float a = 0.f, w = 0.f;
  int32_t n = 0;
  for (int i = tid; i < (int)gridDim.x; i += NT) { a += fetch(sc.part_loss + i); w += fetch(sc.part_weight + i); n += fetch(sc.part_rows + i); }
  a = wave_sum(a);
  w = wave_sum(w);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  __syncthreads();                                                 // s_* were read by thread 0 above
  if (lane == 0) { s_loss[wave] = a; s_weight[wave] = w; s_rows[wave] = n; }
  __syncthreads();
  if (tid != 0) return;
  a = 0.f; w = 0.f; n = 0;
  for (int i = 0; i < WAVES; ++i) { a += s_loss[i]; w += s_weight[i]; n += s_rows[i]; }
  const float denom = kind == MMSKIN_CRITERION_CE ? w : (float)B;  // torch's weighted mean; the reference's plain .mean()
  *sc.denom = denom;
  if (reduction == MMSKIN_REDUCE_SUM) *loss = a;
  if (reduction == MMSKIN_REDUCE_MEAN) *loss = a / denom;          // all rows ignored: 0 / 0 = nan, as torch
  if (meter && n > 0) {
    // n times the batch's mean loss: the sum itself except under class weights, where torch's mean divides by their sum
    meter->loss_sum += kind == MMSKIN_CRITERION_CE ? (double)a / (double)w * (double)n : (double)a;
    meter->rows += n;
  }
  __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ backward
template <typename T, int KPL>
__global__ __launch_bounds__(NT) void criterion_backward_kernel(const T* __restrict__ logits, const void* __restrict__ targets,
                                                                const float* __restrict__ weight, int kind, int reduction,
                                                                float gamma, int B, int C, const float* __restrict__ dloss,
                                                                const float* __restrict__ side, const float* __restrict__ denom,
                                                                T* __restrict__ dlogits) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * ROWS_PER_WG, r1 = min(r0 + ROWS_PER_WG, B);
  const float scale = reduction == MMSKIN_REDUCE_MEAN ? denom[0] : 1.f;
  for (int r = r0 + wave; r < r1; r += WAVES) {
    const T* zrow = logits + (int64_t)r * C;
    T* drow = dlogits + (int64_t)r * C;
    float z[KPL];
    load_row<T, KPL>(zrow, C, lane, z);
    const float m = side[2 * (int64_t)r], ls = side[2 * (int64_t)r + 1];
    const float g = reduction == MMSKIN_REDUCE_NONE ? dloss[r] : dloss[0] / scale;
    if (kind == MMSKIN_CRITERION_SOFT) {
      const float* trow = (const float*)targets + (int64_t)r * C;
      float tw[KPL], a = 0.f;
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        const int c = lane + 64 * k;
        tw[k] = c < C ? trow[c] * (weight ? weight[c] : 1.f) : 0.f;
        a += tw[k];
      }
      const float total = wave_sum(a);
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        const int c = lane + 64 * k;
        if (c < C) drow[c] = from_f32<T>(g * (expf((z[k] - m) - ls) * total - tw[k]));
      }
      continue;
    }
    const int64_t y = ((const int64_t*)targets)[r];
    const bool valid = y >= 0 && y < C;
    float coef = 0.f;
    if (valid) {
      coef = g * (weight ? weight[y] : 1.f);
      if (kind == MMSKIN_CRITERION_FOCAL) coef *= focal_slope(ls - (to_f32(zrow[y]) - m), gamma);
    }
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
      const int c = lane + 64 * k;
      if (c < C) drow[c] = from_f32<T>(valid ? coef * (expf((z[k] - m) - ls) - (c == y ? 1.f : 0.f)) : 0.f);   // an ignored row: zeros, whatever g is
    }
  }
}

int check_shape(const char* fn, int dtype, int kind, int reduction, float gamma, int B, int C) {
  ARG_CHECK(B >= 1 && B <= MAX_B, "%s: batch %d is outside 1 .. %d", fn, B, MAX_B);
  ARG_CHECK(C >= 2 && C <= MAX_C, "%s: %d classes; the kernel holds 2 .. %d", fn, C, MAX_C);
  ARG_CHECK(dtype == 0 || dtype == 1, "%s: logits dtype %d is neither fp32 (0) nor bf16 (1)", fn, dtype);
  ARG_CHECK(kind == MMSKIN_CRITERION_CE || kind == MMSKIN_CRITERION_FOCAL || kind == MMSKIN_CRITERION_SOFT, "%s: unknown kind %d", fn, kind);
  ARG_CHECK(reduction == MMSKIN_REDUCE_NONE || reduction == MMSKIN_REDUCE_SUM || reduction == MMSKIN_REDUCE_MEAN, "%s: unknown reduction %d", fn,
            reduction);
  ARG_CHECK(kind != MMSKIN_CRITERION_SOFT || reduction == MMSKIN_REDUCE_MEAN, "%s: the soft-target criterion reduces by `mean` only, as the "
            "reference (got reduction %d)", fn, reduction);
  ARG_CHECK(kind != MMSKIN_CRITERION_FOCAL || gamma == 0.f || gamma >= 1.f, "%s: focal gamma %g; 0 or >= 1 only (the derivative is unbounded at "
            "pt = 1 for 0 < gamma < 1)", fn, (double)gamma);
  return MMSKIN_OK;
}

}  // namespace

extern "C" int64_t mmskin_criterion_scratch_floats(int B, int C, int kind) {
  if (B < 1 || B > MAX_B || C < 2 || C > MAX_C || kind < MMSKIN_CRITERION_CE || kind > MMSKIN_CRITERION_SOFT) return -1;
  return (int64_t)carve_scratch(nullptr, B).floats;
}

extern "C" int mmskin_criterion_forward(const void* logits, int logits_dtype, const void* targets, const float* weight, int kind, int reduction,
                                        float gamma, int B, int C, float* loss, float* scratch, int32_t* ticket, void* meter, float* probs_out,
                                        void* stream) {
  if (int rc = check_shape("criterion_forward", logits_dtype, kind, reduction, gamma, B, C)) return rc;
  ARG_CHECK(logits && targets && loss && scratch && ticket, "criterion_forward: null argument");
  const Scratch sc = carve_scratch(scratch, B);
  const dim3 grid(ceil_div(B, ROWS_PER_WG));
#define LAUNCH(T, KPL)                                                                                                                      \
  hipLaunchKernelGGL((criterion_forward_kernel<T, KPL>), grid, dim3(NT), 0, ST(stream), (const T*)logits, targets, weight, kind, reduction, \
                     gamma, B, C, loss, sc, ticket, (MeterBlock*)meter, probs_out)
  if (logits_dtype == 1) { if (C <= 64) LAUNCH(bf16_t, 1); else LAUNCH(bf16_t, 16); }
  else { if (C <= 64) LAUNCH(float, 1); else LAUNCH(float, 16); }
#undef LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_criterion_backward(const void* logits, int logits_dtype, const void* targets, const float* weight, int kind, int reduction,
                                         float gamma, int B, int C, const float* dloss, const float* scratch, void* dlogits, void* stream) {
  if (int rc = check_shape("criterion_backward", logits_dtype, kind, reduction, gamma, B, C)) return rc;
  ARG_CHECK(logits && targets && dloss && scratch && dlogits, "criterion_backward: null argument");
  const Scratch sc = carve_scratch(const_cast<float*>(scratch), B);
  const dim3 grid(ceil_div(B, ROWS_PER_WG));
#define LAUNCH(T, KPL)                                                                                                                       \
  hipLaunchKernelGGL((criterion_backward_kernel<T, KPL>), grid, dim3(NT), 0, ST(stream), (const T*)logits, targets, weight, kind, reduction, \
                     gamma, B, C, dloss, (const float*)sc.side, (const float*)sc.denom, (T*)dlogits)
  if (logits_dtype == 1) { if (C <= 64) LAUNCH(bf16_t, 1); else LAUNCH(bf16_t, 16); }
  else { if (C <= 64) LAUNCH(float, 1); else LAUNCH(float, 16); }
#undef LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
