// Metadata-sensitivity sweeps (interpretability/flip_rate.py:164-256, inference_all_folds.py:116-140,
// analyze_prediction_uncertainty.py:166-272) without their per-row host loops: the two kernels on either side of the batched
// fusion-head calls that mmskin.sweep.MetadataSweep drives.
//
//   variants   codes + raw numerics + a table of V one-column mutations (+ an optional missing mask) -> the V encoded metadata
//              batches [V][B][out_width], i.e. mutate_metadata / simulate_missing_metadata, OneHotEncoder, fillna(-1),
//              StandardScaler and the pad-or-cut to the checkpoint's vocab_size in one pass.  One thread per output element,
//              every element written exactly once, no atomics.  The cell is meta_encode.h's, the one metadata_encode_kernel
//              (preprocess.hip) calls, so an unmutated, unmasked variant equals its output bit for bit.
//   reduce     logits [V][B][C] + baseline logits [B][C] (+ labels) -> soft-max, prediction, top-2 margin, entropy / KL / JS /
//              confidence change per (v, b), and the flip / transition / confusion COUNTS added to the caller's counters.
//              One wave per (v, b) row, one lane per class (C <= 64); a workgroup serves one variant, counts into an LDS
//              histogram and adds every non-zero cell to global memory once.  Integer adds: the counters do not depend on the
//              order in which workgroups finish.
//
// tests/sweep_oracle.py restates both in numpy; the variants kernel matches it bit for bit, the reduce kernel exactly in its
// integer outputs and in the margin.
#include "../../include/mmskin.h"
#include "common.h"
#include "meta_encode.h"

#pragma clang fp contract(off)

namespace {

static_assert(sizeof(mmskin_meta_variant) == 32, "table record layout is part of the ABI (include/mmskin.h)");

constexpr int NT = 256;                  // threads per workgroup
constexpr int MAX_C = 64;                // reduce: one lane per class
constexpr int ROWS_PER_WG = 64;          // reduce: rows of one variant per workgroup (16 per wave)

// ------------------------------------------------------------------------------------------------ variants
__global__ __launch_bounds__(NT) void metadata_variants_kernel(const int32_t* __restrict__ codes, int n_cat,
                                                               const int32_t* __restrict__ col_offset, int onehot_width,
                                                               const float* __restrict__ numeric, int n_num,
                                                               const float* __restrict__ mean, const float* __restrict__ scale,
                                                               float nan_fill, const mmskin_meta_variant* __restrict__ table,
                                                               const uint8_t* __restrict__ mask,
                                                               const int32_t* __restrict__ missing_code, int V, int B,
                                                               int out_width, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  if (i >= (int64_t)V * B * out_width) return;
  const int j = (int)(i % out_width);
  const int64_t vb = i / out_width;
  const int b = (int)(vb % B), v = (int)(vb / B);
  const int n_col = n_cat + n_num;
  float r = 0.f;                                                 // columns past the encoder's width
  if (j < onehot_width) {
    const int col = meta_slot_column(j, n_cat, col_offset);
    int code = codes[(int64_t)b * n_cat + col];
    const mmskin_meta_variant rec = table[v];
    if (rec.column == col) {
      if (rec.op == MMSKIN_META_CAT_SET) code = rec.a;
      else if (rec.op == MMSKIN_META_CAT_TOGGLE) code = code == rec.a ? rec.b : rec.a;
    }
    if (mask && mask[vb * n_col + col]) code = missing_code[col];
    r = meta_onehot_cell(code, j, col_offset[col]);
  } else if (j < onehot_width + n_num) {
    const int k = j - onehot_width;
    float x = numeric[(int64_t)b * n_num + k];
    const mmskin_meta_variant rec = table[v];
    if (rec.column == n_cat + k) {
      if (rec.op == MMSKIN_META_NUM_ADD) x = x + rec.value;      // NaN stays NaN and is filled by the cell
      else if (rec.op == MMSKIN_META_NUM_SET) x = rec.value;
    }
    if (mask && mask[vb * n_col + n_cat + k]) x = nan_fill;
    r = meta_numeric_cell(x, mean[k], scale[k], nan_fill);
  }
  out[i] = r;
}

// ------------------------------------------------------------------------------------------------ reduce
// what one row of logits gives: lane c holds class c (lanes >= C hold nothing)
struct Row {
  float p;        // soft-max probability: exp(x - max) / sum, as torch.softmax
  float q;        // safe_probs: clip(p, 1e-12, 1) / sum of the clipped
  int pred;       // first index of the maximum logit
  float margin;   // top-1 minus top-2 logit
};
__device__ __forceinline__ Row row_stats(float x, int lane, int C) {
  const bool live = lane < C;
  Row r;
  float top = live ? x : -INFINITY;
  r.pred = live ? lane : MAX_C + lane;
  wave_argmax(top, r.pred);
  const float second = wave_max(live && lane != r.pred ? x : -INFINITY);
  r.margin = top - second;
  const float e = live ? expf(x - top) : 0.f;
  r.p = e / wave_sum(e);
  const float clipped = live ? fminf(fmaxf(r.p, 1e-12f), 1.f) : 0.f;
  r.q = clipped / wave_sum(clipped);
  return r;
}

template <typename T>
__global__ __launch_bounds__(NT) void sweep_reduce_kernel(const T* __restrict__ logits, const float* __restrict__ base,
                                                          const int32_t* __restrict__ labels, int V, int B, int C,
                                                          float* __restrict__ probs, int32_t* __restrict__ pred,
                                                          float* __restrict__ margin, float* __restrict__ stats,
                                                          int32_t* __restrict__ flips, int32_t* __restrict__ transitions,
                                                          int32_t* __restrict__ confusion) {
  __shared__ int32_t h_trans[MAX_C * MAX_C];
  __shared__ int32_t h_conf[MAX_C * MAX_C];
  __shared__ int32_t h_flips;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = blockIdx.y, b0 = blockIdx.x * ROWS_PER_WG, b1 = min(b0 + ROWS_PER_WG, B);
  const int CC = C * C;
  for (int i = tid; i < CC; i += NT) { h_trans[i] = 0; h_conf[i] = 0; }
  if (tid == 0) h_flips = 0;
  __syncthreads();

  const bool live = lane < C;
  for (int b = b0 + wave; b < b1; b += NT / 64) {          // uniform per wave: the shuffles below see all 64 lanes
    const int64_t row = (int64_t)v * B + b;
    const Row cur = row_stats(live ? to_f32(logits[row * C + lane]) : 0.f, lane, C);
    const Row ref = row_stats(live ? base[(int64_t)b * C + lane] : 0.f, lane, C);
    // entropy, KL(variant || base), JS(variant, base) on the safe probabilities (analyze_prediction_uncertainty.py:172-189)
    const float m = 0.5f * (cur.q + ref.q);
    const float ent = -wave_sum(live ? cur.q * logf(cur.q) : 0.f);
    const float kl = wave_sum(live ? cur.q * logf(cur.q / ref.q) : 0.f);
    const float kl_cm = wave_sum(live ? cur.q * logf(cur.q / m) : 0.f);
    const float kl_rm = wave_sum(live ? ref.q * logf(ref.q / m) : 0.f);
    const float js = 0.5f * kl_cm + 0.5f * kl_rm;
    const float dconf = __shfl(cur.q, ref.pred, 64) - __shfl(ref.q, ref.pred, 64);
    if (probs && live) probs[row * C + lane] = cur.p;
    if (lane == 0) {
      pred[row] = cur.pred;
      margin[row] = cur.margin;
      stats[row * 4 + 0] = ent;
      stats[row * 4 + 1] = kl;
      stats[row * 4 + 2] = js;
      stats[row * 4 + 3] = dconf;
      atomicAdd(&h_trans[ref.pred * C + cur.pred], 1);
      if (cur.pred != ref.pred) atomicAdd(&h_flips, 1);
      if (labels) {
        const int lab = labels[b];
        if (lab >= 0 && lab < C) atomicAdd(&h_conf[lab * C + cur.pred], 1);   // a label outside [0, C) counts nowhere
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < CC; i += NT) {
    const int t = h_trans[i];
    if (t) atomicAdd(&transitions[(int64_t)v * CC + i], t);
    if (labels) {
      const int c = h_conf[i];
      if (c) atomicAdd(&confusion[(int64_t)v * CC + i], c);
    }
  }
  if (tid == 0 && h_flips) atomicAdd(&flips[v], h_flips);
}

}  // namespace

extern "C" int mmskin_metadata_variants(const int32_t* codes, int n_cat, const int32_t* col_offset, const int32_t* col_offset_host,
                                        int onehot_width, const float* numeric, int n_num, const float* mean, const float* scale,
                                        float nan_fill, const mmskin_meta_variant* variants_host, mmskin_meta_variant* variants_scratch,
                                        int V, const uint8_t* mask, const int32_t* missing_code, float* out, int batch, int out_width,
                                        void* stream) {
  ARG_CHECK(V >= 1 && batch >= 1 && out_width >= 1, "metadata_variants: every extent must be >= 1 (V %d, batch %d, out_width %d)", V, batch,
            out_width);
  if (int rc = check_meta_layout("metadata_variants", n_cat, n_num, onehot_width, col_offset, col_offset_host)) return rc;
  ARG_CHECK((int64_t)V * batch * out_width < ((int64_t)1 << 40) && V <= (1 << 20), "metadata_variants: %d x %d x %d is out of range", V, batch,
            out_width);
  ARG_CHECK(out && variants_host && variants_scratch && (codes || n_cat == 0) && (n_num == 0 || (numeric && mean && scale)) &&
                (!mask || missing_code || n_cat == 0),
            "metadata_variants: null argument");
  for (int v = 0; v < V; ++v) {
    const mmskin_meta_variant& r = variants_host[v];
    if (r.op == MMSKIN_META_NONE) continue;
    ARG_CHECK(r.op == MMSKIN_META_CAT_SET || r.op == MMSKIN_META_CAT_TOGGLE || r.op == MMSKIN_META_NUM_ADD || r.op == MMSKIN_META_NUM_SET,
              "metadata_variants: variant %d: unknown op %d", v, r.op);
    ARG_CHECK(r.column >= 0 && r.column < n_cat + n_num, "metadata_variants: variant %d: column %d is outside the %d columns", v, r.column,
              n_cat + n_num);
    const bool cat_op = r.op == MMSKIN_META_CAT_SET || r.op == MMSKIN_META_CAT_TOGGLE;
    ARG_CHECK(cat_op == (r.column < n_cat), "metadata_variants: variant %d: a %s op on %s column %d", v, cat_op ? "categorical" : "numeric",
              r.column < n_cat ? "categorical" : "numeric", r.column);
    if (cat_op) {
      const int count = col_offset_host[r.column + 1] - col_offset_host[r.column];
      ARG_CHECK(r.a >= -1 && r.a < count && (r.op == MMSKIN_META_CAT_SET || (r.b >= -1 && r.b < count)),
                "metadata_variants: variant %d: code %d / %d outside the %d categories of column %d", v, r.a, r.b, count, r.column);
    }
  }
  // the kernel reads the bytes that were just validated: the upload is part of the call (pageable host memory: the copy has
  // left the host buffer when hipMemcpyAsync returns)
  HIP_CHECK_RET(hipMemcpyAsync(variants_scratch, variants_host, (size_t)V * sizeof(mmskin_meta_variant), hipMemcpyHostToDevice, ST(stream)));
  const int64_t total = (int64_t)V * batch * out_width;
  hipLaunchKernelGGL(metadata_variants_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), codes, n_cat, col_offset,
                     onehot_width, numeric, n_num, mean, scale, nan_fill, variants_scratch, mask, missing_code, V, batch, out_width, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_sweep_reduce(const void* logits, int logits_dtype, const float* base, const int32_t* labels, int V, int batch, int C,
                                   float* probs, int32_t* pred, float* margin, float* stats, int32_t* flips, int32_t* transitions,
                                   int32_t* confusion, void* stream) {
  ARG_CHECK(V >= 1 && batch >= 1, "sweep_reduce: every extent must be >= 1 (V %d, batch %d)", V, batch);
  if (C < 2 || C > MAX_C) {
    mmskin_set_error("sweep_reduce: %d classes; the kernel holds one class per lane, 2 .. %d", C, MAX_C);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  ARG_CHECK(V <= 65535 && (int64_t)V * batch < ((int64_t)1 << 31), "sweep_reduce: %d x %d rows are out of range", V, batch);
  ARG_CHECK(logits_dtype == 0 || logits_dtype == 1, "sweep_reduce: logits dtype %d is neither fp32 (0) nor bf16 (1)", logits_dtype);
  ARG_CHECK(logits && base && pred && margin && stats && flips && transitions && (confusion || !labels), "sweep_reduce: null argument");
  const dim3 grid(ceil_div(batch, ROWS_PER_WG), V);
  if (logits_dtype == 1)
    hipLaunchKernelGGL(sweep_reduce_kernel<bf16_t>, grid, dim3(NT), 0, ST(stream), (const bf16_t*)logits, base, labels, V, batch, C, probs, pred,
                       margin, stats, flips, transitions, confusion);
  else
    hipLaunchKernelGGL(sweep_reduce_kernel<float>, grid, dim3(NT), 0, ST(stream), (const float*)logits, base, labels, V, batch, C, probs, pred,
                       margin, stats, flips, transitions, confusion);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
