// Permutation importance of the metadata on a validation fold (mmskin.permutation.MetadataPermutationImportance): the kernels on
// either side of the batched fusion-head calls.  Breiman's measure, as sklearn.inspection.permutation_importance states it: for
// repeat r and feature group g the columns of g are shuffled among the S samples of the fold, the fold is scored again, and the
// importance is the drop of the score against the unshuffled fold.  The image is encoded once; only the head runs R x G times.
//
// Groups are sets of ENCODED columns (a one-hot block is one group): group[j] = the group of column j, or -1 for a column that is
// never shuffled.  A shuffled row copies whole encoded columns of another sample, so it is bit for bit the encoding of the mixed
// raw row.  Row order of the study: row = (r G + g) S + s, a CELL (r, g) is S consecutive rows.
//
// The generator (counter based, no state): h = mix64(mix64(seed) ^ (r << 40 | g << 20 | i)) with common.h's splitmix finaliser,
// key_i = (h >> 32) << 32 | i, and perm[r][g][.] = the positions i in ascending order of key_i (the keys are distinct: the position
// is part of the key).  It depends on (seed, r, g, S) only.
//
//   indices   one workgroup per cell: the S keys, padded with all-ones to a power of two, in LDS; a bitonic sort; the low words out.
//   rows      x fp32 [S][stride] + the map + the table -> the rows of any range [row0, row1): column j of row (r, g, s) is
//             x[perm[r][g][s]][j] if group[j] == g, else x[s][j].  One thread per 16 bytes where width, stride and the pointers
//             allow (two 16-byte loads, a select, one 16-byte store), one per element otherwise.  Every element is written once.
//   scores    one workgroup per cell, whole cells only.  Per row: p = soft-max in fp32 (e = exp(x - max) taken in fp64 and rounded,
//             summed over c = 0 .. K-1, e / sum), the prediction = the first arg-max of the logits.  Pass 1 leaves the row's own
//             score p[i][y_i], its label and prediction in LDS; pass 2 stages the soft-max of a tile of rows j with all K columns
//             and lets the thread that owns row i count auc_wins2(p[i][y_i], p[j][y_i]) over the j with another label (auc.hip's
//             pair rule and column choice: N^2 compares); pass 3 sums per class and counts the confusion cells, one thread per
//             cell, by walking the rows.  Integers only, and no atomics: each sum has one owner.
//   finalize  one thread per cell: accuracy, balanced accuracy (mean recall over the classes that occur) and macro one-vs-rest AUC
//             (mean over the classes that have a positive and a negative row; NaN if none or if a probability was NaN) in fp64,
//             and the drop against the baseline; then one thread per (metric, group): mean and deviation (ddof = 0) over r, in order.
//
// tests/permutation_oracle.py restates all of it in numpy.
#include "../../include/mmskin.h"
#include "auc_pairs.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int MAX_S = MMSKIN_PERMUTATION_MAX_SAMPLES;   // 4096: the sort's keys are 32 KiB of LDS, the scores' row state 32 KiB
constexpr int MAX_K = 64;                // classes: label and prediction of a row are one byte each
constexpr int TILE_FLOATS = 4096;        // 16 KiB of staged probabilities: 64 rows at K = 64
constexpr int NO_LABEL = 0xFF;

// ------------------------------------------------------------------------------------------------ indices
__global__ __launch_bounds__(NT) void permutation_indices_kernel(uint64_t key, int G, int S, int n, int32_t* __restrict__ perm) {
  __shared__ uint64_t keys[MAX_S];
  const int tid = threadIdx.x;
  const uint64_t cell = blockIdx.x, r = cell / G, g = cell - r * G;
  for (int i = tid; i < n; i += NT) {
    const uint64_t h = mix64(key ^ ((r << 40) | (g << 20) | (uint64_t)i));
    keys[i] = i < S ? ((h >> 32) << 32) | (uint64_t)i : ~0ull;     // the padding sorts last: no key has an all-ones position
  }
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += NT) {
        const int o = i ^ j;                                       // o < n: n is a power of two and j < n
        if (o > i) {
          const uint64_t a = keys[i], b = keys[o];
          if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[o] = a; }
        }
      }
    }
  __syncthreads();
  for (int i = tid; i < S; i += NT) perm[cell * S + i] = (int32_t)(uint32_t)keys[i];
}

// ------------------------------------------------------------------------------------------------ rows
// the sample whose row supplies group g's columns of row (cell, s); a table entry outside 0 .. S-1 reads the sample's own row
__device__ __forceinline__ int source_row(const int32_t* __restrict__ perm, int64_t cell, int s, int S) {
  const int p = perm[cell * S + s];
  return (unsigned)p < (unsigned)S ? p : s;
}

__global__ __launch_bounds__(NT) void permuted_rows_vec4_kernel(const float* __restrict__ x, int x_stride, const int32_t* __restrict__ group,
                                                                const int32_t* __restrict__ perm, int G, int S, int64_t row0,
                                                                int64_t n_rows, int width, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  const int chunks = width >> 2;
  if (i >= n_rows * chunks) return;
  const int q = (int)(i % chunks);
  const int64_t row = row0 + i / chunks, cell = row / S;
  const int s = (int)(row - cell * S), g = (int)(cell % G);
  const int4 m = *reinterpret_cast<const int4*>(group + 4 * q);
  float4 v = *reinterpret_cast<const float4*>(x + (int64_t)s * x_stride + 4 * q);
  if (m.x == g || m.y == g || m.z == g || m.w == g) {
    const float4 o = *reinterpret_cast<const float4*>(x + (int64_t)source_row(perm, cell, s, S) * x_stride + 4 * q);
    v.x = m.x == g ? o.x : v.x;
    v.y = m.y == g ? o.y : v.y;
    v.z = m.z == g ? o.z : v.z;
    v.w = m.w == g ? o.w : v.w;
  }
  *reinterpret_cast<float4*>(out + 4 * i) = v;
}

__global__ __launch_bounds__(NT) void permuted_rows_scalar_kernel(const float* __restrict__ x, int x_stride, const int32_t* __restrict__ group,
                                                                  const int32_t* __restrict__ perm, int G, int S, int64_t row0,
                                                                  int64_t n_rows, int width, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  if (i >= n_rows * width) return;
  const int j = (int)(i % width);
  const int64_t row = row0 + i / width, cell = row / S;
  const int s = (int)(row - cell * S), g = (int)(cell % G);
  const int src = group[j] == g ? source_row(perm, cell, s, S) : s;
  out[i] = x[(int64_t)src * x_stride + j];
}

// ------------------------------------------------------------------------------------------------ scores
// the row's soft-max pieces: top = max, e_c = (float)exp((double)(x_c - top)) summed over c = 0 .. K-1 in fp32; returns the sum
__device__ __forceinline__ float softmax_sum(const float* __restrict__ row, int K, float* top_out) {
  float top = -INFINITY, sum = 0.f;
  for (int c = 0; c < K; ++c) top = fmaxf(top, row[c]);
  for (int c = 0; c < K; ++c) sum += (float)exp((double)(row[c] - top));
  *top_out = top;
  return sum;
}

__global__ __launch_bounds__(NT) void permutation_scores_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int S,
                                                                int K, int TJ, int64_t cell0, int32_t* __restrict__ confusion,
                                                                int64_t* __restrict__ counts) {
  __shared__ float s_tile[TILE_FLOATS];
  __shared__ float s_own[MAX_S];           // p[i][y_i]
  __shared__ uint16_t s_yp[MAX_S];         // label (NO_LABEL: outside [0, K)) | prediction << 8
  __shared__ uint16_t s_wins[MAX_S];       // <= 2 S = 8192
  __shared__ int32_t s_nan[NT / 64];
  const int tid = threadIdx.x;
  const float* cell_logits = logits + (int64_t)blockIdx.x * S * K;
  const int64_t cell = cell0 + blockIdx.x;

  int32_t nans = 0;
  for (int i = tid; i < S; i += NT) {
    const float* row = cell_logits + (int64_t)i * K;
    const int64_t y = labels[i];
    const bool valid = y >= 0 && y < K;
    float top;
    const float sum = softmax_sum(row, K, &top);
    int pred = 0;
    float best = row[0];
    for (int c = 1; c < K; ++c)
      if (row[c] > best || best != best) { best = row[c]; pred = c; }        // the first arg-max; a NaN never wins
    float own = 0.f;
    if (valid) {
      own = (float)exp((double)(row[y] - top)) / sum;
      for (int c = 0; c < K; ++c) {
        const float p = (float)exp((double)(row[c] - top)) / sum;
        nans += p != p;
      }
    }
    s_own[i] = own;
    s_yp[i] = (uint16_t)((valid ? (int)y : NO_LABEL) | (pred << 8));
    s_wins[i] = 0;
  }

  for (int j0 = 0; j0 < S; j0 += TJ) {
    const int rows = min(TJ, S - j0);
    __syncthreads();                                               // the last tile is consumed (first pass: pass 1 is complete)
    for (int r = tid; r < rows; r += NT) {
      const float* row = cell_logits + (int64_t)(j0 + r) * K;
      float top;
      const float sum = softmax_sum(row, K, &top);
      for (int c = 0; c < K; ++c) s_tile[r * K + c] = (float)exp((double)(row[c] - top)) / sum;   // r < TJ: inside TJ * K <= TILE_FLOATS
    }
    __syncthreads();
    for (int i = tid; i < S; i += NT) {
      const int yi = s_yp[i] & 0xFF;
      if (yi == NO_LABEL) continue;
      const float si = s_own[i];
      int32_t a = 0;
      for (int r = 0; r < rows; ++r) {
        const int yj = s_yp[j0 + r] & 0xFF;
        const int32_t w = auc_wins2(si, s_tile[r * K + yi]);
        a += (yj != NO_LABEL && yj != yi) ? w : 0;
      }
      s_wins[i] = (uint16_t)(s_wins[i] + a);                       // row i has one owner
    }
  }

  for (int o = 32; o > 0; o >>= 1) nans += __shfl_xor(nans, o, 64);
  if ((tid & 63) == 0) s_nan[tid >> 6] = nans;
  __syncthreads();

  int64_t* cnt = counts + cell * (3 * K + 1);
  if (tid < K) {
    int64_t pos = 0, valid = 0, wins = 0;
    for (int i = 0; i < S; ++i) {
      const int y = s_yp[i] & 0xFF;
      valid += y != NO_LABEL;
      if (y == tid) { ++pos; wins += s_wins[i]; }
    }
    cnt[tid] = pos;
    cnt[K + tid] = valid - pos;
    cnt[2 * K + tid] = wins;
  }
  if (tid == NT - 1) {
    int64_t n = 0;
    for (int w = 0; w < NT / 64; ++w) n += s_nan[w];
    cnt[3 * K] = n;
  }
  int32_t* conf = confusion + cell * K * K;
  for (int e = tid; e < K * K; e += NT) {
    const uint16_t want = (uint16_t)((e / K) | ((e % K) << 8));
    int32_t n = 0;
    for (int i = 0; i < S; ++i) n += s_yp[i] == want;
    conf[e] = n;
  }
}

// ------------------------------------------------------------------------------------------------ finalize
__global__ __launch_bounds__(NT) void permutation_metrics_kernel(const int32_t* __restrict__ confusion, const int64_t* __restrict__ counts,
                                                                 const double* __restrict__ baseline, int R, int G, int K,
                                                                 double* __restrict__ metrics, double* __restrict__ importances) {
  const int cell = blockIdx.x * NT + threadIdx.x;
  if (cell >= R * G) return;
  const int r = cell / G, g = cell - r * G;
  const int32_t* cm = confusion + (int64_t)cell * K * K;
  const int64_t* cnt = counts + (int64_t)cell * (3 * K + 1);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int64_t n = 0, hits = 0;
  double recall_sum = 0.0;
  int present = 0;
  for (int a = 0; a < K; ++a) {
    int64_t true_n = 0;
    for (int b = 0; b < K; ++b) true_n += cm[a * K + b];
    n += true_n;
    hits += cm[a * K + a];
    if (true_n > 0) {
      recall_sum += (double)cm[a * K + a] / (double)true_n;
      ++present;
    }
  }
  double auc_sum = 0.0;
  int ranked = 0;
  for (int c = 0; c < K; ++c) {
    const double pairs = 2.0 * (double)cnt[c] * (double)cnt[K + c];
    if (pairs > 0.0) {
      auc_sum += (double)cnt[2 * K + c] / pairs;
      ++ranked;
    }
  }
  const double m[3] = {n > 0 ? (double)hits / (double)n : nan, present > 0 ? recall_sum / (double)present : nan,
                       (ranked > 0 && cnt[3 * K] == 0) ? auc_sum / (double)ranked : nan};
  for (int k = 0; k < 3; ++k) {
    const int64_t at = ((int64_t)k * G + g) * R + r;
    metrics[at] = m[k];
    importances[at] = baseline[k] - m[k];
  }
}

__global__ __launch_bounds__(NT) void permutation_stats_kernel(const double* __restrict__ importances, int R, int n, double* __restrict__ mean,
                                                               double* __restrict__ std) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const double* v = importances + (int64_t)i * R;
  double sum = 0.0;
  for (int r = 0; r < R; ++r) sum += v[r];
  const double mu = sum / (double)R;
  double sq = 0.0;
  for (int r = 0; r < R; ++r) sq += (v[r] - mu) * (v[r] - mu);
  mean[i] = mu;
  std[i] = sqrt(sq / (double)R);
}

// ------------------------------------------------------------------------------------------------ host
// the study's extents, checked once for every entry point; `what` names the caller in the message
int study_extents(const char* what, int R, int G, int S) {
  ARG_CHECK(R >= 1 && G >= 1 && S >= 1, "%s: every extent must be >= 1 (R %d, G %d, S %d)", what, R, G, S);
  ARG_CHECK(R <= (1 << 20) && G <= (1 << 20) && (int64_t)R * G <= (1 << 24), "%s: %d repeats of %d groups are out of range", what, R, G);
  ARG_CHECK(S <= MAX_S, "%s: %d samples; a cell is sorted and scored in LDS, which holds at most %d", what, S, MAX_S);
  return MMSKIN_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mmskin_permutation_indices(uint64_t seed, int R, int G, int S, int32_t* perm, void* stream) {
  if (int rc = study_extents("permutation_indices", R, G, S)) return rc;
  ARG_CHECK(perm, "permutation_indices: null argument");
  int n = 2;
  while (n < S) n <<= 1;
  hipLaunchKernelGGL(permutation_indices_kernel, dim3((unsigned)(R * G)), dim3(NT), 0, ST(stream), mix64(seed), G, S, n, perm);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_permuted_rows(const float* x, int x_stride, const int32_t* group, const int32_t* perm, int R, int G, int S, int width,
                                    int64_t row0, int64_t row1, float* out, void* stream) {
  if (int rc = study_extents("permuted_rows", R, G, S)) return rc;
  ARG_CHECK(width >= 1 && width <= (1 << 20) && x_stride >= width, "permuted_rows: width %d with a row stride of %d is out of range", width,
            x_stride);
  const int64_t rows = (int64_t)R * G * S;
  ARG_CHECK(row0 >= 0 && row0 < row1 && row1 <= rows, "permuted_rows: rows [%lld, %lld) are not a range of the study's %lld rows",
            (long long)row0, (long long)row1, (long long)rows);
  ARG_CHECK((row1 - row0) * width < ((int64_t)1 << 38), "permuted_rows: %lld rows x %d are out of range", (long long)(row1 - row0), width);
  ARG_CHECK(x && group && perm && out, "permuted_rows: null argument");
  const int64_t n_rows = row1 - row0;
  if (width % 4 == 0 && x_stride % 4 == 0 && aligned16(x) && aligned16(group) && aligned16(out)) {
    const int64_t total = n_rows * (width / 4);
    hipLaunchKernelGGL(permuted_rows_vec4_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), x, x_stride, group, perm, G,
                       S, row0, n_rows, width, out);
  } else {
    const int64_t total = n_rows * width;
    hipLaunchKernelGGL(permuted_rows_scalar_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), x, x_stride, group, perm,
                       G, S, row0, n_rows, width, out);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_permutation_scores(const float* logits, const int64_t* labels, int R, int G, int S, int K, int64_t row0, int64_t row1,
                                         int32_t* confusion, int64_t* counts, void* stream) {
  if (int rc = study_extents("permutation_scores", R, G, S)) return rc;
  if (K < 2 || K > MAX_K) {
    mmskin_set_error("permutation_scores: %d classes; the kernel holds a label in one byte, 2 .. %d", K, MAX_K);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  const int64_t rows = (int64_t)R * G * S;
  ARG_CHECK(row0 >= 0 && row0 <= row1 && row1 <= rows, "permutation_scores: rows [%lld, %lld) are not a range of the study's %lld rows",
            (long long)row0, (long long)row1, (long long)rows);
  ARG_CHECK(row0 % S == 0 && row1 % S == 0, "permutation_scores: rows [%lld, %lld) split a cell: cut the study at multiples of S = %d",
            (long long)row0, (long long)row1, S);
  ARG_CHECK(labels && confusion && counts && (logits || row0 == row1), "permutation_scores: null argument");
  if (row0 == row1) return MMSKIN_OK;
  hipLaunchKernelGGL(permutation_scores_kernel, dim3((unsigned)((row1 - row0) / S)), dim3(NT), 0, ST(stream), logits, labels, S, K, TILE_FLOATS / K,
                     row0 / S, confusion, counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_permutation_finalize(const int32_t* confusion, const int64_t* counts, const double* baseline, int R, int G, int K,
                                           double* metrics, double* importances, double* mean, double* std, void* stream) {
  if (int rc = study_extents("permutation_finalize", R, G, 1)) return rc;
  if (K < 2 || K > MAX_K) {
    mmskin_set_error("permutation_finalize: %d classes; the kernels hold 2 .. %d", K, MAX_K);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  ARG_CHECK(confusion && counts && baseline && metrics && importances && mean && std, "permutation_finalize: null argument");
  hipLaunchKernelGGL(permutation_metrics_kernel, dim3(ceil_div(R * G, NT)), dim3(NT), 0, ST(stream), confusion, counts, baseline, R, G, K,
                     metrics, importances);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(permutation_stats_kernel, dim3(ceil_div(3 * G, NT)), dim3(NT), 0, ST(stream), importances, R, 3 * G, mean, std);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
