// Calibration of a fold's probabilities (mmskin.calibration): reliability tables as exact integers, the Brier and NLL sums, the
// metric columns with their bootstrap summary, and the sufficient statistics of temperature scaling.  The contract is in
// include/mmskin.h; tests/calibration_oracle.py restates all of it in numpy.
//
//   codes      the per-fold pass.  A workgroup takes 64 rows: their K probabilities go to LDS by coalesced loads (the tile is one
//              contiguous run of memory, whatever K is), 64 threads find the rows' first arg-max, then the (table, row) pairs are
//              dealt so that a wave holds one table and 64 consecutive rows: the stores to bin / q / hit [K + 1][N] are coalesced
//              along N and the edges of the table are read from LDS at one address per wave (a broadcast).
//   bins       one workgroup per (replicate, tile of tables).  A tile holds at most CELLS = 2048 (table, bin) cells of 16 bytes:
//              32 KiB of LDS, so K = 64 with 64 bins takes three tiles, not the 100 KiB the whole replicate would.  A thread loads
//              the weight of its row once and walks the tile's tables; per (row, table) with w > 0 it issues two 64-bit LDS atomic
//              adds: w | (w hit) << 32 (count and hits in one cell: both stay below 2^31, so no carry crosses) and w q.  After a
//              barrier the slice is written once.  Unweighted: the rows are cut over blockIdx.z too and the cells are flushed with
//              64-bit integer global atomics into the slice the entry has zeroed.
//   sums       Brier and NLL sums in fp64, one workgroup per (chunk of rows, replicate), then the chunk partials in order.
//   metrics    one thread per replicate: the metric columns (layout: mmskin.h); summary: summarize_column of column_summary.h.
//   stats      temperature scaling: a workgroup stages 64 rows of z (fp64) in LDS once, wave w takes the candidates w, w + 4, ...
//              with one row per lane, reduces the three row values over the lanes by a butterfly and adds them, in tile order, to
//              its own LDS accumulators; the workgroups' partials are added in order by a second tiny launch.
#include <float.h>

#include "../../include/mmskin.h"
#include "column_summary.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_N = MMSKIN_CALIBRATION_MAX_ROWS;       // 2^24
constexpr int MAX_K = MMSKIN_CALIBRATION_MAX_CLASSES;    // 64
constexpr int MAX_BINS = MMSKIN_CALIBRATION_MAX_BINS;    // 64
constexpr int MAX_R = MMSKIN_BOOTSTRAP_MAX_RESAMPLES;    // 8192
constexpr int MAX_G = MMSKIN_TEMPERATURE_MAX_CANDIDATES; // 64
constexpr int SCALE_LOG2 = MMSKIN_CALIBRATION_CONF_SCALE_LOG2;
constexpr int NT = 256;                                  // threads of every workgroup here
constexpr int TILE = 64;                                 // rows of a codes / stats tile: one per lane
constexpr int CELLS = 2048;                              // (table, bin) cells of a bins tile
constexpr int BIN_ROWS = 8192;                           // rows of an unweighted bins workgroup
constexpr int SUM_ROWS = 4096, SUM_CHUNKS = 256;
constexpr int STAT_BLOCKS = 1024;
static_assert(CELLS * 16 <= 64 * 1024 && CELLS >= MAX_BINS, "a bins tile holds at least one table in static LDS");
static_assert((MAX_K + 1) * (int64_t)MAX_N < (1ll << 31), "a code index fits 31 bits");

template <typename T> __host__ __device__ __forceinline__ T lesser(T a, T b) { return b < a ? b : a; }

// ------------------------------------------------------------------------------------------------ codes
__global__ __launch_bounds__(NT) void calibration_codes_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, int N,
                                                               int K, const float* __restrict__ edges, int n_bins,
                                                               uint8_t* __restrict__ bin, int32_t* __restrict__ q, uint8_t* __restrict__ hit) {
  __shared__ float s_p[TILE * (MAX_K + 1)];                        // row r at r (K + 1): an odd pitch for the arg-max walk
  __shared__ float s_edge[(MAX_K + 1) * (MAX_BINS + 1)];
  __shared__ int s_pred[TILE], s_lab[TILE];
  const int tid = threadIdx.x, r0 = blockIdx.x * TILE, rows = min(TILE, N - r0), pitch = K + 1;
  const float* src = probs + (int64_t)r0 * K;
  for (int e = tid; e < rows * K; e += NT) s_p[(e / K) * pitch + e % K] = src[e];
  for (int e = tid; e < (K + 1) * (n_bins + 1); e += NT) s_edge[e] = edges[e];
  if (tid < rows) {
    const int64_t y = labels[r0 + tid];
    s_lab[tid] = (y >= 0 && y < K) ? (int)y : -1;
  }
  __syncthreads();
  if (tid < rows) {
    int best = 0;
    float top = s_p[tid * pitch];
    for (int k = 1; k < K; ++k) {
      const float v = s_p[tid * pitch + k];
      if (v > top) { top = v; best = k; }
    }
    s_pred[tid] = best;
  }
  __syncthreads();
  for (int e = tid; e < (K + 1) * TILE; e += NT) {
    const int t = e / TILE, r = e % TILE;
    if (r >= rows) continue;
    const int col = t == 0 ? s_pred[r] : t - 1;
    const float p = s_p[r * pitch + col];
    const float* edge = s_edge + t * (n_bins + 1);
    int b = 0;
    for (int j = 1; j < n_bins; ++j) b += edge[j] < p;             // <= n_bins - 1
    const int64_t at = (int64_t)t * N + r0 + r;
    bin[at] = (uint8_t)b;
    q[at] = (int32_t)rint((double)p * (double)(1 << SCALE_LOG2));
    hit[at] = (uint8_t)(s_lab[r] == col);
  }
}

// ------------------------------------------------------------------------------------------------ bins
template <bool WEIGHTED>
__global__ __launch_bounds__(NT) void calibration_bins_kernel(int N, int K, int n_bins, int tile_tables, const uint8_t* __restrict__ bin,
                                                              const int32_t* __restrict__ q, const uint8_t* __restrict__ hit,
                                                              const int32_t* __restrict__ weights, int64_t* __restrict__ tables) {
  __shared__ unsigned long long s_ch[CELLS], s_conf[CELLS];        // count | hits << 32, and conf
  const int tid = threadIdx.x, r = blockIdx.x;
  const int t0 = blockIdx.y * tile_tables, t1 = min(t0 + tile_tables, K + 1), cells = (t1 - t0) * n_bins;   // <= CELLS (the host)
  for (int e = tid; e < cells; e += NT) { s_ch[e] = 0; s_conf[e] = 0; }
  __syncthreads();
  const int i0 = WEIGHTED ? 0 : blockIdx.z * BIN_ROWS, i1 = WEIGHTED ? N : min(i0 + BIN_ROWS, N);
  const int32_t* w_r = WEIGHTED ? weights + (int64_t)r * N : nullptr;
  for (int i = i0 + tid; i < i1; i += NT) {
    const uint32_t w = WEIGHTED ? (uint32_t)w_r[i] : 1u;
    if (!w) continue;
    for (int t = t0; t < t1; ++t) {
      const int64_t at = (int64_t)t * N + i;
      const int b = bin[at];
      if (b >= n_bins) continue;
      const int cell = (t - t0) * n_bins + b;                      // < cells
      atomicAdd(&s_ch[cell], (unsigned long long)w | ((unsigned long long)(hit[at] ? w : 0u) << 32));
      atomicAdd(&s_conf[cell], (unsigned long long)w * (unsigned long long)(uint32_t)q[at]);
    }
  }
  __syncthreads();
  int64_t* dst = tables + ((int64_t)r * (K + 1) + t0) * n_bins * 3;
  for (int e = tid; e < cells; e += NT) {
    const unsigned long long ch = s_ch[e], cf = s_conf[e];
    if (WEIGHTED) {
      dst[3 * e] = (int64_t)(ch & 0xffffffffull);
      dst[3 * e + 1] = (int64_t)(ch >> 32);
      dst[3 * e + 2] = (int64_t)cf;
    } else if (ch) {
      unsigned long long* d = reinterpret_cast<unsigned long long*>(dst + 3 * e);
      atomicAdd(d, ch & 0xffffffffull);
      if (ch >> 32) atomicAdd(d + 1, ch >> 32);
      if (cf) atomicAdd(d + 2, cf);
    }
  }
}

// ------------------------------------------------------------------------------------------------ sums
inline int sum_chunks(int N) { return lesser(ceil_div(N, SUM_ROWS), SUM_CHUNKS); }

__global__ __launch_bounds__(NT) void calibration_sums_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, int N, int K,
                                                              const int32_t* __restrict__ weights, int chunk_rows,
                                                              double* __restrict__ partial) {
  __shared__ double s_red[2][NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x, r = blockIdx.y;
  const int i0 = (int)lesser<int64_t>((int64_t)chunk * chunk_rows, N), i1 = (int)lesser<int64_t>((int64_t)i0 + chunk_rows, N);
  const int32_t* w_r = weights ? weights + (int64_t)r * N : nullptr;
  double brier = 0.0, nll = 0.0;
  for (int i = i0 + tid; i < i1; i += NT) {
    const int32_t w = w_r ? w_r[i] : 1;
    const int64_t y = labels[i];
    if (!w || y < 0 || y >= K) continue;
    const float* p = probs + (int64_t)i * K;
    double sq = 0.0;
    for (int k = 0; k < K; ++k) {
      const double d = (double)p[k] - (k == (int)y ? 1.0 : 0.0);
      sq += d * d;
    }
    brier += (double)w * sq;
    nll += (double)w * -log((double)fmaxf(p[y], FLT_MIN));
  }
  brier = wave_sum_f64(brier);
  nll = wave_sum_f64(nll);
  if (lane == 0) { s_red[0][wave] = brier; s_red[1][wave] = nll; }
  __syncthreads();
  if (tid < 2) {
    double total = 0.0;
    for (int k = 0; k < NT / 64; ++k) total += s_red[tid][k];
    partial[((int64_t)r * gridDim.x + chunk) * 2 + tid] = total;
  }
}

// out[e] = partial[0][e] + partial[1][e] + ... in that order, for e < width; partial is [groups][count][width] -> out [groups][width]
__global__ __launch_bounds__(NT) void ordered_sum_kernel(const double* __restrict__ partial, int groups, int count, int width,
                                                         double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= (int64_t)groups * width) return;
  const int64_t g = e / width, x = e % width;
  double total = 0.0;
  for (int c = 0; c < count; ++c) total += partial[(g * count + c) * width + x];
  out[e] = total;
}

// ------------------------------------------------------------------------------------------------ metrics
__global__ __launch_bounds__(NT) void calibration_metrics_kernel(const int64_t* __restrict__ tables, const double* __restrict__ sums, int R,
                                                                 int K, int n_bins, double* __restrict__ metrics) {
  const int r = blockIdx.x * NT + threadIdx.x;
  if (r >= R) return;
  const double nan = nan64(), scale = (double)(1 << SCALE_LOG2);
  double* col = metrics + r;                                       // column m of replicate r: col[m R]
  double class_sum = 0.0;
  int64_t W = 0;
  for (int t = 0; t <= K; ++t) {
    const int64_t* tab = tables + ((int64_t)r * (K + 1) + t) * n_bins * 3;
    int64_t count = 0, hits = 0, conf = 0, gap = 0;
    double worst = 0.0;
    for (int b = 0; b < n_bins; ++b) {
      const int64_t n = tab[3 * b], h = tab[3 * b + 1], c = tab[3 * b + 2];
      const int64_t d = h * (1ll << SCALE_LOG2) - c;               // |d| <= n 2^30 < 2^61
      const int64_t a = d < 0 ? -d : d;
      count += n; hits += h; conf += c; gap += a;
      if (n > 0) worst = fmax(worst, (double)a / (scale * (double)n));
    }
    const double ece = count > 0 ? (double)gap / (scale * (double)count) : nan;
    if (t == 0) {
      W = count;
      col[0] = ece;
      col[(int64_t)1 * R] = count > 0 ? worst : nan;
      col[(int64_t)3 * R] = count > 0 ? (double)(conf - hits * (1ll << SCALE_LOG2)) / (scale * (double)count) : nan;
    } else {
      col[(int64_t)(5 + t) * R] = ece;
      class_sum += ece;
    }
  }
  col[(int64_t)2 * R] = class_sum / (double)K;
  col[(int64_t)4 * R] = W > 0 ? sums[2 * r] / (double)W : nan;
  col[(int64_t)5 * R] = W > 0 ? sums[2 * r + 1] / (double)W : nan;
}

__global__ __launch_bounds__(NT_COL) void calibration_summary_kernel(const double* __restrict__ metrics, int B, int n, int M, double q_lo,
                                                                     double q_hi, double* __restrict__ summary) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x;
  for (int i = threadIdx.x; i < B; i += NT_COL) s_val[i] = metrics[(int64_t)m * B + i];
  __syncthreads();
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary);
}

// ------------------------------------------------------------------------------------------------ temperature
struct Betas { double v[MAX_G]; };

__device__ __forceinline__ double logit_of(float v, int from_probs) { return from_probs ? log((double)fmaxf(v, FLT_MIN)) : (double)v; }

inline int stat_blocks(int N) { return lesser(ceil_div(N, TILE), STAT_BLOCKS); }

__global__ __launch_bounds__(NT) void temperature_stats_kernel(const float* __restrict__ src, int from_probs, const int64_t* __restrict__ labels,
                                                               int N, int K, Betas betas, int G, double* __restrict__ partial) {
  __shared__ double s_z[TILE * (MAX_K + 1)];                       // 33 KiB: row r at r (K + 1)
  __shared__ double s_acc[MAX_G * 3];
  __shared__ int s_lab[TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pitch = K + 1;
  for (int e = tid; e < G * 3; e += NT) s_acc[e] = 0.0;
  const int tiles = (N + TILE - 1) / TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * TILE, rows = min(TILE, N - r0);
    __syncthreads();                                               // the last tile's readers are done (and s_acc is zero)
    const float* from = src + (int64_t)r0 * K;
    for (int e = tid; e < rows * K; e += NT) s_z[(e / K) * pitch + e % K] = logit_of(from[e], from_probs);
    if (tid < TILE) {
      const int64_t y = tid < rows ? labels[r0 + tid] : -1;
      s_lab[tid] = (y >= 0 && y < K) ? (int)y : -1;
    }
    __syncthreads();
    const int y = s_lab[lane];
    const double* z = s_z + lane * pitch;
    double top = 0.0, zy = 0.0;
    if (y >= 0) {
      top = z[0];
      for (int k = 1; k < K; ++k) top = fmax(top, z[k]);
      zy = z[y] - top;
    }
    for (int g = wave; g < G; g += NT / 64) {                      // uniform in the wave
      const double beta = betas.v[g];
      double nll = 0.0, d1 = 0.0, d2 = 0.0;
      if (y >= 0) {
        double s = 0.0, s1 = 0.0;
        for (int k = 0; k < K; ++k) {
          const double d = z[k] - top, e = exp(beta * d);
          s += e; s1 += e * d;
        }
        const double mean = s1 / s;
        double s2 = 0.0;
        for (int k = 0; k < K; ++k) {
          const double d = z[k] - top, c = d - mean;
          s2 += exp(beta * d) * c * c;
        }
        nll = log(s) - beta * zy;
        d1 = mean - zy;
        d2 = s2 / s;
      }
      nll = wave_sum_f64(nll); d1 = wave_sum_f64(d1); d2 = wave_sum_f64(d2);
      if (lane == 0) { s_acc[3 * g] += nll; s_acc[3 * g + 1] += d1; s_acc[3 * g + 2] += d2; }   // this wave owns candidate g
    }
  }
  __syncthreads();
  for (int e = tid; e < G * 3; e += NT) partial[(int64_t)blockIdx.x * G * 3 + e] = s_acc[e];
}

__global__ __launch_bounds__(NT) void temperature_apply_kernel(const float* __restrict__ src, int from_probs, int N, int K, double beta,
                                                               float* __restrict__ out) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const float* row = src + (int64_t)i * K;
  double top = logit_of(row[0], from_probs);
  for (int k = 1; k < K; ++k) top = fmax(top, logit_of(row[k], from_probs));
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += exp(beta * (logit_of(row[k], from_probs) - top));
  for (int k = 0; k < K; ++k) out[(int64_t)i * K + k] = (float)(exp(beta * (logit_of(row[k], from_probs) - top)) / s);
}

// ------------------------------------------------------------------------------------------------ host
int limits(const char* what, int N, int K, int n_bins, int R) {
  if (N < 1 || N > MAX_N) {
    mmskin_set_error("%s: %d rows; the codes are indexed in 31 bits, which holds 1 .. MMSKIN_CALIBRATION_MAX_ROWS = %d", what, N, MAX_N);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (K < 2 || K > MAX_K) {
    mmskin_set_error("%s: %d classes; the kernels hold 2 .. MMSKIN_CALIBRATION_MAX_CLASSES = %d", what, K, MAX_K);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (n_bins < 1 || n_bins > MAX_BINS) {
    mmskin_set_error("%s: %d bins; a table's cells live in LDS, which holds 1 .. MMSKIN_CALIBRATION_MAX_BINS = %d", what, n_bins, MAX_BINS);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (R < 1 || R > MAX_R) {
    mmskin_set_error("%s: %d replicates; a metric column is sorted in LDS, which holds 1 .. MMSKIN_BOOTSTRAP_MAX_RESAMPLES = %d", what, R,
                     MAX_R);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

int candidates_ok(const char* what, int G) {
  if (G < 1 || G > MAX_G) {
    mmskin_set_error("%s: %d candidates; one launch holds 1 .. MMSKIN_TEMPERATURE_MAX_CANDIDATES = %d", what, G, MAX_G);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

int beta_ok(const char* what, double beta) {
  ARG_CHECK(beta > 0.0 && beta <= DBL_MAX, "%s: beta = %g must be finite and positive", what, beta);
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_calibration_metric_columns(int K) { return (K < 2 || K > MAX_K) ? -1 : 6 + K; }

extern "C" int64_t mmskin_calibration_sums_scratch_doubles(int N, int R) {
  return (N < 1 || N > MAX_N || R < 1 || R > MAX_R) ? -1 : (int64_t)2 * sum_chunks(N) * R;
}

extern "C" int64_t mmskin_temperature_scratch_doubles(int N, int G) {
  return (N < 1 || N > MAX_N || G < 1 || G > MAX_G) ? -1 : (int64_t)3 * G * stat_blocks(N);
}

extern "C" int mmskin_calibration_codes(const float* probs, const int64_t* labels, int N, int K, const float* edges, int n_bins, uint8_t* bin,
                                        int32_t* q, uint8_t* hit, void* stream) {
  if (int rc = limits("calibration_codes", N, K, n_bins, 1)) return rc;
  ARG_CHECK(probs && labels && edges && bin && q && hit, "calibration_codes: null argument");
  hipLaunchKernelGGL(calibration_codes_kernel, dim3(ceil_div(N, TILE)), dim3(NT), 0, ST(stream), probs, labels, N, K, edges, n_bins, bin, q, hit);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_calibration_bins(int N, int K, int n_bins, const uint8_t* bin, const int32_t* q, const uint8_t* hit,
                                       const int32_t* weights, int R, int64_t* tables, void* stream) {
  if (int rc = limits("calibration_bins", N, K, n_bins, R)) return rc;
  ARG_CHECK(bin && q && hit && tables, "calibration_bins: null argument");
  const int tile_tables = lesser(K + 1, CELLS / n_bins), tiles = ceil_div(K + 1, tile_tables);
  if (weights) {
    hipLaunchKernelGGL(calibration_bins_kernel<true>, dim3(R, tiles), dim3(NT), 0, ST(stream), N, K, n_bins, tile_tables, bin, q, hit, weights,
                       tables);
  } else {
    HIP_CHECK_RET(hipMemsetAsync(tables, 0, (size_t)(K + 1) * n_bins * 3 * sizeof(int64_t), ST(stream)));
    hipLaunchKernelGGL(calibration_bins_kernel<false>, dim3(1, tiles, ceil_div(N, BIN_ROWS)), dim3(NT), 0, ST(stream), N, K, n_bins, tile_tables,
                       bin, q, hit, weights, tables);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_calibration_sums(const float* probs, const int64_t* labels, int N, int K, const int32_t* weights, int R, double* scratch,
                                       double* sums, void* stream) {
  if (int rc = limits("calibration_sums", N, K, 1, R)) return rc;
  ARG_CHECK(probs && labels && scratch && sums, "calibration_sums: null argument");
  if (!weights) R = 1;
  const int chunks = sum_chunks(N);
  hipLaunchKernelGGL(calibration_sums_kernel, dim3(chunks, R), dim3(NT), 0, ST(stream), probs, labels, N, K, weights, ceil_div(N, chunks),
                     scratch);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(ordered_sum_kernel, dim3(ceil_div(2 * R, NT)), dim3(NT), 0, ST(stream), scratch, R, chunks, 2, sums);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_calibration_finalize(const int64_t* tables, const double* sums, int R, int K, int n_bins, double q_lo, double q_hi,
                                           double* metrics, double* summary, void* stream) {
  if (int rc = limits("calibration_finalize", 1, K, n_bins, R)) return rc;
  ARG_CHECK(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "calibration_finalize: the quantiles (%g, %g) must satisfy 0 <= low <= high <= 1", q_lo,
            q_hi);
  ARG_CHECK(tables && sums && metrics && summary, "calibration_finalize: null argument");
  const int M = 6 + K;
  hipLaunchKernelGGL(calibration_metrics_kernel, dim3(ceil_div(R, NT)), dim3(NT), 0, ST(stream), tables, sums, R, K, n_bins, metrics);
  HIP_CHECK_RET(hipGetLastError());
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)calibration_summary_kernel, (int)column_lds_bytes(MAX_R)));
  hipLaunchKernelGGL(calibration_summary_kernel, dim3(M), dim3(NT_COL), column_lds_bytes(R), ST(stream), metrics, R, pow2_at_least(R), M, q_lo,
                     q_hi, summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_temperature_stats(const float* src, int from_probs, const int64_t* labels, int N, int K, const double* betas, int G,
                                        double* scratch, double* out, void* stream) {
  if (int rc = limits("temperature_stats", N, K, 1, 1)) return rc;
  if (int rc = candidates_ok("temperature_stats", G)) return rc;
  ARG_CHECK(src && labels && betas && scratch && out, "temperature_stats: null argument");
  Betas b = {};
  for (int g = 0; g < G; ++g) {
    if (int rc = beta_ok("temperature_stats", betas[g])) return rc;
    b.v[g] = betas[g];
  }
  const int blocks = stat_blocks(N);
  hipLaunchKernelGGL(temperature_stats_kernel, dim3(blocks), dim3(NT), 0, ST(stream), src, from_probs, labels, N, K, b, G, scratch);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(ordered_sum_kernel, dim3(ceil_div(3 * G, NT)), dim3(NT), 0, ST(stream), scratch, 1, blocks, 3 * G, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_temperature_apply(const float* src, int from_probs, int N, int K, double beta, float* out, void* stream) {
  if (int rc = limits("temperature_apply", N, K, 1, 1)) return rc;
  if (int rc = beta_ok("temperature_apply", beta)) return rc;
  ARG_CHECK(src && out, "temperature_apply: null argument");
  hipLaunchKernelGGL(temperature_apply_kernel, dim3(ceil_div(N, NT)), dim3(NT), 0, ST(stream), src, from_probs, N, K, beta, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
