// Per-sample predictive uncertainty (mmskin.uncertainty.PredictiveUncertainty): the three kernels around T stochastic passes of a
// batch.  The contract is in include/mmskin.h; tests/uncertainty_oracle.py restates all of it in numpy.
//
//   views      the dihedral views of a batch for test-time augmentation.  A workgroup takes one 32 x 32 tile of one plane, reads it
//              ONCE into LDS (one dword per element whatever the element size, rows 33 dwords apart: the transposed reads of the
//              odd-k views walk 33-dword steps, which are 32 different banks) and stores it to every selected view.  In every view
//              the lanes of a wave write consecutive addresses of one destination row.  A pure permutation: bit-exact.
//   reduce     logits [T][N][C] -> mean probability, its standard deviation over the passes, the votes, the prediction and the
//              seven statistics of a row.  One wave per row, one lane per class, fp64; the passes are walked in order t = 0 .. T - 1
//              twice (the second walk forms the deviations about the mean: a one-pass sum of squares would lose a standard
//              deviation next to 0).  Sums over the classes are butterflies: every lane ends with the same value, and lanes past C
//              add zeros, so a row's result does not depend on the other rows or on the grid.  No atomics.
//   risk       counts: thread i holds score i and walks all j through LDS tiles (N^2 compares, as auc.hip); the j range is cut into
//              chunks over blockIdx.y and the four integers are added to the row's cells with integer atomics (the entry zeroes
//              them).  summary: ONE workgroup.  Rows with equal scores share n_lt, so a tie group is known by the rank slot it
//              starts at: the group's rows mark that slot, the slot's thread spreads the group over its n_eq slots, and then the
//              thread of rank k forms e(k) / k from its group's four integers.  The sums are taken in a fixed order (thread t its
//              slots t, t + 1024, ..., a butterfly over the lanes, the waves in order); everything else is an integer.
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int MAX_T = MMSKIN_UNCERTAINTY_MAX_PASSES;       // 4096
constexpr int MAX_C = MMSKIN_UNCERTAINTY_MAX_CLASSES;      // 64: one lane per class
constexpr int MAX_N = MMSKIN_BOOTSTRAP_MAX_ROWS;           // 16384: risk-coverage rows
constexpr int TILE = 32;                                   // views: a tile is TILE x TILE elements
constexpr int PITCH = TILE + 1;
constexpr int TJ = 1024;                                   // risk counts: j rows per LDS tile
constexpr int TARGET_WGS = 1024;
constexpr int NT_SUM = 1024;                               // risk summary: the one workgroup
static_assert(MAX_N <= 0x4000, "the summary keeps row + 1 in 15 bits beside a start flag");

typedef unsigned long long u64;

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double nan_f64() { return __longlong_as_double(0x7ff8000000000000ll); }

// ------------------------------------------------------------------------------------------------ views
// source element of destination (i, j) in view v (square planes for the odd-k views: the host checks)
__device__ __forceinline__ void view_source(int v, int i, int j, int H, int W, int& sy, int& sx) {
  switch (v) {
    case 0: sy = i; sx = j; break;
    case 1: sy = j; sx = W - 1 - i; break;
    case 2: sy = H - 1 - i; sx = W - 1 - j; break;
    case 3: sy = H - 1 - j; sx = i; break;
    case 4: sy = i; sx = W - 1 - j; break;
    case 5: sy = H - 1 - j; sx = W - 1 - i; break;
    case 6: sy = H - 1 - i; sx = j; break;
    default: sy = j; sx = i; break;
  }
}

template <typename E>
__global__ __launch_bounds__(NT) void dihedral_views_kernel(const E* __restrict__ src, E* __restrict__ dst, int H, int W, int tiles_x,
                                                            int tiles, int64_t slab, int view_mask) {
  __shared__ uint32_t s_tile[TILE * PITCH];
  const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;            // 32 x 8
  const int64_t plane = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / tiles_x) * TILE, x0 = (tile % tiles_x) * TILE;
  const int th = min(TILE, H - y0), tw = min(TILE, W - x0);                   // >= 1 by the grid
  const E* from = src + plane * H * W;
  for (int r = ty; r < th; r += NT / TILE)
    if (tx < tw) s_tile[r * PITCH + tx] = (uint32_t)from[(int64_t)(y0 + r) * W + x0 + tx];
  __syncthreads();
  int slot = 0;
  for (int v = 0; v < 8; ++v) {
    if (!((view_mask >> v) & 1)) continue;
    // the destination tile: the (i, j) whose source lies in this tile
    const bool transposed = v & 1;
    const bool rows_flip = v == 2 || v == 6 || v == 1 || v == 5;             // i runs against the tile's x (odd k) or y (even k)
    const bool cols_flip = v == 2 || v == 4 || v == 3 || v == 5;
    const int dh = transposed ? tw : th, dw = transposed ? th : tw;
    const int lo_i = transposed ? x0 : y0, lo_j = transposed ? y0 : x0;       // the tile's origin along the axis i / j walks
    const int ext_i = transposed ? W : H, ext_j = transposed ? H : W;
    const int i0 = rows_flip ? ext_i - lo_i - dh : lo_i;
    const int j0 = cols_flip ? ext_j - lo_j - dw : lo_j;
    E* to = dst + (int64_t)slot * slab + plane * H * W;
    for (int r = ty; r < dh; r += NT / TILE) {
      if (tx >= dw) continue;
      const int i = i0 + r, j = j0 + tx;                                      // inside [0, H) x [0, W): the views are bijections
      int sy, sx;
      view_source(v, i, j, H, W, sy, sx);
      to[(int64_t)i * W + j] = (E)s_tile[(sy - y0) * PITCH + (sx - x0)];
    }
    ++slot;
  }
}

// ------------------------------------------------------------------------------------------------ reduce
__global__ __launch_bounds__(NT) void uncertainty_reduce_kernel(const float* __restrict__ logits, int64_t pass_stride, int64_t row_stride, int T,
                                                                int N, int C, double* __restrict__ mean_prob, double* __restrict__ prob_std,
                                                                int32_t* __restrict__ votes, int32_t* __restrict__ pred,
                                                                double* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * (NT / 64) + wave;                     // uniform in the wave
  if (n >= N) return;
  const bool live = lane < C;
  const float* row = logits + (int64_t)n * row_stride + lane;
  double sum_p = 0.0, sum_h = 0.0;
  int my_votes = 0, bad = 0;
  for (int t = 0; t < T; ++t) {
    const float xf = live ? row[(int64_t)t * pass_stride] : 0.f;
    bad |= !(fabsf(xf) <= 3.402823466e+38f);                       // inf or NaN
    float top = live ? xf : -INFINITY;
    int arg = live ? lane : MAX_C + lane;
    wave_argmax(top, arg);
    my_votes += arg == lane;
    const double e = live ? exp((double)xf - (double)top) : 0.0;
    const double p = e / wave_sum_f64(e);
    sum_p += p;
    sum_h += wave_sum_f64(p > 0.0 ? p * log(p) : 0.0);             // 0 log 0 = 0
  }
  bad = wave_max_i32(bad);
  const double mean = sum_p / (double)T;
  double sum_d2 = 0.0;
  if (!bad)
    for (int t = 0; t < T; ++t) {
      const float xf = live ? row[(int64_t)t * pass_stride] : 0.f;
      const double top = (double)wave_max(live ? xf : -INFINITY);
      const double e = live ? exp((double)xf - top) : 0.0;
      const double d = e / wave_sum_f64(e) - mean;
      sum_d2 += d * d;
    }
  const double sd = sqrt(sum_d2 / (double)T);
  double conf = live ? mean : -1.0;
  int best = live ? lane : MAX_C + lane;
  wave_argmax(conf, best);
  const double second = wave_max_f64(live && lane != best ? mean : -1.0);
  const double h_mean = -wave_sum_f64(live && mean > 0.0 ? mean * log(mean) : 0.0);
  const double h_exp = -sum_h / (double)T;
  const int top_votes = wave_max_i32(live ? my_votes : 0);
  const double sd_pred = shfl_f64(sd, best);
  const double nan = nan_f64();
  if (live) {
    mean_prob[(int64_t)n * C + lane] = bad ? nan : mean;
    prob_std[(int64_t)n * C + lane] = bad ? nan : sd;
    votes[(int64_t)n * C + lane] = bad ? 0 : my_votes;
  }
  if (lane == 0) pred[n] = bad ? -1 : best;
  if (lane < 7) {
    double v;
    switch (lane) {
      case 0: v = conf; break;
      case 1: v = conf - second; break;
      case 2: v = h_mean; break;
      case 3: v = h_exp; break;
      case 4: v = fmax(h_mean - h_exp, 0.0); break;
      case 5: v = 1.0 - (double)top_votes / (double)T; break;
      default: v = sd_pred; break;
    }
    stats[(int64_t)n * 7 + lane] = bad ? nan : v;
  }
}

// ------------------------------------------------------------------------------------------------ risk-coverage
__global__ __launch_bounds__(NT) void risk_coverage_counts_kernel(const double* __restrict__ score, const uint8_t* __restrict__ wrong, int N,
                                                                  int chunk, int32_t* __restrict__ counts) {
  __shared__ double s_score[TJ];
  __shared__ int32_t s_wrong[TJ];
  const int tid = threadIdx.x, i = blockIdx.x * NT + tid;
  const int jbeg = blockIdx.y * chunk, jend = min(jbeg + chunk, N);             // chunk is a multiple of TJ; jbeg < N by the grid
  const double si = i < N ? score[i] : 0.0;
  int n_lt = 0, n_eq = 0, e_lt = 0, e_eq = 0;
  for (int j0 = jbeg; j0 < jend; j0 += TJ) {
    const int rows = min(TJ, jend - j0);
    __syncthreads();                                                            // the previous tile is consumed
    for (int r = tid; r < rows; r += NT) { s_score[r] = score[j0 + r]; s_wrong[r] = wrong[j0 + r] != 0; }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {                                            // one address per wave: a broadcast
      const double sj = s_score[r];
      const int w = s_wrong[r], lt = sj < si, eq = sj == si;                    // a NaN is neither
      n_lt += lt; n_eq += eq; e_lt += lt & w; e_eq += eq & w;
    }
  }
  if (i < N) {
    int32_t* cell = counts + (int64_t)i * 4;
    if (n_lt) atomicAdd(cell, n_lt);
    if (n_eq) atomicAdd(cell + 1, n_eq);
    if (e_lt) atomicAdd(cell + 2, e_lt);
    if (e_eq) atomicAdd(cell + 3, e_eq);
  }
}

// the fixed-order sum of one value per thread over the workgroup; every thread returns with it
// (wave sums, then the wave totals in ascending order: not faithfulness.hip's block_tree_sum, whose order differs)
__device__ __forceinline__ double block_sum_f64(double v, double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum_f64(v);
  __syncthreads();                                                              // s_red is free again
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double total = 0.0;
  for (int w = 0; w < NT_SUM / 64; ++w) total += s_red[w];
  return total;
}

__global__ __launch_bounds__(NT_SUM) void risk_coverage_summary_kernel(const int32_t* __restrict__ counts, const uint8_t* __restrict__ wrong,
                                                                       int N, double* __restrict__ out) {
  __shared__ uint16_t s_owner[MAX_N];        // per rank slot: (a row of the tie group that holds it) + 1, | 0x8000 on the group's first slot
  __shared__ double s_red[NT_SUM / 64];
  __shared__ u64 s_wins2;
  __shared__ int32_t s_wrong, s_groups;
  const int tid = threadIdx.x;
  for (int k = tid; k < N; k += NT_SUM) s_owner[k] = 0;
  if (tid == 0) { s_wins2 = 0; s_wrong = 0; s_groups = 0; }
  __syncthreads();
  u64 wins2 = 0;
  int n_wrong = 0;
  for (int i = tid; i < N; i += NT_SUM) {
    const int32_t* c = counts + (int64_t)i * 4;
    const int n_lt = c[0], n_eq = c[1], e_lt = c[2], e_eq = c[3];
    if (n_eq > 0 && n_lt >= 0 && n_lt < N) s_owner[n_lt] = (uint16_t)((i + 1) | 0x8000);   // the group's rows race: any of them serves
    if (wrong[i]) {                                                             // against the correct rows: 2 per win, 1 per tie
      ++n_wrong;
      wins2 += (u64)(2 * (int64_t)(n_lt - e_lt) + (n_eq - e_eq));
    }
  }
  if (wins2) atomicAdd(&s_wins2, wins2);
  if (n_wrong) atomicAdd(&s_wrong, n_wrong);
  __syncthreads();
  int groups = 0;
  for (int g = tid; g < N; g += NT_SUM) {
    const uint16_t o = s_owner[g];
    if (!(o & 0x8000)) continue;                                                // not a first slot (a spread entry carries no flag)
    ++groups;
    const int n_eq = counts[(int64_t)((o & 0x7fff) - 1) * 4 + 1];
    for (int m = 1; m < n_eq && g + m < N; ++m) s_owner[g + m] = o & 0x7fff;
  }
  if (groups) atomicAdd(&s_groups, groups);
  __syncthreads();
  const int E = s_wrong, first_wrong_rank = N - E;                              // with all errors last, ranks > N - E are errors
  double aurc = 0.0, best = 0.0;
  for (int k = tid; k < N; k += NT_SUM) {
    const int rank = k + 1, o = s_owner[k] & 0x7fff;
    double term = nan_f64();                                                    // counts that are no ranking: NaN
    if (o) {
      const int32_t* c = counts + (int64_t)(o - 1) * 4;
      const int n_lt = c[0], n_eq = c[1], e_lt = c[2], e_eq = c[3];
      const double e = (double)e_lt + (double)((int64_t)(rank - n_lt) * e_eq) / (double)n_eq;
      term = e / (double)rank;
    }
    aurc += term;
    if (rank > first_wrong_rank) best += (double)(rank - first_wrong_rank) / (double)rank;
  }
  aurc = block_sum_f64(aurc, s_red) / (double)N;
  best = block_sum_f64(best, s_red) / (double)N;
  if (tid == 0) {
    out[0] = aurc;
    out[1] = best;
    out[2] = aurc - best;
    out[3] = (E > 0 && E < N) ? (double)s_wins2 / (2.0 * (double)E * (double)(N - E)) : nan_f64();
    out[4] = (double)E / (double)N;
    out[5] = (double)N;
    out[6] = (double)E;
    out[7] = (double)s_groups;
  }
}

int risk_limits(const char* what, int N) {
  if (N < 1 || N > MAX_N) {
    mmskin_set_error("%s: N = %d rows; the ranking is held in LDS, which holds 1 .. MMSKIN_BOOTSTRAP_MAX_ROWS = %d", what, N, MAX_N);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_dihedral_views(const void* src, void* dst, int B, int C, int H, int W, int elem_bytes, int view_mask, void* stream) {
  ARG_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1, "dihedral_views: every extent must be >= 1 (B %d, C %d, H %d, W %d)", B, C, H, W);
  ARG_CHECK(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, "dihedral_views: elem_bytes = %d is not 1, 2 or 4", elem_bytes);
  ARG_CHECK(view_mask >= 1 && view_mask <= 0xff, "dihedral_views: view_mask = 0x%x selects no view of the 8 (bits 0 .. 7)", view_mask);
  ARG_CHECK(!(view_mask & 0xaa) || H == W, "dihedral_views: view_mask = 0x%x holds a quarter-turn view, which needs H == W (H %d, W %d)",
            view_mask, H, W);
  ARG_CHECK(src && dst, "dihedral_views: null argument");
  ARG_CHECK(src != dst, "dihedral_views: src == dst; the views are written out of place");
  const int tiles_x = ceil_div(W, TILE), tiles_y = ceil_div(H, TILE);
  const int64_t tiles = (int64_t)tiles_x * tiles_y, planes = (int64_t)B * C, slab = planes * H * W;
  ARG_CHECK(tiles * planes < ((int64_t)1 << 31) && slab < ((int64_t)1 << 40), "dihedral_views: B x C x H x W = %d x %d x %d x %d is out of range",
            B, C, H, W);
  const dim3 grid((unsigned)(tiles * planes));
  if (elem_bytes == 1)
    hipLaunchKernelGGL(dihedral_views_kernel<uint8_t>, grid, dim3(NT), 0, ST(stream), (const uint8_t*)src, (uint8_t*)dst, H, W, tiles_x, (int)tiles,
                       slab, view_mask);
  else if (elem_bytes == 2)
    hipLaunchKernelGGL(dihedral_views_kernel<uint16_t>, grid, dim3(NT), 0, ST(stream), (const uint16_t*)src, (uint16_t*)dst, H, W, tiles_x,
                       (int)tiles, slab, view_mask);
  else
    hipLaunchKernelGGL(dihedral_views_kernel<uint32_t>, grid, dim3(NT), 0, ST(stream), (const uint32_t*)src, (uint32_t*)dst, H, W, tiles_x,
                       (int)tiles, slab, view_mask);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_uncertainty_reduce(const float* logits, int64_t pass_stride, int64_t row_stride, int T, int N, int C, double* mean_prob,
                                         double* prob_std, int32_t* votes, int32_t* pred, double* stats, void* stream) {
  if (T < 1 || T > MAX_T) {
    mmskin_set_error("uncertainty_reduce: T = %d passes; one call holds 1 .. MMSKIN_UNCERTAINTY_MAX_PASSES = %d", T, MAX_T);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  if (C < 2 || C > MAX_C) {
    mmskin_set_error("uncertainty_reduce: C = %d classes; the kernel holds one class per lane, 2 .. MMSKIN_UNCERTAINTY_MAX_CLASSES = %d", C,
                     MAX_C);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  ARG_CHECK(N >= 1 && N <= (1 << 24), "uncertainty_reduce: N = %d rows is outside 1 .. 2^24", N);
  ARG_CHECK(row_stride >= C, "uncertainty_reduce: row_stride = %lld is below the %d classes of a row", (long long)row_stride, C);
  ARG_CHECK(pass_stride >= 0 && pass_stride < ((int64_t)1 << 40) && row_stride < ((int64_t)1 << 32),
            "uncertainty_reduce: pass_stride = %lld / row_stride = %lld is out of range", (long long)pass_stride, (long long)row_stride);
  ARG_CHECK(logits && mean_prob && prob_std && votes && pred && stats, "uncertainty_reduce: null argument");
  hipLaunchKernelGGL(uncertainty_reduce_kernel, dim3(ceil_div(N, NT / 64)), dim3(NT), 0, ST(stream), logits, pass_stride, row_stride, T, N, C,
                     mean_prob, prob_std, votes, pred, stats);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_risk_coverage(const double* score, const uint8_t* wrong, int N, int32_t* counts, void* stream) {
  if (int rc = risk_limits("risk_coverage", N)) return rc;
  ARG_CHECK(score && wrong && counts, "risk_coverage: null argument");
  HIP_CHECK_RET(hipMemsetAsync(counts, 0, (size_t)N * 4 * sizeof(int32_t), ST(stream)));
  const int iblocks = ceil_div(N, NT), tiles = ceil_div(N, TJ);
  int chunks = ceil_div(TARGET_WGS, iblocks);                      // enough chunks for TARGET_WGS workgroups, at most one per tile
  if (chunks > tiles) chunks = tiles;
  const int chunk = ceil_div(tiles, chunks) * TJ;                  // rows per chunk: whole tiles
  chunks = ceil_div(N, chunk);
  hipLaunchKernelGGL(risk_coverage_counts_kernel, dim3(iblocks, chunks), dim3(NT), 0, ST(stream), score, wrong, N, chunk, counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_risk_coverage_summary(const int32_t* counts, const uint8_t* wrong, int N, double* out, void* stream) {
  if (int rc = risk_limits("risk_coverage_summary", N)) return rc;
  ARG_CHECK(counts && wrong && out, "risk_coverage_summary: null argument");
  hipLaunchKernelGGL(risk_coverage_summary_kernel, dim3(1), dim3(NT_SUM), 0, ST(stream), counts, wrong, N, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
