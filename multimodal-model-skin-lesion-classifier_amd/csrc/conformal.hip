// Split-conformal prediction sets of a fold (mmskin.conformal.ConformalPredictor): the nonconformity scores of every class, R random
// calibration / test splits scored as exact integers, one workgroup per replicate, and the sets of a fitted threshold.  The contract
// is in include/mmskin.h; tests/conformal_oracle.py restates all of it in numpy.
//
//   score       a workgroup takes 64 rows: their C probabilities go to LDS as fp64 by coalesced loads; the (row, class) pairs are
//               dealt over the threads and each counts the classes that stand above its own (conformal_order.h): the rank, and the
//               class at every rank.  One thread per row then walks its row in rank order with the running fp64 sum and leaves the
//               score of every class where its probability was.  The tile is written out three ways, all coalesced: score [N][C],
//               rank [N][C] and, for the replicate kernel, score_t [C][N].  With a threshold the same pass writes the sets: apply.
//   replicates  one workgroup per replicate r.  Phase 1, the split: u_i = the high word of mix64(key ^ (r << 32 | i)) in LDS; the
//               calibration rows are the `take` rows with the smallest key (u_i << 16 | i), found by a radix select: six passes of
//               one byte, a 256-bin LDS histogram each (integer atomics), the byte where the running count crosses `take` picked
//               by one wave.  Stratified: one select per class over that class's rows.  The flag replaces u_i in place.
//               Phase 2, the threshold: the caller's `order` lists the rows by ascending true-label score, so the k-th smallest
//               calibration score is the row at which the count of flagged rows along `order` reaches k: a wave counts its
//               contiguous segment by ballots, the wave that holds k walks it again.  Mondrian: one segment per class.
//               Phase 3, the counts over the test rows: lane = row, score_t read coalesced, the classes in a uniform loop; the
//               per-class count is one ballot per wave, the rest integer LDS atomics.  Nothing floats but the comparisons.
//   metrics     one thread per replicate; summary: summarize_column of column_summary.h, unchanged.
#include <float.h>
#include <math.h>

#include "../../include/mmskin.h"
#include "column_summary.h"
#include "common.h"
#include "conformal_order.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_N = MMSKIN_CONFORMAL_MAX_ROWS;         // 32768: a row index fits the low 16 bits of a split key
constexpr int MAX_M = 1 << 24;                           // rows of a score / apply call
constexpr int MAX_C = MMSKIN_CONFORMAL_MAX_CLASSES;      // 64: a set is one 64-bit mask
constexpr int MAX_R = MMSKIN_BOOTSTRAP_MAX_RESAMPLES;    // 8192
constexpr int MAX_WAVES = 16;
constexpr int NT = 256, TILE = 64;                       // the score pass
constexpr uint64_t U_STREAM = 0xFFFFFFFFull;             // the replicate number no split uses: the stream of the rows' u
static_assert(MAX_N <= 65536 && MAX_C <= 64, "a split key is u << 16 | row; a set is a 64-bit mask");
static_assert((size_t)MAX_N * 4 + 8 * 1024 <= 160 * 1024, "a replicate's flags must fit one workgroup's LDS");

__host__ __device__ constexpr int count_columns(int C) { return 8 + 5 * C; }
__host__ __device__ constexpr int metric_columns(int C) { return 6 + 2 * C; }

// counts [8 + 5 C] of a replicate (mmskin.h)
enum { N_TEST = 0, COVERED, TOTAL_SIZE, EMPTY, SINGLETON, SINGLETON_HIT, HIST = 6 };
__host__ __device__ constexpr int at_hist(int) { return HIST; }
__host__ __device__ constexpr int at_size_cov(int C) { return HIST + C + 1; }
__host__ __device__ constexpr int at_class_n(int C) { return HIST + 2 * (C + 1); }
__host__ __device__ constexpr int at_class_cov(int C) { return HIST + 2 * (C + 1) + C; }
__host__ __device__ constexpr int at_class_in(int C) { return HIST + 2 * (C + 1) + 2 * C; }
static_assert(at_class_in(MAX_C) + MAX_C == count_columns(MAX_C), "the layout fills the 8 + 5 C cells");

__device__ __forceinline__ uint64_t row_hash(uint64_t key, uint64_t r, int64_t i) { return mix64(key ^ ((r << 32) | (uint64_t)(uint32_t)i)); }
// u in [0, 1) of a row: the top 53 bits of its hash
__device__ __forceinline__ double row_u(uint64_t key, int64_t i) { return (double)(row_hash(key, U_STREAM, i) >> 11) * 0x1p-53; }

// ------------------------------------------------------------------------------------------------ score / apply
template <typename T>
__global__ __launch_bounds__(NT) void conformal_score_kernel(const T* __restrict__ probs, int64_t N, int C, int kind, int randomized, double lam,
                                                             int k_reg, uint64_t key, int64_t row0, const double* __restrict__ qhat,
                                                             double* __restrict__ score, double* __restrict__ score_t,
                                                             uint8_t* __restrict__ rank, uint64_t* __restrict__ mask, int32_t* __restrict__ size) {
  __shared__ double s_p[TILE * (MAX_C + 1)];                       // row r at r (C + 1); the probabilities, then the scores in place
  __shared__ uint8_t s_ord[TILE * MAX_C], s_rank[TILE * MAX_C];    // the class at rank j + 1 of row r at [r C + j]; the rank of class c
  const int tid = threadIdx.x, pitch = C + 1;
  const int64_t r0 = (int64_t)blockIdx.x * TILE;
  const int rows = (int)(N - r0 < TILE ? N - r0 : TILE);
  const T* src = probs + r0 * C;
  for (int e = tid; e < rows * C; e += NT) s_p[(e / C) * pitch + e % C] = (double)src[e];
  __syncthreads();
  for (int e = tid; e < rows * C; e += NT) {
    const int r = e / C, c = e % C;
    const double* p = s_p + r * pitch;
    int above = 0;
    for (int j = 0; j < C; ++j) above += stands_above(p[j], j, p[c], c);   // <= C - 1: a class does not stand above itself
    s_ord[r * C + above] = (uint8_t)c;
    s_rank[e] = (uint8_t)(above + 1);
  }
  __syncthreads();
  if (tid < rows) {
    double* p = s_p + tid * pitch;
    const double u = randomized ? row_u(key, row0 + r0 + tid) : 1.0;
    double above = 0.0;                                            // the probabilities of the classes ranked strictly above, in rank order
    for (int j = 0; j < C; ++j) {
      const int c = s_ord[tid * C + j] < C ? s_ord[tid * C + j] : 0;
      const double pc = p[c];
      double s;
      if (kind == MMSKIN_CONFORMAL_LAC) {
        s = 1.0 - pc;
      } else {
        s = above + u * pc;
        if (kind == MMSKIN_CONFORMAL_RAPS) s = s + lam * (double)(j + 1 - k_reg > 0 ? j + 1 - k_reg : 0);
        above += pc;
      }
      p[c] = s;
    }
    if (qhat) {
      uint64_t m = 0;
      int n = 0;
      for (int c = 0; c < C; ++c)
        if (in_set(p[c], qhat[c])) { m |= 1ull << c; ++n; }
      mask[r0 + tid] = m;
      size[r0 + tid] = n;
    }
  }
  __syncthreads();
  if (score)
    for (int e = tid; e < rows * C; e += NT) score[r0 * C + e] = s_p[(e / C) * pitch + e % C];
  if (rank)
    for (int e = tid; e < rows * C; e += NT) rank[r0 * C + e] = s_rank[e];
  if (score_t)
    for (int e = tid; e < C * TILE; e += NT) {
      const int c = e / TILE, r = e % TILE;
      if (r < rows) score_t[(int64_t)c * N + r0 + r] = s_p[r * pitch + c];
    }
}

// ------------------------------------------------------------------------------------------------ replicates
// The rows of a segment are members[p0 .. p1) (members == nullptr: the rows p0 .. p1 themselves), s_u[row] their draws.  Leaves
// s_u[row] = 1 for the `take` rows of the segment with the smallest key (s_u[row] << 16 | row) and 0 for the others.  Every
// argument is uniform over the workgroup; ends with a barrier.  A row outside [0, N) is skipped, never followed.
__device__ void select_smallest(uint32_t* s_u, const int32_t* __restrict__ members, int N, int p0, int p1, int take, int* s_hist, int* s_pick) {
  const int tid = threadIdx.x, nt = blockDim.x;
  uint64_t prefix = 0;                                             // the bytes of the take-th smallest key found so far
  int need = take;                                                 // its rank among the keys that share them
  if (take > 0 && take < p1 - p0) {
    for (int shift = 40; shift >= 0; shift -= 8) {
      for (int e = tid; e < 256; e += nt) s_hist[e] = 0;
      __syncthreads();
      for (int p = p0 + tid; p < p1; p += nt) {
        const int row = members ? members[p] : p;
        if ((unsigned)row >= (unsigned)N) continue;
        const uint64_t k = ((uint64_t)s_u[row] << 16) | (uint64_t)row;
        if ((k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(int)((k >> shift) & 255)], 1);
      }
      __syncthreads();
      if (tid < 64) {                                              // one wave: lane l owns the bins 4 l .. 4 l + 3
        int c[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = s_hist[4 * tid + k]; sum += c[k]; }
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(incl, o, 64);
          if (tid >= o) incl += up;
        }
        int run = incl - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (run < need && need <= run + c[k]) { s_pick[0] = 4 * tid + k; s_pick[1] = need - run; }
          run += c[k];
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | (uint64_t)(s_pick[0] & 255);
      need = s_pick[1];
    }
  }
  for (int p = p0 + tid; p < p1; p += nt) {
    const int row = members ? members[p] : p;
    if ((unsigned)row >= (unsigned)N) continue;
    const uint64_t k = ((uint64_t)s_u[row] << 16) | (uint64_t)row;
    s_u[row] = take >= p1 - p0 ? 1u : (take <= 0 ? 0u : (uint32_t)(k <= prefix));
  }
  __syncthreads();
}

// The conformal quantile of the calibration rows among order[p0 .. p1) (ascending true-label score): with n their number, the
// ceil((n + 1)(1 - alpha))-th smallest of their scores, +inf when that index exceeds n (n = 0 included).  Uniform arguments; every
// thread returns the value; ends with a barrier.
__device__ double segment_quantile(const uint32_t* s_flag, const int32_t* __restrict__ order, const int64_t* __restrict__ labels,
                                   const double* __restrict__ score_t, int N, int C, int p0, int p1, double alpha, int* s_wave, double* s_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int len = p1 > p0 ? p1 - p0 : 0, seg = ((len + waves - 1) / waves + 63) / 64 * 64;
  const int a = min(p0 + wave * seg, p0 + len), b = min(a + seg, p0 + len);
  int mine = 0;
  for (int q0 = a; q0 < b; q0 += 64) {
    const int q = q0 + lane;
    bool f = false;
    if (q < b) {
      const int row = order[q];
      f = (unsigned)row < (unsigned)N && s_flag[row] != 0;
    }
    mine += __popcll(__ballot(f));
  }
  if (lane == 0) s_wave[wave] = mine;
  if (tid == 0) *s_out = __longlong_as_double(0x7ff0000000000000ll);
  __syncthreads();
  int n = 0, before = 0;
  for (int k = 0; k < waves; ++k) {
    if (k < wave) before += s_wave[k];
    n += s_wave[k];
  }
  const double at = ceil((double)(n + 1) * (1.0 - alpha));         // >= 1: alpha < 1
  if (at <= (double)n) {
    const int k = (int)at;
    if (before < k && k <= before + mine) {                        // uniform in the wave: this wave's segment holds the k-th
      int run = before;
      for (int q0 = a; q0 < b; q0 += 64) {
        const int q = q0 + lane;
        bool f = false;
        int row = 0;
        if (q < b) {
          row = order[q];
          f = (unsigned)row < (unsigned)N && s_flag[row] != 0;
        }
        const uint64_t bal = __ballot(f);
        const int pc = __popcll(bal);
        if (run + pc >= k) {
          if (f && run + __popcll(bal & ((1ull << lane) - 1ull)) + 1 == k) {
            const int64_t y = labels[row];
            if (y >= 0 && y < C) *s_out = score_t[y * N + row];
          }
          break;
        }
        run += pc;
      }
    }
  }
  __syncthreads();
  const double q = *s_out;
  __syncthreads();                                                 // read by all before the next call resets it
  return q;
}

__global__ __launch_bounds__(1024) void conformal_replicates_kernel(uint64_t key, int flags, int fit, int N, int C, int n_cal, double alpha,
                                                                    const int64_t* __restrict__ labels, const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ members, const int32_t* __restrict__ class_start,
                                                                    const int32_t* __restrict__ cal_count, const double* __restrict__ score_t,
                                                                    int r0, double* __restrict__ qhat, int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_hist[256], s_pick[2], s_wave[MAX_WAVES], s_start[MAX_C + 1], s_take[MAX_C], s_cnt[count_columns(MAX_C)];
  __shared__ double s_q[MAX_C], s_one;
  uint32_t* s_u = reinterpret_cast<uint32_t*>(lds);                // N cells: the draws, then the calibration flags
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)r0 + blockIdx.x;
  const bool stratified = (flags & MMSKIN_CONFORMAL_STRATIFIED) != 0, mondrian = (flags & MMSKIN_CONFORMAL_MONDRIAN) != 0;
  const int W = count_columns(C);

  if (stratified || mondrian)
    for (int c = tid; c <= C; c += nt) s_start[c] = min(max(class_start[c], 0), N);
  if (stratified)
    for (int c = tid; c < C; c += nt) s_take[c] = cal_count[c];
  for (int e = tid; e < W; e += nt) s_cnt[e] = 0;
  if (tid < 2) s_pick[tid] = 0;

  // phase 1: the split.  fit: every row calibrates.  Replicate 0: the identity order, the first rows (of every class).
  if (fit || (r == 0 && !stratified)) {
    for (int i = tid; i < N; i += nt) s_u[i] = (fit || i < n_cal) ? 1u : 0u;
    __syncthreads();
  } else if (r == 0) {
    for (int i = tid; i < N; i += nt) s_u[i] = 0u;
    __syncthreads();
    for (int c = 0; c < C; ++c)
      for (int p = s_start[c] + tid; p < s_start[c + 1]; p += nt) {
        const int row = members[p];
        if ((unsigned)row < (unsigned)N) s_u[row] = (p - s_start[c] < s_take[c]) ? 1u : 0u;
      }
    __syncthreads();
  } else {
    for (int i = tid; i < N; i += nt) s_u[i] = (uint32_t)(row_hash(key, (uint64_t)r, i) >> 32);
    __syncthreads();
    if (!stratified) {
      select_smallest(s_u, nullptr, N, 0, N, n_cal, s_hist, s_pick);
    } else {
      for (int c = 0; c < C; ++c) select_smallest(s_u, members, N, s_start[c], s_start[c + 1], s_take[c], s_hist, s_pick);
    }
  }

  // phase 2: the threshold(s)
  if (!mondrian) {
    const double q = segment_quantile(s_u, order, labels, score_t, N, C, 0, N, alpha, s_wave, &s_one);
    for (int c = tid; c < C; c += nt) s_q[c] = q;
  } else {
    for (int c = 0; c < C; ++c) {
      const double q = segment_quantile(s_u, order, labels, score_t, N, C, s_start[c], s_start[c + 1], alpha, s_wave, &s_one);
      if (tid == 0) s_q[c] = q;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += nt) qhat[r * C + c] = s_q[c];
  if (!counts) return;                                             // fit: there is no test row

  // phase 3: the counts over the test rows; a wave's 64 lanes hold 64 consecutive rows
  int* s_hist_sz = s_cnt + at_hist(C);
  int* s_size_cov = s_cnt + at_size_cov(C);
  int* s_class_n = s_cnt + at_class_n(C);
  int* s_class_cov = s_cnt + at_class_cov(C);
  int* s_class_in = s_cnt + at_class_in(C);
  for (int i0 = wave * 64; i0 < N; i0 += nt) {
    const int i = i0 + lane;
    int y = -1;
    if (i < N && s_u[i] == 0) {
      const int64_t lab = labels[i];
      if (lab >= 0 && lab < C) y = (int)lab;
    }
    const bool test = y >= 0;
    int sz = 0;
    bool covered = false;
    for (int c = 0; c < C; ++c) {
      const bool in = test && in_set(score_t[(int64_t)c * N + i], s_q[c]);
      sz += in;
      if (c == y) covered = in;
      const uint64_t bal = __ballot(in);
      if (lane == 0 && bal) atomicAdd(&s_class_in[c], __popcll(bal));
    }
    if (test) {
      atomicAdd(&s_hist_sz[sz], 1);                                // sz <= C
      atomicAdd(&s_class_n[y], 1);
      if (covered) { atomicAdd(&s_size_cov[sz], 1); atomicAdd(&s_class_cov[y], 1); }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int n_test = 0, covered = 0, total = 0;
    for (int s = 0; s <= C; ++s) { n_test += s_hist_sz[s]; covered += s_size_cov[s]; total += s * s_hist_sz[s]; }
    s_cnt[N_TEST] = n_test; s_cnt[COVERED] = covered; s_cnt[TOTAL_SIZE] = total;
    s_cnt[EMPTY] = s_hist_sz[0]; s_cnt[SINGLETON] = s_hist_sz[1]; s_cnt[SINGLETON_HIT] = s_size_cov[1];
  }
  __syncthreads();
  for (int e = tid; e < W; e += nt) counts[r * W + e] = s_cnt[e];
}

// ------------------------------------------------------------------------------------------------ metrics, summary
__global__ __launch_bounds__(256) void conformal_metrics_kernel(const int64_t* __restrict__ counts, const double* __restrict__ qhat, int R, int C,
                                                                double* __restrict__ metrics) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int64_t* cnt = counts + (int64_t)r * count_columns(C);
  const double nan = nan64(), n = (double)cnt[N_TEST];
  double* col = metrics + r;                                       // column m of replicate r: col[m R]
  col[0] = n > 0 ? (double)cnt[COVERED] / n : nan;
  col[(int64_t)1 * R] = n > 0 ? (double)cnt[TOTAL_SIZE] / n : nan;
  col[(int64_t)2 * R] = n > 0 ? (double)cnt[SINGLETON] / n : nan;
  col[(int64_t)3 * R] = cnt[SINGLETON] > 0 ? (double)cnt[SINGLETON_HIT] / (double)cnt[SINGLETON] : nan;
  col[(int64_t)4 * R] = n > 0 ? (double)cnt[EMPTY] / n : nan;
  double worst = nan;
  for (int c = 0; c < C; ++c) {
    const int64_t rows = cnt[at_class_n(C) + c];
    const double cov = rows > 0 ? (double)cnt[at_class_cov(C) + c] / (double)rows : nan;
    if (rows > 0 && !(worst <= cov)) worst = cov;                  // the minimum over the classes with a test row
    col[(int64_t)(6 + c) * R] = cov;
    col[(int64_t)(6 + C + c) * R] = qhat[(int64_t)r * C + c];
  }
  col[(int64_t)5 * R] = worst;
}

__global__ __launch_bounds__(NT_COL) void conformal_summary_kernel(const double* __restrict__ metrics, int B, int n, int M, double q_lo,
                                                                   double q_hi, double* __restrict__ summary) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* s_val = reinterpret_cast<double*>(lds);
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds) + B;
  const int m = blockIdx.x;
  for (int i = threadIdx.x; i < B; i += NT_COL) s_val[i] = metrics[(int64_t)m * B + i];
  __syncthreads();
  summarize_column(s_val, s_key, B, n, m, M, q_lo, q_hi, summary);
}

// ------------------------------------------------------------------------------------------------ host
// The one workspace of a study: the scores class-major for the replicate kernel, and the metric columns of its R replicates.
struct Workspace {
  double* score_t;   // [C][N]
  double* metrics;   // [6 + 2 C][R]
  size_t bytes;
};
Workspace carve(void* base, int N, int C, int R) {
  Carver cv(base);
  Workspace w;
  w.score_t = cv.take<double>((size_t)C * N);
  w.metrics = cv.take<double>((size_t)metric_columns(C) * R);
  w.bytes = cv.cur;
  return w;
}

int classes_ok(const char* what, int C) {
  ARG_CHECK(C >= 2 && C <= MAX_C, "%s: num_classes = %d; a set is one 64-bit mask, which holds 2 .. MMSKIN_CONFORMAL_MAX_CLASSES = %d", what, C,
            MAX_C);
  return MMSKIN_OK;
}
int fold_ok(const char* what, int N, int C) {
  if (int rc = classes_ok(what, C)) return rc;
  ARG_CHECK(N >= 1 && N <= MAX_N, "%s: n_rows = %d; a replicate's split lives in LDS, which holds 1 .. MMSKIN_CONFORMAL_MAX_ROWS = %d", what, N,
            MAX_N);
  return MMSKIN_OK;
}
int replicates_ok(const char* what, int R) {
  ARG_CHECK(R >= 1 && R <= MAX_R, "%s: n_resamples = %d; a metric column is sorted in LDS, which holds 1 .. MMSKIN_BOOTSTRAP_MAX_RESAMPLES = %d",
            what, R, MAX_R);
  return MMSKIN_OK;
}
int alpha_ok(const char* what, double alpha) {
  ARG_CHECK(alpha > 0.0 && alpha < 1.0, "%s: alpha = %g must lie in (0, 1)", what, alpha);
  return MMSKIN_OK;
}
int score_ok(const char* what, int64_t rows, int C, int kind, double lam, int k_reg) {
  if (int rc = classes_ok(what, C)) return rc;
  ARG_CHECK(rows >= 1 && rows <= MAX_M, "%s: n_rows = %lld is outside 1 .. 2^24", what, (long long)rows);
  ARG_CHECK(kind == MMSKIN_CONFORMAL_LAC || kind == MMSKIN_CONFORMAL_APS || kind == MMSKIN_CONFORMAL_RAPS,
            "%s: score = %d is none of MMSKIN_CONFORMAL_LAC, _APS, _RAPS", what, kind);
  ARG_CHECK(k_reg >= 0, "%s: k_reg = %d must be >= 0", what, k_reg);
  ARG_CHECK(lam >= 0.0 && lam <= DBL_MAX, "%s: lam = %g must be finite and >= 0", what, lam);
  return MMSKIN_OK;
}

int replicate_threads(int N) { return N <= 4096 ? 256 : (N <= 8192 ? 512 : 1024); }

template <typename T>
int launch_score(const void* probs, int64_t rows, int C, int kind, int randomized, double lam, int k_reg, uint64_t seed, int64_t row0,
                 const double* qhat, double* score, double* score_t, uint8_t* rank, uint64_t* mask, int32_t* size, void* stream) {
  hipLaunchKernelGGL(conformal_score_kernel<T>, dim3((unsigned)((rows + TILE - 1) / TILE)), dim3(NT), 0, ST(stream), (const T*)probs, rows, C, kind,
                     randomized, lam, k_reg, mix64(seed), row0, qhat, score, score_t, rank, mask, size);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_conformal_count_columns(int C) { return (C < 2 || C > MAX_C) ? -1 : count_columns(C); }
extern "C" int mmskin_conformal_metric_columns(int C) { return (C < 2 || C > MAX_C) ? -1 : metric_columns(C); }

extern "C" int64_t mmskin_conformal_workspace_bytes(int N, int C, int R) {
  return (N < 1 || N > MAX_N || C < 2 || C > MAX_C || R < 1 || R > MAX_R) ? -1 : (int64_t)carve(nullptr, N, C, R).bytes;
}

extern "C" int mmskin_conformal_score(const void* probs, int probs_fp64, int64_t N, int C, int kind, int randomized, double lam, int k_reg,
                                      uint64_t seed, int64_t row0, double* score, uint8_t* rank, void* workspace, void* stream) {
  if (int rc = score_ok("conformal_score", N, C, kind, lam, k_reg)) return rc;
  ARG_CHECK(row0 >= 0, "conformal_score: row0 = %lld must be >= 0", (long long)row0);
  ARG_CHECK(!workspace || N <= MAX_N, "conformal_score: n_rows = %lld; a study's workspace holds 1 .. MMSKIN_CONFORMAL_MAX_ROWS = %d",
            (long long)N, MAX_N);
  ARG_CHECK(probs && (score || rank || workspace), "conformal_score: null argument");
  double* score_t = workspace ? carve(workspace, (int)N, C, 1).score_t : nullptr;
  return probs_fp64 ? launch_score<double>(probs, N, C, kind, randomized, lam, k_reg, seed, row0, nullptr, score, score_t, rank, nullptr, nullptr, stream)
                    : launch_score<float>(probs, N, C, kind, randomized, lam, k_reg, seed, row0, nullptr, score, score_t, rank, nullptr, nullptr, stream);
}

extern "C" int mmskin_conformal_apply(const void* probs, int probs_fp64, int64_t M, int C, int kind, int randomized, double lam, int k_reg,
                                      uint64_t seed, int64_t row0, const double* qhat, uint64_t* mask, int32_t* size, void* stream) {
  if (int rc = score_ok("conformal_apply", M, C, kind, lam, k_reg)) return rc;
  ARG_CHECK(row0 >= 0, "conformal_apply: row0 = %lld must be >= 0", (long long)row0);
  ARG_CHECK(probs && qhat && mask && size, "conformal_apply: null argument");
  return probs_fp64 ? launch_score<double>(probs, M, C, kind, randomized, lam, k_reg, seed, row0, qhat, nullptr, nullptr, nullptr, mask, size, stream)
                    : launch_score<float>(probs, M, C, kind, randomized, lam, k_reg, seed, row0, qhat, nullptr, nullptr, nullptr, mask, size, stream);
}

extern "C" int mmskin_conformal_study(uint64_t seed, int N, int C, int R, int n_cal, double alpha, int flags, const int64_t* labels,
                                      const int32_t* order, const int32_t* members, const int32_t* class_start, const int32_t* cal_count,
                                      int r0, int r1, const void* workspace, double* qhat, int64_t* counts, void* stream) {
  if (int rc = fold_ok("conformal_study", N, C)) return rc;
  if (int rc = replicates_ok("conformal_study", R)) return rc;
  if (int rc = alpha_ok("conformal_study", alpha)) return rc;
  ARG_CHECK(n_cal >= 1 && n_cal <= N - 1, "conformal_study: n_cal = %d must leave a calibration and a test row: 1 .. n_rows - 1 = %d", n_cal, N - 1);
  ARG_CHECK((flags & ~(MMSKIN_CONFORMAL_STRATIFIED | MMSKIN_CONFORMAL_MONDRIAN)) == 0, "conformal_study: unknown flags %d", flags);
  ARG_CHECK(r0 >= 0 && r0 <= r1 && r1 <= R, "conformal_study: replicates [%d, %d) are not a range of the study's %d", r0, r1, R);
  ARG_CHECK(labels && order && workspace && qhat && counts, "conformal_study: null argument");
  ARG_CHECK(!(flags & MMSKIN_CONFORMAL_STRATIFIED) || (members && class_start && cal_count),
            "conformal_study: a stratified split needs members, class_start and cal_count");
  ARG_CHECK(!(flags & MMSKIN_CONFORMAL_MONDRIAN) || class_start, "conformal_study: class-conditional thresholds need class_start");
  if (r0 == r1) return MMSKIN_OK;
  const double* score_t = carve(const_cast<void*>(workspace), N, C, R).score_t;
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)conformal_replicates_kernel, MAX_N * 4));
  hipLaunchKernelGGL(conformal_replicates_kernel, dim3((unsigned)(r1 - r0)), dim3(replicate_threads(N)), (size_t)N * 4, ST(stream), mix64(seed), flags,
                     0, N, C, n_cal, alpha, labels, order, members, class_start, cal_count, score_t, r0, qhat, counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_conformal_fit(int N, int C, double alpha, int flags, const int64_t* labels, const int32_t* order,
                                    const int32_t* class_start, const void* workspace, double* qhat, void* stream) {
  if (int rc = fold_ok("conformal_fit", N, C)) return rc;
  if (int rc = alpha_ok("conformal_fit", alpha)) return rc;
  ARG_CHECK((flags & ~MMSKIN_CONFORMAL_MONDRIAN) == 0, "conformal_fit: unknown flags %d", flags);
  ARG_CHECK(labels && order && workspace && qhat, "conformal_fit: null argument");
  ARG_CHECK(!(flags & MMSKIN_CONFORMAL_MONDRIAN) || class_start, "conformal_fit: class-conditional thresholds need class_start");
  const double* score_t = carve(const_cast<void*>(workspace), N, C, 1).score_t;
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)conformal_replicates_kernel, MAX_N * 4));
  hipLaunchKernelGGL(conformal_replicates_kernel, dim3(1), dim3(replicate_threads(N)), (size_t)N * 4, ST(stream), (uint64_t)0, flags, 1, N, C, N, alpha,
                     labels, order, (const int32_t*)nullptr, class_start, (const int32_t*)nullptr, score_t, 0, qhat, (int64_t*)nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_conformal_finalize(const int64_t* counts, const double* qhat, int N, int C, int R, double q_lo, double q_hi, void* workspace,
                                         double* summary, void* stream) {
  if (int rc = fold_ok("conformal_finalize", N, C)) return rc;
  if (int rc = replicates_ok("conformal_finalize", R)) return rc;
  ARG_CHECK(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "conformal_finalize: the quantiles (%g, %g) must satisfy 0 <= low <= high <= 1", q_lo, q_hi);
  ARG_CHECK(counts && qhat && workspace && summary, "conformal_finalize: null argument");
  const int M = metric_columns(C);
  double* metrics = carve(workspace, N, C, R).metrics;
  hipLaunchKernelGGL(conformal_metrics_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, ST(stream), counts, qhat, R, C, metrics);
  HIP_CHECK_RET(hipGetLastError());
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)conformal_summary_kernel, (int)column_lds_bytes(MAX_R)));
  hipLaunchKernelGGL(conformal_summary_kernel, dim3(M), dim3(NT_COL), column_lds_bytes(R), ST(stream), metrics, R, pow2_at_least(R), M, q_lo, q_hi,
                     summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
