// LIME explanations of the metadata on the model itself (mmskin.lime.MetadataLime): the kernels on either side of the batched
// fusion-head calls, and the weighted ridge fits behind them.  The reference runs lime's LimeTabularExplainer(mode="regression",
// discretize_continuous=False).explain_instance(row, predict_fn, num_features=15) on a random-forest surrogate
// (src/scripts/data_preprocessing/lime_padufes20.py); here predict_fn is the network, and the image is encoded once.
//
// Features are the F <= 128 encoded columns.  mean / scale fp64 [F] are the StandardScaler of the encoded training rows.  For an
// explained row x and N neighbourhood rows per sample (sample-major row order, row = b N + s):
//     row_0 = x (bit for bit);   row_s[f] = n(s, f) * (float)scale[f] + (float)mean[f]   (or + x[f]: sample_around_instance), fp32
//     z = ((double)row - mean) / scale;   d_s^2 = sum_f (z_s - z_0)^2;   w_s = sqrt(exp(-d_s^2 / (0.5625 F)))
//     y[s, c] = soft-max or logit of the head on row_s
// and per class c, sklearn's Ridge(alpha, fit_intercept=True).fit(Z, y, sample_weight=w) in closed form, first with alpha = 0.01 on
// all features to choose the K with the largest |beta0_j z_0j|, then with alpha = 1 on those.
//
// The generator (counter based, no state): h = mix64(mix64(seed) ^ (sample << 40 | s << 8 | f)) with common.h's splitmix finaliser,
// hi / lo = its 32-bit halves, u1 = ((hi >> 9) + 0.5) 2^-23, u2 = ((lo >> 9) + 0.5) 2^-23 (both exact in fp32, inside (0, 1)),
// n = sqrtf(-2 logf(u1)) cosf(6.2831855f u2): Box-Muller in fp32.  n depends on (seed, sample, s, f) only -- not on N, F, the batch
// or the row range of the call -- so any cut of the rows gives the bytes of one full call.
//
//   neighbourhood  one wave per row: lanes own columns lane, lane + 64, ...; the row is formed, written, and its distance reduced
//                  over the wave in a fixed xor tree in the same pass.  Every element of the range is written once.
//   reduce         sum_s w a a^T for a = [z (F), 1, y (C)], rows i <= F against all F + 1 + C columns, plus sum w y^2: every sum the
//                  fits need.  Rows are grouped in SLABs of 256 by their index s WITHIN the sample, and each (sample, slab) owns
//                  one block of partial sums in the caller's accumulator.  A workgroup owns a 32 x 64 tile of one block; a thread
//                  owns 8 x 1 of it in registers and adds its slab's rows in ascending s, 32 rows staged in LDS at a time (w a_i
//                  as 32 x 32 and a_j as 32 x 64 doubles, 24 KiB, + the 32 rows' soft-max).  It starts from the value in memory, so
//                  a slab split between two calls continues the same sequence: the sums do not depend on where the rows were cut.
//   finish         the slabs' partials added in ascending slab order (one thread per element).
//   solve          one workgroup per (sample, class): centres the sums, Cholesky of G + 0.01 I in LDS, two triangular solves,
//                  ranks |beta0 z_0|, gathers G_UU + I from the untouched upper triangle into the lower one, Cholesky and solves
//                  again, then intercept, score, local prediction and the |beta| order.  The F x (F + 1) fp64 matrix + vectors is
//                  140 KiB at F = 128, inside the 160 KiB of a CU: that is what bounds F.
//   accumulate     one thread per class: |beta| added over b, k in order into the caller's fp64 [F][C] sums.
// No atomics anywhere; FMA contraction is off, so the arithmetic is the one written here.  tests/lime_oracle.py restates all of it.
#include "../../include/mmskin.h"
#include "common.h"

#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int MAX_F = 128, MAX_C = 64;
constexpr int SLAB = 256;                // rows of a sample per block of partial sums
constexpr int TI = 32, TJ = 64, RS = 32; // reduce: tile rows (z, 1), tile columns (z, 1, y), rows staged at a time
constexpr double ALPHA_SELECT = 0.01, ALPHA_FIT = 1.0;

__host__ __device__ inline int64_t block_doubles(int F, int C) { return (int64_t)(F + 1) * (F + 1 + C) + C; }
inline int slabs_of(int N) { return (N + SLAB - 1) / SLAB; }

// ------------------------------------------------------------------------------------------------ neighbourhood
__device__ __forceinline__ float lime_normal(uint64_t key, uint64_t sample, uint32_t s, int f) {
  const uint64_t h = mix64(key ^ ((sample << 40) | ((uint64_t)s << 8) | (uint64_t)f));
  const float u1 = ((float)(uint32_t)(h >> 41) + 0.5f) * 0x1p-23f;
  const float u2 = ((float)((uint32_t)h >> 9) + 0.5f) * 0x1p-23f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

template <typename WT>
__global__ __launch_bounds__(NT) void lime_neighbourhood_kernel(const float* __restrict__ x, int x_stride, const double* __restrict__ mean,
                                                                const double* __restrict__ scale, int F, int N, uint64_t key,
                                                                int64_t sample0, int around, double kw2, int64_t row0, int64_t n_rows,
                                                                int out_width, float* __restrict__ out, WT* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int64_t local = blockIdx.x * (int64_t)(NT / 64) + (threadIdx.x >> 6);
  if (local >= n_rows) return;                                    // uniform per wave: the shuffles below see all 64 lanes
  const int64_t r = row0 + local, b = r / N;
  const uint32_t s = (uint32_t)(r - b * N);
  const float* xb = x + b * x_stride;
  double d2 = 0.0;
  for (int j = lane; j < out_width; j += 64) {
    float v = 0.f;                                                // columns past F
    if (j < F) {
      const float xv = xb[j];
      v = xv;
      if (s != 0) v = lime_normal(key, (uint64_t)(sample0 + b), s, j) * (float)scale[j] + (around ? xv : (float)mean[j]);
      const double z = ((double)v - mean[j]) / scale[j], z0 = ((double)xv - mean[j]) / scale[j];
      d2 += (z - z0) * (z - z0);
    }
    out[local * out_width + j] = v;
  }
  for (int o = 32; o > 0; o >>= 1) d2 += __shfl_xor(d2, o, 64);
  if (lane == 0) w[local] = (WT)sqrt(exp(-(d2 / kw2)));
}

// ------------------------------------------------------------------------------------------------ reduce
template <typename LT, typename WT>
__global__ __launch_bounds__(NT) void lime_reduce_kernel(const float* __restrict__ rows, int width, const WT* __restrict__ w,
                                                         const LT* __restrict__ logits, const double* __restrict__ mean,
                                                         const double* __restrict__ scale, int F, int C, int N, int output, int64_t row0,
                                                         int64_t row1, int64_t slab0, int slabs, double* __restrict__ acc) {
  __shared__ double ai[RS][TI];            // w a_i
  __shared__ double aj[RS][TJ];
  __shared__ float yv[RS][MAX_C + 1];
  __shared__ double wv[RS];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int A = F + 1 + C;
  const int i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
  const int64_t slab = slab0 + blockIdx.z, b = slab / slabs, p = slab - b * slabs;
  int64_t lo = b * N + p * SLAB, hi = lo + SLAB;
  if (hi > (b + 1) * N) hi = (b + 1) * N;
  if (lo < row0) lo = row0;
  if (hi > row1) hi = row1;
  double* part = acc + slab * block_doubles(F, C);
  const int j = j0 + lane, ib = i0 + 8 * g;
  double a[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) a[q] = (ib + q <= F && j < A) ? part[(int64_t)(ib + q) * A + j] : 0.0;
  const bool yy = j > F && j < A && F >= ib && F < ib + 8;       // the owner of (row "1", column y_c) also sums w y_c^2
  const int yk = 8 * g + (F - ib);
  double ayy = yy ? part[(int64_t)(F + 1) * A + (j - F - 1)] : 0.0;
  const bool need_y = j0 + TJ > F + 1;
  for (int64_t r0 = lo; r0 < hi; r0 += RS) {
    const int nr = (int)(hi - r0 < RS ? hi - r0 : RS);
    __syncthreads();                                              // the last round's reads are over
    if (tid < nr) {
      wv[tid] = (double)w[r0 + tid - row0];
      if (need_y) {
        const int64_t base = (r0 + tid - row0) * C;
        if (output == MMSKIN_LIME_PROB) {
          // exp(x - max) rounded to fp32 from the fp64 exp (so the value does not depend on an fp32 exp's last bit), summed in
          // c = 0 .. C-1 order and divided, all in fp32
          float top = -INFINITY, sum = 0.f;
          for (int c = 0; c < C; ++c) top = fmaxf(top, to_f32(logits[base + c]));
          for (int c = 0; c < C; ++c) {
            const float e = (float)exp((double)(to_f32(logits[base + c]) - top));
            yv[tid][c] = e;
            sum += e;
          }
          for (int c = 0; c < C; ++c) yv[tid][c] = yv[tid][c] / sum;
        } else {
          for (int c = 0; c < C; ++c) yv[tid][c] = to_f32(logits[base + c]);
        }
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nr * (TI + TJ); idx += NT) {
      const int r = idx / (TI + TJ), k = idx - r * (TI + TJ);
      const bool is_i = k < TI;
      const int col = is_i ? i0 + k : j0 + (k - TI), limit = is_i ? F + 1 : A;
      double v = 0.0;
      if (col < F) v = ((double)rows[(r0 + r - row0) * width + col] - mean[col]) / scale[col];
      else if (col == F) v = 1.0;
      else if (col < limit) v = (double)yv[r][col - F - 1];
      if (is_i) ai[r][k] = wv[r] * v;
      else aj[r][k - TI] = v;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double vj = aj[r][lane];
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] += ai[r][8 * g + q] * vj;
      if (yy) ayy += (ai[r][yk] * vj) * vj;
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (ib + q <= F && j < A) part[(int64_t)(ib + q) * A + j] = a[q];
  if (yy) part[(int64_t)(F + 1) * A + (j - F - 1)] = ayy;
}

// ------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(NT) void lime_finish_kernel(const double* __restrict__ acc, int64_t E, int slabs, int64_t total,
                                                         double* __restrict__ sums, int32_t* __restrict__ status, int n_status) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  if (i < n_status) status[i] = 0;
  if (i >= total) return;
  const int64_t b = i / E, e = i - b * E;
  double s = 0.0;
  for (int p = 0; p < slabs; ++p) s += acc[(b * slabs + p) * E + e];
  sums[i] = s;
}

// ------------------------------------------------------------------------------------------------ solve
// In-place Cholesky of the lower triangle (diagonal included) of the n x n matrix m; false on a pivot that is not positive.  The
// verdict is uniform: every thread reads the same pivot behind a barrier.
__device__ bool cholesky_lower(double* m, int ld, int n, int tid) {
  for (int k = 0; k < n; ++k) {
    __syncthreads();
    const double piv = m[k * ld + k];
    if (!(piv > 0.0)) return false;
    const double d = sqrt(piv);
    __syncthreads();                                              // everyone holds the pivot before it is overwritten
    for (int i = k + tid; i < n; i += NT) m[i * ld + k] = i == k ? d : m[i * ld + k] / d;
    __syncthreads();
    const int rem = n - k - 1;
    for (int idx = tid; idx < rem * rem; idx += NT) {
      const int i = k + 1 + idx / rem, j = k + 1 + idx % rem;
      if (j <= i) m[i * ld + j] -= m[i * ld + k] * m[j * ld + k];
    }
  }
  __syncthreads();
  return true;
}

// L L^T sol = t with the factor in m's lower triangle; t is used up, u is scratch
__device__ void cholesky_solve(const double* m, int ld, int n, double* t, double* u, double* sol, int tid) {
  for (int k = 0; k < n; ++k) {
    __syncthreads();
    const double yk = t[k] / m[k * ld + k];
    if (tid == 0) u[k] = yk;
    for (int i = k + 1 + tid; i < n; i += NT) t[i] -= m[i * ld + k] * yk;
  }
  for (int k = n - 1; k >= 0; --k) {
    __syncthreads();
    const double bk = u[k] / m[k * ld + k];
    if (tid == 0) sol[k] = bk;
    for (int i = tid; i < k; i += NT) u[i] -= m[k * ld + i] * bk;
  }
  __syncthreads();
}

inline size_t solve_lds_bytes(int F) { return ((size_t)F * (F + 1) + 9 * (size_t)F) * sizeof(double) + 3 * (size_t)F * sizeof(int); }

__global__ __launch_bounds__(NT) void lime_solve_kernel(const double* __restrict__ sums, const float* __restrict__ x, int x_stride,
                                                        const double* __restrict__ mean, const double* __restrict__ scale, int F, int C,
                                                        int K, double* __restrict__ coef, int32_t* __restrict__ feature,
                                                        double* __restrict__ intercept, double* __restrict__ score,
                                                        double* __restrict__ local_pred, double* __restrict__ dense,
                                                        int32_t* __restrict__ status) {
  extern __shared__ double lds[];
  const int ld = F + 1;
  double* mat = lds;                       // lower triangle: the factor being built; strict upper triangle: G, kept
  double* zbar = mat + (size_t)F * ld;
  double* z0 = zbar + F;
  double* gd = z0 + F;                     // G's diagonal
  double* rv = gd + F;                     // R
  double* t = rv + F;
  double* u = t + F;
  double* beta0 = u + F;
  double* beta = beta0 + F;
  double* gb = beta + F;                   // G_UU beta, then |beta0 z_0|
  int* keep = (int*)(gb + F);
  int* pos = keep + F;
  int* U = pos + F;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / C, c = blockIdx.x - b * C;
  const int A = F + 1 + C;
  const double* S = sums + (int64_t)b * block_doubles(F, C);
  const double W = S[(int64_t)F * A + F];
  const double ybar = S[(int64_t)F * A + F + 1 + c] / W;
  for (int j = tid; j < F; j += NT) {
    zbar[j] = S[(int64_t)F * A + j] / W;
    z0[j] = ((double)x[(int64_t)b * x_stride + j] - mean[j]) / scale[j];
  }
  __syncthreads();
  for (int idx = tid; idx < F * F; idx += NT) {
    const int i = idx / F, j = idx - i * F;
    const int lo = i < j ? i : j, hi = i < j ? j : i;            // one value for both triangles
    const double gv = S[(int64_t)lo * A + hi] - (W * zbar[lo]) * zbar[hi];
    if (i == j) {
      gd[i] = gv;
      mat[i * ld + i] = gv + ALPHA_SELECT;
    } else {
      mat[i * ld + j] = gv;
    }
  }
  for (int j = tid; j < F; j += NT) {
    rv[j] = S[(int64_t)j * A + F + 1 + c] - (W * zbar[j]) * ybar;
    t[j] = rv[j];
  }
  const double syy = S[(int64_t)(F + 1) * A + c] - (W * ybar) * ybar;
  if (!cholesky_lower(mat, ld, F, tid)) {
    if (tid == 0) status[blockIdx.x] = 1;
    return;
  }
  cholesky_solve(mat, ld, F, t, u, beta0, tid);
  // the K largest |beta0_j z_0j|, ties to the lower index; U = the kept features in ascending order
  for (int j = tid; j < F; j += NT) gb[j] = fabs(beta0[j] * z0[j]);
  __syncthreads();
  for (int j = tid; j < F; j += NT) {
    int rank = 0;
    for (int i = 0; i < F; ++i) rank += gb[i] > gb[j] || (gb[i] == gb[j] && i < j);
    keep[j] = rank < K;
  }
  __syncthreads();
  for (int j = tid; j < F; j += NT) {
    int n = 0;
    for (int i = 0; i < j; ++i) n += keep[i];
    pos[j] = n;
    if (keep[j]) U[n] = j;
  }
  __syncthreads();
  for (int idx = tid; idx < K * K; idx += NT) {
    const int p = idx / K, q = idx - p * K;
    if (q < p) mat[p * ld + q] = mat[U[q] * ld + U[p]];          // U[q] < U[p]: read above the diagonal, written below it
  }
  __syncthreads();                                               // the diagonal is read by nobody above, but is by the factorisation
  for (int p = tid; p < K; p += NT) {
    mat[p * ld + p] = gd[U[p]] + ALPHA_FIT;
    t[p] = rv[U[p]];
  }
  if (!cholesky_lower(mat, ld, K, tid)) {
    if (tid == 0) status[blockIdx.x] = 2;
    return;
  }
  cholesky_solve(mat, ld, K, t, u, beta, tid);
  for (int p = tid; p < K; p += NT) {
    double s = 0.0;
    for (int q = 0; q < K; ++q) {
      const int lo = p < q ? p : q, hi = p < q ? q : p;
      s += (p == q ? gd[U[p]] : mat[U[lo] * ld + U[hi]]) * beta[q];
    }
    gb[p] = s;
  }
  __syncthreads();
  const int64_t bc = blockIdx.x;
  if (tid == 0) {
    double zb = 0.0, zx = 0.0, br = 0.0, bgb = 0.0;
    for (int p = 0; p < K; ++p) {
      zb += zbar[U[p]] * beta[p];
      zx += z0[U[p]] * beta[p];
      br += beta[p] * rv[U[p]];
      bgb += beta[p] * gb[p];
    }
    const double icpt = ybar - zb, rss = syy - 2.0 * br + bgb;
    intercept[bc] = icpt;
    local_pred[bc] = icpt + zx;
    score[bc] = syy > 0.0 ? 1.0 - rss / syy : (rss == 0.0 ? 1.0 : 0.0);   // a constant target: sklearn's r2_score convention
  }
  for (int p = tid; p < K; p += NT) {
    const double ap = fabs(beta[p]);
    int rank = 0;
    for (int q = 0; q < K; ++q) rank += fabs(beta[q]) > ap || (fabs(beta[q]) == ap && q < p);
    coef[bc * K + rank] = beta[p];
    feature[bc * K + rank] = U[p];
  }
  if (dense)
    for (int j = tid; j < F; j += NT) dense[bc * F + j] = keep[j] ? beta[pos[j]] : 0.0;
}

__global__ void lime_accumulate_kernel(const double* __restrict__ coef, const int32_t* __restrict__ feature, int B, int C, int K,
                                       double* __restrict__ abs_sum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k) {
      const int64_t i = ((int64_t)b * C + c) * K + k;
      abs_sum[(int64_t)feature[i] * C + c] += fabs(coef[i]);
    }
}

// ------------------------------------------------------------------------------------------------ host
int lime_extents(const char* what, int batch, int N, int F, int C) {
  ARG_CHECK(batch >= 1 && N >= 1 && F >= 1, "%s: every extent must be >= 1 (batch %d, N %d, F %d)", what, batch, N, F);
  ARG_CHECK(F <= MAX_F, "%s: %d features; the solver's LDS matrix holds at most %d", what, F, MAX_F);
  ARG_CHECK(C >= 0 && C <= MAX_C, "%s: %d classes; at most %d", what, C, MAX_C);
  ARG_CHECK(N <= (1 << 24) && batch <= (1 << 16) && (int64_t)batch * slabs_of(N) <= 65535, "%s: %d samples of %d rows are out of range", what,
            batch, N);
  return MMSKIN_OK;
}

int lime_range(const char* what, int batch, int N, int64_t row0, int64_t row1) {
  ARG_CHECK(row0 >= 0 && row0 <= row1 && row1 <= (int64_t)batch * N, "%s: rows [%lld, %lld) are not a range of the %lld rows", what,
            (long long)row0, (long long)row1, (long long)batch * N);
  return MMSKIN_OK;
}

struct SolveWorkspace {
  double* sums;
  int32_t* status;
};
size_t carve_solve(void* base, int batch, int F, int C, SolveWorkspace* ws) {
  Carver cv(base);
  ws->sums = cv.take<double>((size_t)batch * block_doubles(F, C));
  ws->status = cv.take<int32_t>((size_t)batch * C);
  return cv.cur;
}

}  // namespace

extern "C" int64_t mmskin_lime_accumulator_doubles(int batch, int N, int F, int C) {
  if (lime_extents("lime_accumulator_doubles", batch, N, F, C) != MMSKIN_OK || C < 1) return -1;
  return (int64_t)batch * slabs_of(N) * block_doubles(F, C);
}

extern "C" int64_t mmskin_lime_solve_workspace_bytes(int batch, int F, int C) {
  if (lime_extents("lime_solve_workspace_bytes", batch, 1, F, C) != MMSKIN_OK || C < 1) return -1;
  SolveWorkspace ws;
  return (int64_t)carve_solve(nullptr, batch, F, C, &ws);
}

extern "C" int mmskin_lime_neighbourhood(const float* x, int x_stride, int batch, const double* mean, const double* scale, int F, int N,
                                         uint64_t seed, int64_t sample0, int around_instance, int64_t row0, int64_t row1, float* out,
                                         int out_width, void* w, int w_dtype, void* stream) {
  if (int rc = lime_extents("lime_neighbourhood", batch, N, F, 0)) return rc;
  if (int rc = lime_range("lime_neighbourhood", batch, N, row0, row1)) return rc;
  ARG_CHECK(out_width >= F && out_width <= (1 << 20) && x_stride >= F, "lime_neighbourhood: out_width %d and x_stride %d must be at least "
            "F = %d", out_width, x_stride, F);
  ARG_CHECK(sample0 >= 0 && sample0 + batch <= (1 << 24), "lime_neighbourhood: samples [%lld, %lld) are outside the generator's 2^24",
            (long long)sample0, (long long)sample0 + batch);
  ARG_CHECK(w_dtype == MMSKIN_LIME_W_F32 || w_dtype == MMSKIN_LIME_W_F64, "lime_neighbourhood: weight dtype %d is neither fp32 (0) nor fp64 (1)",
            w_dtype);
  ARG_CHECK(x && mean && scale && out && w, "lime_neighbourhood: null argument");
  const int64_t n = row1 - row0;
  if (n == 0) return MMSKIN_OK;
  const dim3 grid((unsigned)((n + NT / 64 - 1) / (NT / 64)));
  const double kw2 = 0.5625 * F;                                   // (0.75 sqrt F)^2
  const uint64_t key = mix64(seed);
  if (w_dtype == MMSKIN_LIME_W_F64)
    hipLaunchKernelGGL(lime_neighbourhood_kernel<double>, grid, dim3(NT), 0, ST(stream), x, x_stride, mean, scale, F, N, key, sample0,
                       around_instance != 0, kw2, row0, n, out_width, out, (double*)w);
  else
    hipLaunchKernelGGL(lime_neighbourhood_kernel<float>, grid, dim3(NT), 0, ST(stream), x, x_stride, mean, scale, F, N, key, sample0,
                       around_instance != 0, kw2, row0, n, out_width, out, (float*)w);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_lime_reduce(const float* rows, int width, const void* w, int w_dtype, const void* logits, int logits_dtype, int output,
                                  const double* mean, const double* scale, int batch, int N, int F, int C, int64_t row0, int64_t row1,
                                  double* acc, void* stream) {
  if (int rc = lime_extents("lime_reduce", batch, N, F, C)) return rc;
  ARG_CHECK(C >= 1, "lime_reduce: %d classes", C);
  if (int rc = lime_range("lime_reduce", batch, N, row0, row1)) return rc;
  ARG_CHECK(width >= F && width <= (1 << 20), "lime_reduce: a row width of %d is not at least F = %d", width, F);
  ARG_CHECK(w_dtype == MMSKIN_LIME_W_F32 || w_dtype == MMSKIN_LIME_W_F64, "lime_reduce: weight dtype %d is neither fp32 (0) nor fp64 (1)",
            w_dtype);
  ARG_CHECK(logits_dtype == 0 || logits_dtype == 1, "lime_reduce: logits dtype %d is neither fp32 (0) nor bf16 (1)", logits_dtype);
  ARG_CHECK(output == MMSKIN_LIME_PROB || output == MMSKIN_LIME_LOGIT, "lime_reduce: output %d is neither PROB (0) nor LOGIT (1)", output);
  ARG_CHECK(mean && scale && acc && ((rows && w && logits) || row0 == row1), "lime_reduce: null argument");
  if (row0 == row1) return MMSKIN_OK;
  const int slabs = slabs_of(N);
  auto slab_of = [&](int64_t r) { return (r / N) * slabs + (r % N) / SLAB; };
  const int64_t slab0 = slab_of(row0), n_slabs = slab_of(row1 - 1) - slab0 + 1;
  const dim3 grid(ceil_div(F + 1 + C, TJ), ceil_div(F + 1, TI), (unsigned)n_slabs);
#define LIME_REDUCE(LT, WT)                                                                                                              \
  hipLaunchKernelGGL((lime_reduce_kernel<LT, WT>), grid, dim3(NT), 0, ST(stream), rows, width, (const WT*)w, (const LT*)logits, mean, scale, \
                     F, C, N, output, row0, row1, slab0, slabs, acc)
  if (logits_dtype == 1) {
    if (w_dtype == MMSKIN_LIME_W_F64) LIME_REDUCE(bf16_t, double);
    else LIME_REDUCE(bf16_t, float);
  } else {
    if (w_dtype == MMSKIN_LIME_W_F64) LIME_REDUCE(float, double);
    else LIME_REDUCE(float, float);
  }
#undef LIME_REDUCE
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_lime_solve(const double* acc, const float* x, int x_stride, const double* mean, const double* scale, int batch, int N,
                                 int F, int C, int K, double* coef, int32_t* feature, double* intercept, double* score, double* local_pred,
                                 double* dense, double* abs_sum, void* workspace, void* stream) {
  if (int rc = lime_extents("lime_solve", batch, N, F, C)) return rc;
  ARG_CHECK(C >= 1, "lime_solve: %d classes", C);
  ARG_CHECK(K >= 1 && K <= F, "lime_solve: num_features %d is not in 1 .. F = %d", K, F);
  ARG_CHECK(x_stride >= F, "lime_solve: x_stride %d is not at least F = %d", x_stride, F);
  ARG_CHECK(acc && x && mean && scale && coef && feature && intercept && score && local_pred && workspace, "lime_solve: null argument");
  SolveWorkspace ws;
  carve_solve(workspace, batch, F, C, &ws);
  const int64_t E = block_doubles(F, C), total = (int64_t)batch * E;
  hipLaunchKernelGGL(lime_finish_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), acc, E, slabs_of(N), total, ws.sums,
                     ws.status, batch * C);
  HIP_CHECK_RET(hipGetLastError());
  // one size for every F: the attribute is set once per device
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)lime_solve_kernel, (int)solve_lds_bytes(MAX_F)));
  hipLaunchKernelGGL(lime_solve_kernel, dim3(batch * C), dim3(NT), solve_lds_bytes(F), ST(stream), ws.sums, x, x_stride, mean, scale, F, C, K, coef,
                     feature, intercept, score, local_pred, dense, ws.status);
  HIP_CHECK_RET(hipGetLastError());
  // the verdict of the factorisations: the call waits for it (pageable host memory, then the stream)
  std::vector<int32_t> status((size_t)batch * C);
  HIP_CHECK_RET(hipMemcpyAsync(status.data(), ws.status, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ST(stream)));
  HIP_CHECK_RET(hipStreamSynchronize(ST(stream)));
  for (size_t i = 0; i < status.size(); ++i)
    if (status[i] != 0) {
      mmskin_set_error("lime_solve: sample %d, class %d: a pivot of the %s Cholesky factorisation is not positive (the sums are not those of "
                       "a weighted neighbourhood); nothing was written for it", (int)(i / C), (int)(i % C),
                       status[i] == 1 ? "selection (G + 0.01 I)" : "final (G_UU + I)");
      return MMSKIN_ERR_NUMERIC;
    }
  if (abs_sum) {
    hipLaunchKernelGGL(lime_accumulate_kernel, dim3(1), dim3(MAX_C), 0, ST(stream), coef, feature, batch, C, K, abs_sum);
    HIP_CHECK_RET(hipGetLastError());
  }
  return MMSKIN_OK;
}
