// nn.Linear for gfx950, forward and backward, on one of four routes (linear_path): the implicit-GEMM conv kernels as a 1x1 conv
// (exact fp32, bf16 operands, or bf16 operands zero-padded to 64-multiple widths) or the strided exact-f32 MFMA GEMM of this file
// (v_mfma_f32_16x16x4_f32), which mmskin_bmm shares.  With it: the fp32 <-> bf16 conversion / pad / un-pad / transpose passes in front
// of those GEMMs, the column sums behind the bias gradient, and the library scratch buffer.
#include <stdlib.h>
#include <string.h>

#include "../../include/mmskin.h"
#include "conv.h"
#include "head_internal.h"

// Library-owned scratch for split reductions (split-K partial tiles, column-sum partial rows).  The head's
// C entry points carry no workspace argument (they mirror nn.Linear / nn.LayerNorm call sites), so the
// buffer is allocated lazily and only ever grows; every user runs on the caller's stream, in order.
// One buffer PER DEVICE (the process model is one process per GPU, but nothing here may hand device 0's memory to a launch on
// device 1); `slot` separates the regions two nested entry points use at the same time: mmskin_linear_forward_ex's fallback holds
// its fp32 side copies in slot 1 while it calls mmskin_linear_forward, which (like every other user) takes slot 0.
float* head_scratch(size_t bytes, int slot) {
  constexpr int MAXDEV = 16;
  static float* buf[2][MAXDEV] = {};
  static size_t cap[2][MAXDEV] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAXDEV) return nullptr;
  if (bytes > cap[slot][d]) {
    if (buf[slot][d]) (void)hipFree(buf[slot][d]);   // implicit device sync: no kernel still reads the old buffer
    size_t want = bytes < (size_t)(8 << 20) ? (size_t)(8 << 20) : bytes;
    if (hipMalloc((void**)&buf[slot][d], want) != hipSuccess) { buf[slot][d] = nullptr; cap[slot][d] = 0; return nullptr; }
    cap[slot][d] = want;
  }
  return buf[slot][d];
}
// out[i] = sum_s part[s*n + i]
__global__ void split_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int S, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float t = 0.f;
    for (int s2 = 0; s2 < S; ++s2) t += part[(int64_t)s2 * n + i];
    out[i] = t;
  }
}

// ------------------------------------------------------------------ generic strided f32 GEMM
// C[m][n] = sum_k A(m,k) * B(n,k) (+ bias[n]) ; A(m,k) = a[m*sam + k*sak] ; B(n,k) = b[n*sbn + k*sbk]
// The head's GEMMs have M = batch (256) and N, K <= 2048: tiny for a 256-CU chip, so the kernel is built
// for latency, not throughput: 32x32 output tiles (many workgroups), K-steps of 128 (16 + 16 independent loads per thread in flight;
// with K-steps of 32 a K = 512 GEMM was 16 dependent load -> barrier -> multiply rounds, 12 - 16 us for 0.13 GFLOP) with the next
// step's operands prefetched into registers while the current one is multiplied on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32, one 16x16 fragment per wave).
#define LG_BK 128
#define LG_T 32
#define LG_PK 130  // pitch of a [row][k] tile (k-contiguous source): 2 row + g distinct over a half wave's 16 rows x 2 k
#define LG_PM 48   // pitch of a [k][row] tile (row-contiguous source)
#define LG_EPT (LG_T * LG_BK / 256)   // elements per thread and operand
template <bool KC> __device__ __forceinline__ int lg_idx(int row, int k) { return KC ? row * LG_PK + k : k * LG_PM + row; }

constexpr int LG_LDS = LG_BK * LG_PM > LG_T * LG_PK ? LG_BK * LG_PM : LG_T * LG_PK;   // floats per operand tile
// one 32 x 32 output tile (bx, by) of C = A B^T (+ bias, ReLU); As / Bs: LG_LDS floats each
template <bool A_KC, bool B_KC>
__device__ __forceinline__ void gemm_f32_tile(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ c,
                                              const float* __restrict__ bias, int M, int N, int K, int64_t sam, int64_t sak, int64_t sbn,
                                              int64_t sbk, int64_t ldc, int relu, int bx, int by, float* As, float* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int m0 = by * LG_T, n0 = bx * LG_T;
  const int wm = wid >> 1, wn = wid & 1;
  f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ra[LG_EPT], rb[LG_EPT];
  // element e = tid + 256*i of a 32 x LG_BK tile: k-contiguous sources walk k fastest, else rows fastest
  auto coords = [&](bool kc, int e, int& row, int& kk) { if (kc) { row = e / LG_BK; kk = e % LG_BK; } else { row = e % LG_T; kk = e / LG_T; } };
#define LG_FETCH(k0)                                                                                    \
  _Pragma("unroll") for (int i = 0; i < LG_EPT; ++i) {                                                  \
    int row, kk;                                                                                        \
    coords(A_KC, tid + 256 * i, row, kk);                                                               \
    ra[i] = (m0 + row < M && (k0) + kk < K) ? a[(int64_t)(m0 + row) * sam + (int64_t)((k0) + kk) * sak] : 0.f; \
    coords(B_KC, tid + 256 * i, row, kk);                                                               \
    rb[i] = (n0 + row < N && (k0) + kk < K) ? b[(int64_t)(n0 + row) * sbn + (int64_t)((k0) + kk) * sbk] : 0.f; \
  }
  LG_FETCH(0)
  for (int k0 = 0; k0 < K; k0 += LG_BK) {
#pragma unroll
    for (int i = 0; i < LG_EPT; ++i) {
      int row, kk;
      coords(A_KC, tid + 256 * i, row, kk);
      As[lg_idx<A_KC>(row, kk)] = ra[i];
      coords(B_KC, tid + 256 * i, row, kk);
      Bs[lg_idx<B_KC>(row, kk)] = rb[i];
    }
    __syncthreads();
    if (k0 + LG_BK < K) { LG_FETCH(k0 + LG_BK) }   // in flight while this step is multiplied
#pragma unroll
    for (int s = 0; s < LG_BK / 4; ++s) {
      float fa = As[lg_idx<A_KC>(wm * 16 + l15, 4 * s + g)];
      float fb = Bs[lg_idx<B_KC>(wn * 16 + l15, 4 * s + g)];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fb, fa, acc, 0, 0, 0);
    }
    __syncthreads();
  }
#undef LG_FETCH
  // D[i = n][j = m]: lane holds m = l15, n = 4g + reg
  const int m = m0 + wm * 16 + l15;
  if (m < M) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int n = n0 + wn * 16 + 4 * g + r;
      if (n < N) {
        float v = acc[r] + (bias ? bias[n] : 0.f);
        if (relu) v = fmaxf(v, 0.f);
        c[(int64_t)m * ldc + n] = v;
      }
    }
  }
}
template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ c, const float* __restrict__ bias, int M,
                                                       int N, int K, int64_t sam, int64_t sak, int64_t sbn,
                                                       int64_t sbk, int64_t ldc, int relu, int kchunk, int64_t sab,
                                                       int64_t sbb, int64_t scb) {
  __shared__ float As[LG_LDS];
  __shared__ float Bs[LG_LDS];
  if (kchunk < 0) {   // batched: blockIdx.z = batch index (no split-K)
    a += (int64_t)blockIdx.z * sab; b += (int64_t)blockIdx.z * sbb; c += (int64_t)blockIdx.z * scb;
  }
  // split-K (kchunk > 0): slice blockIdx.z covers k in [z*kchunk, (z+1)*kchunk) and writes its own M x ldc
  // partial matrix; the caller sums the slices.  Used by the weight-gradient GEMMs whose K is batch*tokens.
  if (kchunk > 0) {
    const int kb = blockIdx.z * kchunk;
    a += (int64_t)kb * sak; b += (int64_t)kb * sbk;
    c += (int64_t)blockIdx.z * M * ldc;
    K = min(kchunk, K - kb);
  }
  gemm_f32_tile<A_KC, B_KC>(a, b, c, bias, M, N, K, sam, sak, sbn, sbk, ldc, relu, blockIdx.x, blockIdx.y, As, Bs);
}
// Backward of a small Linear (M = batch rows) in ONE launch: the tiles of dx = g w, the tiles of dw = g^T x and the column sums db = sum_m g,
// selected by block index (three dependent-free launches of 5 - 11 us each were 4.5 us of launch latency apiece: 16 Linear layers per head step)
__global__ __launch_bounds__(256) void linear_bwd_small_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ x,
                                                               float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, int M, int K,
                                                               int N, int nx_dx, int n_dx, int nx_dw, int n_dw) {
  __shared__ float As[LG_LDS];
  __shared__ float Bs[LG_LDS];
  int b = blockIdx.x;
  if (b < n_dx) {   // dx[m][k] = sum_n g[m][n] w[n][k]
    gemm_f32_tile<true, false>(g, w, dx, nullptr, M, K, N, N, 1, 1, K, K, 0, b % nx_dx, b / nx_dx, As, Bs);
    return;
  }
  b -= n_dx;
  if (b < n_dw) {   // dw[n][k] = sum_m g[m][n] x[m][k]
    gemm_f32_tile<false, false>(g, x, dw, nullptr, N, K, M, 1, N, 1, K, K, 0, b % nx_dw, b / nx_dw, As, Bs);
    return;
  }
  b -= n_dw;        // db: 32 columns x 8 row lanes, four independent sums per lane
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5, n = b * 32 + cx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (n < N) {
    int m = ry;
    for (; m + 24 < M; m += 32) {
      s0 += g[(int64_t)m * N + n]; s1 += g[(int64_t)(m + 8) * N + n]; s2 += g[(int64_t)(m + 16) * N + n]; s3 += g[(int64_t)(m + 24) * N + n];
    }
    for (; m < M; m += 8) s0 += g[(int64_t)m * N + n];
  }
  As[ry * 32 + cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ry == 0 && n < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += As[i * 32 + cx];
    db[n] = t;
  }
}

static int gemm_f32(const float* a, const float* b, float* c, const float* bias, int M, int N, int K, int64_t sam,
                    int64_t sak, int64_t sbn, int64_t sbk, int64_t ldc, int relu, hipStream_t st, int batch = 1,
                    int64_t sab = 0, int64_t sbb = 0, int64_t scb = 0) {
  if (M <= 0 || N <= 0) return MMSKIN_OK;
  dim3 grid(ceil_div(N, LG_T), ceil_div(M, LG_T));
  const bool akc = sak == 1, bkc = sbk == 1;
  // few output tiles but a long contraction (dW = dY^T X over batch*tokens rows): split K over blockIdx.z
  int S = 1, kchunk = 0;
  float* out = c;
  const int tiles = grid.x * grid.y;
  if (batch > 1) {
    grid.z = batch;
  } else if (K >= 4096 && tiles < 256 && !bias && !relu && ldc == N) {
    S = ceil_div(512, tiles);
    if (S > ceil_div(K, 512)) S = ceil_div(K, 512);
    if (S > 1) {
      kchunk = ceil_div(ceil_div(K, S), LG_BK) * LG_BK;
      S = ceil_div(K, kchunk);
      out = head_scratch((size_t)S * M * N * sizeof(float));
      if (!out) { mmskin_set_error("gemm_f32: split-K scratch allocation failed"); return MMSKIN_ERR_HIP; }
      grid.z = S;
    }
  }
  const int zmode = batch > 1 ? -1 : S > 1 ? kchunk : 0;   // what blockIdx.z means to the kernel: batch index / K slice / nothing
  const auto kern = akc ? (bkc ? gemm_f32_kernel<true, true> : gemm_f32_kernel<true, false>) : (bkc ? gemm_f32_kernel<false, true> : gemm_f32_kernel<false, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a, b, out, bias, M, N, K, sam, sak, sbn, sbk, ldc, relu, zmode, sab, sbb, scb);
  HIP_CHECK_RET(hipGetLastError());
  if (S > 1) {
    const int64_t n = (int64_t)M * N;
    hipLaunchKernelGGL(split_reduce_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, st, out, c, S, n);
    HIP_CHECK_RET(hipGetLastError());
  }
  return MMSKIN_OK;
}

// out[k][n] = in[n][k]  (rows x cols -> cols x rows), 32x32 tiles through LDS
__global__ void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    if (r < rows && c < cols) tile[i][threadIdx.x] = in[(int64_t)r * cols + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[(int64_t)c * rows + r] = tile[threadIdx.x][i];
  }
}

// Linear layers over batch x tokens rows with 64-multiple widths run on the exact-f32 implicit-GEMM conv kernels
static inline bool linear_big(int M, int K, int N) { return M >= 2048 && K % 64 == 0 && N % 64 == 0; }
// MMSKIN_LINEAR_DTYPE=bf16: those GEMMs take bf16 operands (fp32 accumulate, fp32 tensors at the boundary): the inputs are
// converted into library scratch, the bf16 MFMA kernels run, the result is converted back.  Default fp32 (parity mode).
// The mode is a process-wide setting: MMSKIN_LINEAR_DTYPE at first use, or mmskin_set_linear_dtype() at any time.
static int g_linear_dtype = -1;   // -1: not read yet; MMSKIN_F32 / MMSKIN_BF16
static inline bool linear_bf16() {
  if (g_linear_dtype < 0) { const char* e = getenv("MMSKIN_LINEAR_DTYPE"); g_linear_dtype = (e && !strcmp(e, "bf16")) ? 1 : 0; }
  return g_linear_dtype == 1;
}
// n elements: n / 4 four-element chunks, then the n % 4 elements behind them one by one (block 0); nothing at or past n is touched
__global__ void f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(in)[i];
    reinterpret_cast<uint2*>(out)[i] = make_uint2(f32_to_bf16_bits(v.x) | (f32_to_bf16_bits(v.y) << 16),
                                                  f32_to_bf16_bits(v.z) | (f32_to_bf16_bits(v.w) << 16));
  }
  const int64_t t = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) out[t] = (bf16_t)f32_to_bf16_bits(in[t]);
}
__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const uint2 v = reinterpret_cast<const uint2*>(in)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(bf16_bits_to_f32(v.x & 0xffffu), bf16_bits_to_f32(v.x >> 16),
                                                    bf16_bits_to_f32(v.y & 0xffffu), bf16_bits_to_f32(v.y >> 16));
  }
  const int64_t t = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) out[t] = bf16_bits_to_f32(in[t]);
}
// out[k][n] (bf16) = in[n][k] (fp32)
__global__ void transpose_f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int rows, int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    if (r < rows && c < cols) tile[i][threadIdx.x] = in[(int64_t)r * cols + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[(int64_t)c * rows + r] = (bf16_t)f32_to_bf16_bits(tile[threadIdx.x][i]);
  }
}
// one conversion / pad / un-pad pass over n chunks on stream st, and the launcher's return
#define WIDE_LAUNCH(kern, n, ...)                                                                \
  do {                                                                                           \
    hipLaunchKernelGGL(kern, dim3(grid1d_wide(n)), dim3(256), 0, st, __VA_ARGS__);               \
    HIP_CHECK_RET(hipGetLastError());                                                            \
    return MMSKIN_OK;                                                                            \
  } while (0)
// flat conversions of n > 0 elements (any n: the kernels finish the n % 4 tail; n < 4 is still one block)
static int cvt_to_bf16(const float* in, bf16_t* out, int64_t n, hipStream_t st) { WIDE_LAUNCH(f32_to_bf16_kernel, (n + 3) / 4, in, out, n); }
static int cvt_to_f32(const bf16_t* in, float* out, int64_t n, hipStream_t st) { WIDE_LAUNCH(bf16_to_f32_kernel, (n + 3) / 4, in, out, n); }

// ---- Linear layers whose widths are not multiples of 64 (DaViT's 96 / 288-wide first stage over 200 704 tokens) on the bf16 GEMM
// kernels: operands are converted into zero-padded bf16 copies (the conversion pass exists anyway), the GEMM runs on the padded
// widths, and the result is un-padded while it is widened (+ bias / activation).  Zero pad columns contribute exact zeros.

static inline bool linear_big_padded(int M, int K, int N) {
  return M >= 2048 && K % 8 == 0 && N % 8 == 0 && K >= 32 && N >= 32 && !(K % 64 == 0 && N % 64 == 0);
}
// The route of a Linear call, decided here and nowhere else.  The two shape classes are disjoint (padded widths are never both
// 64-multiples), and exact-fp32 mode has no padded route: those shapes are LIN_SMALL there.
enum LinearPath { LIN_SMALL, LIN_BIG_F32, LIN_BIG_BF16, LIN_PADDED_BF16 };
static LinearPath linear_path(int M, int K, int N) {
  const bool bf16 = linear_bf16();
  if (bf16 && linear_big_padded(M, K, N)) return LIN_PADDED_BF16;
  if (linear_big(M, K, N)) return bf16 ? LIN_BIG_BF16 : LIN_BIG_F32;
  return LIN_SMALL;
}
static inline bool linear_bf16_gemm(LinearPath p) { return p == LIN_BIG_BF16 || p == LIN_PADDED_BF16; }
// out [rows_pad][cols_pad] bf16 <- in [rows][cols] fp32, zeros elsewhere; one 16-byte chunk (8 values) per thread
__global__ void f32_to_bf16_pad_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t rows, int cols, int64_t rows_pad,
                                       int cols_pad) {
  const int cpr = cols_pad / 8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows_pad * cpr; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 8;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (r < rows && c < cols) {
      const float4 a = *reinterpret_cast<const float4*>(in + r * cols + c), b = *reinterpret_cast<const float4*>(in + r * cols + c + 4);
      o = make_uint4(f32_to_bf16_bits(a.x) | (f32_to_bf16_bits(a.y) << 16), f32_to_bf16_bits(a.z) | (f32_to_bf16_bits(a.w) << 16),
                     f32_to_bf16_bits(b.x) | (f32_to_bf16_bits(b.y) << 16), f32_to_bf16_bits(b.z) | (f32_to_bf16_bits(b.w) << 16));
    }
    *reinterpret_cast<uint4*>(out + r * cols_pad + c) = o;
  }
}
// out [rows][cols] fp32 <- act(in [rows][cols_pad] bf16 + bias); act 0 none / 1 ReLU / 2 exact GELU
__global__ void bf16_unpad_bias_act_kernel(const bf16_t* __restrict__ in, const float* __restrict__ bias, float* __restrict__ out,
                                           int64_t rows, int cols, int cols_pad, int act, const float* __restrict__ res) {
  const int cpr = cols / 8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows * cpr; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 8;
    Chunk<bf16_t> v;
    v.load(in + r * cols_pad + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = v.v[e] + (bias ? bias[c + e] : 0.f);
      if (act == 1) t = fmaxf(t, 0.f);
      else if (act == 2) t = 0.5f * t * (1.f + erff(t * 0.70710678118654752f));
      v.v[e] = t;
    }
    if (res) {   // y = residual + act(...): the block's skip connection in the same pass
      const float4 r0 = *reinterpret_cast<const float4*>(res + r * cols + c), r1 = *reinterpret_cast<const float4*>(res + r * cols + c + 4);
      v.v[0] += r0.x; v.v[1] += r0.y; v.v[2] += r0.z; v.v[3] += r0.w; v.v[4] += r1.x; v.v[5] += r1.y; v.v[6] += r1.z; v.v[7] += r1.w;
    }
    *reinterpret_cast<float4*>(out + r * cols + c) = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
    *reinterpret_cast<float4*>(out + r * cols + c + 4) = make_float4(v.v[4], v.v[5], v.v[6], v.v[7]);
  }
}
// out[k][n] (bf16, row pitch out_pitch) = in[n][k] (fp32): the transposed weight inside a zero-filled padded matrix
__global__ void transpose_f32_to_bf16_pitch_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int rows, int cols, int out_pitch) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    if (r < rows && c < cols) tile[i][threadIdx.x] = in[(int64_t)r * cols + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[(int64_t)c * out_pitch + r] = (bf16_t)f32_to_bf16_bits(tile[threadIdx.x][i]);
  }
}
static int cvt_to_bf16_pad(const float* in, bf16_t* out, int64_t rows, int cols, int64_t rows_pad, int cols_pad, hipStream_t st) {
  WIDE_LAUNCH(f32_to_bf16_pad_kernel, rows_pad * (cols_pad / 8), in, out, rows, cols, rows_pad, cols_pad);
}
static int unpad_bias_act(const bf16_t* in, const float* bias, float* out, int64_t rows, int cols, int cols_pad, int act, hipStream_t st,
                          const float* res = nullptr) {
  WIDE_LAUNCH(bf16_unpad_bias_act_kernel, rows * (cols / 8), in, bias, out, rows, cols, cols_pad, act, res);
}

__global__ void relu_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ out, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = y[i] > 0.f ? dy[i] : 0.f;
}
// blockIdx.y = row group (rows [y*per, (y+1)*per)) -> out[y*N + n]; one group = plain column sum
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, float* __restrict__ out, int M, int N,
                                                     int per) {
  __shared__ float red[8][32];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;     // 32 columns x 8 row lanes per block
  const int n = blockIdx.x * 32 + cx;
  const int m_end = min(M, ((int)blockIdx.y + 1) * per);
  out += (int64_t)blockIdx.y * N;
  float s = 0.f;
  if (n < N)
    for (int m = blockIdx.y * per + ry; m < m_end; m += 8) s += x[(int64_t)m * N + n];
  red[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && n < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][cx];
    out[n] = t;
  }
}

__global__ void add4_inplace_kernel(float* __restrict__ y, const float* __restrict__ b, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 a = reinterpret_cast<float4*>(y)[i];
    const float4 c = reinterpret_cast<const float4*>(b)[i];
    a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
    reinterpret_cast<float4*>(y)[i] = a;
  }
}

// out[c] = sum_r part[r][c] for c < ncols (c < split -> out0[c], else out1[c - split]; either may be null): 16 columns x 64 row lanes
// per block -- narrow outputs (96 .. 768 columns) still spread over 6 .. 48 workgroups, and a lane adds R / 64 rows
__global__ __launch_bounds__(1024) void rows_sum_kernel(const float* __restrict__ part, int R, int ncols, int split, float* __restrict__ out0,
                                                        float* __restrict__ out1) {
  __shared__ float red[64][17];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;
  float s0 = 0.f, s1 = 0.f;
  if (c < ncols) {
    int r = ry;
    for (; r + 64 < R; r += 128) { s0 += part[(int64_t)r * ncols + c]; s1 += part[(int64_t)(r + 64) * ncols + c]; }
    if (r < R) s0 += part[(int64_t)r * ncols + c];
  }
  red[ry][cx] = s0 + s1;
  __syncthreads();
  if (ry == 0 && c < ncols) {
    float t = 0.f;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) t += red[k][cx];
    float* out = c < split ? out0 : out1;
    if (out) out[c < split ? c : c - split] = t;
  }
}
int rows_sum(const float* part, int R, int ncols, int split, float* out0, float* out1, hipStream_t st) {
  hipLaunchKernelGGL(rows_sum_kernel, dim3(ceil_div(ncols, 16)), dim3(1024), 0, st, part, R, ncols, split, out0, out1);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// Column sums with float4 loads: CW chunk columns x (256 / CW) row lanes per block, two rows in flight per lane, one partial row
// per block, rows_sum adds the blocks.  CVT: the same pass also writes the bf16 copy (row pitch cols_pad, zero pad columns) a
// bf16-operand GEMM consumes -- Linear backward needs both from dy (bias gradient and the dgrad / wgrad operand), so dy is read once.
// GELU: x is the gradient w.r.t. gelu(z); it is multiplied by gelu'(z) on the way in (the exact-erf GELU of nn.GELU), so a Linear ->
// GELU pair's backward reads dy and z once and never writes the fp32 gradient of the pre-activation.
__device__ __forceinline__ float gelu_grad(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * __expf(-0.5f * z * z);
}
// STAR: x is the gradient w.r.t. StarReLU(z) = s * relu(z)^2 + b; it is multiplied by 2 s relu(z) on the way in, and the block's sums
// of x * relu(z)^2 and x (the gradients of s and b) go to star_part[2 * block] -- star_pair_sum adds the blocks in a fixed order.
template <bool STAR>
__device__ __forceinline__ float4 star_grad4(float4 v, float4 z, float s2, float& as, float& ab) {
  if (!STAR) return v;
  const float rx = fmaxf(z.x, 0.f), ry = fmaxf(z.y, 0.f), rz = fmaxf(z.z, 0.f), rw = fmaxf(z.w, 0.f);
  as += (v.x * rx * rx + v.y * ry * ry) + (v.z * rz * rz + v.w * rw * rw);
  ab += (v.x + v.y) + (v.z + v.w);
  return make_float4(v.x * s2 * rx, v.y * s2 * ry, v.z * s2 * rz, v.w * s2 * rw);
}
template <bool CVT, bool GELU = false, bool STAR = false>
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ x, int64_t M, int N, int rows_per_block, int CW, int lanes,
                                                      float* __restrict__ part, bf16_t* __restrict__ out16, int cols_pad,
                                                      const float* __restrict__ zg = nullptr, const float* __restrict__ star_s = nullptr,
                                                      float* __restrict__ star_part = nullptr) {
  extern __shared__ float cs_red[];           // [lanes][CW * 4]
  const int cx = threadIdx.x % CW, ly = threadIdx.x / CW;
  const float s2 = STAR ? 2.f * star_s[0] : 0.f;
  float st_s = 0.f, st_b = 0.f;
  const int c4 = blockIdx.y * CW + cx, col = c4 * 4;
  const int ncol4 = (CVT ? cols_pad : N) / 4;
  const bool real = col < N;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  if (ly < lanes && c4 < ncol4) {
    int64_t r = r0 + ly;
    for (; r + lanes < r1; r += 2 * lanes) {
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if (real) { v0 = *reinterpret_cast<const float4*>(x + r * N + col); v1 = *reinterpret_cast<const float4*>(x + (r + lanes) * N + col); }
      if (GELU && real) {
        const float4 z0 = *reinterpret_cast<const float4*>(zg + r * N + col), z1 = *reinterpret_cast<const float4*>(zg + (r + lanes) * N + col);
        v0.x *= gelu_grad(z0.x); v0.y *= gelu_grad(z0.y); v0.z *= gelu_grad(z0.z); v0.w *= gelu_grad(z0.w);
        v1.x *= gelu_grad(z1.x); v1.y *= gelu_grad(z1.y); v1.z *= gelu_grad(z1.z); v1.w *= gelu_grad(z1.w);
      }
      if (STAR && real) {
        v0 = star_grad4<STAR>(v0, *reinterpret_cast<const float4*>(zg + r * N + col), s2, st_s, st_b);
        v1 = star_grad4<STAR>(v1, *reinterpret_cast<const float4*>(zg + (r + lanes) * N + col), s2, st_s, st_b);
      }
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
      if (CVT) {
        *reinterpret_cast<uint2*>(out16 + r * cols_pad + col) = make_uint2(f32_to_bf16_bits(v0.x) | (f32_to_bf16_bits(v0.y) << 16), f32_to_bf16_bits(v0.z) | (f32_to_bf16_bits(v0.w) << 16));
        *reinterpret_cast<uint2*>(out16 + (r + lanes) * cols_pad + col) = make_uint2(f32_to_bf16_bits(v1.x) | (f32_to_bf16_bits(v1.y) << 16), f32_to_bf16_bits(v1.z) | (f32_to_bf16_bits(v1.w) << 16));
      }
    }
    if (r < r1) {
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (real) v0 = *reinterpret_cast<const float4*>(x + r * N + col);
      if (GELU && real) {
        const float4 z0 = *reinterpret_cast<const float4*>(zg + r * N + col);
        v0.x *= gelu_grad(z0.x); v0.y *= gelu_grad(z0.y); v0.z *= gelu_grad(z0.z); v0.w *= gelu_grad(z0.w);
      }
      if (STAR && real) v0 = star_grad4<STAR>(v0, *reinterpret_cast<const float4*>(zg + r * N + col), s2, st_s, st_b);
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      if (CVT) *reinterpret_cast<uint2*>(out16 + r * cols_pad + col) = make_uint2(f32_to_bf16_bits(v0.x) | (f32_to_bf16_bits(v0.y) << 16), f32_to_bf16_bits(v0.z) | (f32_to_bf16_bits(v0.w) << 16));
    }
    *reinterpret_cast<float4*>(cs_red + ((size_t)ly * CW + cx) * 4) = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CW * 4; i += 256) {
    const int cc = blockIdx.y * CW * 4 + i;
    if (cc < N) {
      float t = 0.f;
      for (int l = 0; l < lanes; ++l) t += cs_red[(size_t)l * CW * 4 + i];
      part[(int64_t)blockIdx.x * N + cc] = t;
    }
  }
  if (STAR) {
    __shared__ float st_red[2][4];
    st_s = wave_sum(st_s); st_b = wave_sum(st_b);
    if ((threadIdx.x & 63) == 0) { st_red[0][threadIdx.x >> 6] = st_s; st_red[1][threadIdx.x >> 6] = st_b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float* o = star_part + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
      o[0] = (st_red[0][0] + st_red[0][1]) + (st_red[0][2] + st_red[0][3]);
      o[1] = (st_red[1][0] + st_red[1][1]) + (st_red[1][2] + st_red[1][3]);
    }
  }
}
// out[0..1] = sum over the nb pairs part[2 i], part[2 i + 1], in a fixed order (one block): the StarReLU scalar gradients
__global__ __launch_bounds__(256) void star_pair_sum_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
  __shared__ float red[2][4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { a += part[2 * i]; b += part[2 * i + 1]; }
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}
int star_pair_sum(const float* part, int nb, float* out, hipStream_t st) {
  hipLaunchKernelGGL(star_pair_sum_kernel, dim3(1), dim3(256), 0, st, part, nb, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
struct Colsum4Plan { int CW, lanes, gy, nbx, rpb; };
static inline Colsum4Plan colsum4_plan(int64_t M, int ncol4) {
  Colsum4Plan g;
  g.CW = ncol4 <= 32 ? ncol4 : 32;
  g.lanes = 256 / g.CW;
  g.gy = ceil_div(ncol4, g.CW);
  int64_t want = 1024 / g.gy;
  if (want < 1) want = 1;
  int64_t rpb = (M + want - 1) / want;
  const int64_t lo = (int64_t)g.lanes * 4;                  // a lane adds at least four rows
  if (rpb < lo) rpb = lo;
  g.rpb = (int)rpb;
  g.nbx = (int)((M + rpb - 1) / rpb);
  return g;
}
static inline size_t colsum4_part_bytes(int N) { return (size_t)1024 * N * sizeof(float); }
// out[N] = column sums of x [M][N]; out16 != null: also the bf16 copy [M][cols_pad].  part: colsum4_part_bytes(N) of scratch.
// star_s / star_sb (with z_gelu as the StarReLU pre-activation z): the StarReLU derivative instead of GELU's, and star_sb[0..1] = the
// gradients of its s and b; star_part: 2 * colsum4_blocks floats.
static inline int colsum4_blocks(int64_t M, int ncol4) { const Colsum4Plan g = colsum4_plan(M, ncol4); return g.nbx * g.gy; }
static int colsum4(const float* x, float* out, int64_t M, int N, float* part, bf16_t* out16, int cols_pad, hipStream_t st,
                   const float* z_gelu = nullptr, const float* star_s = nullptr, float* star_sb = nullptr, float* star_part = nullptr) {
  const Colsum4Plan g = colsum4_plan(M, (out16 ? cols_pad : N) / 4);
  const size_t lds = (size_t)g.lanes * g.CW * 4 * sizeof(float);
  if (out16 && z_gelu && star_s) {
    hipLaunchKernelGGL((colsum4_kernel<true, false, true>), dim3(g.nbx, g.gy), dim3(256), lds, st, x, M, N, g.rpb, g.CW, g.lanes, part, out16,
                       cols_pad, z_gelu, star_s, star_part);
    HIP_CHECK_RET(hipGetLastError());
    int rc = star_pair_sum(star_part, g.nbx * g.gy, star_sb, st);
    if (rc) return rc;
    return out ? rows_sum(part, g.nbx, N, N, out, nullptr, st) : MMSKIN_OK;
  }
  if (out16 && z_gelu) hipLaunchKernelGGL((colsum4_kernel<true, true>), dim3(g.nbx, g.gy), dim3(256), lds, st, x, M, N, g.rpb, g.CW, g.lanes, part, out16, cols_pad, z_gelu);
  else if (out16) hipLaunchKernelGGL(colsum4_kernel<true>, dim3(g.nbx, g.gy), dim3(256), lds, st, x, M, N, g.rpb, g.CW, g.lanes, part, out16, cols_pad);
  else hipLaunchKernelGGL(colsum4_kernel<false>, dim3(g.nbx, g.gy), dim3(256), lds, st, x, M, N, g.rpb, g.CW, g.lanes, part, out16, cols_pad);
  HIP_CHECK_RET(hipGetLastError());
  return rows_sum(part, g.nbx, N, N, out, nullptr, st);
}
static int colsum(const float* x, float* out, int M, int N, hipStream_t st) {
  if (N % 4 == 0 && M >= 2048) {
    float* part = head_scratch(colsum4_part_bytes(N));
    if (!part) { mmskin_set_error("colsum: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    return colsum4(x, out, M, N, part, nullptr, 0, st);
  }
  const int G = M >= 2048 ? (M / 256 > 128 ? 128 : M / 256) : 1;
  if (G <= 1) {
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 32)), dim3(256), 0, st, x, out, M, N, M);
  } else {
    float* part = head_scratch((size_t)G * N * sizeof(float));
    if (!part) { mmskin_set_error("colsum: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 32), G), dim3(256), 0, st, x, part, M, N, ceil_div(M, G));
    hipLaunchKernelGGL(split_reduce_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, part, out, G, (int64_t)N);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
// h16 [rows][cols_pad] (bf16, zero pad columns) = gelu(z [rows][cols]): the operand of the MLP's second Linear straight from the
// pre-activation -- gelu(z) is never written in fp32 (4 values per thread)
__global__ void gelu_to_bf16_kernel(const float* __restrict__ z, bf16_t* __restrict__ h16, int64_t rows, int cols, int cols_pad) {
  const int cpr = cols_pad / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows * cpr; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 4;
    uint2 o = make_uint2(0u, 0u);
    if (c < cols) {
      const float4 v = *reinterpret_cast<const float4*>(z + r * cols + c);
      o = make_uint2(f32_to_bf16_bits(gelu_exact(v.x)) | (f32_to_bf16_bits(gelu_exact(v.y)) << 16),
                     f32_to_bf16_bits(gelu_exact(v.z)) | (f32_to_bf16_bits(gelu_exact(v.w)) << 16));
    }
    *reinterpret_cast<uint2*>(h16 + r * cols_pad + c) = o;
  }
}
// h16 = bf16(s relu(z)^2 + b) (timm StarReLU), zero pad columns: the operand of the MLP's second Linear
__global__ void star_relu_to_bf16_kernel(const float* __restrict__ z, const float* __restrict__ sp, const float* __restrict__ bp,
                                         bf16_t* __restrict__ h16, int64_t rows, int cols, int cols_pad) {
  const int cpr = cols_pad / 4;
  const float s = sp[0], b = bp[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows * cpr; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 4;
    uint2 o = make_uint2(0u, 0u);
    if (c < cols) {
      const float4 v = *reinterpret_cast<const float4*>(z + r * cols + c);
      const float rx = fmaxf(v.x, 0.f), ry = fmaxf(v.y, 0.f), rz = fmaxf(v.z, 0.f), rw = fmaxf(v.w, 0.f);
      o = make_uint2(f32_to_bf16_bits(s * (rx * rx) + b) | (f32_to_bf16_bits(s * (ry * ry) + b) << 16),
                     f32_to_bf16_bits(s * (rz * rz) + b) | (f32_to_bf16_bits(s * (rw * rw) + b) << 16));
    }
    *reinterpret_cast<uint2*>(h16 + r * cols_pad + c) = o;
  }
}

// ------------------------------------------------------------------ scratch layouts and bf16 GEMM operands
// Places a scratch layout: `layout` runs once on a null base for the byte count, that much of head_scratch is taken, and `layout`
// runs again on the buffer -- the request and the carve-up are one piece of code.  False when the allocation failed; a layout that
// takes nothing (every operand was handed in ready) touches no buffer.
template <typename F>
static bool carve_scratch(F layout, int slot = 0) {
  Carver size(nullptr);
  layout(size);
  if (!size.cur) return true;
  void* buf = head_scratch(size.cur, slot);
  if (!buf) return false;
  Carver c(buf);
  layout(c);
  return true;
}
// fp32 [rows][cols] -> a bf16 GEMM operand: the padded route writes [rows_pad][cols_pad] with zeros around it (its kernel also when a
// width happens to need no padding), the 64-multiple route converts the flat range
static int cvt_operand(bool padded, const float* in, bf16_t* out, int64_t rows, int cols, int64_t rows_pad, int cols_pad, hipStream_t st) {
  return padded ? cvt_to_bf16_pad(in, out, rows, cols, rows_pad, cols_pad, st) : cvt_to_bf16(in, out, rows * cols, st);
}
// The bf16 operands of a forward GEMM on LIN_BIG_BF16 / LIN_PADDED_BF16.  The caller names what it has; linear_operands() lays
// out scratch as [x][w][y16] (each only if needed), converts x, then w, and leaves what launch_conv_fwd<bf16_t> reads in x16 / w16.
struct LinOperands {
  const float* x = nullptr;      // fp32 input, converted per call ...
  const bf16_t* x16 = nullptr;   // ... or the operand already in bf16 ([M][mmskin_linear_x16_pitch], zero pad columns)
  bf16_t* x16_keep = nullptr;    // the conversion of x goes here instead of into scratch: the caller hands it back to the backward's
                                 // weight-gradient GEMM (no second conversion of x, half the saved bytes)
  const float* w = nullptr;      // fp32 weight, converted per call ...
  const bf16_t* w16 = nullptr;   // ... or a cached bf16 conversion of a frozen weight
  bool hold_x = false;           // x's scratch region stays in the layout even when nothing is converted into it
  bf16_t* y16 = nullptr;         // out, padded route: room for the GEMM's bf16 result [M][pad64(N)]
};
static int linear_operands(LinearPath path, LinOperands& o, int M, int K, int N, const char* who, hipStream_t st) {
  const bool padded = path == LIN_PADDED_BF16;
  const int Kp = padded ? pad64(K) : K, Np = padded ? pad64(N) : N;
  bf16_t *xs = nullptr, *ws = nullptr;
  const bool placed = carve_scratch([&](Carver& c) {
    if (o.hold_x || !o.x16) xs = c.take<bf16_t>((size_t)M * Kp);
    if (!o.w16) ws = c.take<bf16_t>((size_t)Np * Kp);
    if (padded) o.y16 = c.take<bf16_t>((size_t)M * Np);
  });
  if (!placed) { mmskin_set_error("%s: scratch allocation failed", who); return MMSKIN_ERR_HIP; }
  int rc;
  if (!o.x16) {
    bf16_t* xc = o.x16_keep ? o.x16_keep : xs;
    if ((rc = cvt_operand(padded, o.x, xc, M, K, M, Kp, st))) return rc;
    o.x16 = xc;
  }
  if (!o.w16) {
    if ((rc = cvt_operand(padded, o.w, ws, N, K, Np, Kp, st))) return rc;
    o.w16 = ws;
  }
  return MMSKIN_OK;
}
// y (fp32 or bf16) = epilogue f of x (fp32 / bf16) w^T (fp32 / cached bf16) on LIN_BIG_BF16: what mmskin_linear_forward_ex and
// mmskin_linear_lane launch once they have filled f (`fused`: f asks for anything beyond a plain bf16 store)
static int linear_big_bf16_ex(const void* x, int x_dtype, const void* w, int w_dtype, FwdFuse& f, bool fused, void* y, int y_dtype, int M,
                              int K, int N, const char* who, hipStream_t st) {
  LinOperands op;
  if (x_dtype == 1) op.x16 = reinterpret_cast<const bf16_t*>(x); else op.x = reinterpret_cast<const float*>(x);
  if (w_dtype == 1) op.w16 = reinterpret_cast<const bf16_t*>(w); else op.w = reinterpret_cast<const float*>(w);
  const int rc = linear_operands(LIN_BIG_BF16, op, M, K, N, who, st);
  if (rc) return rc;
  ConvShape s = {M, 1, 1, K, N, 1, 1, 1, 0};
  if (y_dtype == 0) f.out_f32 = reinterpret_cast<float*>(y);
  return launch_conv_fwd<bf16_t>(s, op.x16, op.w16, reinterpret_cast<bf16_t*>(y), nullptr, nullptr, st, (fused || y_dtype == 0) ? &f : nullptr);
}

// ------------------------------------------------------------------ Linear forward / backward
// y = act(x w^T + b) on whichever route the shape and mode select; op names x (fp32, or already bf16: large bf16 GEMM routes only), w
// (fp32) and optionally where to keep x's bf16 copy.  res (those routes only): y = res + act(...), res fp32 [M][N] -- a transformer
// block's residual add.
static int linear_forward_impl(LinOperands op, const float* b, const float* res, float* y, int M, int K, int N, int relu, void* stream) {
  const float *x = op.x, *w = op.w;
  const LinearPath path = linear_path(M, K, N);
  ARG_CHECK(!res || linear_bf16_gemm(path), "linear_forward: the fused residual needs the bf16 large-GEMM path (shape / mode)");
  ARG_CHECK((x || op.x16) && w && y && M > 0 && K > 0 && N > 0, "linear_forward: bad argument");
  ARG_CHECK(!op.x16 || linear_bf16_gemm(path), "linear_forward: a bf16 operand needs the bf16 large-GEMM path (shape / mode)");
  ARG_CHECK(relu >= 0 && relu <= 2, "linear_forward: activation %d (0 none, 1 ReLU, 2 exact GELU)", relu);
  hipStream_t st = ST(stream);
  int rc;
  if (linear_bf16_gemm(path)) {
    op.hold_x = true;   // this entry's layout is [x][w]([y16]) whether or not x is converted into it
    if ((rc = linear_operands(path, op, M, K, N, "linear_forward", st))) return rc;
    if (path == LIN_PADDED_BF16) {   // the GEMM runs on the padded widths; bias / activation / residual ride the un-padding pass
      const int Np = pad64(N);
      ConvShape s = {M, 1, 1, pad64(K), Np, 1, 1, 1, 0};
      if ((rc = launch_conv_fwd<bf16_t>(s, op.x16, op.w16, op.y16, nullptr, nullptr, st, nullptr))) return rc;
      return unpad_bias_act(op.y16, b, y, M, N, Np, relu, st, res);
    }
    // bf16 operands, fp32 accumulate; bias + activation + the widening to fp32 all happen in the GEMM epilogue
    ConvShape s = {M, 1, 1, K, N, 1, 1, 1, 0};
    const bool res_epi = res && N % 128 == 0;   // the residual epilogue stores whole 128-column tiles; other widths add in a pass of their own
    FwdFuse f; f.bias = b; f.relu = relu == 1; f.gelu = relu == 2; f.out_f32 = y; f.res_f32 = res_epi ? res : nullptr;
    if ((rc = launch_conv_fwd<bf16_t>(s, op.x16, op.w16, reinterpret_cast<bf16_t*>(y), nullptr, nullptr, st, &f))) return rc;
    if (res && !res_epi) WIDE_LAUNCH(add4_inplace_kernel, (int64_t)M * N / 4, y, res, (int64_t)M * N / 4);
    return MMSKIN_OK;
  }
  if (path == LIN_BIG_F32) {   // tokens x hidden GEMMs of the text encoders: the exact-f32 implicit-GEMM kernel as a 1x1 conv
    ConvShape s = {M, 1, 1, K, N, 1, 1, 1, 0};
    FwdFuse f; f.bias = b; f.relu = relu == 1; f.gelu = relu == 2;
    return launch_conv_fwd<float>(s, x, w, y, nullptr, nullptr, st, (b || relu) ? &f : nullptr);
  }
  rc = gemm_f32(x, w, y, b, M, N, K, K, 1, K, 1, N, relu == 1, st);
  if (rc || relu != 2) return rc;
  return mmskin_gelu_forward(y, y, (int64_t)M * N, stream);   // in place: element i only
}

struct LinearBwdOpt {
  const void* x16_kept = nullptr;   // in x's place: the bf16 operand copy the forward kept ([M][mmskin_linear_x16_pitch])
  const float* star_s = nullptr;    // z_gelu is a StarReLU pre-activation: 2 s relu(z) instead of gelu'(z) ...
  float* star_sb = nullptr;         // ... and the gradients of its s and b land in star_sb[0..1]
};
static int linear_backward_impl(const float* dy, const float* x, const float* w, const float* y_relu, const float* z_gelu, float* dy_scratch,
                                float* dx, float* dw, float* db, int M, int K, int N, void* stream, const LinearBwdOpt& o = LinearBwdOpt()) {
  ARG_CHECK(dy && M > 0 && K > 0 && N > 0, "linear_backward: bad argument");
  ARG_CHECK(!(y_relu && z_gelu), "linear_backward: one activation");
  hipStream_t st = ST(stream);
  const float* g = dy;
  const LinearPath path = linear_path(M, K, N);
  const bool bf16_gemm = linear_bf16_gemm(path);
  ARG_CHECK(!o.x16_kept || bf16_gemm, "linear_backward: the kept bf16 operand belongs to the bf16 large-GEMM path (mode changed since the forward?)");
  ARG_CHECK(!o.star_s || (bf16_gemm && z_gelu && o.star_sb), "linear_backward: StarReLU needs the bf16 large-GEMM path, z and the scalar gradients");
  int rc;
  if (z_gelu && !bf16_gemm) {   // no conversion pass to fold the GELU derivative into: its own pass
    ARG_CHECK(dy_scratch, "linear_backward: dy_scratch required with z_gelu");
    if ((rc = mmskin_gelu_backward(dy, z_gelu, dy_scratch, (int64_t)M * N, stream))) return rc;
    g = dy_scratch; z_gelu = nullptr;
  }
  if (y_relu) {
    ARG_CHECK(dy_scratch, "linear_backward: dy_scratch required with y_relu");
    hipLaunchKernelGGL(relu_mask_kernel, dim3(grid1d((int64_t)M * N)), dim3(256), 0, st, dy, y_relu, dy_scratch, (int64_t)M * N);
    HIP_CHECK_RET(hipGetLastError());
    g = dy_scratch;
  }
  if (bf16_gemm) {
    const bool padded = path == LIN_PADDED_BF16;
    const int Kp = padded ? pad64(K) : K, Np = padded ? pad64(N) : N;
    ConvShape s = {M, 1, 1, Kp, Np, 1, 1, 1, 0};
    const size_t slab_bytes = conv_wgrad_slab_bytes(s);
    const size_t star_floats = o.star_s ? (size_t)2 * colsum4_blocks(M, Np / 4) : 0;
    bf16_t *g16 = nullptr, *t16 = nullptr, *w16 = nullptr;   // dy; dx (padded route) or x; w transposed
    WgradSlab slab = {nullptr, slab_bytes / sizeof(float)};
    float *star_part = nullptr, *part = nullptr;
    const bool placed = carve_scratch([&](Carver& c) {
      g16 = c.take<bf16_t>((size_t)M * Np);
      t16 = c.take<bf16_t>((size_t)M * Kp);
      w16 = c.take<bf16_t>((size_t)Np * Kp);
      slab.p = reinterpret_cast<float*>(c.take<unsigned char>(slab_bytes));
      if (star_floats) star_part = c.take<float>(star_floats);
      part = reinterpret_cast<float*>(c.take<unsigned char>(colsum4_part_bytes(N)));
    });
    if (!placed) { mmskin_set_error("linear_backward: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    if (db || z_gelu) {   // bias gradient (and the GELU / StarReLU derivative) from the pass that converts dy
      if ((rc = colsum4(g, db, M, N, part, g16, Np, st, z_gelu, o.star_s, o.star_sb, star_part))) return rc;
      db = nullptr;
    } else if ((rc = cvt_operand(padded, g, g16, M, N, M, Np, st))) return rc;
    if (dx) {
      ARG_CHECK(w, "linear_backward: w required for dx");
      if (padded) {
        HIP_CHECK_RET(hipMemsetAsync(w16, 0, (size_t)Np * Kp * 2, st));
        hipLaunchKernelGGL(transpose_f32_to_bf16_pitch_kernel, dim3(ceil_div(K, 32), ceil_div(N, 32)), dim3(32, 8), 0, st, w, w16, N, K, Np);
        HIP_CHECK_RET(hipGetLastError());
        if ((rc = launch_conv_dgrad<bf16_t>(s, g16, w16, t16, (const bf16_t*)nullptr, st))) return rc;   // dx [M][Kp] in bf16, un-padded while widened
        if ((rc = unpad_bias_act(t16, nullptr, dx, M, K, Kp, 0, st))) return rc;
      } else {
        hipLaunchKernelGGL(transpose_f32_to_bf16_kernel, dim3(ceil_div(K, 32), ceil_div(N, 32)), dim3(32, 8), 0, st, w, w16, N, K);
        HIP_CHECK_RET(hipGetLastError());
        // dx = g w as a FORWARD 1x1 conv over the transposed weight (w16 [K][N] is its [Cout][Cin] layout): the light epilogue writes
        // fp32 straight into dx -- no bf16 round trip and widening pass (10 us x 57 per DaViT step)
        ConvShape sd = {M, 1, 1, N, K, 1, 1, 1, 0};
        FwdFuse f; f.out_f32 = dx;
        if ((rc = launch_conv_fwd<bf16_t>(sd, g16, w16, reinterpret_cast<bf16_t*>(dx), nullptr, nullptr, st, &f))) return rc;
      }
    }
    if (dw) {
      ARG_CHECK(x || o.x16_kept, "linear_backward: x required for dw");
      const bf16_t* xo = reinterpret_cast<const bf16_t*>(o.x16_kept);
      if (!xo) { if ((rc = cvt_operand(padded, x, t16, M, K, M, Kp, st))) return rc; xo = t16; }
      // padded operands: the reduction drops the pad rows / channels and writes the [N][K] gradient directly
      if ((rc = launch_conv_wgrad<bf16_t>(s, g16, xo, slab, dw, st, padded ? N : 0, padded ? K : 0))) return rc;
    }
    if (db && (rc = colsum(g, db, M, N, st))) return rc;
    return MMSKIN_OK;
  }
  if (path == LIN_BIG_F32) {
    ConvShape s = {M, 1, 1, K, N, 1, 1, 1, 0};
    const size_t slab_bytes = conv_wgrad_slab_bytes(s);
    float* wt = nullptr;
    WgradSlab slab = {nullptr, slab_bytes / sizeof(float)};
    const bool placed = carve_scratch([&](Carver& c) {
      wt = c.take<float>((size_t)N * K);
      slab.p = reinterpret_cast<float*>(c.take<unsigned char>(slab_bytes));
    });
    if (!placed) { mmskin_set_error("linear_backward: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    if (dx) {
      ARG_CHECK(w, "linear_backward: w required for dx");
      hipLaunchKernelGGL(transpose_f32_kernel, dim3(ceil_div(K, 32), ceil_div(N, 32)), dim3(32, 8), 0, st, w, wt, N, K);
      HIP_CHECK_RET(hipGetLastError());
      if ((rc = launch_conv_dgrad<float>(s, g, wt, dx, (const float*)nullptr, st))) return rc;
    }
    if (dw) {
      ARG_CHECK(x, "linear_backward: x required for dw");
      if ((rc = launch_conv_wgrad<float>(s, g, x, slab, dw, st))) return rc;
    }
    if (db && (rc = colsum(g, db, M, N, st))) return rc;
    return MMSKIN_OK;
  }
  if (M < 4096 && (dx || dw || db)) {   // (a longer contraction takes the split-K form of the separate launches)
    ARG_CHECK((!dx || w) && (!dw || x), "linear_backward: w / x required");
    const int nx_dx = ceil_div(K, LG_T), n_dx = dx ? nx_dx * ceil_div(M, LG_T) : 0;
    const int nx_dw = ceil_div(K, LG_T), n_dw = dw ? nx_dw * ceil_div(N, LG_T) : 0;
    const int n_db = db ? ceil_div(N, 32) : 0;
    hipLaunchKernelGGL(linear_bwd_small_kernel, dim3(n_dx + n_dw + n_db), dim3(256), 0, st, g, w, x, dx, dw, db, M, K, N, nx_dx, n_dx, nx_dw, n_dw);
    HIP_CHECK_RET(hipGetLastError());
    return MMSKIN_OK;
  }
  if (dx) {  // dx[m][k] = sum_n g[m][n] * w[n][k]
    ARG_CHECK(w, "linear_backward: w required for dx");
    if ((rc = gemm_f32(g, w, dx, nullptr, M, K, N, N, 1, 1, K, K, 0, st))) return rc;
  }
  if (dw) {  // dw[n][k] = sum_m g[m][n] * x[m][k]
    ARG_CHECK(x, "linear_backward: x required for dw");
    if ((rc = gemm_f32(g, x, dw, nullptr, N, K, M, 1, N, 1, K, K, 0, st))) return rc;
  }
  if (db && (rc = colsum(g, db, M, N, st))) return rc;
  return MMSKIN_OK;
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

int mmskin_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int K, int N, int relu,
                          void* stream) {
  LinOperands op; op.x = x; op.w = w;
  return linear_forward_impl(op, b, nullptr, y, M, K, N, relu, stream);
}
// Row pitch (elements) of the bf16 operand copy the current mode's large-GEMM path makes of an [M][K] input, 0 when this shape / mode
// does not take that path (then there is nothing to keep).
// The route linear_path gives M x K x N in the current mode (MMSKIN_LINEAR_* in mmskin.h mirror LinearPath), -1 on a bad shape
int mmskin_linear_route(int M, int K, int N) {
  static_assert(LIN_SMALL == MMSKIN_LINEAR_SMALL && LIN_BIG_F32 == MMSKIN_LINEAR_BIG_F32 && LIN_BIG_BF16 == MMSKIN_LINEAR_BIG_BF16 &&
                LIN_PADDED_BF16 == MMSKIN_LINEAR_PADDED_BF16, "mmskin.h documents the LinearPath values");
  return (M > 0 && K > 0 && N > 0) ? (int)linear_path(M, K, N) : -1;
}
int mmskin_linear_x16_pitch(int M, int K, int N) {
  const LinearPath path = (M > 0 && K > 0 && N > 0) ? linear_path(M, K, N) : LIN_SMALL;
  return path == LIN_PADDED_BF16 ? pad64(K) : path == LIN_BIG_BF16 ? K : 0;
}
// y = act(x16 w^T + b) with the operand already in bf16 (e.g. written by mmskin_gelu_forward_bf16): no conversion pass
int mmskin_linear_forward_x16(const void* x16, const float* w, const float* b, const float* res, float* y, int M, int K, int N, int relu,
                              void* stream) {
  ARG_CHECK(x16, "linear_forward_x16: null operand");
  LinOperands op; op.x16 = reinterpret_cast<const bf16_t*>(x16); op.w = w;
  return linear_forward_impl(op, b, res, y, M, K, N, relu, stream);
}
int mmskin_gelu_forward_bf16(const float* z, void* h16, int64_t rows, int cols, int cols_pad, void* stream) {
  ARG_CHECK(z && h16 && rows > 0 && cols > 0 && cols % 4 == 0 && cols_pad % 4 == 0 && cols_pad >= cols, "gelu_forward_bf16: bad argument");
  hipStream_t st = ST(stream);
  WIDE_LAUNCH(gelu_to_bf16_kernel, rows * (cols_pad / 4), z, reinterpret_cast<bf16_t*>(h16), rows, cols, cols_pad);
}
int mmskin_star_relu_forward_bf16(const float* z, const float* s, const float* b, void* h16, int64_t rows, int cols, int cols_pad, void* stream) {
  ARG_CHECK(z && s && b && h16 && rows > 0 && cols > 0 && cols % 4 == 0 && cols_pad % 4 == 0 && cols_pad >= cols, "star_relu_forward_bf16: bad argument");
  hipStream_t st = ST(stream);
  WIDE_LAUNCH(star_relu_to_bf16_kernel, rows * (cols_pad / 4), z, s, b, reinterpret_cast<bf16_t*>(h16), rows, cols, cols_pad);
}
int mmskin_linear_forward_keep(const float* x, const float* w, const float* b, const float* res, float* y, void* x16_keep, int M, int K,
                               int N, int relu, void* stream) {
  ARG_CHECK(x16_keep && mmskin_linear_x16_pitch(M, K, N) > 0, "linear_forward_keep: no bf16 operand copy for this shape / mode");
  LinOperands op; op.x = x; op.w = w; op.x16_keep = reinterpret_cast<bf16_t*>(x16_keep);
  return linear_forward_impl(op, b, res, y, M, K, N, relu, stream);
}

// Linear with bf16 tensors at either end (the inference lane of the transformer encoders in bf16-operand mode): x and / or y may be
// bf16, so consecutive layers hand activations over without fp32 <-> bf16 conversion passes.  Shapes off the large-GEMM path (or
// fp32 operand mode) fall back to the fp32 entry point through scratch conversions.
int mmskin_linear_forward_ex(const void* x, int x_dtype, const float* w, const float* b, void* y, int y_dtype, int M, int K, int N,
                             int act, void* stream) {
  ARG_CHECK(x && w && y && M > 0 && K > 0 && N > 0, "linear_forward_ex: bad argument");
  ARG_CHECK((x_dtype == 0 || x_dtype == 1) && (y_dtype == 0 || y_dtype == 1) && act >= 0 && act <= 2, "linear_forward_ex: dtype / activation");
  hipStream_t st = ST(stream);
  int rc;
  if (linear_path(M, K, N) == LIN_BIG_BF16) {
    FwdFuse f; f.bias = b; f.relu = act == 1; f.gelu = act == 2;
    return linear_big_bf16_ex(x, x_dtype, w, 0, f, b || act, y, y_dtype, M, K, N, "linear_forward_ex", st);
  }
  // fp32 copies of a bf16 x / y around the fp32 entry point, which may itself use head_scratch: slot 1 keeps them out of its way
  float *xs = nullptr, *ys = nullptr;
  const bool placed = carve_scratch([&](Carver& c) {
    if (x_dtype == 1) xs = c.take<float>((size_t)M * K);
    if (y_dtype == 1) ys = c.take<float>((size_t)M * N);
  }, 1);
  if (!placed) { mmskin_set_error("linear_forward_ex: scratch allocation failed"); return MMSKIN_ERR_HIP; }
  const float* xf = reinterpret_cast<const float*>(x);
  if (x_dtype == 1) {
    if ((rc = cvt_to_f32(reinterpret_cast<const bf16_t*>(x), xs, (int64_t)M * K, st))) return rc;
    xf = xs;
  }
  float* yf = y_dtype == 1 ? ys : reinterpret_cast<float*>(y);
  if ((rc = mmskin_linear_forward(xf, w, b, yf, M, K, N, act, stream))) return rc;
  if (y_dtype == 1) return cvt_to_bf16(yf, reinterpret_cast<bf16_t*>(y), (int64_t)M * N, st);
  return MMSKIN_OK;
}

// The lane Linear with everything a frozen transformer block hangs on its GEMMs fused into the epilogue:
//   y = residual + gamma * dropout(act(x w^T + b))          (each of residual / gamma / dropout optional)
// x fp32 or bf16; w fp32 (converted per call) or bf16 (a cached conversion of a frozen weight: no per-step conversion pass);
// residual fp32 [M][N]; with any of the three, y must be fp32 (the residual stream).  bf16-operand mode and the large-GEMM shape
// class only: the op has no fp32 formulation (the caller composes the separate ops instead).
int mmskin_linear_lane(const void* x, int x_dtype, const void* w, int w_dtype, const float* b, const float* gamma,
                       const float* residual, float drop_p, uint64_t seed, uint64_t offset, void* y, int y_dtype, int M, int K,
                       int N, int act, void* stream) {
  ARG_CHECK(x && w && y && M > 0 && K > 0 && N > 0, "linear_lane: bad argument");
  ARG_CHECK((x_dtype == 0 || x_dtype == 1) && (w_dtype == 0 || w_dtype == 1) && (y_dtype == 0 || y_dtype == 1) && act >= 0 && act <= 2,
            "linear_lane: dtype / activation");
  ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "linear_lane: dropout probability %f", (double)drop_p);
  ARG_CHECK(linear_path(M, K, N) == LIN_BIG_BF16, "linear_lane: M=%d K=%d N=%d is off the large bf16 GEMM path (rows >= 2048, 64-multiple widths, "
            "MMSKIN_LINEAR_DTYPE=bf16)", M, K, N);
  const bool tr = gamma || residual || drop_p > 0.f;
  ARG_CHECK(!tr || (y_dtype == 0 && N % 128 == 0), "linear_lane: residual / layer scale / dropout need an fp32 result and N %% 128 == 0");
  FwdFuse f; f.bias = b; f.relu = act == 1; f.gelu = act == 2;
  f.gamma = gamma; f.res_f32 = residual; f.drop_p = drop_p; f.seed = seed; f.offset = offset;
  return linear_big_bf16_ex(x, x_dtype, w, w_dtype, f, b || act || tr, y, y_dtype, M, K, N, "linear_lane", ST(stream));
}

int mmskin_linear_backward(const float* dy, const float* x, const float* w, const float* y_relu, float* dy_scratch,
                           float* dx, float* dw, float* db, int M, int K, int N, void* stream) {
  return linear_backward_impl(dy, x, w, y_relu, nullptr, dy_scratch, dx, dw, db, M, K, N, stream);
}
// Backward of h = gelu(x w^T + b) given dh and the saved pre-activation z [M][N]: the GELU derivative is applied inside the pass that
// converts the gradient for the bf16 GEMMs (and sums it for db), so d(z) never exists in fp32.  dy_scratch [M][N]: used off the bf16 path.
int mmskin_linear_gelu_backward(const float* dh, const float* x, const float* w, const float* z, float* dy_scratch, float* dx, float* dw,
                                float* db, int M, int K, int N, void* stream) {
  ARG_CHECK(z, "linear_gelu_backward: z required");
  return linear_backward_impl(dh, x, w, nullptr, z, dy_scratch, dx, dw, db, M, K, N, stream);
}
// Backward with the bf16 operand copy kept by mmskin_linear_forward_keep in x's place (x16 [M][mmskin_linear_x16_pitch]); y_relu /
// z_gelu as in the two entry points above (at most one).
int mmskin_linear_backward_keep(const float* dy, const void* x16, const float* w, const float* y_relu, const float* z_gelu, float* dy_scratch,
                                float* dx, float* dw, float* db, int M, int K, int N, void* stream) {
  ARG_CHECK(x16, "linear_backward_keep: x16 required");
  LinearBwdOpt o; o.x16_kept = x16;
  return linear_backward_impl(dy, nullptr, w, y_relu, z_gelu, dy_scratch, dx, dw, db, M, K, N, stream, o);
}

// Backward of h = StarReLU(x w^T) = s relu(z)^2 + b given dh, the kept bf16 operand and z [M][N]: 2 s relu(z) is applied inside the pass
// that converts dh for the bf16 GEMMs, and the same pass leaves the gradients of s and b in dsb[0..1] (fixed-order block sums).
int mmskin_linear_star_relu_backward_keep(const float* dh, const void* x16, const float* w, const float* z, const float* s, float* dsb,
                                          float* dx, float* dw, float* db, int M, int K, int N, void* stream) {
  ARG_CHECK(x16 && z && s && dsb, "linear_star_relu_backward_keep: x16, z, s and dsb required");
  ARG_CHECK(N % 4 == 0, "linear_star_relu_backward_keep: N=%d (needs N %% 4 == 0)", N);
  LinearBwdOpt o; o.x16_kept = x16; o.star_s = s; o.star_sb = dsb;
  return linear_backward_impl(dh, nullptr, w, nullptr, z, nullptr, dx, dw, db, M, K, N, stream, o);
}

int mmskin_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, int64_t sam, int64_t sak, int64_t sab,
               int64_t sbn, int64_t sbk, int64_t sbb, int64_t ldc, int64_t scb, void* stream) {
  ARG_CHECK(a && b && c && batch > 0 && M > 0 && N > 0 && K > 0, "bmm: bad argument");
  if (batch == 1) return gemm_f32(a, b, c, nullptr, M, N, K, sam, sak, sbn, sbk, ldc, 0, ST(stream));
  ARG_CHECK(batch <= 65535, "bmm: batch %d exceeds the grid limit", batch);
  return gemm_f32(a, b, c, nullptr, M, N, K, sam, sak, sbn, sbk, ldc, 0, ST(stream), batch, sab, sbb, scb);
}
int mmskin_colsum(const float* x, float* out, int M, int N, void* stream) {
  ARG_CHECK(x && out && M > 0 && N > 0, "colsum: bad argument");
  return colsum(x, out, M, N, ST(stream));
}
int mmskin_set_linear_dtype(int dtype) {
  ARG_CHECK(dtype == 0 || dtype == 1, "set_linear_dtype: dtype %d (MMSKIN_F32 = 0, MMSKIN_BF16 = 1)", dtype);
  g_linear_dtype = dtype;
  return MMSKIN_OK;
}
int mmskin_get_linear_dtype(void) { return linear_bf16() ? 1 : 0; }

}  // extern "C"
