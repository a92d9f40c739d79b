// BatchNorm and the column reductions behind it (declarations in ops.h): the producers of per-workgroup fp32 partial rows (column_stats,
// bn_bwd_reduce, slice_stats), the ONE fp64 column reducer that finalizes them (col_sums_kernel + finalize_columns: bn_finalize,
// bn_bwd_finalize, bn_table_finalize, bias_grad_finalize), the coefficient kernels and the apply passes.  Replaces the ATen batch_norm
// forward + backward kernels the reference reaches through torchvision's ResNet (multimodalIntraInterModal.py:167).
#include <stdlib.h>

#include <type_traits>

#include "ops_internal.h"

// ------------------------------------------------------------------ row-partial pre-reduction
// in[nrows][cols] -> out[G][cols]: group g sums rows [g*per, (g+1)*per).  Conv epilogues / wgrad splits
// leave up to ~25k partial rows; reducing them in one finalize block per 64 channels was latency-bound
// (200 us per BatchNorm), so a wide first stage brings the row count down to <= 64 first.
template <typename OUT>
__global__ __launch_bounds__(512) void partial_reduce_kernel(const float* __restrict__ in0,
                                                             const float* __restrict__ in1, int nrows, int cols,
                                                             int G, OUT* __restrict__ out) {
  __shared__ OUT red[8][64];
  const float* in = blockIdx.z ? in1 : in0;
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int per = (nrows + G - 1) / G;
  const int r0 = blockIdx.y * per;
  const int r1 = min(nrows, r0 + per);
  OUT a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  if (c < cols) {
    int r = r0 + ry;
    for (; r + 24 < r1; r += 32) {
      a0 += (OUT)in[(size_t)r * cols + c];
      a1 += (OUT)in[(size_t)(r + 8) * cols + c];
      a2 += (OUT)in[(size_t)(r + 16) * cols + c];
      a3 += (OUT)in[(size_t)(r + 24) * cols + c];
    }
    for (; r < r1; r += 8) a0 += (OUT)in[(size_t)r * cols + c];
  }
  red[ry][cx] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (ry == 0 && c < cols) {
    OUT s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += red[i][cx];
    out[((size_t)blockIdx.z * G + blockIdx.y) * cols + c] = s;
  }
}

// float4 variant for wide matrices (wgrad split slabs): 64 threads cover 256 columns, 8 row lanes
__global__ __launch_bounds__(512) void partial_reduce4_kernel(const float* __restrict__ in, int nrows, int cols,
                                                              int G, float* __restrict__ out) {
  __shared__ float4 red[8][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + cx) * 4;
  const int per = (nrows + G - 1) / G;
  const int r0 = blockIdx.y * per;
  const int r1 = min(nrows, r0 + per);
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  if (c < cols) {
    int r = r0 + ry;
    for (; r + 8 < r1; r += 16) {
      float4 u = *reinterpret_cast<const float4*>(in + (size_t)r * cols + c);
      float4 v = *reinterpret_cast<const float4*>(in + (size_t)(r + 8) * cols + c);
      a0.x += u.x; a0.y += u.y; a0.z += u.z; a0.w += u.w;
      a1.x += v.x; a1.y += v.y; a1.z += v.z; a1.w += v.w;
    }
    for (; r < r1; r += 8) {
      float4 u = *reinterpret_cast<const float4*>(in + (size_t)r * cols + c);
      a0.x += u.x; a0.y += u.y; a0.z += u.z; a0.w += u.w;
    }
  }
  red[ry][cx] = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
  __syncthreads();
  if (ry == 0 && c < cols) {
    float4 s = red[0][cx];
#pragma unroll
    for (int i = 1; i < 8; ++i) { s.x += red[i][cx].x; s.y += red[i][cx].y; s.z += red[i][cx].z; s.w += red[i][cx].w; }
    *reinterpret_cast<float4*>(out + (size_t)blockIdx.y * cols + c) = s;
  }
}

template <typename OUT>
int partial_reduce(const float* in0, const float* in1, int nrows, int cols, int G, OUT* out, hipStream_t st) {
  if constexpr (sizeof(OUT) == 4) {
    if (!in1 && cols % 4 == 0) {
      hipLaunchKernelGGL(partial_reduce4_kernel, dim3(ceil_div(cols, 256), G), dim3(512), 0, st, in0, nrows, cols, G,
                         reinterpret_cast<float*>(out));
      HIP_CHECK_RET(hipGetLastError());
      return MMSKIN_OK;
    }
  }
  hipLaunchKernelGGL(partial_reduce_kernel<OUT>, dim3(ceil_div(cols, 64), G, in1 ? 2 : 1), dim3(512), 0, st, in0, in1,
                     nrows, cols, G, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
template int partial_reduce<float>(const float*, const float*, int, int, int, float*, hipStream_t);
template int partial_reduce<double>(const float*, const float*, int, int, int, double*, hipStream_t);

static inline int reduce_groups(int nrows) {
  int g = (nrows + 31) / 32;
  return g > 64 ? 64 : (g < 1 ? 1 : g);
}

// partial-row counts up to this are reduced by the finalize kernel itself (one launch instead of two)
// MMSKIN_BN_SINGLE_ROWS (default 512): layers 3 - 4 of ResNet-50 at batch 256 leave 98 - 392 partial rows (64 - 256 with the
// pipelined conv kernel's tiles) -- one 1024-thread finalize launch (16 row lanes x 2 chains) instead of pre-reduction + finalize
static inline int bn_single_stage_rows() {
  static const int v = env_knob("MMSKIN_BN_SINGLE_ROWS", 512);
  return v;
}

// channel c's BatchNorm-backward coefficients (dz = cA g + cB x + cC) and parameter gradients from s1 = sum dz, s2 = sum dz x
__device__ __forceinline__ void bn_bwd_coeffs(int c, double s1, double s2, double count, const float* __restrict__ gamma, const float* __restrict__ mean,
                                              const float* __restrict__ invstd, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, int n_grad,
                                              int acc_bc, const float* __restrict__ s2_override) {
  if (s2_override) s2 = (double)s2_override[c];
  double mu = mean[c], is = invstd[c], g = gamma ? gamma[c] : 1.0;
  double dg = is * (s2 - mu * s1);   // sum dz * xhat
  if (dgamma && c < n_grad) dgamma[c] = (float)dg;
  if (dbeta && c < n_grad) dbeta[c] = (float)s1;
  double A = g * is;
  cA[c] = (float)A;
  const float vb = (float)(-A * is * dg / count), vc = (float)(A * (-s1 / count + mu * is * dg / count));
  if (acc_bc) { cB[c] += vb; cC[c] += vc; }   // running sums over the consumers of a shared input (DenseNet's deferred x / constant terms)
  else { cB[c] = vb; cC[c] = vc; }
}

// ------------------------------------------------------------------ the fp64 column reducer of the finalize kernels
// Lane (cx, ry) of a CB x RL block sums rows ry, ry + RL, ... of column c = blockIdx.x * CB + cx in fp64, for NQ (1 or 2) quantities
// addressed as q[r * row_stride + c].  CHAINS (1 or 4) independent accumulators per lane and quantity keep 2 * CHAINS loads in flight and
// are combined as (a0 + a1) + (a2 + a3); row lane 0 then adds the RL lane sums in index order and calls Epi::apply(c, s0, s1, a...).
// Layouts: two split slabs are two pointers with row_stride = C; the interleaved [row][2][C] slab is q1 = q0 + C, row_stride = 2 * C.
// (The epilogue's operands are kernel arguments of their own, not one struct: a struct argument is loaded whole at kernel entry and held
// in scalar registers through the loop.)
template <typename IN, int NQ, int RL, int CB, int CHAINS, class Epi, class... A>
__global__ __launch_bounds__(CB * RL) void col_sums_kernel(const IN* __restrict__ q0, const IN* __restrict__ q1, int nrows, int row_stride, int C,
                                                           A... a) {
  static_assert((NQ == 1 || NQ == 2) && (CHAINS == 1 || CHAINS == 4), "col_sums_kernel: form");
  __shared__ double red[NQ][RL][CB];
  const int cx = threadIdx.x % CB, ry = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cx;
  auto at = [&](int k, int r) { return (double)(k ? q1 : q0)[(size_t)r * row_stride + c]; };
  double s[2] = {0.0, 0.0};
  if (c < C) {
    int r = ry;
    if constexpr (CHAINS == 4) {
      double a[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
      for (; r + 3 * RL < nrows; r += 4 * RL) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < NQ; ++k) a[j][k] += at(k, r + j * RL);
      }
      for (; r < nrows; r += RL) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) a[0][k] += at(k, r);
      }
#pragma unroll
      for (int k = 0; k < NQ; ++k) s[k] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
    } else {
      for (; r < nrows; r += RL) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) s[k] += at(k, r);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) red[k][ry][cx] = s[k];
  __syncthreads();
  if (ry == 0 && c < C) {
    s[0] = 0.0; s[1] = 0.0;
#pragma unroll
    for (int i = 0; i < RL; ++i) {
#pragma unroll
      for (int k = 0; k < NQ; ++k) s[k] += red[k][i][cx];
    }
    Epi::apply(c, s[0], s[1], a...);
  }
}

// The per-channel epilogues: what a finalize kernel does with its column's sums (operands after the sums: the kernel's trailing arguments).
struct BnFwdEpi {   // (sum x, sum x^2) -> scale / shift, saved and running statistics: bn_fwd_coeffs' operands
  template <class... A> static __device__ __forceinline__ void apply(int c, double s, double q, A... a) { bn_fwd_coeffs(c, s, q, a...); }
};
struct BnBwdEpi {   // (sum dz, sum dz x) -> dgamma / dbeta and the cA | cB | cC vectors: bn_bwd_coeffs' operands
  template <class... A> static __device__ __forceinline__ void apply(int c, double s1, double s2, A... a) { bn_bwd_coeffs(c, s1, s2, a...); }
};
struct BnTableEpi {   // (sum x, sum x^2) -> batch mean / biased variance
  static __device__ __forceinline__ void apply(int c, double s, double q, double count, float* __restrict__ mean, float* __restrict__ var) {
    double m = s / count, v = q / count - m * m;
    mean[c] = (float)m;
    var[c] = (float)(v < 0.0 ? 0.0 : v);
  }
};
struct BiasGradEpi {   // sum -> bias gradient
  static __device__ __forceinline__ void apply(int c, double s, double, float* __restrict__ db) { db[c] = (float)s; }
};

int col_reduce_scratch_check(int slabs, int nrows, int cols_total, size_t doubles) {
  const int G = reduce_groups(nrows);
  ARG_CHECK(slabs >= 1 && nrows >= 1 && cols_total >= 1 && (size_t)slabs * G * cols_total <= doubles,
            "finalize_columns: %d slab(s) x %d groups x %d columns exceed the %zu doubles of reduction scratch", slabs, G, cols_total, doubles);
  return MMSKIN_OK;
}

// A launch form of col_sums_kernel: CB columns x RL row lanes (CB * RL threads), CHAINS accumulators per lane and quantity.
template <int RL_, int CB_, int CHAINS_>
struct ColForm { static constexpr int RL = RL_, CB = CB_, CHAINS = CHAINS_; };
struct NoMidForm {};   // a call site whose small form serves every single-stage row count
template <class F, int NQ, class Epi, typename IN, class... A>
static void launch_col_sums(const IN* q0, const IN* q1, int nrows, int row_stride, int C, hipStream_t st, A... a) {
  hipLaunchKernelGGL((col_sums_kernel<IN, NQ, F::RL, F::CB, F::CHAINS, Epi, A...>), dim3(ceil_div(C, F::CB)), dim3(F::CB * F::RL), 0, st, q0, q1,
                     nrows, row_stride, C, a...);
}

// The one dispatcher of the four finalize entries.  Slab: NQ quantities at q0 (and q1), `nrows` rows of `row_stride` floats, columns < C used;
// q1 inside q0's first row (q0 < q1 < q0 + row_stride) is the interleaved layout -- ONE slab of row_stride columns -- otherwise every quantity
// is a slab of its own.  Stage decision, made here and nowhere else:
//   nrows > bn_single_stage_rows() and scratch given : partial_reduce<double> to G = reduce_groups(nrows) <= 64 rows, then Small on those
//                                                      (slabs * G * row_stride doubles of scratch: checked against scratch.doubles)
//   nrows > 64 and the site has a Mid form            : Mid
//   otherwise                                         : Small
// (both stages in one launch behind a ticket per column block: +1.3 ms per step, profiles/r04_experiments.txt (11))
template <int NQ, class Small, class Mid, class Epi, class... A>
static int finalize_columns(const float* q0, const float* q1, int nrows, int row_stride, int C, ColScratch scratch, hipStream_t st, A... a) {
  constexpr bool has_mid = !std::is_same<Mid, NoMidForm>::value;
  if (scratch.p && nrows > bn_single_stage_rows()) {
    const bool interleaved = NQ == 2 && q1 > q0 && q1 - q0 < row_stride;
    const int slabs = NQ == 2 && !interleaved ? 2 : 1;
    if (int rc = col_reduce_scratch_check(slabs, nrows, row_stride, scratch.doubles)) return rc;
    const int G = reduce_groups(nrows);
    if (int rc = partial_reduce<double>(q0, slabs == 2 ? q1 : nullptr, nrows, row_stride, G, scratch.p, st)) return rc;
    const double* t1 = NQ == 1 ? nullptr : interleaved ? scratch.p + (q1 - q0) : scratch.p + (size_t)G * row_stride;
    launch_col_sums<Small, NQ, Epi>(static_cast<const double*>(scratch.p), t1, G, row_stride, C, st, a...);
  } else if (has_mid && nrows > 64) {
    if constexpr (has_mid) launch_col_sums<Mid, NQ, Epi>(q0, q1, nrows, row_stride, C, st, a...);
  } else {
    launch_col_sums<Small, NQ, Epi>(q0, q1, nrows, row_stride, C, st, a...);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// The launch forms, site by site (every one measured: profiles/r04_experiments.txt).  64 columns x 4 row lanes x 4 chains is the small form of
// the two BatchNorm finalizes; up to bn_single_stage_rows() partial rows (ResNet-50 layers 3 - 4 at batch 256) take 16 row lanes in ONE
// launch.  The backward's 16-lane form has CB = 16 (256 threads, 4 KB of LDS): a block that small fits on a CU beside a weight-gradient ring
// workgroup of the other stream (208 VGPRs x 8 waves, 121 - 132 KB of LDS), where the 1024-thread form waited for a ring workgroup to
// retire -- i.e. for the whole weight-gradient launch (profiles/r04_experiments.txt (8)).  The statistics table has 64 columns x 16 row lanes
// and one chain throughout (a DenseNet growth slice has 32 channels: with 4 lanes one workgroup walked up to 512 rows in 18 us).
int bn_finalize(const float* stat_sum, const float* stat_sq, int nrows, int C, double count, const float* gamma, const float* beta, float eps,
                float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* save_mean, float* save_invstd,
                ColScratch scratch, hipStream_t st) {
  return finalize_columns<2, ColForm<4, 64, 4>, ColForm<16, 64, 4>, BnFwdEpi>(stat_sum, stat_sq, nrows, C, C, scratch, st, count, gamma, beta, eps, momentum,
                                                                             running_mean, running_var, scale, shift, save_mean, save_invstd);
}
int bn_bwd_finalize(const float* partial, int nrows, int C, double count, const float* gamma, const float* save_mean, const float* save_invstd,
                    float* dgamma, float* dbeta, float* cA, float* cB, float* cC, ColScratch scratch, hipStream_t st, int n_grad,
                    bool accumulate_bc, const float* sum_dz_x) {
  return finalize_columns<2, ColForm<4, 64, 4>, ColForm<16, 16, 4>, BnBwdEpi>(partial, partial + C, nrows, 2 * C, C, scratch, st, count, gamma, save_mean,
                                                                             save_invstd, dgamma, dbeta, cA, cB, cC, n_grad < 0 ? C : n_grad,
                                                                             accumulate_bc ? 1 : 0, sum_dz_x);
}
int bn_table_finalize(const float* stat_sum, const float* stat_sq, int nrows, int stride, int C, double count, float* mean, float* var,
                      ColScratch scratch, hipStream_t st) {
  return finalize_columns<2, ColForm<16, 64, 1>, NoMidForm, BnTableEpi>(stat_sum, stat_sq, nrows, stride, C, scratch, st, count, mean, var);
}
int bias_grad_finalize(const float* partial, int nrows, int stride, int C, float* db, ColScratch scratch, hipStream_t st) {
  return finalize_columns<1, ColForm<4, 64, 1>, NoMidForm, BiasGradEpi>(partial, nullptr, nrows, stride, C, scratch, st, db);
}

// ------------------------------------------------------------------ BN forward
__global__ void bn_eval_coeffs_kernel(int C, const float* gamma, const float* beta, const float* rm,
                                      const float* rv, float eps, float* scale, float* shift) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
  }
}
int bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                   const float* running_var, float eps, float* scale, float* shift, hipStream_t st) {
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, C, gamma, beta,
                     running_mean, running_var, eps, scale, shift);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// Thread mapping of the two apply passes (bn_apply, bn_bwd_apply): column-stationary.  A 256-thread block is CW chunk columns x RL row
// lanes (CW = min(C / EPC, 256), RL = 256 / CW; threads past CW * RL idle when CW does not divide 256, blockIdx.y walks column blocks
// when a row has more than 256 chunks), so a thread's channels are fixed for the launch: it loads its per-channel coefficients into
// registers once and then does APPLY_ROWS rows, RL apart (rows r0 + j * RL, r0 = blockIdx.x * RL * APPLY_ROWS + ry), issuing every
// payload load of the group before the first use.  For each j the block still touches RL consecutive rows = up to 256 consecutive
// chunks, as with one chunk per thread.  No loop: blockIdx.x covers every row group (many short workgroups stream faster than few
// long ones, ew_grid); the last group of a launch takes its rows one at a time.
constexpr int APPLY_ROWS = 4;
struct ApplyGeom { int CPR, CW, RL; unsigned gx, gy; };
static inline int apply_geom(size_t rows, int CPR, ApplyGeom* g, const char* who) {
  g->CPR = CPR;
  g->CW = CPR < EW_BLOCK ? CPR : EW_BLOCK;
  g->RL = EW_BLOCK / g->CW;
  const size_t per_block = (size_t)g->RL * APPLY_ROWS, gx = (rows + per_block - 1) / per_block;
  ARG_CHECK(gx <= 0x7fffffffu && ceil_div(CPR, g->CW) <= 65535, "%s: %zu rows x %d chunks per row", who, rows, CPR);
  g->gx = gx ? (unsigned)gx : 1u;
  g->gy = (unsigned)ceil_div(CPR, g->CW);
  return MMSKIN_OK;
}
// the calling thread's chunk column and first row; false: an idle thread
__device__ __forceinline__ bool apply_thread(const ApplyGeom& g, int* col, size_t* r0) {
  const int ry = (int)threadIdx.x / g.CW;
  *col = (int)blockIdx.y * g.CW + ((int)threadIdx.x - ry * g.CW);
  *r0 = (size_t)blockIdx.x * ((size_t)g.RL * APPLY_ROWS) + ry;
  return ry < g.RL && *col < g.CPR;
}

// N rows of one chunk column, `stride` elements apart, from element offset `off` (chunk index `chunk`, `cstride` chunks apart)
template <typename T, int RELU, int RES, bool NT, int N>
__device__ __forceinline__ void bn_apply_rows(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                              uint8_t* __restrict__ mask_bits, size_t off, size_t stride, size_t chunk, size_t cstride,
                                              const float* scale, const float* shift, const float* rscale, const float* rshift,
                                              float relu_cap) {
  constexpr int EPC = DT<T>::EPC;
  Chunk<T> v[N], r[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (NT) v[j].load_nt(x + off + j * stride); else v[j].load(x + off + j * stride);     // the raw conv output is read once more only in backward
    if (RES) { if (NT) r[j].load_nt(res + off + j * stride); else r[j].load(res + off + j * stride); }
  }
  if (N > 1) __builtin_amdgcn_sched_barrier(0);   // every load of the group is issued before the first use
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t bits = 0;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      float t = v[j].v[e] * scale[e] + shift[e];
      if (RES == 1) t += r[j].v[e];
      if (RES == 2) t += r[j].v[e] * rscale[e] + rshift[e];
      // SiLU is its own instantiation: as a run-time branch its exp + divide were if-converted into the ReLU path
      // and made the (HBM-bound) pass VALU-bound -- 3x slower BatchNorm-apply on every backbone
      if (RELU == 2) t = t / (1.f + __expf(-t));
      else if (RELU == 1) { t = fmaxf(t, 0.f); if (relu_cap > 0.f) t = fminf(t, relu_cap); }
      v[j].v[e] = t;
      bits |= (from_f32<T>(t) != 0 && t > 0.f ? 1u : 0u) << e;   // bit = (stored y > 0)
    }
    v[j].store(y + off + j * stride);
    if (mask_bits) mask_bits[chunk + j * cstride] = (uint8_t)bits;   // one byte per 16-byte chunk: the ReLU mask for backward
  }
}

template <typename T, int RELU, int RES, bool NT = false>  // RELU: 0 none, 1 relu / capped relu, 2 SiLU; RES: 0 none, 1 plain residual, 2 residual*rscale + rshift
__global__ __launch_bounds__(EW_BLOCK) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift,
                                                            const float* __restrict__ rscale,
                                                            const float* __restrict__ rshift, T* __restrict__ y,
                                                            uint8_t* __restrict__ mask_bits, size_t rows, ApplyGeom g,
                                                            float relu_cap) {
  constexpr int EPC = DT<T>::EPC;
  int col;
  size_t r0;
  if (!apply_thread(g, &col, &r0) || r0 >= rows) return;
  float sc[EPC], sh[EPC], rsc[EPC], rsh[EPC];   // this thread's channels: constant for the launch
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    sc[e] = scale[col * EPC + e]; sh[e] = shift[col * EPC + e];
    if (RES == 2) { rsc[e] = rscale[col * EPC + e]; rsh[e] = rshift[col * EPC + e]; }
  }
  const size_t chunk = r0 * g.CPR + col, cstride = (size_t)g.RL * g.CPR;
  if (r0 + (size_t)(APPLY_ROWS - 1) * g.RL < rows) {
    bn_apply_rows<T, RELU, RES, NT, APPLY_ROWS>(x, res, y, mask_bits, chunk * EPC, cstride * EPC, chunk, cstride, sc, sh, rsc, rsh, relu_cap);
  } else {
    for (size_t r = r0, ch = chunk; r < rows; r += g.RL, ch += cstride)
      bn_apply_rows<T, RELU, RES, NT, 1>(x, res, y, mask_bits, ch * EPC, 0, ch, 0, sc, sh, rsc, rsh, relu_cap);
  }
}

template <typename T>
int bn_apply(const T* x, const T* res, const float* scale, const float* shift, const float* rscale,
             const float* rshift, T* y, size_t rows, int C, bool relu, hipStream_t st, uint8_t* mask_bits,
             float relu_cap) {
  constexpr int EPC = DT<T>::EPC;
  ARG_CHECK(C % EPC == 0 && C >= EPC, "bn_apply: C=%d", C);
  ApplyGeom g;
  if (int rc = apply_geom(rows, C / EPC, &g, "bn_apply")) return rc;
  const dim3 grid(g.gx, g.gy);
  int mode = res ? (rscale ? 2 : 1) : 0;
#ifdef MMSKIN_ABLATE   // `make ablate` only: upper bound of folding the plain BN + ReLU apply into its consumers (wrong results, valid timing)
  { static const int abl = [] { const char* v = getenv("MMSKIN_BN_ABLATE"); return v ? atoi(v) : 0; }(); if ((abl & 1) && mode == 0 && relu) return MMSKIN_OK; }
#endif
#define LAUNCH(R, H) hipLaunchKernelGGL((bn_apply_kernel<T, R, H>), grid, dim3(EW_BLOCK), 0, st, x, res, scale, shift, rscale, rshift, y, mask_bits, rows, g, relu_cap)
  if (relu && relu_cap < 0.f) { if (mode == 2) LAUNCH(2, 2); else if (mode == 1) LAUNCH(2, 1); else LAUNCH(2, 0); }
  else if (relu) {
#define LAUNCH_NT(R, H) hipLaunchKernelGGL((bn_apply_kernel<T, R, H, true>), grid, dim3(EW_BLOCK), 0, st, x, res, scale, shift, rscale, rshift, y, mask_bits, rows, g, relu_cap)
    if (mode == 2) LAUNCH_NT(1, 2); else if (mode == 1) LAUNCH_NT(1, 1); else LAUNCH_NT(1, 0);
#undef LAUNCH_NT
  }
  else { if (mode == 2) LAUNCH(0, 2); else if (mode == 1) LAUNCH(0, 1); else LAUNCH(0, 0); }
#undef LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void column_stats_kernel(const T* __restrict__ x, size_t rows, int C,
                                                           ColGeom g, float* partial_sum, float* partial_sq) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float red[2 * 256 * EPC];
  const int cx = threadIdx.x % g.CW, ry = threadIdx.x / g.CW;
  const int col = blockIdx.y * g.CW + cx;
  float acc[2][EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (ry < g.RL && col < g.CPR) {
    size_t r_end = (size_t)(blockIdx.x + 1) * g.RB;
    if (r_end > rows) r_end = rows;
    for (size_t r = (size_t)blockIdx.x * g.RB + ry; r < r_end; r += g.RL) {
      Chunk<T> v;
      v.load(x + (r * g.CPR + col) * EPC);
#pragma unroll
      for (int e = 0; e < EPC; ++e) { acc[0][e] += v.v[e]; acc[1][e] += v.v[e] * v.v[e]; }
    }
  }
  // two quantities into two separate slabs: reuse the NQ=1 reducer twice
  float a1[1][EPC], a2[1][EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) { a1[0][e] = acc[0][e]; a2[0][e] = acc[1][e]; }
  block_col_reduce<EPC, 1>(a1, cx, ry, g.CW, g.RL, col, g.CPR, C, partial_sum, red);
  __syncthreads();
  block_col_reduce<EPC, 1>(a2, cx, ry, g.CW, g.RL, col, g.CPR, C, partial_sq, red);
}

int column_stats_rows(size_t rows, int C) {
  ColGeom a = col_geom(rows, C, 4), b = col_geom(rows, C, 8);
  return a.gx > b.gx ? a.gx : b.gx;
}
template <typename T>
int column_stats(const T* x, size_t rows, int C, float* stat_sum, float* stat_sq, int* nrows_out,
                 hipStream_t st) {
  ARG_CHECK(C % DT<T>::EPC == 0, "column_stats: C=%d", C);
  ColGeom g = col_geom(rows, C, DT<T>::EPC);
  hipLaunchKernelGGL(column_stats_kernel<T>, dim3(g.gx, g.gy), dim3(256), 0, st, x, rows, C, g, stat_sum, stat_sq);
  HIP_CHECK_RET(hipGetLastError());
  *nrows_out = g.gx;
  return MMSKIN_OK;
}

__global__ void bn_eval_table_kernel(const StageDesc* __restrict__ table, const float* __restrict__ params,
                                     const float* __restrict__ buffers, unsigned char* ws, float eps) {
  const StageDesc d = table[blockIdx.y];
  if (!d.has_bn) return;
  float* coef = reinterpret_cast<float*>(ws + d.coef_off);
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < d.Cout; c += gridDim.x * blockDim.x) {
    float sc = params[d.bn_g_off + c] / sqrtf(buffers[d.bn_rv_off + c] + eps);
    coef[c] = sc;
    coef[d.Cout + c] = params[d.bn_b_off + c] - buffers[d.bn_rm_off + c] * sc;
  }
}
int bn_eval_table(const StageDesc* table_dev, int nlayers, int maxC, const float* params, const float* buffers,
                  unsigned char* ws, float eps, hipStream_t st) {
  hipLaunchKernelGGL(bn_eval_table_kernel, dim3(ceil_div(maxC, 256), nlayers), dim3(256), 0, st, table_dev, params, buffers, ws, eps);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// ------------------------------------------------------------------ BN backward
constexpr bool mask_reads_y(int mode) { return mode == MASK_FROM_Y || mode == MASK_FROM_Y6; }
// the mask rules on loaded chunks: yv is read by the MASK_FROM_Y / MASK_FROM_Y6 modes only, scale / shift (the chunk's EPC channels) by
// MASK_FROM_X / MASK_SILU_X only
template <typename T, int MODE>
__device__ __forceinline__ void mask_chunk(Chunk<T>& dz, const Chunk<T>& xv, const Chunk<T>& yv, const float* scale, const float* shift) {
  constexpr int EPC = DT<T>::EPC;
  if (MODE == MASK_FROM_X) {
#pragma unroll
    for (int e = 0; e < EPC; ++e)
      if (!(xv.v[e] * scale[e] + shift[e] > 0.f)) dz.v[e] = 0.f;
  } else if (MODE == MASK_FROM_Y) {
#pragma unroll
    for (int e = 0; e < EPC; ++e)
      if (!(yv.v[e] > 0.f)) dz.v[e] = 0.f;
  } else if (MODE == MASK_FROM_Y6) {
#pragma unroll
    for (int e = 0; e < EPC; ++e)
      if (!(yv.v[e] > 0.f && yv.v[e] < 6.f)) dz.v[e] = 0.f;
  } else if (MODE == MASK_SILU_X) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float t = xv.v[e] * scale[e] + shift[e];
      const float sg = 1.f / (1.f + __expf(-t));
      dz.v[e] *= sg * (1.f + t * (1.f - sg));
    }
  }
}
template <typename T, int MODE>
__device__ __forceinline__ void masked_dy(Chunk<T>& dz, const Chunk<T>& xv, const T* ymask, size_t off,
                                          const float* scale, const float* shift, int c0) {
  Chunk<T> yv;
  if (mask_reads_y(MODE)) yv.load(ymask + off);
  mask_chunk<T, MODE>(dz, xv, yv, scale + c0, shift + c0);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                            const T* __restrict__ ymask,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift, size_t rows, int C,
                                                            ColGeom g, float* partial) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float red[2 * 256 * EPC];
  const int cx = threadIdx.x % g.CW, ry = threadIdx.x / g.CW;
  const int col = blockIdx.y * g.CW + cx;
  float acc[2][EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (ry < g.RL && col < g.CPR) {
    size_t r_end = (size_t)(blockIdx.x + 1) * g.RB;
    if (r_end > rows) r_end = rows;
    const int c0 = col * EPC;
    for (size_t r = (size_t)blockIdx.x * g.RB + ry; r < r_end; r += g.RL) {
      size_t off = (r * g.CPR + col) * EPC;
      Chunk<T> dz, xv;
      dz.load(dy + off);
      xv.load(x + off);
      masked_dy<T, MODE>(dz, xv, ymask, off, scale, shift, c0);
#pragma unroll
      for (int e = 0; e < EPC; ++e) { acc[0][e] += dz.v[e]; acc[1][e] += dz.v[e] * xv.v[e]; }
    }
  }
  block_col_reduce<EPC, 2>(acc, cx, ry, g.CW, g.RL, col, g.CPR, C, partial, red);
}

int bn_bwd_partial_rows(size_t rows, int C) { return column_stats_rows(rows, C); }

template <typename T>
int bn_bwd_reduce(const T* dy, const T* x, const T* ymask, const float* scale, const float* shift,
                  int mask_mode, size_t rows, int C, float* partial, int* nrows_out, hipStream_t st) {
  ARG_CHECK(C % DT<T>::EPC == 0, "bn_bwd_reduce: C=%d", C);
  ColGeom g = col_geom(rows, C, DT<T>::EPC);
#define LAUNCH(M) hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, M>), dim3(g.gx, g.gy), dim3(256), 0, st, dy, x, ymask, scale, shift, rows, C, g, partial)
  if (mask_mode == MASK_FROM_X) LAUNCH(MASK_FROM_X);
  else if (mask_mode == MASK_FROM_Y) LAUNCH(MASK_FROM_Y);
  else if (mask_mode == MASK_FROM_Y6) LAUNCH(MASK_FROM_Y6);
  else if (mask_mode == MASK_SILU_X) LAUNCH(MASK_SILU_X);
  else LAUNCH(MASK_NONE);
#undef LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  *nrows_out = g.gx;
  return MMSKIN_OK;
}

// N rows of one chunk column, `stride` elements apart, from element offset `off`: every load of the group, then row by row
template <typename T, int MODE, bool WRITE_DZ, bool NT, int N>
__device__ __forceinline__ void bn_bwd_apply_rows(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ ymask,
                                                  T* __restrict__ dx, T* __restrict__ dz_out, size_t off, size_t stride,
                                                  const float* scale, const float* shift, const float* a, const float* b, const float* c) {
  constexpr int EPC = DT<T>::EPC;
  Chunk<T> dz[N], xv[N], yv[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (NT) { dz[j].load_nt(dy + off + j * stride); xv[j].load_nt(x + off + j * stride); }
    else { dz[j].load(dy + off + j * stride); xv[j].load(x + off + j * stride); }
    if (mask_reads_y(MODE)) yv[j].load(ymask + off + j * stride);
  }
  if (N > 1) __builtin_amdgcn_sched_barrier(0);   // every load of the group is issued before the first use
#pragma unroll
  for (int j = 0; j < N; ++j) {
    mask_chunk<T, MODE>(dz[j], xv[j], yv[j], scale, shift);
    if (WRITE_DZ) dz[j].store(dz_out + off + j * stride);
    // cA dz + cB x + cC with its roundings pinned (the product cB x, then one fused cA dz + that, then + cC): left to the compiler's
    // contraction, the masked instantiations fused the other product and differed from the unmasked ones in the last bit
#pragma unroll
    for (int e = 0; e < EPC; ++e) xv[j].v[e] = __builtin_fmaf(a[e], dz[j].v[e], b[e] * xv[j].v[e]) + c[e];
    xv[j].store(dx + off + j * stride);
  }
}

template <typename T, int MODE, bool WRITE_DZ, bool NT = false>
__global__ __launch_bounds__(EW_BLOCK) void bn_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ ymask,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ cA,
    const float* __restrict__ cB, const float* __restrict__ cC, T* __restrict__ dx, T* __restrict__ dz_out,
    size_t rows, ApplyGeom g) {
  constexpr int EPC = DT<T>::EPC;
  constexpr bool COEF = MODE == MASK_FROM_X || MODE == MASK_SILU_X;   // the modes that recompute scale * x + shift
  int col;
  size_t r0;
  if (!apply_thread(g, &col, &r0) || r0 >= rows) return;
  float a[EPC], b[EPC], c[EPC], sc[EPC], sh[EPC];   // this thread's channels: constant for the launch
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    a[e] = cA[col * EPC + e]; b[e] = cB[col * EPC + e]; c[e] = cC[col * EPC + e];
    if (COEF) { sc[e] = scale[col * EPC + e]; sh[e] = shift[col * EPC + e]; }
  }
  const size_t off = (r0 * g.CPR + col) * EPC, stride = (size_t)g.RL * g.CPR * EPC;
  if (r0 + (size_t)(APPLY_ROWS - 1) * g.RL < rows) {
    bn_bwd_apply_rows<T, MODE, WRITE_DZ, NT, APPLY_ROWS>(dy, x, ymask, dx, dz_out, off, stride, sc, sh, a, b, c);
  } else {
    size_t o = off;
    for (size_t r = r0; r < rows; r += g.RL, o += stride)
      bn_bwd_apply_rows<T, MODE, WRITE_DZ, NT, 1>(dy, x, ymask, dx, dz_out, o, 0, sc, sh, a, b, c);
  }
}

template <typename T>
int bn_bwd_apply(const T* dy, const T* x, const T* ymask, const float* scale, const float* shift,
                 int mask_mode, const float* cA, const float* cB, const float* cC, T* dx, T* dz_out,
                 size_t rows, int C, hipStream_t st) {
  constexpr int EPC = DT<T>::EPC;
  ARG_CHECK(C % EPC == 0 && C >= EPC, "bn_bwd_apply: C=%d", C);
  ApplyGeom g;
  if (int rc = apply_geom(rows, C / EPC, &g, "bn_bwd_apply")) return rc;
  const dim3 grid(g.gx, g.gy);
#ifdef MMSKIN_ABLATE   // `make ablate` only: upper bound of folding the BN-backward apply into the dgrad / weight-gradient operand loads
  { static const int abl = [] { const char* v = getenv("MMSKIN_BN_ABLATE"); return v ? atoi(v) : 0; }(); if ((abl & 2) && mask_mode == MASK_NONE && !dz_out) return MMSKIN_OK; }
#endif
#define LAUNCH(M, W) hipLaunchKernelGGL((bn_bwd_apply_kernel<T, M, W>), grid, dim3(EW_BLOCK), 0, st, dy, x, ymask, scale, shift, cA, cB, cC, dx, dz_out, rows, g)
  if (mask_mode == MASK_FROM_X) { if (dz_out) LAUNCH(MASK_FROM_X, true); else LAUNCH(MASK_FROM_X, false); }
  else if (mask_mode == MASK_FROM_Y) { if (dz_out) LAUNCH(MASK_FROM_Y, true); else LAUNCH(MASK_FROM_Y, false); }
  else if (mask_mode == MASK_FROM_Y6) { if (dz_out) LAUNCH(MASK_FROM_Y6, true); else LAUNCH(MASK_FROM_Y6, false); }
  else if (mask_mode == MASK_SILU_X) { if (dz_out) LAUNCH(MASK_SILU_X, true); else LAUNCH(MASK_SILU_X, false); }
  else {
    // nontemporal loads of dz / x (each is read for the last time here; dx stays cacheable: the dgrad and the weight-gradient
    // GEMM read it next): same-box A/B 20.74 -> 20.43 ms per step (cacheable / nontemporal, profiles/r02_experiments.txt)
    if (dz_out) LAUNCH(MASK_NONE, true);
    else hipLaunchKernelGGL((bn_bwd_apply_kernel<T, MASK_NONE, false, true>), grid, dim3(EW_BLOCK), 0, st, dy, x, ymask, scale, shift, cA, cB, cC, dx, dz_out, rows, g);
  }
#undef LAUNCH
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

#define INST(T)                                                                                               \
  template int bn_apply<T>(const T*, const T*, const float*, const float*, const float*, const float*, T*, size_t, int, bool, hipStream_t, uint8_t*, float); \
  template int column_stats<T>(const T*, size_t, int, float*, float*, int*, hipStream_t);                       \
  template int bn_bwd_reduce<T>(const T*, const T*, const T*, const float*, const float*, int, size_t, int, float*, int*, hipStream_t); \
  template int bn_bwd_apply<T>(const T*, const T*, const T*, const float*, const float*, int, const float*, const float*, const float*, T*, T*, size_t, int, hipStream_t);
INST(float)
INST(bf16_t)
#undef INST

// ------------------------------------------------------------------ statistics tables (DenseNet, MBConv)
template <typename T>
__global__ __launch_bounds__(256) void slice_stats_kernel(const T* __restrict__ x, int pitch, size_t rows, int C,
                                                          ColGeom g, float* partial_sum, float* partial_sq) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float red[2 * 256 * EPC];
  const int cx = threadIdx.x % g.CW, ry = threadIdx.x / g.CW;
  const int col = blockIdx.y * g.CW + cx;
  float acc[2][EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (ry < g.RL && col < g.CPR) {
    size_t r_end = (size_t)(blockIdx.x + 1) * g.RB;
    if (r_end > rows) r_end = rows;
    for (size_t r = (size_t)blockIdx.x * g.RB + ry; r < r_end; r += g.RL) {
      Chunk<T> v;
      v.load(x + r * pitch + (size_t)col * EPC);
#pragma unroll
      for (int e = 0; e < EPC; ++e) { acc[0][e] += v.v[e]; acc[1][e] += v.v[e] * v.v[e]; }
    }
  }
  block_col_reduce<EPC, 2>(acc, cx, ry, g.CW, g.RL, col, g.CPR, C, partial_sum, red);
}
// NOTE: partial layout here is the interleaved [row][2][C] of block_col_reduce<.,2>; stat_sum points at
// it and stat_sq is unused by the kernel -- bn_table_finalize is told through stride / offsets.
template <typename T>
int slice_stats(const T* x, int pitch, int C, size_t rows, float* stat_sum, float* stat_sq, int* nrows_out,
                hipStream_t st) {
  ARG_CHECK(C % DT<T>::EPC == 0 && pitch % DT<T>::EPC == 0, "slice_stats: C=%d pitch=%d", C, pitch);
  ARG_CHECK(stat_sq == stat_sum + C, "slice_stats: stat_sq must be stat_sum + C (interleaved [row][2][C] slab)");
  ColGeom g = col_geom(rows, C, DT<T>::EPC);
  hipLaunchKernelGGL(slice_stats_kernel<T>, dim3(g.gx, g.gy), dim3(256), 0, st, x, pitch, rows, C, g, stat_sum, stat_sq);
  HIP_CHECK_RET(hipGetLastError());
  *nrows_out = g.gx;
  return MMSKIN_OK;
}

template int slice_stats<float>(const float*, int, int, size_t, float*, float*, int*, hipStream_t);
template int slice_stats<bf16_t>(const bf16_t*, int, int, size_t, float*, float*, int*, hipStream_t);

__global__ void bn_coef_from_table_kernel(const float* __restrict__ mean_tab, const float* __restrict__ var_tab, int C,
                                          int Cp, const float* __restrict__ gamma, const float* __restrict__ beta,
                                          float eps, float momentum, double count, float* running_mean,
                                          float* running_var, int training, float* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cp) return;
  float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f, g = 0.f;
  if (c < C) {
    g = gamma[c];
    float var;
    if (training) {
      mu = mean_tab[c]; var = var_tab[c];
      double unbiased = count > 1.0 ? (double)var * count / (count - 1.0) : (double)var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    } else {
      mu = running_mean[c]; var = running_var[c];
    }
    is = (float)(1.0 / sqrt((double)var + (double)eps));
    sc = g * is;
    sh = beta[c] - mu * sc;
  }
  coef[c] = sc; coef[Cp + c] = sh; coef[2 * Cp + c] = mu; coef[3 * Cp + c] = is; coef[4 * Cp + c] = g;
}
int bn_coef_from_table(const float* mean_tab, const float* var_tab, int C, int Cp, const float* gamma,
                       const float* beta, float eps, float momentum, double count, float* running_mean,
                       float* running_var, bool training, float* coef, hipStream_t st) {
  hipLaunchKernelGGL(bn_coef_from_table_kernel, dim3(ceil_div(Cp, 256)), dim3(256), 0, st, mean_tab, var_tab, C, Cp,
                     gamma, beta, eps, momentum, count, running_mean, running_var, training ? 1 : 0, coef);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
