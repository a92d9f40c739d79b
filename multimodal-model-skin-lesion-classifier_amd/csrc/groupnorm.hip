// GroupNorm(8, C) + ReLU (+ 2x2 max-pool) on NHWC activations (declarations in ops.h): the normalisation of the NAS DynamicCNN trunk
// ([conv -> GroupNorm(8, C) -> ReLU] x layers, optional MaxPool2d(2, 2); dynamicMultimodalmodel.py of the reference).  fp32 or bf16 storage,
// fp32 arithmetic, C a multiple of 64, so a group (C / 8 channels) is a whole number of 16-byte chunks and a chunk never straddles two groups.
//
// Statistics: a workgroup owns a run of pixels of ONE sample; thread (row lane, chunk column) keeps fp64 sum / sum of squares of x - K (K = the first
// element it sees, so the sums carry the spread and not the offset), turns them into (count, mean, M2) and the eight group threads combine the
// lanes by Chan's formula in fp64; a finalize thread per (sample, group) combines the workgroups' partials in index order.  No atomics: the
// result depends on the launch shape only.
// Forward apply: z = relu(gamma * (y - mean) * rstd + beta) written once; with a pool the kernel walks the pooled grid instead, computes the four
// taps and stores ONLY the pooled value and its argmax byte (maxpool2_fwd's format and tie-break) -- the un-pooled z is never stored.
// Backward: the ReLU mask is recomputed from y (gn_pre is the one expression both directions evaluate), the pooled gradient is routed through
// the argmax bytes on the fly.  Pass 1 leaves per-workgroup per-channel sums of dz and dz * xhat (one sample per workgroup, so the per-(sample,
// group) sums of dz * gamma and dz * gamma * xhat follow from them); dgamma / dbeta go through the fp64 column reducer (bias_grad_finalize);
// pass 2 writes dy = rstd * (gamma * dz - (S1 + xhat * S2) / m) once.
// Trunk tail: the last activation's one consumer is AdaptiveAvgPool2d(1), so gn8_relu_gap_apply reduces relu(...) (or its 2x2 maxima)
// straight to feat[n][c] through per-workgroup partial rows and a fixed-order combine, and gn8_relu_gap_backward runs the same two backward
// passes with the gradient dfeat[n][c] / (OH * OW) formed in registers (with a pool: at the window's argmax, recomputed from y).  Neither z,
// nor the pooled tensor, nor argmax bytes, nor a gradient tensor exist for that layer.
#include "ops_internal.h"

namespace {

constexpr int GN_GROUPS = 8;
constexpr int GN_BLOCK = 256;
constexpr int GN_MAX_BLOCKS = 64;   // workgroups per sample at most (sizes the partial slabs)

// Workgroup geometry of the two reductions: CPR chunk columns x RL row lanes (threads beyond RL * CPR idle), PB pixels per workgroup.
struct GnGeom { int CPR, RL, PB, nblk; };
GnGeom gn_geom(int HW, int C, int EPC) {
  GnGeom g;
  g.CPR = C / EPC;
  g.RL = GN_BLOCK / g.CPR;
  int nblk = ceil_div(HW, g.RL * 32);
  if (nblk > GN_MAX_BLOCKS) nblk = GN_MAX_BLOCKS;
  g.PB = ceil_div(ceil_div(HW, nblk), g.RL) * g.RL;
  g.nblk = ceil_div(HW, g.PB);
  return g;
}

// the pre-activation: the one expression forward and backward evaluate, so the recomputed ReLU mask is the forward's
__device__ __forceinline__ float gn_pre(float xhat, float gamma, float beta) { return fmaf(xhat, gamma, beta); }
__device__ __forceinline__ float relu_keep_nan(float p) { return p < 0.f ? 0.f : p; }

template <typename T>
__global__ __launch_bounds__(GN_BLOCK) void gn_stats_kernel(const T* __restrict__ y, int HW, int C, int CPR, int RL, int PB,
                                                            double* __restrict__ partial) {   // [N][nblk][8][3]: count, mean, M2
  constexpr int EPC = DT<T>::EPC;
  __shared__ double red[GN_BLOCK][3];
  const int tid = threadIdx.x, cc = tid % CPR, ry = tid / CPR;
  const int n = blockIdx.y, p0 = blockIdx.x * PB, p1 = min(HW, p0 + PB);
  // fp64 accumulators: on bf16-representable inputs an fp32 sum of d * d rounds ties one way often enough to bias the variance by 1e-6
  // (measured against fp64); three fp64 operations per element stay far below what the loads cost
  double s = 0.0, q = 0.0;
  float K = 0.f;
  int cnt = 0;
  if (ry < RL) {
    const T* base = y + (size_t)n * HW * C + (size_t)cc * EPC;
    for (int p = p0 + ry; p < p1; p += RL) {
      Chunk<T> v;
      v.load(base + (size_t)p * C);
      if (cnt == 0) K = v.v[0];
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const double d = (double)(v.v[e] - K);
        s += d;
        q = fma(d, d, q);
      }
      cnt += EPC;
    }
  }
  double m = 0.0, M2 = 0.0;
  if (cnt) {
    const double nd = cnt;
    m = (double)K + s / nd;
    M2 = q - s * s / nd;
    if (M2 < 0.0) M2 = 0.0;
  }
  red[tid][0] = cnt; red[tid][1] = m; red[tid][2] = M2;
  __syncthreads();
  if (tid < GN_GROUPS) {   // Chan's combination of the lanes of group tid, in index order
    const int cg = CPR / GN_GROUPS;
    double na = 0.0, ma = 0.0, Ma = 0.0;
    for (int r = 0; r < RL; ++r)
      for (int c = 0; c < cg; ++c) {
        const int t = r * CPR + tid * cg + c;
        const double nb = red[t][0];
        if (nb == 0.0) continue;
        const double delta = red[t][1] - ma, nn = na + nb;
        ma += delta * nb / nn;
        Ma += red[t][2] + delta * delta * na * nb / nn;
        na = nn;
      }
    double* out = partial + (((size_t)n * gridDim.x + blockIdx.x) * GN_GROUPS + tid) * 3;
    out[0] = na; out[1] = ma; out[2] = Ma;
  }
}

__global__ void gn_stats_finalize_kernel(const double* __restrict__ partial, int NG, int nblk, float eps, float* __restrict__ mean,
                                         float* __restrict__ rstd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (sample, group)
  if (i >= NG) return;
  const int n = i / GN_GROUPS, g = i - n * GN_GROUPS;
  double na = 0.0, ma = 0.0, Ma = 0.0;
  for (int b = 0; b < nblk; ++b) {
    const double* p = partial + (((size_t)n * nblk + b) * GN_GROUPS + g) * 3;
    const double nb = p[0];
    if (nb == 0.0) continue;
    const double delta = p[1] - ma, nn = na + nb;
    ma += delta * nb / nn;
    Ma += p[2] + delta * delta * na * nb / nn;
    na = nn;
  }
  mean[i] = (float)ma;
  rstd[i] = (float)(1.0 / sqrt(Ma / na + (double)eps));
}

template <typename T>
__global__ __launch_bounds__(EW_BLOCK) void gn_relu_apply_kernel(const T* __restrict__ y, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int HW, int C, int CPR, T* __restrict__ z,
                                                                 size_t nchunks) {
  constexpr int EPC = DT<T>::EPC;
  const int cpg = C / GN_GROUPS;
  for (size_t i = blockIdx.x * (size_t)EW_BLOCK + threadIdx.x; i < nchunks; i += (size_t)gridDim.x * EW_BLOCK) {
    const int c0 = (int)(i % CPR) * EPC;
    const size_t n = i / ((size_t)HW * CPR);
    const float m = mean[n * GN_GROUPS + c0 / cpg], r = rstd[n * GN_GROUPS + c0 / cpg];
    Chunk<T> v;
    v.load(y + i * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v.v[e] = relu_keep_nan(gn_pre((v.v[e] - m) * r, gamma[c0 + e], beta[c0 + e]));
    v.store(z + i * EPC);
  }
}

// The activations of the four taps of the 2x2 window whose first tap is at p00, their maximum and its tap (first maximum, row-major; a NaN
// wins): the one place the pool's decision is made, for the pooled forward, the fused tail and the tail's backward, which recomputes it.
template <typename T>
__device__ __forceinline__ void gn_window_max(const T* __restrict__ p00, int W, int C, float m, float r, const float (&ga)[DT<T>::EPC],
                                              const float (&be)[DT<T>::EPC], Chunk<T>& best, uint8_t (&bi)[DT<T>::EPC]) {
  constexpr int EPC = DT<T>::EPC;
  Chunk<T> v[4];
  v[0].load(p00); v[1].load(p00 + C); v[2].load(p00 + (size_t)W * C); v[3].load(p00 + (size_t)W * C + C);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[k].v[e] = relu_keep_nan(gn_pre((v[k].v[e] - m) * r, ga[e], be[e]));
  best = v[0];
#pragma unroll
  for (int e = 0; e < EPC; ++e) bi[e] = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < EPC; ++e)
      if (v[k].v[e] > best.v[e] || v[k].v[e] != v[k].v[e]) { best.v[e] = v[k].v[e]; bi[e] = (uint8_t)k; }
}

// one thread per pooled chunk
template <typename T>
__global__ __launch_bounds__(EW_BLOCK) void gn_relu_pool_kernel(const T* __restrict__ y, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int H, int W, int C, int CPR,
                                                                T* __restrict__ pooled, uint8_t* __restrict__ idx, size_t nchunks) {
  constexpr int EPC = DT<T>::EPC;
  const int PH = H / 2, PW = W / 2, cpg = C / GN_GROUPS;
  for (size_t i = blockIdx.x * (size_t)EW_BLOCK + threadIdx.x; i < nchunks; i += (size_t)gridDim.x * EW_BLOCK) {
    const int c0 = (int)(i % CPR) * EPC;
    size_t t = i / CPR;
    const int pw = (int)(t % PW); t /= PW;
    const int ph = (int)(t % PH);
    const size_t n = t / PH;
    const float m = mean[n * GN_GROUPS + c0 / cpg], r = rstd[n * GN_GROUPS + c0 / cpg];
    float ga[EPC], be[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; }
    Chunk<T> best;
    uint8_t bi[EPC];
    gn_window_max<T>(y + ((n * H + 2 * ph) * W + 2 * pw) * C + c0, W, C, m, r, ga, be, best, bi);
    best.store(pooled + i * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) idx[i * EPC + e] = bi[e];
  }
}

// The fused tail, forward: a workgroup owns a run of (pooled) pixels of one sample, as in the statistics kernel; thread (row lane, chunk
// column) sums its activations in fp32, the row lanes are combined through LDS in index order: partial[(n * nblk + blk)][C].
template <typename T>
__global__ __launch_bounds__(GN_BLOCK) void gn_relu_gap_kernel(const T* __restrict__ y, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int H, int W, int C, int CPR, int RL, int PB,
                                                               int pool, float* __restrict__ partial) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float red[GN_BLOCK * EPC];   // [RL][C]
  const int tid = threadIdx.x, cc = tid % CPR, ry = tid / CPR, c0 = cc * EPC;
  const int OW = pool ? W / 2 : W, OHW = (pool ? H / 2 : H) * OW;
  const int n = blockIdx.y, p0 = blockIdx.x * PB, p1 = min(OHW, p0 + PB);
  if (ry < RL) {
    const int grp = c0 / (C / GN_GROUPS);
    const float m = mean[n * GN_GROUPS + grp], r = rstd[n * GN_GROUPS + grp];
    float ga[EPC], be[EPC], acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; acc[e] = 0.f; }
    const T* base = y + (size_t)n * H * W * C + c0;
    for (int p = p0 + ry; p < p1; p += RL) {
      Chunk<T> v;
      if (pool) {
        const int ph = p / OW, pw = p - ph * OW;
        uint8_t bi[EPC];
        gn_window_max<T>(base + ((size_t)(2 * ph) * W + 2 * pw) * C, W, C, m, r, ga, be, v, bi);
      } else {
        v.load(base + (size_t)p * C);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v.v[e] = relu_keep_nan(gn_pre((v.v[e] - m) * r, ga[e], be[e]));
      }
#pragma unroll
      for (int e = 0; e < EPC; ++e) acc[e] += v.v[e];
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[ry * C + c0 + e] = acc[e];
  }
  __syncthreads();
  float* out = partial + ((size_t)n * gridDim.x + blockIdx.x) * C;
  for (int c = tid; c < C; c += GN_BLOCK) {
    float s = 0.f;
    for (int r = 0; r < RL; ++r) s += red[r * C + c];
    out[c] = s;
  }
}

// feat[n][c] = the workgroups' partial sums of (n, c) in index order (fp64) / pixels
__global__ void gn_gap_finalize_kernel(const float* __restrict__ partial, int NC, int C, int nblk, double inv_cnt, float* __restrict__ feat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NC) return;
  const int n = i / C, c = i - n * C;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += (double)partial[((size_t)n * nblk + b) * C + c];
  feat[i] = (float)(s * inv_cnt);
}

// Where the gradient at z comes from.  Stored (GAP false): gout is the gradient at z (idx == nullptr) or at the pooled tensor, routed through
// its argmax bytes.  Trunk tail (GAP true): dfeat[n][c] * inv_cnt at every pixel, or with a pool at each window's argmax, recomputed from y.
template <typename T>
struct GnGrad {
  const T* gout;
  const uint8_t* idx;
  const float* dfeat;
  float inv_cnt;
  int pool;
};

// The gradient that reaches z at input pixel (n, h, w), chunk column cc (zero off the argmax, and in the row / column an odd extent leaves
// outside every window).  m, r, ga, be: the thread's statistics and affine parameters (GAP with a pool evaluates the window's activations).
template <typename T, bool GAP>
__device__ __forceinline__ void gn_grad_at(const GnGrad<T>& s, const T* __restrict__ y, size_t n, int h, int w, int H, int W, int CPR, int cc,
                                           float m, float r, const float (&ga)[DT<T>::EPC], const float (&be)[DT<T>::EPC], Chunk<T>& g) {
  constexpr int EPC = DT<T>::EPC;
  const int PH = H / 2, PW = W / 2, ph = h >> 1, pw = w >> 1, tap = (h & 1) * 2 + (w & 1);
  if constexpr (GAP) {
    const int C = CPR * EPC;
#pragma unroll
    for (int e = 0; e < EPC; ++e) g.v[e] = s.dfeat[n * C + cc * EPC + e] * s.inv_cnt;
    if (!s.pool) return;
    if (ph < PH && pw < PW) {
      Chunk<T> best;
      uint8_t bi[EPC];
      gn_window_max<T>(y + (((n * H + 2 * ph) * W + 2 * pw) * CPR + cc) * EPC, W, C, m, r, ga, be, best, bi);
#pragma unroll
      for (int e = 0; e < EPC; ++e)
        if ((int)bi[e] != tap) g.v[e] = 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < EPC; ++e) g.v[e] = 0.f;
    }
  } else {
    if (!s.idx) {
      g.load(s.gout + (((n * H + h) * W + w) * CPR + cc) * EPC);
      return;
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) g.v[e] = 0.f;
    if (ph < PH && pw < PW) {
      const size_t po = (((n * PH + ph) * PW + pw) * CPR + cc) * EPC;
      Chunk<T> t;
      t.load(s.gout + po);
      uint32_t taps[EPC / 4];   // po is a multiple of EPC: the chunk's argmax bytes are EPC / 4 aligned words
#pragma unroll
      for (int j = 0; j < EPC / 4; ++j) taps[j] = *reinterpret_cast<const uint32_t*>(s.idx + po + 4 * j);
#pragma unroll
      for (int e = 0; e < EPC; ++e)
        if ((int)((taps[e >> 2] >> (8 * (e & 3))) & 0xffu) == tap) g.v[e] = t.v[e];
    }
  }
}

// pass 1: partial[(n * nblk + blk)][0][C] = sum dz, [1][C] = sum dz * xhat over the workgroup's pixels of sample n
template <typename T, bool GAP>
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_reduce_kernel(const GnGrad<T> src, const T* __restrict__ y, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int H, int W, int C, int CPR, int RL, int PB,
                                                                 float* __restrict__ partial) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float red[2 * GN_BLOCK * EPC];   // [2][RL][C]
  const int tid = threadIdx.x, cc = tid % CPR, ry = tid / CPR, HW = H * W;
  const int n = blockIdx.y, p0 = blockIdx.x * PB, p1 = min(HW, p0 + PB);
  const int c0 = cc * EPC;
  float acc[2][EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (ry < RL) {
    const int grp = c0 / (C / GN_GROUPS);
    const float m = mean[n * GN_GROUPS + grp], r = rstd[n * GN_GROUPS + grp];
    float ga[EPC], be[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; }
    for (int p = p0 + ry; p < p1; p += RL) {
      const int h = p / W, w = p - h * W;
      Chunk<T> v, g;
      v.load(y + ((size_t)n * HW + p) * C + c0);
      gn_grad_at<T, GAP>(src, y, (size_t)n, h, w, H, W, CPR, cc, m, r, ga, be, g);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float xh = (v.v[e] - m) * r;
        const float dz = gn_pre(xh, ga[e], be[e]) > 0.f ? g.v[e] : 0.f;
        acc[0][e] += dz;
        acc[1][e] = fmaf(dz, xh, acc[1][e]);
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int e = 0; e < EPC; ++e) red[(q * RL + ry) * C + c0 + e] = acc[q][e];
  }
  __syncthreads();
  float* out = partial + ((size_t)n * gridDim.x + blockIdx.x) * 2 * C;
  for (int i = tid; i < 2 * C; i += GN_BLOCK) {
    const int q = i / C, c = i - q * C;
    float s = 0.f;
    for (int r = 0; r < RL; ++r) s += red[(q * RL + r) * C + c];
    out[i] = s;
  }
}

// one wavefront per (sample, group): S1 = sum gamma * sum dz, S2 = sum gamma * sum dz xhat over the group's channels and the sample's
// workgroups, fp64, lane partials combined by a butterfly (every lane adds the same pairs: repeatable)
__global__ __launch_bounds__(64) void gn_group_sums_kernel(const float* __restrict__ partial, const float* __restrict__ gamma, int nblk, int C,
                                                           float* __restrict__ sums) {   // [N * 8][2]
  const int n = blockIdx.x / GN_GROUPS, g = blockIdx.x % GN_GROUPS, cpg = C / GN_GROUPS;
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nblk * cpg; i += 64) {
    const int b = i / cpg, c = g * cpg + (i - b * cpg);
    const float* row = partial + ((size_t)n * nblk + b) * 2 * C;
    const double gm = gamma[c];
    s1 += gm * (double)row[c];
    s2 += gm * (double)row[C + c];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if (threadIdx.x == 0) { sums[2 * blockIdx.x] = (float)s1; sums[2 * blockIdx.x + 1] = (float)s2; }
}

// pass 2: dy = rstd * (gamma * dz - (S1 + xhat * S2) / m), one thread per input chunk
template <typename T, bool GAP>
__global__ __launch_bounds__(EW_BLOCK) void gn_bwd_apply_kernel(const GnGrad<T> src, const T* __restrict__ y, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ sums, int H, int W,
                                                                int C, int CPR, float inv_m, T* __restrict__ dy, size_t nchunks) {
  constexpr int EPC = DT<T>::EPC;
  const int cpg = C / GN_GROUPS;
  for (size_t i = blockIdx.x * (size_t)EW_BLOCK + threadIdx.x; i < nchunks; i += (size_t)gridDim.x * EW_BLOCK) {
    const int cc = (int)(i % CPR), c0 = cc * EPC;
    size_t t = i / CPR;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H);
    const size_t n = t / H;
    const size_t sg = n * GN_GROUPS + c0 / cpg;
    const float m = mean[sg], r = rstd[sg], S1 = sums[2 * sg], S2 = sums[2 * sg + 1];
    float ga[EPC], be[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; }
    Chunk<T> v, g;
    v.load(y + i * EPC);
    gn_grad_at<T, GAP>(src, y, n, h, w, H, W, CPR, cc, m, r, ga, be, g);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float xh = (v.v[e] - m) * r;
      const float dz = gn_pre(xh, ga[e], be[e]) > 0.f ? g.v[e] : 0.f;
      v.v[e] = r * (ga[e] * dz - fmaf(xh, S2, S1) * inv_m);
    }
    v.store(dy + i * EPC);
  }
}

}  // namespace

int gn8_check(int N, int C, int H, int W, int groups, bool pool, const char* who) {
  if (groups != GN_GROUPS || C <= 0 || C % 64 != 0 || C > 1024) {
    mmskin_set_error("%s: GroupNorm with %d groups over %d channels is not supported (8 groups, C a multiple of 64, C <= 1024)", who, groups, C);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  ARG_CHECK(N > 0 && H > 0 && W > 0 && (!pool || (H >= 2 && W >= 2)), "%s: bad shape N = %d, map %dx%d%s", who, N, H, W,
            pool ? " (the 2x2 pool needs at least 2x2)" : "");
  ARG_CHECK((int64_t)H * W <= (int64_t)1 << 24, "%s: map %dx%d too large", who, H, W);
  return MMSKIN_OK;
}
size_t gn8_stat_scratch_bytes(int N) { return (size_t)N * GN_MAX_BLOCKS * GN_GROUPS * 3 * sizeof(double); }
size_t gn8_bwd_partial_bytes(int N, int C) { return (size_t)N * GN_MAX_BLOCKS * 2 * C * sizeof(float); }

template <typename T>
int gn8_stats(const T* y, int N, int HW, int C, float eps, double* scratch, float* mean, float* rstd, hipStream_t st) {
  const GnGeom g = gn_geom(HW, C, DT<T>::EPC);
  hipLaunchKernelGGL(gn_stats_kernel<T>, dim3(g.nblk, N), dim3(GN_BLOCK), 0, st, y, HW, C, g.CPR, g.RL, g.PB, scratch);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3(ceil_div(N * GN_GROUPS, 64)), dim3(64), 0, st, scratch, N * GN_GROUPS, g.nblk, eps, mean, rstd);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

template <typename T>
int gn8_relu_apply(const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int H, int W, int C, T* z,
                   hipStream_t st) {
  constexpr int EPC = DT<T>::EPC;
  const size_t nch = (size_t)N * H * W * (C / EPC);
  hipLaunchKernelGGL(gn_relu_apply_kernel<T>, dim3(ew_grid(nch)), dim3(EW_BLOCK), 0, st, y, mean, rstd, gamma, beta, H * W, C, C / EPC, z, nch);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

template <typename T>
int gn8_relu_pool_apply(const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int H, int W, int C,
                        T* pooled, uint8_t* idx, hipStream_t st) {
  constexpr int EPC = DT<T>::EPC;
  ARG_CHECK(H >= 2 && W >= 2, "gn8_relu_pool_apply: map %dx%d smaller than the window", H, W);
  const size_t nch = (size_t)N * (H / 2) * (W / 2) * (C / EPC);
  hipLaunchKernelGGL(gn_relu_pool_kernel<T>, dim3(ew_grid(nch)), dim3(EW_BLOCK), 0, st, y, mean, rstd, gamma, beta, H, W, C, C / EPC, pooled, idx,
                     nch);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

template <typename T>
int gn8_relu_gap_apply(const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int H, int W, int C,
                       bool pool, float* partial, float* feat, hipStream_t st) {
  ARG_CHECK(!pool || (H >= 2 && W >= 2), "gn8_relu_gap_apply: map %dx%d smaller than the window", H, W);
  const int OHW = pool ? (H / 2) * (W / 2) : H * W;
  const GnGeom g = gn_geom(OHW, C, DT<T>::EPC);
  hipLaunchKernelGGL(gn_relu_gap_kernel<T>, dim3(g.nblk, N), dim3(GN_BLOCK), 0, st, y, mean, rstd, gamma, beta, H, W, C, g.CPR, g.RL, g.PB,
                     (int)pool, partial);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(gn_gap_finalize_kernel, dim3(ceil_div(N * C, 256)), dim3(256), 0, st, partial, N * C, C, g.nblk, 1.0 / (double)OHW, feat);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

namespace {
// the backward of both gradient sources: pass 1, the group sums, dgamma / dbeta through the column reducer, pass 2
template <typename T, bool GAP>
int gn_backward_launch(const GnGrad<T>& src, const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int H,
                       int W, int C, float* partial, float* sums, ColScratch red, float* dgamma, float* dbeta, T* dy, hipStream_t st) {
  constexpr int EPC = DT<T>::EPC;
  const GnGeom g = gn_geom(H * W, C, EPC);
  hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, GAP>), dim3(g.nblk, N), dim3(GN_BLOCK), 0, st, src, y, mean, rstd, gamma, beta, H, W, C, g.CPR, g.RL,
                     g.PB, partial);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(gn_group_sums_kernel, dim3(N * GN_GROUPS), dim3(64), 0, st, partial, gamma, g.nblk, C, sums);
  HIP_CHECK_RET(hipGetLastError());
  if (int rc = bias_grad_finalize(partial, N * g.nblk, 2 * C, C, dbeta, red, st)) return rc;
  if (int rc = bias_grad_finalize(partial + C, N * g.nblk, 2 * C, C, dgamma, red, st)) return rc;
  const size_t nch = (size_t)N * H * W * (C / EPC);
  const float inv_m = 1.f / ((float)(H * W) * (float)(C / GN_GROUPS));
  hipLaunchKernelGGL((gn_bwd_apply_kernel<T, GAP>), dim3(ew_grid(nch)), dim3(EW_BLOCK), 0, st, src, y, mean, rstd, gamma, beta, sums, H, W, C,
                     C / EPC, inv_m, dy, nch);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
}  // namespace

template <typename T>
int gn8_relu_backward(const T* gout, const uint8_t* idx, const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      int N, int H, int W, int C, float* partial, float* sums, ColScratch red, float* dgamma, float* dbeta, T* dy,
                      hipStream_t st) {
  const GnGrad<T> src = {gout, idx, nullptr, 0.f, idx != nullptr};
  return gn_backward_launch<T, false>(src, y, mean, rstd, gamma, beta, N, H, W, C, partial, sums, red, dgamma, dbeta, dy, st);
}

template <typename T>
int gn8_relu_gap_backward(const float* dfeat, const T* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int H,
                          int W, int C, bool pool, float* partial, float* sums, ColScratch red, float* dgamma, float* dbeta, T* dy,
                          hipStream_t st) {
  ARG_CHECK(!pool || (H >= 2 && W >= 2), "gn8_relu_gap_backward: map %dx%d smaller than the window", H, W);
  const int OHW = pool ? (H / 2) * (W / 2) : H * W;
  const GnGrad<T> src = {nullptr, nullptr, dfeat, 1.f / (float)OHW, (int)pool};
  return gn_backward_launch<T, true>(src, y, mean, rstd, gamma, beta, N, H, W, C, partial, sums, red, dgamma, dbeta, dy, st);
}

#define INSTANTIATE(T)                                                                                                                          \
  template int gn8_stats<T>(const T*, int, int, int, float, double*, float*, float*, hipStream_t);                                              \
  template int gn8_relu_apply<T>(const T*, const float*, const float*, const float*, const float*, int, int, int, int, T*, hipStream_t);        \
  template int gn8_relu_pool_apply<T>(const T*, const float*, const float*, const float*, const float*, int, int, int, int, T*, uint8_t*,       \
                                      hipStream_t);                                                                                             \
  template int gn8_relu_backward<T>(const T*, const uint8_t*, const T*, const float*, const float*, const float*, const float*, int, int, int,  \
                                    int, float*, float*, ColScratch, float*, float*, T*, hipStream_t);                                          \
  template int gn8_relu_gap_apply<T>(const T*, const float*, const float*, const float*, const float*, int, int, int, int, bool, float*, float*, \
                                     hipStream_t);                                                                                              \
  template int gn8_relu_gap_backward<T>(const float*, const T*, const float*, const float*, const float*, const float*, int, int, int, int,     \
                                        bool, float*, float*, ColScratch, float*, float*, T*, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(bf16_t)
