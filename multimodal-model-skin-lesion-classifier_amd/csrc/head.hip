// Transformer / fusion-head operators for gfx950 that are not a dense layer: LayerNorm (fp32 in, fp32 and / or bf16 out), the small
// softmax-attention kernel families (one workgroup or one wave per (batch, head), window attention) with row softmax, the pointwise
// gates / dropout / concat / GELU / StarReLU / LayerScale ops, the MD-Net fusion pool, Adam over a flat parameter range, embedding
// gather, and the custom-CNN direct conv and pooling.  Replaces nn.LayerNorm / sigmoid gates / MetaBlock / gated-residual pointwise
// math / small softmax attention / embedding gather of multimodalIntraInterModal.py:172-412, metablock.py:27-32,
// gatedResidualBlock.py:12-17, tab_transformer.py:40-60.  Row reductions (LayerNorm, softmax) are wavefront-shuffle reductions, one
// 64-lane wave per row.  nn.Linear, the strided fp32 GEMM / bmm and the column sums live in linear.hip.
#include <stdlib.h>
#include <string.h>

#include "../../include/mmskin.h"
#include "head_internal.h"

// ------------------------------------------------------------------ LayerNorm
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ b, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd, int M,
                                                            int N, float eps, int relu) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (int64_t)row * N;
  float s = 0.f;
  for (int i = lane; i < N; i += 64) s += xr[i];
  const float mu = wave_sum(s) / (float)N;
  float q = 0.f;
  for (int i = lane; i < N; i += 64) { float d = xr[i] - mu; q += d * d; }
  const float rs = 1.0f / sqrtf(wave_sum(q) / (float)N + eps);
  for (int i = lane; i < N; i += 64) {
    float v = (xr[i] - mu) * rs * g[i] + (b ? b[i] : 0.f);
    if (relu) v = fmaxf(v, 0.f);
    y[(int64_t)row * N + i] = v;
  }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

__global__ __launch_bounds__(256) void layernorm_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ g, const float* __restrict__ b,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dx,
                                                               int M, int N, int relu) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float mu = mean[row], rs = rstd[row];
  const float* xr = x + (int64_t)row * N;
  const float* dr = dy + (int64_t)row * N;
  float c1 = 0.f, c2 = 0.f;
  for (int i = lane; i < N; i += 64) {
    float xh = (xr[i] - mu) * rs;
    float d = dr[i];
    if (relu && !(xh * g[i] + (b ? b[i] : 0.f) > 0.f)) d = 0.f;
    float dg = d * g[i];
    c1 += dg; c2 += dg * xh;
  }
  c1 = wave_sum(c1) / (float)N; c2 = wave_sum(c2) / (float)N;
  for (int i = lane; i < N; i += 64) {
    float xh = (xr[i] - mu) * rs;
    float d = dr[i];
    if (relu && !(xh * g[i] + (b ? b[i] : 0.f) > 0.f)) d = 0.f;
    dx[(int64_t)row * N + i] = rs * (d * g[i] - c1 - xh * c2);
  }
}

// gamma/beta gradients: blockIdx.y = row group -> part[(y*2 + {0,1})*N + n]; 64 columns x 4 row lanes per block
__global__ __launch_bounds__(256) void layernorm_bwd_gb_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ g, const float* __restrict__ b,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               float* __restrict__ part, int M, int N, int relu, int per) {
  __shared__ float red[2][4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cx;
  const int m_end = min(M, ((int)blockIdx.y + 1) * per);
  float sg = 0.f, sb = 0.f;
  if (n < N) {
    const float gn = g[n], bn = b ? b[n] : 0.f;
    for (int m = blockIdx.y * per + ry; m < m_end; m += 4) {
      float xh = (x[(int64_t)m * N + n] - mean[m]) * rstd[m];
      float d = dy[(int64_t)m * N + n];
      if (relu && !(xh * gn + bn > 0.f)) d = 0.f;
      sg += d * xh; sb += d;
    }
  }
  red[0][ry][cx] = sg; red[1][ry][cx] = sb;
  __syncthreads();
  if (ry == 0 && n < N) {
    part[((int64_t)blockIdx.y * 2) * N + n] = (red[0][0][cx] + red[0][1][cx]) + (red[0][2][cx] + red[0][3][cx]);
    part[((int64_t)blockIdx.y * 2 + 1) * N + n] = (red[1][0][cx] + red[1][1][cx]) + (red[1][2][cx] + red[1][3][cx]);
  }
}
// dg[n] = sum_y part[(2y)*N + n], db[n] = sum_y part[(2y+1)*N + n]
__global__ void layernorm_gb_reduce_kernel(const float* __restrict__ part, float* dg, float* db, int G, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float sg = 0.f, sb = 0.f;
  for (int y = 0; y < G; ++y) { sg += part[((int64_t)y * 2) * N + n]; sb += part[((int64_t)y * 2 + 1) * N + n]; }
  if (dg) dg[n] = sg;
  if (db) db[n] = sb;
}

// Row-in-registers LayerNorm (N % 4 == 0, N <= 2048, no ReLU): LPR lanes own one row (LPR = 32 for N <= 128 so a 64-wide wave
// carries two rows instead of idling 40 lanes), NJ float4 chunks per lane, ONE pass over memory.
//   forward : y as fp32 and / or bf16 (what a bf16-operand Linear consumes), mean / rstd when a backward follows
//   backward: dx AND the lane's running sums of dy * xhat / dy over all the rows it visits -> part[slot][2][N]; a second small
//             kernel adds the slots.  Replaces dx pass + column pass + serial 1-3 block reduction (94 us per LayerNorm of the
//             DaViT stage-1 shape, three reads of dy and x) by one read of each.
template <int LPR> __device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int NJ, int LPR>
__global__ __launch_bounds__(256) void layernorm_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                 const float* __restrict__ b, float* __restrict__ y32,
                                                                 bf16_t* __restrict__ y16, float* __restrict__ mean,
                                                                 float* __restrict__ rstd, int M, int N, float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, sub = lane / LPR, sl = lane % LPR;
  const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + sub;
  const bool live = row < M;
  const float* xr = x + (int64_t)(live ? row : 0) * N;
  float4 v[NJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = (j * LPR + sl) * 4;
    v[j] = (live && i < N) ? *reinterpret_cast<const float4*>(xr + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  }
  const float mu = row_sum<LPR>(s) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = (j * LPR + sl) * 4;
    if (i < N) { const float a = v[j].x - mu, c = v[j].y - mu, d = v[j].z - mu, e = v[j].w - mu; q += (a * a + c * c) + (d * d + e * e); }
  }
  const float rs = 1.0f / sqrtf(row_sum<LPR>(q) / (float)N + eps);
  if (!live) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = (j * LPR + sl) * 4;
    if (i >= N) continue;
    const float4 gg = *reinterpret_cast<const float4*>(g + i), bb = b ? *reinterpret_cast<const float4*>(b + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 o = make_float4((v[j].x - mu) * rs * gg.x + bb.x, (v[j].y - mu) * rs * gg.y + bb.y,
                                 (v[j].z - mu) * rs * gg.z + bb.z, (v[j].w - mu) * rs * gg.w + bb.w);
    if (y32) *reinterpret_cast<float4*>(y32 + (int64_t)row * N + i) = o;
    if (y16) *reinterpret_cast<uint2*>(y16 + (int64_t)row * N + i) = make_uint2(f32_to_bf16_bits(o.x) | (f32_to_bf16_bits(o.y) << 16),
                                                                                f32_to_bf16_bits(o.z) | (f32_to_bf16_bits(o.w) << 16));
  }
  if (sl == 0 && mean) { mean[row] = mu; rstd[row] = rs; }
}

template <int NJ, int LPR>
__global__ __launch_bounds__(256) void layernorm_bwd_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ g, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ dx,
                                                                 float* __restrict__ part, int M, int N) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, sub = lane / LPR, sl = lane % LPR;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), nslots = gridDim.x * 4;
  float4 gg[NJ], ag[NJ], ab[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = (j * LPR + sl) * 4;
    gg[j] = i < N ? *reinterpret_cast<const float4*>(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    ag[j] = ab[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float invN = 1.0f / (float)N;
  for (int base = slot * RPW; base < M; base += nslots * RPW) {   // wave-uniform trip count: the shuffles below run converged
    const int row = base + sub;
    const bool live = row < M;
    const int64_t off = (int64_t)(live ? row : 0) * N;
    const float mu = mean[live ? row : 0], rs = rstd[live ? row : 0];
    float4 xh[NJ], dg[NJ];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = (j * LPR + sl) * 4;
      const bool ok = live && i < N;
      const float4 xv = ok ? *reinterpret_cast<const float4*>(x + off + i) : make_float4(mu, mu, mu, mu);
      const float4 d = ok ? *reinterpret_cast<const float4*>(dy + off + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      xh[j] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
      dg[j] = make_float4(d.x * gg[j].x, d.y * gg[j].y, d.z * gg[j].z, d.w * gg[j].w);
      c1 += (dg[j].x + dg[j].y) + (dg[j].z + dg[j].w);
      c2 += (dg[j].x * xh[j].x + dg[j].y * xh[j].y) + (dg[j].z * xh[j].z + dg[j].w * xh[j].w);
      ag[j].x += d.x * xh[j].x; ag[j].y += d.y * xh[j].y; ag[j].z += d.z * xh[j].z; ag[j].w += d.w * xh[j].w;
      ab[j].x += d.x; ab[j].y += d.y; ab[j].z += d.z; ab[j].w += d.w;
    }
    c1 = row_sum<LPR>(c1) * invN; c2 = row_sum<LPR>(c2) * invN;
    if (dx && live) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int i = (j * LPR + sl) * 4;
        if (i < N)
          *reinterpret_cast<float4*>(dx + off + i) = make_float4(rs * (dg[j].x - c1 - xh[j].x * c2), rs * (dg[j].y - c1 - xh[j].y * c2),
                                                                 rs * (dg[j].z - c1 - xh[j].z * c2), rs * (dg[j].w - c1 - xh[j].w * c2));
      }
    }
  }
  if (!part) return;
  // the block's 4 * RPW row groups meet in LDS (gamma sums, then beta sums through the same buffer): one partial row per block
  __shared__ float red[4 * RPW][NJ * LPR * 4];
  const int wv = (threadIdx.x >> 6) * RPW + sub;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = (j * LPR + sl) * 4;
      if (i < N) *reinterpret_cast<float4*>(&red[wv][i]) = which ? ab[j] : ag[j];
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += 256) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 4 * RPW; ++r) t += red[r][n];
      part[((int64_t)blockIdx.x * 2 + which) * N + n] = t;
    }
    __syncthreads();
  }
}
// NJ / LPR dispatch: N <= 128 -> two rows per wave; else the smallest NJ with 256 * NJ >= N
#define LN_ROWS_DISPATCH(N, CALL)                                                                   \
  do {                                                                                              \
    if ((N) <= 128) { CALL(1, 32); }                                                                \
    else if ((N) <= 256) { CALL(1, 64); }                                                           \
    else if ((N) <= 512) { CALL(2, 64); }                                                           \
    else if ((N) <= 768) { CALL(3, 64); }                                                           \
    else if ((N) <= 1024) { CALL(4, 64); }                                                          \
    else if ((N) <= 1536) { CALL(6, 64); }                                                          \
    else { CALL(8, 64); }                                                                           \
  } while (0)
static inline bool ln_rows_ok(int N, int relu) { return !relu && N % 4 == 0 && N <= 2048; }

// ------------------------------------------------------------------ pointwise gates
__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + __expf(-z)); }

#define EW_LOOP(n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ void sigmoid_gate_fwd_kernel(const float* z, const float* v, float* out, int64_t n) {
  EW_LOOP(n) out[i] = (1.f / (1.f + expf(-z[i]))) * v[i];
}
__global__ void sigmoid_gate_bwd_kernel(const float* dout, const float* z, const float* v, float* dz, float* dv, int64_t n) {
  EW_LOOP(n) {
    float s = 1.f / (1.f + expf(-z[i]));
    float d = dout[i];
    dz[i] = d * v[i] * s * (1.f - s);
    dv[i] = d * s;
  }
}
__global__ void gated_mix_fwd_kernel(const float* z, const float* a, const float* q, float* out, int64_t n) {
  EW_LOOP(n) {
    float gt = 1.f / (1.f + expf(-z[i]));
    out[i] = gt * a[i] + (1.f - gt) * q[i];
  }
}
__global__ void gated_mix_bwd_kernel(const float* dout, const float* z, const float* a, const float* q, float* dz,
                                     float* da, float* dq, int64_t n) {
  EW_LOOP(n) {
    float gt = 1.f / (1.f + expf(-z[i]));
    float d = dout[i];
    dz[i] = d * (a[i] - q[i]) * gt * (1.f - gt);
    da[i] = d * gt;
    dq[i] = d * (1.f - gt);
  }
}
__global__ void metablock_gate_fwd_kernel(const float* V, const float* t1, const float* t2, float* out, int64_t n) {
  EW_LOOP(n) out[i] = 1.f / (1.f + expf(-(tanhf(V[i] * t1[i]) + t2[i])));
}
__global__ void metablock_gate_bwd_kernel(const float* dout, const float* V, const float* t1, const float* t2,
                                          float* dV, float* dt1, float* dt2, int64_t n) {
  EW_LOOP(n) {
    float u = tanhf(V[i] * t1[i]);
    float o = 1.f / (1.f + expf(-(u + t2[i])));
    float ds = dout[i] * o * (1.f - o);
    float dp = ds * (1.f - u * u);
    dt2[i] = ds;
    dV[i] = dp * t1[i];
    dt1[i] = dp * V[i];
  }
}

__global__ void dropout_fwd_kernel(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed,
                                   uint64_t offset) {
  const float scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
  EW_LOOP(n) {
    uint64_t h = mix64(mix64(seed) ^ (offset + (uint64_t)i));
    float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    uint8_t keep = u >= p ? 1 : 0;
    mask[i] = keep;
    y[i] = keep ? x[i] * scale : 0.f;
  }
}
// dropout on attention PROBABILITIES laid out [rows][L] (the unfused softmax-attention chain): the (row, key) generator of common.h, so the
// unfused chain drops exactly what the fused kernels drop
__global__ void attn_dropout_fwd_kernel(const float* x, float* y, uint8_t* mask, int64_t n, int L, float p, uint64_t seed, uint64_t offset) {
  const float scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
  const AttnDropKey dk = attn_drop_key(seed, offset, p);
  const int Lh = (L + 1) >> 1;
  EW_LOOP(n) {
    const uint64_t row = (uint64_t)i / (uint64_t)L;
    const int key = (int)((uint64_t)i - row * (uint64_t)L);
    const uint8_t keep = attn_keep(dk, attn_row_base(row, Lh), key) ? 1 : 0;
    mask[i] = keep;
    y[i] = keep ? x[i] * scale : 0.f;
  }
}
__global__ void dropout_bwd_kernel(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p) {
  const float scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
  EW_LOOP(n) dx[i] = mask[i] ? dy[i] * scale : 0.f;
}
__global__ void concat2_fwd_kernel(const float* a, const float* b, float* out, int M, int Na, int Nb) {
  const int N = Na + Nb;
  EW_LOOP((int64_t)M * N) {
    int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
    out[i] = n < Na ? a[(int64_t)m * Na + n] : b[(int64_t)m * Nb + n - Na];
  }
}
__global__ void concat2_bwd_kernel(const float* dout, float* da, float* db, int M, int Na, int Nb) {
  const int N = Na + Nb;
  EW_LOOP((int64_t)M * N) {
    int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
    if (n < Na) da[(int64_t)m * Na + n] = dout[i];
    else db[(int64_t)m * Nb + n - Na] = dout[i];
  }
}

// ------------------------------------------------------------------ small softmax attention
// one workgroup per (b, h); L*L scores in LDS; one wave per score row for the softmax.  Training-mode
// dropout on the attention probabilities (nn.MultiheadAttention(dropout=p) inside the TabTransformer's
// encoder layers) uses the same counter-based generator as the dropout op: element gi of call `offset`.
// (the generator: attn_keep / AttnDropKey in common.h, shared with the fused kernels of flash_attn*.hip)
__global__ __launch_bounds__(256) void attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, float* __restrict__ o,
                                                            float* __restrict__ p, int L, int Dh, float drop_p,
                                                            uint64_t seed, uint64_t offset) {
  extern __shared__ float sc[];  // [L][L]
  const int64_t base = (int64_t)blockIdx.x * L * Dh;
  const float scale = 1.0f / sqrtf((float)Dh);
  for (int idx = threadIdx.x; idx < L * L; idx += 256) {
    int i = idx / L, j = idx - i * L;
    float s = 0.f;
    for (int d = 0; d < Dh; ++d) s += q[base + i * Dh + d] * k[base + j * Dh + d];
    sc[idx] = s * scale;
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wid; i < L; i += 4) {
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, sc[i * L + j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < L; j += 64) { float e = expf(sc[i * L + j] - mx); sc[i * L + j] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int j = lane; j < L; j += 64) {
      float pv = sc[i * L + j] * inv;
      const int64_t gi = (int64_t)blockIdx.x * L * L + i * L + j;
      p[gi] = pv;   // the pure softmax is what backward needs; the dropout mask is recomputed there
      if (drop_p > 0.f) pv = attn_keep(attn_drop_key(seed, offset, drop_p), attn_row_base((uint64_t)blockIdx.x * L + i, (L + 1) >> 1), j) ? pv * (1.f / (1.f - drop_p)) : 0.f;
      sc[i * L + j] = pv;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * Dh; idx += 256) {
    int i = idx / Dh, d = idx - i * Dh;
    float s = 0.f;
    for (int j = 0; j < L; ++j) s += sc[i * L + j] * v[base + j * Dh + d];
    o[base + idx] = s;
  }
}
__global__ __launch_bounds__(256) void attention_bwd_kernel(const float* __restrict__ dO, const float* __restrict__ q,
                                                            const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ p, float* __restrict__ dq,
                                                            float* __restrict__ dk, float* __restrict__ dv, int L,
                                                            int Dh, float drop_p, uint64_t seed, uint64_t offset) {
  extern __shared__ float ds[];  // [L][L]
  const int64_t base = (int64_t)blockIdx.x * L * Dh;
  const int64_t pbase = (int64_t)blockIdx.x * L * L;
  const float* pp = p + pbase;
  const float scale = 1.0f / sqrtf((float)Dh);
  const float dscale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  for (int idx = threadIdx.x; idx < L * L; idx += 256) {   // dropout factor of every probability
    const int i = idx / L, j = idx - i * L;
    ds[idx] = (drop_p > 0.f && !attn_keep(attn_drop_key(seed, offset, drop_p), attn_row_base((uint64_t)blockIdx.x * L + i, (L + 1) >> 1), j)) ? 0.f : dscale;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * Dh; idx += 256) {  // dV = P'^T dO,  P' = P * factor
    int j = idx / Dh, d = idx - j * Dh;
    float s = 0.f;
    for (int i = 0; i < L; ++i) s += pp[i * L + j] * ds[i * L + j] * dO[base + i * Dh + d];
    dv[base + idx] = s;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * L; idx += 256) {  // dP = (dO V^T) * factor
    int i = idx / L, j = idx - i * L;
    float s = 0.f;
    for (int d = 0; d < Dh; ++d) s += dO[base + i * Dh + d] * v[base + j * Dh + d];
    ds[idx] *= s;
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wid; i < L; i += 4) {
    float dot = 0.f;
    for (int j = lane; j < L; j += 64) dot += ds[i * L + j] * pp[i * L + j];
    dot = wave_sum(dot);
    for (int j = lane; j < L; j += 64) ds[i * L + j] = pp[i * L + j] * (ds[i * L + j] - dot) * scale;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < L * Dh; idx += 256) {
    int i = idx / Dh, d = idx - i * Dh;
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < L; ++j) {
      s1 += ds[i * L + j] * k[base + j * Dh + d];   // dq[i]
      s2 += ds[j * L + i] * q[base + j * Dh + d];   // dk[i]
    }
    dq[base + idx] = s1;
    dk[base + idx] = s2;
  }
}

// ------------------------------------------------------------------ small softmax attention, one WAVE per (batch, head)
// L <= 64 tokens, Dh = 32 or 64 (window attention of DaViT / Swin-style encoders, TabTransformer columns): lane i owns query
// row i -- its scores, its softmax and its output row live in that lane's registers, so the softmax needs no cross-lane step --
// and the key / value rows, which are the same for every lane, come through SCALAR loads (one s_load per 16 values, fed to v_fma
// as the SGPR operand): no LDS staging, no barrier.  q / k / v / o are addressed by (batch, head, token) element strides, so the
// kernel reads the packed [B, L, 3, H, Dh] output of a fused qkv Linear in place and writes the token-major [B, L, H, Dh] tensor
// the output projection wants.  The backward recomputes the probabilities from the saved row log-sum-exp (no [B, H, L, L] tensor
// is ever stored), forms dS / P' rows in the lanes that own the query rows, passes them through a wave-private LDS tile and
// re-reads them by COLUMN with lane j owning key row j for dK / dV.  fp32 throughout (exact-parity path: it replaces the
// one-workgroup-per-head kernel above, 507 / 605 us forward / backward on DaViT's 12 288 windows of 49 tokens).
struct AttnRowsArgs {
  int64_t qs_b, qs_h, qs_l;     // element strides of q / k / v (and dq / dk / dv)
  int64_t os_b, os_h, os_l;     // element strides of o (and dO)
  int nheads, H, L, Dh;
  float scale, drop_p;
  uint64_t seed, offset;
  int win_ws, win_nwy, win_nwx;   // > 0: "batch" b is window (image, wy, wx) of a [image][nwy*ws][nwx*ws] token grid, row l its token (l / ws, l % ws)
};
// Base offsets of (batch b, head h), the token offset of the lane's row and the stepping of the wave-uniform walk over the other
// rows (token offset t: ++t, and + wrap after every ws-th row).  Window mode reads / writes the tokens where they sit in the
// image-major activation: window partition / reverse are this index arithmetic, not copies (timm davit.py window_partition / window_reverse).
__device__ __forceinline__ void rows_geom(const AttnRowsArgs& p, int b, int h, int row, int64_t& qbase, int64_t& obase, int& lrow,
                                          int& ws, int& wrap) {
  if (p.win_ws > 0) {
    const int nw = p.win_nwy * p.win_nwx, img = b / nw, w = b - img * nw, wy = w / p.win_nwx, wx = w - wy * p.win_nwx;
    const int Wimg = p.win_nwx * p.win_ws;
    const int64_t t0 = ((int64_t)img * (p.win_nwy * p.win_ws) + wy * p.win_ws) * Wimg + wx * p.win_ws;
    qbase = t0 * p.qs_l + h * p.qs_h; obase = t0 * p.os_l + h * p.os_h;
    lrow = (row / p.win_ws) * Wimg + row % p.win_ws;
    ws = p.win_ws; wrap = Wimg - p.win_ws;
  } else {
    qbase = b * p.qs_b + h * p.qs_h; obase = b * p.os_b + h * p.os_h;
    lrow = row; ws = 0x7fffffff; wrap = 0;
  }
}
#define ROWS_STEP(t, x) do { ++t; if (++x == g_ws) { x = 0; t += g_wrap; } } while (0)

// (pointers are separate __restrict__ kernel parameters, not struct members: the no-alias guarantee is what lets the compiler turn
// the wave-uniform key / value reads into scalar loads.  The loops over the OTHER token are rolled -- unrolled, the scheduler hoists
// every row's s_load and spills 2 000 SGPRs -- so a lane's score row lives in a wave-private LDS column, one ds op per 32 FMAs.)
template <int DH>
__global__ __launch_bounds__(256) void attention_rows_fwd_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                                 const float* __restrict__ gv, float* __restrict__ gout,
                                                                 float* __restrict__ glse, const AttnRowsArgs p) {
  extern __shared__ float rows_lds[];                        // per wave: S [L][64]
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int head = blockIdx.x * 4 + wave;                    // wave-uniform
  if (head >= p.nheads) return;
  const int lane = threadIdx.x & 63;
  const int L = p.L;
  float* Ss = rows_lds + (size_t)wave * L * 64 + lane;
  const int b = head / p.H, h = head - b * p.H;
  const bool act = lane < L;
  const int row = act ? lane : 0;                            // idle lanes shadow row 0; nothing of theirs is stored
  int64_t qbase, obase;
  int lrow, g_ws, g_wrap;
  rows_geom(p, b, h, row, qbase, obase, lrow, g_ws, g_wrap);
  g_ws = __builtin_amdgcn_readfirstlane(g_ws); g_wrap = __builtin_amdgcn_readfirstlane(g_wrap);
  const float* __restrict__ qrow = gq + qbase + lrow * p.qs_l;
  const float* __restrict__ kb = gk + qbase;
  const float* __restrict__ vb = gv + qbase;
  float qv[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(qrow + d);
    qv[d] = t.x * p.scale; qv[d + 1] = t.y * p.scale; qv[d + 2] = t.z * p.scale; qv[d + 3] = t.w * p.scale;
  }
  float mx = -INFINITY;
  int jt = 0, jx = 0;
#pragma unroll 1
  for (int j = 0; j < L; ++j) {
    const float* __restrict__ kr = kb + jt * p.qs_l;         // uniform address: scalar loads
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) a = fmaf(qv[d], kr[d], a);
    Ss[j * 64] = a;
    mx = fmaxf(mx, a);
    ROWS_STEP(jt, jx);
  }
  const float keep_scale = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const AttnDropKey dkey = attn_drop_key(p.seed, p.offset, p.drop_p);
  float ov[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) ov[d] = 0.f;
  float sum = 0.f;
  jt = 0; jx = 0;
#pragma unroll 1
  for (int j = 0; j < L; ++j) {
    const float* __restrict__ vr = vb + jt * p.qs_l;
    float e = expf(Ss[j * 64] - mx);
    sum += e;                                                // the softmax denominator counts dropped probabilities too
    if (p.drop_p > 0.f) e = attn_keep(dkey, attn_row_base((uint64_t)head * L + row, (L + 1) >> 1), j) ? e * keep_scale : 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) ov[d] = fmaf(e, vr[d], ov[d]);
    ROWS_STEP(jt, jx);
  }
  const float inv = 1.f / sum;
  if (act) {
    if (glse) glse[(int64_t)head * L + lane] = mx + logf(sum);
    float* __restrict__ orow = gout + obase + lrow * p.os_l;
#pragma unroll
    for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(orow + d) = make_float4(ov[d] * inv, ov[d + 1] * inv, ov[d + 2] * inv, ov[d + 3] * inv);
  }
}

template <int DH>
__global__ __launch_bounds__(256) void attention_rows_bwd_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                                 const float* __restrict__ gv, const float* __restrict__ go,
                                                                 const float* __restrict__ gdO, const float* __restrict__ glse,
                                                                 float* __restrict__ gdq, float* __restrict__ gdk,
                                                                 float* __restrict__ gdv, const AttnRowsArgs p) {
  extern __shared__ float rows_lds[];                        // per wave: dS [L][L+1] | P' [L][L+1]
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int head = blockIdx.x * 4 + wave;
  if (head >= p.nheads) return;
  const int lane = threadIdx.x & 63;
  const int L = p.L, LP = L + 1;
  float* dSs = rows_lds + (size_t)wave * 2 * L * LP;
  float* Pps = dSs + L * LP;
  const int b = head / p.H, h = head - b * p.H;
  const bool act = lane < L;
  const int row = act ? lane : 0;
  int64_t qbase, obase;
  int lrow, g_ws, g_wrap;
  rows_geom(p, b, h, row, qbase, obase, lrow, g_ws, g_wrap);
  g_ws = __builtin_amdgcn_readfirstlane(g_ws); g_wrap = __builtin_amdgcn_readfirstlane(g_wrap);
  const float* __restrict__ qb = gq + qbase;
  const float* __restrict__ kb = gk + qbase;
  const float* __restrict__ vb = gv + qbase;
  const float* __restrict__ dob = gdO + obase;
  {
    // ---- phase A: lane i = query row i.  p_ij from the saved row log-sum-exp, dP'_ij = dO_i . v_j, delta_i = dO_i . o_i,
    // dS_ij = p_ij (f_ij dP'_ij - delta_i) scale  (f = dropout factor);  dq_i = sum_j dS_ij k_j
    const float* __restrict__ qrow = qb + lrow * p.qs_l;
    const float* __restrict__ dorow = dob + lrow * p.os_l;
    const float* __restrict__ orow = go + obase + lrow * p.os_l;
    float qv[DH], gvv[DH], acc[DH];
    float delta = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(qrow + d);
      qv[d] = t.x * p.scale; qv[d + 1] = t.y * p.scale; qv[d + 2] = t.z * p.scale; qv[d + 3] = t.w * p.scale;
      const float4 u = *reinterpret_cast<const float4*>(dorow + d);
      gvv[d] = u.x; gvv[d + 1] = u.y; gvv[d + 2] = u.z; gvv[d + 3] = u.w;
      const float4 w = *reinterpret_cast<const float4*>(orow + d);
      delta = fmaf(u.x, w.x, fmaf(u.y, w.y, fmaf(u.z, w.z, fmaf(u.w, w.w, delta))));
      acc[d] = 0.f; acc[d + 1] = 0.f; acc[d + 2] = 0.f; acc[d + 3] = 0.f;
    }
    const float lse = glse[(int64_t)head * L + row];
    const float keep_scale = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
    const AttnDropKey dkey = attn_drop_key(p.seed, p.offset, p.drop_p);
    int jt = 0, jx = 0;
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      const float* __restrict__ kr = kb + jt * p.qs_l;
      const float* __restrict__ vr = vb + jt * p.qs_l;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) { a = fmaf(qv[d], kr[d], a); c = fmaf(gvv[d], vr[d], c); }
      const float pj = expf(a - lse);
      float f = 1.f;
      if (p.drop_p > 0.f) f = attn_keep(dkey, attn_row_base((uint64_t)head * L + row, (L + 1) >> 1), j) ? keep_scale : 0.f;
      const float ds = pj * (f * c - delta) * p.scale;
      if (act) { dSs[lane * LP + j] = ds; Pps[lane * LP + j] = pj * f; }
#pragma unroll
      for (int d = 0; d < DH; ++d) acc[d] = fmaf(ds, kr[d], acc[d]);
      ROWS_STEP(jt, jx);
    }
    if (act) {
      float* __restrict__ dqrow = gdq + qbase + lrow * p.qs_l;
#pragma unroll
      for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(dqrow + d) = make_float4(acc[d], acc[d + 1], acc[d + 2], acc[d + 3]);
    }
  }
  // ---- phase B: lane j = key row j.  dk_j = sum_i dS_ij q_i, dv_j = sum_i P'_ij dO_i  (columns of the wave's LDS tiles)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float ak[DH], av[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) { ak[d] = 0.f; av[d] = 0.f; }
  int it = 0, ix = 0;
#pragma unroll 1
  for (int i = 0; i < L; ++i) {
    const float dsi = dSs[i * LP + row], ppi = Pps[i * LP + row];
    const float* __restrict__ qr = qb + it * p.qs_l;         // uniform: scalar loads
    const float* __restrict__ gr = dob + it * p.os_l;
#pragma unroll
    for (int d = 0; d < DH; ++d) { ak[d] = fmaf(dsi, qr[d], ak[d]); av[d] = fmaf(ppi, gr[d], av[d]); }
    ROWS_STEP(it, ix);
  }
  if (act) {
    float* __restrict__ dkrow = gdk + qbase + lrow * p.qs_l;
    float* __restrict__ dvrow = gdv + qbase + lrow * p.qs_l;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      *reinterpret_cast<float4*>(dkrow + d) = make_float4(ak[d], ak[d + 1], ak[d + 2], ak[d + 3]);
      *reinterpret_cast<float4*>(dvrow + d) = make_float4(av[d], av[d + 1], av[d + 2], av[d + 3]);
    }
  }
}

// ------------------------------------------------------------------ MD-Net fusion (multimodalMDNet.py:7-55,88-101)
// pooled[n][c] = mean_hw( sigmoid(z[n][c]) * f + sigmoid(tanh(f * t1[n][c]) + t2[n][c]) ),  f = feat[n][c][hw]:
// MetaNet channel gate + spatial MetaBlock + element-wise sum + global average pool in one pass over the
// feature map (NCHW fp32); one 64-lane wave per (n, c) plane.
__global__ __launch_bounds__(256) void mdnet_fuse_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ z,
                                                             const float* __restrict__ t1, const float* __restrict__ t2,
                                                             float* __restrict__ pooled, int64_t NC, int HW) {
  const int64_t nc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (nc >= NC) return;
  const int lane = threadIdx.x & 63;
  const float g = 1.f / (1.f + expf(-z[nc])), a = t1[nc], b = t2[nc];
  float s = 0.f;
  for (int i = lane; i < HW; i += 64) {
    float f = feat[nc * HW + i];
    s += g * f + 1.f / (1.f + expf(-(tanhf(f * a) + b)));
  }
  s = wave_sum(s);
  if (lane == 0) pooled[nc] = s / (float)HW;
}
__global__ __launch_bounds__(256) void mdnet_fuse_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ feat,
                                                             const float* __restrict__ z, const float* __restrict__ t1,
                                                             const float* __restrict__ t2, float* __restrict__ dfeat,
                                                             float* __restrict__ dz, float* __restrict__ dt1,
                                                             float* __restrict__ dt2, int64_t NC, int HW) {
  const int64_t nc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (nc >= NC) return;
  const int lane = threadIdx.x & 63;
  const float g = 1.f / (1.f + expf(-z[nc])), a = t1[nc], b = t2[nc];
  const float dp = dpooled[nc] / (float)HW;
  float sf = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < HW; i += 64) {
    float f = feat[nc * HW + i];
    float u = tanhf(f * a);
    float o = 1.f / (1.f + expf(-(u + b)));
    float ds = dp * o * (1.f - o);        // d/d(u + b)
    float du = ds * (1.f - u * u);        // d/d(f * a)
    if (dfeat) dfeat[nc * HW + i] = dp * g + du * a;
    sf += f; s1 += du * f; s2 += ds;
  }
  sf = wave_sum(sf); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (lane == 0) {
    dz[nc] = dp * sf * g * (1.f - g);
    dt1[nc] = s1;
    dt2[nc] = s2;
  }
}

// ------------------------------------------------------------------ embedding
__global__ void embedding_fwd_kernel(const float* table, const int64_t* ids, float* out, int B, int ncols, int card, int E) {
  EW_LOOP((int64_t)B * ncols * E) {
    int e = (int)(i % E);
    int64_t t = i / E;
    int col = (int)(t % ncols);
    int64_t id = ids[t];
    if (id < 0) id = 0;
    if (id >= card) id = card - 1;
    out[i] = table[((int64_t)col * card + id) * E + e];
  }
}
__global__ void embedding_bwd_kernel(const float* dout, const int64_t* ids, float* dtable, int B, int ncols, int card, int E) {
  EW_LOOP((int64_t)ncols * card * E) {  // deterministic: each table element sums its own batch rows
    int e = (int)(i % E);
    int64_t t = i / E;
    int id = (int)(t % card), col = (int)(t / card);
    float s = 0.f;
    for (int bb = 0; bb < B; ++bb) {
      int64_t v = ids[(int64_t)bb * ncols + col];   // clamped as the forward clamps it: the row that was read gets the gradient
      if (v < 0) v = 0;
      if (v >= card) v = card - 1;
      if (v == id) s += dout[((int64_t)bb * ncols + col) * E + e];
    }
    dtable[i] = s;
  }
}

// ------------------------------------------------------------------ custom-cnn direct kernels (NCHW)
__global__ void direct_conv_fwd_kernel(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H,
                                       int W, int Cout, int kh, int kw, int stride, int pad, int OH, int OW, int relu) {
  EW_LOOP((int64_t)N * Cout * OH * OW) {
    int ow = (int)(i % OW);
    int64_t t = i / OW;
    int oh = (int)(t % OH); t /= OH;
    int co = (int)(t % Cout);
    int n = (int)(t / Cout);
    float s = b ? b[co] : 0.f;
    for (int c = 0; c < Cin; ++c)
      for (int r = 0; r < kh; ++r) {
        int h = oh * stride - pad + r;
        if ((unsigned)h >= (unsigned)H) continue;
        for (int q = 0; q < kw; ++q) {
          int ww = ow * stride - pad + q;
          if ((unsigned)ww >= (unsigned)W) continue;
          s += x[(((int64_t)n * Cin + c) * H + h) * W + ww] * w[((co * Cin + c) * kh + r) * kw + q];
        }
      }
    if (relu) s = fmaxf(s, 0.f);
    y[i] = s;
  }
}
// one workgroup per weight element (and one per bias): block-wide reduction over (n, oh, ow)
__global__ __launch_bounds__(256) void direct_conv_bwd_kernel(const float* dy, const float* x, const float* y_relu,
                                                              float* dw, float* db, int N, int Cin, int H, int W,
                                                              int Cout, int kh, int kw, int stride, int pad, int OH,
                                                              int OW) {
  __shared__ float red[4];
  const int nw = Cout * Cin * kh * kw;
  const int id = blockIdx.x;
  const bool is_bias = id >= nw;
  int co, c = 0, r = 0, q = 0;
  if (is_bias) co = id - nw;
  else { q = id % kw; int t = id / kw; r = t % kh; t /= kh; c = t % Cin; co = t / Cin; }
  float s = 0.f;
  const int64_t total = (int64_t)N * OH * OW;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    int ow = (int)(i % OW);
    int64_t t = i / OW;
    int oh = (int)(t % OH);
    int n = (int)(t / OH);
    int64_t yo = (((int64_t)n * Cout + co) * OH + oh) * OW + ow;
    float d = dy[yo];
    if (y_relu && !(y_relu[yo] > 0.f)) d = 0.f;
    if (is_bias) s += d;
    else {
      int h = oh * stride - pad + r, ww = ow * stride - pad + q;
      if ((unsigned)h < (unsigned)H && (unsigned)ww < (unsigned)W) s += d * x[(((int64_t)n * Cin + c) * H + h) * W + ww];
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = red[0] + red[1] + red[2] + red[3];
    if (is_bias) { if (db) db[co] = tot; } else dw[id] = tot;
  }
}
__global__ __launch_bounds__(64) void pool_gap_fwd_kernel(const float* x, float* y, int32_t* idx, int C, int H, int W,
                                                          int k, int PH, int PW) {
  const int nc = blockIdx.x;  // n*C + c
  const float* xp = x + (int64_t)nc * H * W;
  float s = 0.f;
  for (int pi = threadIdx.x; pi < PH * PW; pi += 64) {
    int ph = pi / PW, pw = pi - ph * PW;
    float best = -INFINITY;
    int bi = (ph * k) * W + pw * k;
    for (int r = 0; r < k; ++r)
      for (int q = 0; q < k; ++q) {
        int h = ph * k + r, w = pw * k + q;
        float v = xp[h * W + w];
        if (v > best || v != v) { best = v; bi = h * W + w; }
      }
    idx[(int64_t)nc * PH * PW + pi] = bi;
    s += best;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) y[nc] = s / (float)(PH * PW);
}
__global__ void pool_gap_bwd_kernel(const float* dy, const int32_t* idx, float* dx, int64_t NC, int HW, int PHW) {
  EW_LOOP(NC * PHW) {
    int64_t nc = i / PHW;
    dx[nc * HW + idx[i]] = dy[nc] / (float)PHW;
  }
}

// ------------------------------------------------------------------ row softmax / GELU (BERT-style encoder layers)
// y[r][j] = softmax_j(x[r][j] * scale + mask_add[b][j]), b = r / rows_per_batch; one wave per row
// bias (optional): [rows_per_batch][L] added to every batch's scores (per-head relative-position bias of BEiT)
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mask_add,
                                                          const float* __restrict__ bias, float* __restrict__ y, int64_t rows,
                                                          int L, int64_t rows_per_batch, float scale, int causal) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + r * L;
  const float* mk = mask_add ? mask_add + (r / rows_per_batch) * L : nullptr;
  const float* bs = bias ? bias + (r % rows_per_batch) * L : nullptr;
  const int jend = causal ? (int)(r % L) + 1 : L;      // causal (GPT-2): query i attends keys 0..i (square score matrices)
  float mx = -INFINITY;
  for (int j = lane; j < jend; j += 64) mx = fmaxf(mx, xr[j] * scale + (mk ? mk[j] : 0.f) + (bs ? bs[j] : 0.f));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < jend; j += 64) sum += expf(xr[j] * scale + (mk ? mk[j] : 0.f) + (bs ? bs[j] : 0.f) - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int j = lane; j < L; j += 64)
    y[r * L + j] = j < jend ? expf(xr[j] * scale + (mk ? mk[j] : 0.f) + (bs ? bs[j] : 0.f) - mx) * inv : 0.f;
}
// y = x + gamma[c] * b  (LayerScale residual), and its pieces backward
__global__ void scale_add_fwd_kernel(const float* __restrict__ x, const float* __restrict__ b, const float* __restrict__ gamma,
                                     float* __restrict__ y, int64_t n, int C) {
  EW_LOOP(n) y[i] = x[i] + gamma[i % C] * b[i];
}
__global__ void scale_mul_kernel(const float* __restrict__ dy, const float* __restrict__ v, float* __restrict__ out, int64_t n, int C,
                                 int per_channel) {
  EW_LOOP(n) out[i] = dy[i] * (per_channel ? v[i % C] : v[i]);
}
// out[b][e] = mean over tokens [start, L) of x[b][t][e]; backward spreads dout / (L - start)
__global__ void token_mean_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int L, int E, int start) {
  EW_LOOP((int64_t)B * E) {
    const int e = (int)(i % E); const int64_t b = i / E;
    float s2 = 0.f;
    for (int t = start; t < L; ++t) s2 += x[(b * L + t) * E + e];
    out[i] = s2 / (float)(L - start);
  }
}
__global__ void token_mean_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dx, int B, int L, int E, int start) {
  EW_LOOP((int64_t)B * L * E) {
    const int e = (int)(i % E); const int64_t t2 = i / E;
    const int t = (int)(t2 % L); const int64_t b = t2 / L;
    dx[i] = t >= start ? dout[b * E + e] / (float)(L - start) : 0.f;
  }
}
// dx = (dy - sum_j dy*y) * y * scale
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                          float* __restrict__ dx, int64_t rows, int L, float scale) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float dot = 0.f;
  for (int j = lane; j < L; j += 64) dot += dy[r * L + j] * y[r * L + j];
  dot = wave_sum(dot);
  for (int j = lane; j < L; j += 64) dx[r * L + j] = (dy[r * L + j] - dot) * y[r * L + j] * scale;
}
// GPT-2's "gelu_new": 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))
__global__ void gelu_tanh_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  EW_LOOP(n) { const float v = x[i]; y[i] = 0.5f * v * (1.f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v))); }
}
__global__ void gelu_tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n) {
  EW_LOOP(n) {
    const float v = x[i];
    const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
    const float t = tanhf(u);
    const float du = 0.7978845608028654f * (1.f + 3.f * 0.044715f * v * v);
    dx[i] = dy[i] * (0.5f * (1.f + t) + 0.5f * v * (1.f - t * t) * du);
  }
}
__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, int64_t n, int64_t nb) {
  EW_LOOP(n) y[i] = a[i] + b[i % nb];   // b broadcasts over the leading dimension when nb < n
}
__global__ void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  EW_LOOP(n) y[i] = 0.5f * x[i] * (1.f + erff(x[i] * 0.70710678118654752f));
}
__global__ void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n) {
  EW_LOOP(n) {
    const float v = x[i];
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * v * v);
    dx[i] = dy[i] * (cdf + v * pdf);
  }
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

int mmskin_layernorm_forward(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd,
                             int M, int N, float eps, int relu, void* stream) {
  ARG_CHECK(x && g && y && mean && rstd && M > 0 && N > 0, "layernorm_forward: bad argument");
  if (ln_rows_ok(N, relu)) {
#define CALL(NJ, LPR) hipLaunchKernelGGL((layernorm_fwd_rows_kernel<NJ, LPR>), dim3(ceil_div(M, 4 * (64 / LPR))), dim3(256), 0, ST(stream), x, g, b, y, (bf16_t*)nullptr, mean, rstd, M, N, eps)
    LN_ROWS_DISPATCH(N, CALL);
#undef CALL
  } else {
    hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, ST(stream), x, g, b, y, mean, rstd, M, N, eps, relu);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_layernorm_forward_mixed(const float* x, const float* g, const float* b, float* y_f32, void* y_bf16, int M, int N,
                                   float eps, void* stream) {
  ARG_CHECK(x && g && (y_f32 || y_bf16) && M > 0 && N > 0, "layernorm_forward_mixed: bad argument");
  ARG_CHECK(N % 4 == 0 && N <= 2048, "layernorm_forward_mixed: N=%d (needs N %% 4 == 0 and N <= 2048)", N);
#define CALL(NJ, LPR) hipLaunchKernelGGL((layernorm_fwd_rows_kernel<NJ, LPR>), dim3(ceil_div(M, 4 * (64 / LPR))), dim3(256), 0, ST(stream), x, g, b, y_f32, reinterpret_cast<bf16_t*>(y_bf16), (float*)nullptr, (float*)nullptr, M, N, eps)
  LN_ROWS_DISPATCH(N, CALL);
#undef CALL
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_layernorm_backward(const float* dy, const float* x, const float* g, const float* b, const float* mean,
                              const float* rstd, float* dx, float* dg, float* db, int M, int N, int relu, void* stream) {
  ARG_CHECK(dy && x && g && mean && rstd && M > 0 && N > 0, "layernorm_backward: bad argument");
  if (!b) db = nullptr;     // a LayerNorm without bias has no bias gradient
  if (ln_rows_ok(N, relu)) {
    // <= 1024 workgroups; every wave keeps >= 8 rows so its column sums amortise the slot it writes
    const int rpw = N <= 128 ? 2 : 1;
    int G = ceil_div(M, 4 * rpw * 8);
    if (G > 1024) G = 1024;
    if (G < 1) G = 1;
    const int R = G;
    float* part = nullptr;
    if (dg || db) {
      part = head_scratch((size_t)R * 2 * N * sizeof(float));
      if (!part) { mmskin_set_error("layernorm_backward: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    }
#define CALL(NJ, LPR) hipLaunchKernelGGL((layernorm_bwd_rows_kernel<NJ, LPR>), dim3(G), dim3(256), 0, ST(stream), dy, x, g, mean, rstd, dx, part, M, N)
    LN_ROWS_DISPATCH(N, CALL);
#undef CALL
    HIP_CHECK_RET(hipGetLastError());
    if (part) return rows_sum(part, R, 2 * N, N, dg, db, ST(stream));
    return MMSKIN_OK;
  }
  if (dx) {
    hipLaunchKernelGGL(layernorm_bwd_dx_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, ST(stream), dy, x, g, b, mean, rstd, dx, M, N, relu);
    HIP_CHECK_RET(hipGetLastError());
  }
  if (dg || db) {
    int G = ceil_div(M, 64);
    if (G > 256) G = 256;
    float* part = head_scratch((size_t)G * 2 * N * sizeof(float));
    if (!part) { mmskin_set_error("layernorm_backward: scratch allocation failed"); return MMSKIN_ERR_HIP; }
    hipLaunchKernelGGL(layernorm_bwd_gb_kernel, dim3(ceil_div(N, 64), G), dim3(256), 0, ST(stream), dy, x, g, b, mean, rstd,
                       part, M, N, relu, ceil_div(M, G));
    hipLaunchKernelGGL(layernorm_gb_reduce_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, ST(stream), part, dg, db, G, N);
    HIP_CHECK_RET(hipGetLastError());
  }
  return MMSKIN_OK;
}

#define EW_LAUNCH(kern, n, ...)                                                                  \
  do {                                                                                           \
    if ((n) > 0) {                                                                               \
      hipLaunchKernelGGL(kern, dim3(grid1d(n)), dim3(256), 0, ST(stream), __VA_ARGS__);          \
      HIP_CHECK_RET(hipGetLastError());                                                          \
    }                                                                                            \
    return MMSKIN_OK;                                                                            \
  } while (0)

int mmskin_sigmoid_gate_forward(const float* z, const float* v, float* out, int64_t n, void* stream) {
  EW_LAUNCH(sigmoid_gate_fwd_kernel, n, z, v, out, n);
}
int mmskin_sigmoid_gate_backward(const float* dout, const float* z, const float* v, float* dz, float* dv, int64_t n, void* stream) {
  EW_LAUNCH(sigmoid_gate_bwd_kernel, n, dout, z, v, dz, dv, n);
}
int mmskin_gated_mix_forward(const float* z, const float* a, const float* q, float* out, int64_t n, void* stream) {
  EW_LAUNCH(gated_mix_fwd_kernel, n, z, a, q, out, n);
}
int mmskin_gated_mix_backward(const float* dout, const float* z, const float* a, const float* q, float* dz, float* da,
                              float* dq, int64_t n, void* stream) {
  EW_LAUNCH(gated_mix_bwd_kernel, n, dout, z, a, q, dz, da, dq, n);
}
int mmskin_metablock_gate_forward(const float* V, const float* t1, const float* t2, float* out, int64_t n, void* stream) {
  EW_LAUNCH(metablock_gate_fwd_kernel, n, V, t1, t2, out, n);
}
int mmskin_metablock_gate_backward(const float* dout, const float* V, const float* t1, const float* t2, float* dV,
                                   float* dt1, float* dt2, int64_t n, void* stream) {
  EW_LAUNCH(metablock_gate_bwd_kernel, n, dout, V, t1, t2, dV, dt1, dt2, n);
}
int mmskin_dropout_forward(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed, uint64_t offset,
                           void* stream) {
  EW_LAUNCH(dropout_fwd_kernel, n, x, y, mask, n, p, seed, offset);
}
int mmskin_attn_dropout_forward(const float* x, float* y, uint8_t* mask, int64_t n, int L, float p, uint64_t seed, uint64_t offset,
                                void* stream) {
  ARG_CHECK(L > 0 && n % L == 0, "attn_dropout_forward: n=%lld is not rows x L=%d", (long long)n, L);
  EW_LAUNCH(attn_dropout_fwd_kernel, n, x, y, mask, n, L, p, seed, offset);
}
// ---- Adam (torch.optim.Adam semantics: L2 weight decay added to the gradient, bias-corrected moments) over ONE flat fp32 range:
// the optimizer step of the reference's training loop (train_pad_20.py:54,113) as a single pass over the backbone's parameter arena
// instead of torch's multi-tensor launches (6 x 49 us for ResNet-50).  16-byte accesses; n % 4 handled by a scalar tail.
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        int64_t n, float step_size, float b1c, float b2, float b2c, float eps, float wd, float inv_bc2_sqrt) {   // b1c = 1 - beta1, b2c = 1 - beta2 (formed in double on the host, like torch's scalars)
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto upd = [&](float& pv, float gv, float& mv, float& vv) {
    gv += wd * pv;
    mv += b1c * (gv - mv);
    vv = b2 * vv + b2c * gv * gv;
    pv -= step_size * mv / (sqrtf(vv) * inv_bc2_sqrt + eps);
  };
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    upd(pv.x, gv.x, mv.x, vv.x); upd(pv.y, gv.y, mv.y, vv.y); upd(pv.z, gv.z, mv.z, vv.z); upd(pv.w, gv.w, mv.w, vv.w);
    reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    upd(p[i], g[i], m[i], v[i]);
  }
}
int mmskin_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int64_t step, void* stream) {
  ARG_CHECK(step >= 1 && n >= 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step: step=%lld / 16-byte alignment", (long long)step);
  if (n == 0) return MMSKIN_OK;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(adam_step_kernel, dim3(grid1d(n / 4)), dim3(256), 0, ST(stream), p, g, m, v, n, (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)(1.0 / sqrt(bc2)));
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_dropout_backward(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream) {
  EW_LAUNCH(dropout_bwd_kernel, n, dy, mask, dx, n, p);
}
int mmskin_concat2_forward(const float* a, const float* b, float* out, int M, int Na, int Nb, void* stream) {
  EW_LAUNCH(concat2_fwd_kernel, (int64_t)M * (Na + Nb), a, b, out, M, Na, Nb);
}
int mmskin_concat2_backward(const float* dout, float* da, float* db, int M, int Na, int Nb, void* stream) {
  EW_LAUNCH(concat2_bwd_kernel, (int64_t)M * (Na + Nb), dout, da, db, M, Na, Nb);
}

int mmskin_attention_forward(const float* q, const float* k, const float* v, float* o, float* p, int B, int H, int L,
                             int Dh, float drop_p, uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(q && k && v && o && p && B > 0 && H > 0 && L > 0 && Dh > 0, "attention_forward: bad argument");
  ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "attention_forward: dropout %f", drop_p);
  ARG_CHECK((size_t)L * L * 4 <= 64 * 1024, "attention_forward: L=%d too long for the small-attention kernel", L);
  hipLaunchKernelGGL(attention_fwd_kernel, dim3(B * H), dim3(256), (size_t)L * L * 4, ST(stream), q, k, v, o, p, L, Dh, drop_p, seed, offset);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* p,
                              float* dq, float* dk, float* dv, int B, int H, int L, int Dh, float drop_p,
                              uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(dO && q && k && v && p && dq && dk && dv, "attention_backward: null argument");
  ARG_CHECK((size_t)L * L * 4 <= 64 * 1024, "attention_backward: L=%d too long", L);
  hipLaunchKernelGGL(attention_bwd_kernel, dim3(B * H), dim3(256), (size_t)L * L * 4, ST(stream), dO, q, k, v, p, dq, dk, dv, L, Dh, drop_p, seed, offset);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// One wave per (batch, head): L <= 64, Dh % 32 == 0; q / k / v (and their gradients) share one set of (batch, head, token) element
// strides, o (and dO) another; lse [B*H][L] carries the row log-sum-exp from forward to backward instead of the probabilities.
static int attn_rows_args(AttnRowsArgs& a, int B, int H, int L, int Dh, const int64_t* qkv_strides, const int64_t* o_strides, float scale,
                          float drop_p, uint64_t seed, uint64_t offset, const char* what) {
  ARG_CHECK(B > 0 && H > 0 && L > 0 && L <= 64 && (Dh == 32 || Dh == 64), "%s: needs L <= 64 and Dh 32 or 64 (L=%d Dh=%d)", what, L, Dh);
  ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "%s: dropout %f", what, (double)drop_p);
  for (int i = 0; i < 3; ++i)
    ARG_CHECK(qkv_strides[i] % 4 == 0 && o_strides[i] % 4 == 0, "%s: strides must keep rows 16-byte aligned", what);
  a.qs_b = qkv_strides[0]; a.qs_h = qkv_strides[1]; a.qs_l = qkv_strides[2];
  a.os_b = o_strides[0]; a.os_h = o_strides[1]; a.os_l = o_strides[2];
  a.nheads = B * H; a.H = H; a.L = L; a.Dh = Dh; a.scale = scale; a.drop_p = drop_p; a.seed = seed; a.offset = offset;
  a.win_ws = 0; a.win_nwy = 0; a.win_nwx = 0;
  return MMSKIN_OK;
}
static int attn_rows_fwd_launch(const float* q, const float* k, const float* v, float* o, float* lse, const AttnRowsArgs& a, void* stream) {
  const size_t lds = (size_t)4 * a.L * 64 * sizeof(float);
  if (a.Dh == 32) hipLaunchKernelGGL(attention_rows_fwd_kernel<32>, dim3((a.nheads + 3) / 4), dim3(256), lds, ST(stream), q, k, v, o, lse, a);
  else hipLaunchKernelGGL(attention_rows_fwd_kernel<64>, dim3((a.nheads + 3) / 4), dim3(256), lds, ST(stream), q, k, v, o, lse, a);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
static int attn_rows_bwd_launch(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                                float* dq, float* dk, float* dv, const AttnRowsArgs& a, void* stream) {
  const size_t lds = (size_t)4 * 2 * a.L * (a.L + 1) * sizeof(float);
  // up to 4 waves x 2 tiles x 64 x 65 floats
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(attention_rows_bwd_kernel<32>), 4 * 2 * 64 * 65 * 4));
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(attention_rows_bwd_kernel<64>), 4 * 2 * 64 * 65 * 4));
  if (a.Dh == 32) hipLaunchKernelGGL(attention_rows_bwd_kernel<32>, dim3((a.nheads + 3) / 4), dim3(256), lds, ST(stream), q, k, v, o, dO, lse, dq, dk, dv, a);
  else hipLaunchKernelGGL(attention_rows_bwd_kernel<64>, dim3((a.nheads + 3) / 4), dim3(256), lds, ST(stream), q, k, v, o, dO, lse, dq, dk, dv, a);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
// Window attention on an image-major token grid [B][nwy*ws][nwx*ws] (DaViT SpatialBlock, timm davit.py:window_partition /
// window_reverse around WindowAttention): window (image, wy, wx) attends over its ws*ws tokens where they sit -- no partition /
// reverse copies.  token_stride / head_stride: element strides of q / k / v (and dq / dk / dv) and of o (and dO); lse is
// [B*nwy*nwx][H][ws*ws] (private to the forward / backward pair).
static int attn_window_args(AttnRowsArgs& a, int B, int nwy, int nwx, int ws, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok,
                            int64_t o_head, float scale, float drop_p, uint64_t seed, uint64_t offset, const char* what) {
  ARG_CHECK(B > 0 && nwy > 0 && nwx > 0 && ws > 0 && ws * ws <= 64, "%s: needs ws*ws <= 64 (ws=%d)", what, ws);
  ARG_CHECK((int64_t)B * nwy * nwx * H < (int64_t)1 << 30, "%s: too many windows", what);
  const int64_t qs[3] = {0, q_head, q_tok}, os[3] = {0, o_head, o_tok};
  int rc = attn_rows_args(a, B * nwy * nwx, H, ws * ws, Dh, qs, os, scale, drop_p, seed, offset, what);
  if (rc) return rc;
  a.win_ws = ws; a.win_nwy = nwy; a.win_nwx = nwx;
  return MMSKIN_OK;
}
int mmskin_window_attention_forward(const float* q, const float* k, const float* v, float* o, float* lse, int B, int nwy, int nwx, int ws,
                                    int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head, float scale,
                                    float drop_p, uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(q && k && v && o, "window_attention_forward: null argument");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "window_attention_forward: 16-byte aligned tensors required");
  AttnRowsArgs a;
  int rc = attn_window_args(a, B, nwy, nwx, ws, H, Dh, q_tok, q_head, o_tok, o_head, scale, drop_p, seed, offset, "window_attention_forward");
  if (rc) return rc;
  return attn_rows_fwd_launch(q, k, v, o, lse, a, stream);
}
int mmskin_window_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                                     float* dq, float* dk, float* dv, int B, int nwy, int nwx, int ws, int H, int Dh, int64_t q_tok,
                                     int64_t q_head, int64_t o_tok, int64_t o_head, float scale, float drop_p, uint64_t seed,
                                     uint64_t offset, void* stream) {
  ARG_CHECK(dO && q && k && v && o && lse && dq && dk && dv, "window_attention_backward: null argument");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) == 0,
            "window_attention_backward: 16-byte aligned tensors required");
  AttnRowsArgs a;
  int rc = attn_window_args(a, B, nwy, nwx, ws, H, Dh, q_tok, q_head, o_tok, o_head, scale, drop_p, seed, offset, "window_attention_backward");
  if (rc) return rc;
  return attn_rows_bwd_launch(dO, q, k, v, o, lse, dq, dk, dv, a, stream);
}
int mmskin_attention_rows_forward(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int L, int Dh,
                                  const int64_t* qkv_strides, const int64_t* o_strides, float scale, float drop_p, uint64_t seed,
                                  uint64_t offset, void* stream) {
  ARG_CHECK(q && k && v && o && qkv_strides && o_strides, "attention_rows_forward: null argument");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "attention_rows_forward: 16-byte aligned tensors required");
  AttnRowsArgs a;
  int rc = attn_rows_args(a, B, H, L, Dh, qkv_strides, o_strides, scale, drop_p, seed, offset, "attention_rows_forward");
  if (rc) return rc;
  return attn_rows_fwd_launch(q, k, v, o, lse, a, stream);
}
int mmskin_attention_rows_backward(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                                   float* dq, float* dk, float* dv, int B, int H, int L, int Dh, const int64_t* qkv_strides,
                                   const int64_t* o_strides, float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(dO && q && k && v && o && lse && dq && dk && dv && qkv_strides && o_strides, "attention_rows_backward: null argument");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) == 0,
            "attention_rows_backward: 16-byte aligned tensors required");
  AttnRowsArgs a;
  int rc = attn_rows_args(a, B, H, L, Dh, qkv_strides, o_strides, scale, drop_p, seed, offset, "attention_rows_backward");
  if (rc) return rc;
  return attn_rows_bwd_launch(dO, q, k, v, o, lse, dq, dk, dv, a, stream);
}

int mmskin_mdnet_fuse_forward(const float* feat, const float* z, const float* t1, const float* t2, float* pooled,
                              int64_t NC, int HW, void* stream) {
  ARG_CHECK(feat && z && t1 && t2 && pooled && NC > 0 && HW > 0, "mdnet_fuse_forward: bad argument");
  hipLaunchKernelGGL(mdnet_fuse_fwd_kernel, dim3((unsigned)((NC + 3) / 4)), dim3(256), 0, ST(stream), feat, z, t1, t2, pooled, NC, HW);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_mdnet_fuse_backward(const float* dpooled, const float* feat, const float* z, const float* t1, const float* t2,
                               float* dfeat, float* dz, float* dt1, float* dt2, int64_t NC, int HW, void* stream) {
  ARG_CHECK(dpooled && feat && z && t1 && t2 && dz && dt1 && dt2 && NC > 0 && HW > 0, "mdnet_fuse_backward: bad argument");
  hipLaunchKernelGGL(mdnet_fuse_bwd_kernel, dim3((unsigned)((NC + 3) / 4)), dim3(256), 0, ST(stream), dpooled, feat, z, t1, t2,
                     dfeat, dz, dt1, dt2, NC, HW);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int mmskin_softmax_forward(const float* x, const float* mask_add, const float* bias, float* y, int64_t rows, int L,
                           int64_t rows_per_batch, float scale, int causal, void* stream) {
  ARG_CHECK(x && y && rows > 0 && L > 0 && rows_per_batch > 0, "softmax_forward: bad argument");
  hipLaunchKernelGGL(softmax_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ST(stream), x, mask_add, bias, y, rows, L,
                     rows_per_batch, scale, causal);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_softmax_backward(const float* dy, const float* y, float* dx, int64_t rows, int L, float scale, void* stream) {
  ARG_CHECK(dy && y && dx && rows > 0 && L > 0, "softmax_backward: bad argument");
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ST(stream), dy, y, dx, rows, L, scale);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_scale_add_forward(const float* x, const float* b, const float* gamma, float* y, int64_t n, int C, void* stream) {
  ARG_CHECK(x && b && gamma && y && n > 0 && C > 0, "scale_add_forward: bad argument");
  EW_LAUNCH(scale_add_fwd_kernel, n, x, b, gamma, y, n, C);
}
/* out = dy * v, v per channel (per_channel = 1: v[C]) or elementwise (v[n]) */
int mmskin_scale_mul(const float* dy, const float* v, float* out, int64_t n, int C, int per_channel, void* stream) {
  ARG_CHECK(dy && v && out && n > 0 && C > 0, "scale_mul: bad argument");
  EW_LAUNCH(scale_mul_kernel, n, dy, v, out, n, C, per_channel);
}
int mmskin_token_mean_forward(const float* x, float* out, int B, int L, int E, int start, void* stream) {
  ARG_CHECK(x && out && B > 0 && L > start && E > 0, "token_mean_forward: bad argument");
  EW_LAUNCH(token_mean_fwd_kernel, (int64_t)B * E, x, out, B, L, E, start);
}
int mmskin_token_mean_backward(const float* dout, float* dx, int B, int L, int E, int start, void* stream) {
  ARG_CHECK(dout && dx && B > 0 && L > start && E > 0, "token_mean_backward: bad argument");
  EW_LAUNCH(token_mean_bwd_kernel, (int64_t)B * L * E, dout, dx, B, L, E, start);
}
int mmskin_add(const float* a, const float* b, float* y, int64_t n, int64_t nb, void* stream) {
  ARG_CHECK(a && b && y && n > 0 && nb > 0 && n % nb == 0, "add: bad argument");
  EW_LAUNCH(add_kernel, n, a, b, y, n, nb);
}
int mmskin_gelu_forward(const float* x, float* y, int64_t n, void* stream) { EW_LAUNCH(gelu_fwd_kernel, n, x, y, n); }
int mmskin_gelu_tanh_forward(const float* x, float* y, int64_t n, void* stream) { EW_LAUNCH(gelu_tanh_fwd_kernel, n, x, y, n); }
int mmskin_gelu_tanh_backward(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
  EW_LAUNCH(gelu_tanh_bwd_kernel, n, dy, x, dx, n);
}
// StarReLU (timm metaformer.py): y = s relu(z)^2 + b with learnable scalars s, b (device pointers).  Backward: dz = dy 2 s relu(z) and
// dsb[0..1] = (sum dy relu(z)^2, sum dy) -- per-block partials over a grid fixed by n, then one block adds them in a fixed order.
__global__ void star_relu_fwd_kernel(const float* __restrict__ z, const float* __restrict__ sp, const float* __restrict__ bp,
                                     float* __restrict__ y, int64_t n) {
  const float s = sp[0], b = bp[0];
  EW_LOOP(n) { const float r = fmaxf(z[i], 0.f); y[i] = s * (r * r) + b; }
}
constexpr int STAR_EW_BLOCKS = 1024;
__global__ __launch_bounds__(256) void star_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ sp,
                                                            float* __restrict__ dz, float* __restrict__ part, int64_t n) {
  __shared__ float red[2][4];
  const float s2 = 2.f * sp[0];
  float as = 0.f, ab = 0.f;
  EW_LOOP(n) {
    const float g = dy[i], r = fmaxf(z[i], 0.f);
    as += g * r * r; ab += g;
    if (dz) dz[i] = g * s2 * r;
  }
  as = wave_sum(as); ab = wave_sum(ab);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = as; red[1][threadIdx.x >> 6] = ab; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    part[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}
int mmskin_star_relu_forward(const float* z, const float* s, const float* b, float* y, int64_t n, void* stream) {
  ARG_CHECK(z && s && b && y && n > 0, "star_relu_forward: bad argument");
  EW_LAUNCH(star_relu_fwd_kernel, n, z, s, b, y, n);
}
int mmskin_star_relu_backward(const float* dy, const float* z, const float* s, float* dz, float* dsb, int64_t n, void* stream) {
  ARG_CHECK(dy && z && s && dsb && n > 0, "star_relu_backward: bad argument");
  int64_t nb = (n + 255) / 256;
  if (nb > STAR_EW_BLOCKS) nb = STAR_EW_BLOCKS;
  float* part = head_scratch((size_t)2 * nb * sizeof(float));
  if (!part) { mmskin_set_error("star_relu_backward: scratch allocation failed"); return MMSKIN_ERR_HIP; }
  hipLaunchKernelGGL(star_relu_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, ST(stream), dy, z, s, dz, part, n);
  HIP_CHECK_RET(hipGetLastError());
  return star_pair_sum(part, (int)nb, dsb, ST(stream));
}
int mmskin_gelu_backward(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
  EW_LAUNCH(gelu_bwd_kernel, n, dy, x, dx, n);
}

int mmskin_embedding_forward(const float* table, const int64_t* ids, float* out, int B, int ncols, int card, int E,
                             void* stream) {
  EW_LAUNCH(embedding_fwd_kernel, (int64_t)B * ncols * E, table, ids, out, B, ncols, card, E);
}
int mmskin_embedding_backward(const float* dout, const int64_t* ids, float* dtable, int B, int ncols, int card, int E,
                              void* stream) {
  EW_LAUNCH(embedding_bwd_kernel, (int64_t)ncols * card * E, dout, ids, dtable, B, ncols, card, E);
}

int mmskin_direct_conv2d_forward(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H, int W,
                                 int Cout, int kh, int kw, int stride, int pad, int relu, void* stream) {
  int OH = (H + 2 * pad - kh) / stride + 1, OW = (W + 2 * pad - kw) / stride + 1;
  EW_LAUNCH(direct_conv_fwd_kernel, (int64_t)N * Cout * OH * OW, x, w, b, y, N, Cin, H, W, Cout, kh, kw, stride, pad, OH, OW, relu);
}
int mmskin_direct_conv2d_backward(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int N,
                                  int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, void* stream) {
  ARG_CHECK(dy && x && dw, "direct_conv2d_backward: null argument");
  int OH = (H + 2 * pad - kh) / stride + 1, OW = (W + 2 * pad - kw) / stride + 1;
  int blocks = Cout * Cin * kh * kw + (db ? Cout : 0);
  hipLaunchKernelGGL(direct_conv_bwd_kernel, dim3(blocks), dim3(256), 0, ST(stream), dy, x, y_relu, dw, db, N, Cin, H, W,
                     Cout, kh, kw, stride, pad, OH, OW);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_pool_gap_forward(const float* x, float* y, int32_t* idx, int N, int C, int H, int W, int k, void* stream) {
  ARG_CHECK(x && y && idx && k > 0 && H >= k && W >= k, "pool_gap_forward: bad argument");
  hipLaunchKernelGGL(pool_gap_fwd_kernel, dim3(N * C), dim3(64), 0, ST(stream), x, y, idx, C, H, W, k, H / k, W / k);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
int mmskin_pool_gap_backward(const float* dy, const int32_t* idx, float* dx, int N, int C, int H, int W, int k,
                             void* stream) {
  ARG_CHECK(dy && idx && dx, "pool_gap_backward: null argument");
  HIP_CHECK_RET(hipMemsetAsync(dx, 0, (size_t)N * C * H * W * sizeof(float), ST(stream)));
  int64_t NC = (int64_t)N * C;
  int PHW = (H / k) * (W / k);
  EW_LAUNCH(pool_gap_bwd_kernel, NC * PHW, dy, idx, dx, NC, H * W, PHW);
}

}  // extern "C"
