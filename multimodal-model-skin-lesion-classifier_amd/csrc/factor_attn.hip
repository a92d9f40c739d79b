// Factorized attention with convolutional relative position encoding (timm coat.py FactorAttnConvRelPosEnc + ConvRelPosEnc) and the
// class-token-aware convolutional position encoding (coat.py ConvPosEnc) of the CoaT-Lite encoders, gfx950, fp32, forward and backward,
// on the TOKEN-MAJOR packed qkv [B, N, 3, 8, Ch] a fused qkv Linear writes; the output [B, N, 8 * Ch] is what the projection reads.
// No permute / contiguous copies on either side (the rule of channel_attn.hip).  N = 1 + H * W: token 0 is the class token.
//
//     ksm  = softmax(k over the N tokens)                   per (batch, head, channel): a COLUMN softmax, class token included
//     F    = ksm^T v                                        [B, 8, Ch, Ch]
//     crpe = q_img . (dwconv_w(v_img) + bias_w)             heads 0-1: 3x3, heads 2-4: 5x5, heads 5-7: 7x7; class row 0
//     att  = scale * q F + crpe
//
// Forward, three launches:
//   fa_reduce_kernel<Ch, true>   grid (batch * head, chunks of FA_CHUNK tokens): the chunk's k in LDS -> column maxima m and exp-sums s,
//                                then P[i][j] = sum_n exp(k[n][i] - m[i]) v[n][j] with thread (j, token lane) holding a column of P in
//                                registers (e rows are LDS broadcasts, v is read once, Ch contiguous floats per token).
//   fa_combine_fwd_kernel        per (batch, head): chunk partials in chunk order with the usual max rescaling -> F (normalised) and the
//                                column statistics (M, S) the backward recomputes ksm from.
//   fa_apply_fwd_kernel          grid (spatial tiles, batch, head groups): a thread owns ONE channel (its up to 49 window weights live in
//                                registers, zero outside the head's window) and walks the tile's pixels; lanes run along channels, so every
//                                q / v / att access is a contiguous run of the token row.  q rows and F sit in LDS for the q F product.
//                                conv(v) is never stored.
// Backward, with G = dO . q on image tokens:
//   dF = scale * sum_n q[n]^T dO[n]                        fa_reduce_kernel<Ch, false> + fa_combine_bwd_kernel
//   dW[c][tap] = sum G[p][c] v[p + tap][c], db = sum G     fa_wgrad_kernel<3, true> + finalize (double, strip order)
//   dq = scale * dO F^T + dO . (conv(v) + b)
//   dv = ksm dF + dwconv_dgrad(G)
//   dk[n][i] = ksm[n][i] * (sum_j dF[i][j] v[n][j] - sum_j dF[i][j] F[i][j])          the column softmax's correction in closed form
//   -- ONE token reduction and one apply pass (fa_apply_bwd_kernel); ksm and conv(v) are recomputed, d(qkv) is written packed.
// Every sum runs in a fixed order (lanes, chunks, strips): no floating-point atomics, results are bitwise repeatable.
//
// The position encoding on a token tensor (x [B, 1 + H * W, C], y = x + dwconv3(x_img) + b on the image rows, class row passed
// through) uses the same one-channel-per-thread layout: cpe_tok_kernel (forward and, with flipped taps, the data gradient) and
// fa_wgrad_kernel<1, false> for dw / db.
#include "../../include/mmskin.h"
#include <stdlib.h>

#include "common.h"

namespace {

#define FA_HEADS 8
#define FA_CHUNK 128          // tokens per reduce workgroup (the chunk's k / q: 32 KiB of LDS at Ch = 64)
#define FA_FMAX 4224          // floats of one [HG][Ch][Ch + 1] matrix block in the apply kernels
#define FA_ROWMAX 2304        // floats of one staged [slots][CW] row block

__host__ __device__ __forceinline__ int fa_part_stride(int CH) { return 2 * CH + CH * CH; }

// ---------------------------------------------------------------------------------------------------------------- token reduction
// part[(bh * nchunk + chunk)] = { m[CH], s[CH], P[CH][CH] };  SOFTMAX: a = k, b = v, P = sum exp(a - m)^T b;  else P = sum a^T b (m, s unused)
template <int CH, bool SOFTMAX>
__global__ __launch_bounds__(256) void fa_reduce_kernel(const float* __restrict__ a, int64_t a_tok, int64_t a_b, const float* __restrict__ b,
                                                        int64_t b_tok, int64_t b_b, float* __restrict__ part, int N, int nchunk) {
  constexpr int TL = 256 / CH;      // token lanes
  __shared__ __attribute__((aligned(16))) float at[FA_CHUNK][CH];
  __shared__ float P[CH][CH];
  __shared__ float red[256];
  __shared__ float colm[CH], cols[CH];
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, bi = bh / FA_HEADS, h = bh - bi * FA_HEADS, c = blockIdx.y;
  const int n0 = c * FA_CHUNK, cnt = min(N - n0, FA_CHUNK);
  const float* ap = a + bi * a_b + (int64_t)h * CH + (int64_t)n0 * a_tok;
  const float* bp = b + bi * b_b + (int64_t)h * CH + (int64_t)n0 * b_tok;
  for (int e = tid; e < cnt * (CH / 4); e += 256) {        // all of a thread's loads in flight together
    const int n = e / (CH / 4), q4 = e - n * (CH / 4);
    *reinterpret_cast<float4*>(&at[n][4 * q4]) = *reinterpret_cast<const float4*>(ap + (int64_t)n * a_tok + 4 * q4);
  }
  __syncthreads();
  const int j = tid % CH, tl = tid / CH;
  const bool active = tl < TL;
  if (SOFTMAX) {
    float m = -INFINITY;
    if (active) for (int n = tl; n < cnt; n += TL) m = fmaxf(m, at[n][j]);
    if (active) red[tl * CH + j] = m;
    __syncthreads();
    if (tid < CH) {
      float t = -INFINITY;
      for (int l = 0; l < TL; ++l) t = fmaxf(t, red[l * CH + tid]);
      colm[tid] = t;
    }
    __syncthreads();
    for (int e = tid; e < cnt * CH; e += 256) {
      const int n = e / CH, i = e - n * CH;
      at[n][i] = expf(at[n][i] - colm[i]);
    }
    __syncthreads();
    float s = 0.f;
    if (active) for (int n = tl; n < cnt; n += TL) s += at[n][j];
    if (active) red[tl * CH + j] = s;
    __syncthreads();
    if (tid < CH) {
      float t = 0.f;
      for (int l = 0; l < TL; ++l) t += red[l * CH + tid];
      cols[tid] = t;
    }
    __syncthreads();
  }
  float acc[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) acc[i] = 0.f;
  if (active) {
    for (int nb = tl; nb < cnt; nb += 4 * TL) {            // four tokens per trip: their loads of b in flight together
      float bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = nb + u * TL;
        bv[u] = n < cnt ? bp[(int64_t)n * b_tok + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = min(nb + u * TL, cnt - 1);           // past the end: bv = 0
#pragma unroll
        for (int i = 0; i < CH; i += 4) {
          const float4 e4 = *reinterpret_cast<const float4*>(&at[n][i]);
          acc[i] = fmaf(e4.x, bv[u], acc[i]); acc[i + 1] = fmaf(e4.y, bv[u], acc[i + 1]);
          acc[i + 2] = fmaf(e4.z, bv[u], acc[i + 2]); acc[i + 3] = fmaf(e4.w, bv[u], acc[i + 3]);
        }
      }
    }
  }
  for (int l = 0; l < TL; ++l) {                           // token lanes in lane order
    if (tl == l) {
#pragma unroll
      for (int i = 0; i < CH; ++i) P[i][j] = l == 0 ? acc[i] : P[i][j] + acc[i];
    }
    __syncthreads();
  }
  float* out = part + ((int64_t)bh * nchunk + c) * fa_part_stride(CH);
  if (tid < CH) { out[tid] = SOFTMAX ? colm[tid] : 0.f; out[CH + tid] = SOFTMAX ? cols[tid] : 0.f; }
  for (int e = tid; e < CH * CH; e += 256) out[2 * CH + e] = P[e / CH][e % CH];
}

// F[bh][i][j] = sum_c P_c[i][j] exp(m_c[i] - M[i]) / S[i],  stats[bh] = { M[CH], S[CH] }
__global__ __launch_bounds__(256) void fa_combine_fwd_kernel(const float* __restrict__ part, int nchunk, int CH, float* __restrict__ F,
                                                             float* __restrict__ stats) {
  __shared__ float M[64], S[64];
  const int bh = blockIdx.x, PS = fa_part_stride(CH), tid = threadIdx.x;
  const float* src = part + (int64_t)bh * nchunk * PS;
  if (tid < CH) {
    float m = -INFINITY;
    for (int c = 0; c < nchunk; ++c) m = fmaxf(m, src[(int64_t)c * PS + tid]);
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += src[(int64_t)c * PS + CH + tid] * expf(src[(int64_t)c * PS + tid] - m);
    M[tid] = m; S[tid] = s;
    stats[(int64_t)bh * 2 * CH + tid] = m; stats[(int64_t)bh * 2 * CH + CH + tid] = s;
  }
  __syncthreads();
  for (int e = tid; e < CH * CH; e += 256) {
    const int i = e / CH;
    float t = 0.f;
    for (int c = 0; c < nchunk; ++c) t += src[(int64_t)c * PS + 2 * CH + e] * expf(src[(int64_t)c * PS + i] - M[i]);
    F[(int64_t)bh * CH * CH + e] = t / S[i];
  }
}
// dF[bh][i][j] = scale * sum_c P_c[i][j]
__global__ __launch_bounds__(256) void fa_combine_bwd_kernel(const float* __restrict__ part, int nchunk, int CH, float scale,
                                                             float* __restrict__ dF) {
  const int bh = blockIdx.x, PS = fa_part_stride(CH);
  const float* src = part + (int64_t)bh * nchunk * PS + 2 * CH;
  for (int e = threadIdx.x; e < CH * CH; e += 256) {
    float t = 0.f;
    for (int c = 0; c < nchunk; ++c) t += src[(int64_t)c * PS + e];
    dF[(int64_t)bh * CH * CH + e] = t * scale;
  }
}

// ---------------------------------------------------------------------------------------------------------------- apply passes
struct FaArgs {
  int B, N, H, W, CH, C;
  int HG, CW, PL;          // heads / channels per workgroup, pixel lanes (256 / CW)
  int TH, TW, tiles_x;     // spatial tile
  float scale;
  const float* w[3];       // crpe conv_list weights [2Ch,1,3,3] [3Ch,1,5,5] [3Ch,1,7,7]
  const float* bias[3];
};

// the 7x7-embedded window of channel c (zeros outside the head's own window) and its bias
__device__ __forceinline__ int fa_radius(int head) { return head < 2 ? 1 : (head < 5 ? 2 : 3); }
__device__ __forceinline__ void fa_load_window(const FaArgs& p, int c, float (&w)[49], float& bias, int& r) {
  const int head = c / p.CH, wi = head < 2 ? 0 : (head < 5 ? 1 : 2);
  r = wi + 1;
  const int k = 2 * r + 1, lc = c - (wi == 0 ? 0 : (wi == 1 ? 2 : 5)) * p.CH;
  const float* src = p.w[wi] + (int64_t)lc * k * k;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const bool in = dy >= -r && dy <= r && dx >= -r && dx <= r;
      w[(dy + 3) * 7 + dx + 3] = in ? src[(dy + r) * k + (dx + r)] : 0.f;
    }
  bias = p.bias[wi][lc];
}
// sum over the window of w[tap] * f(y + s * dy, x + s * dx): s = +1 is the convolution, s = -1 its data gradient
template <int SGN, typename Fn>
__device__ __forceinline__ float fa_window_sum(const float (&w)[49], int r, int y, int x, int H, int W, Fn f) {
  float acc = 0.f;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
    const int yy = y + SGN * dy;
    if (dy < -r || dy > r || (unsigned)yy >= (unsigned)H) continue;
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const int xx = x + SGN * dx;
      if (dx < -r || dx > r || (unsigned)xx >= (unsigned)W) continue;
      acc = fmaf(w[(dy + 3) * 7 + dx + 3], f(yy, xx), acc);
    }
  }
  return acc;
}

// slot s of a tile -> token n (or -1), pixel (y, x); the class token is the extra last slot of tile 0
__device__ __forceinline__ int fa_slot_token(const FaArgs& p, int s, int& y, int& x) {
  const int tile = blockIdx.x, ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  if (s == p.TH * p.TW) { y = -1; x = -1; return tile == 0 ? 0 : -1; }
  y = ty * p.TH + s / p.TW; x = tx * p.TW + s % p.TW;
  return (y < p.H && x < p.W) ? 1 + y * p.W + x : -1;
}

__global__ __launch_bounds__(256) void fa_apply_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ F,
                                                           float* __restrict__ att, const FaArgs p) {
  __shared__ float Fs[FA_FMAX];        // [HG][CH][CH + 1]
  __shared__ float qs[FA_ROWMAX];      // [slots][CW]
  const int tid = threadIdx.x, b = blockIdx.y, hg = blockIdx.z;
  const int CH = p.CH, CW = p.CW, C = p.C, nslots = p.TH * p.TW + 1;
  const int64_t tok = 3 * (int64_t)C;
  const float* qb = qkv + (int64_t)b * p.N * tok + (int64_t)hg * CW;
  for (int e = tid; e < p.HG * CH * CH; e += 256) {
    const int hl = e / (CH * CH), r = e - hl * CH * CH;
    Fs[(hl * CH + r / CH) * (CH + 1) + r % CH] = F[((int64_t)(b * FA_HEADS + hg * p.HG + hl)) * CH * CH + r];
  }
  for (int e = tid; e < nslots * CW; e += 256) {
    const int s = e / CW, cl = e - s * CW;
    int y, x;
    const int n = fa_slot_token(p, s, y, x);
    qs[e] = n >= 0 ? qb[(int64_t)n * tok + cl] : 0.f;
  }
  __syncthreads();
  const int cl = tid % CW, pl = tid / CW;
  if (pl >= p.PL) return;
  const int c = hg * CW + cl, hl = cl / CH, j = cl - hl * CH;
  float w[49], bias;
  int r;
  fa_load_window(p, c, w, bias, r);
  const float* vb = qkv + (int64_t)b * p.N * tok + 2 * C + c;
  const float* Fh = Fs + hl * CH * (CH + 1) + j;
  for (int s = pl; s < nslots; s += p.PL) {
    int y, x;
    const int n = fa_slot_token(p, s, y, x);
    if (n < 0) continue;
    const float* qr = qs + s * CW + hl * CH;
    float acc = 0.f;
    for (int i = 0; i < CH; ++i) acc = fmaf(qr[i], Fh[i * (CH + 1)], acc);
    acc *= p.scale;
    if (n > 0) {
      const float conv = fa_window_sum<1>(w, r, y, x, p.H, p.W, [&](int yy, int xx) { return vb[(int64_t)(1 + yy * p.W + xx) * tok]; });
      acc = fmaf(qs[s * CW + cl], conv + bias, acc);
    }
    att[((int64_t)b * p.N + n) * C + c] = acc;
  }
}

__global__ __launch_bounds__(256) void fa_apply_bwd_kernel(const float* __restrict__ dO, const float* __restrict__ qkv,
                                                           const float* __restrict__ F, const float* __restrict__ dF,
                                                           const float* __restrict__ stats, float* __restrict__ dqkv, const FaArgs p) {
  __shared__ float Fs[FA_FMAX], dFs[FA_FMAX];                 // [HG][CH][CH + 1]
  __shared__ float dos[FA_ROWMAX], vs[FA_ROWMAX], ks[FA_ROWMAX];   // [slots][CW]: dO, v, ksm
  __shared__ float Ds[256];                                   // [CW]: sum_j dF[i][j] F[i][j]
  const int tid = threadIdx.x, b = blockIdx.y, hg = blockIdx.z;
  const int CH = p.CH, CW = p.CW, C = p.C, nslots = p.TH * p.TW + 1;
  const int64_t tok = 3 * (int64_t)C;
  const float* qb = qkv + (int64_t)b * p.N * tok + (int64_t)hg * CW;
  const float* dob = dO + (int64_t)b * p.N * C + (int64_t)hg * CW;
  for (int e = tid; e < p.HG * CH * CH; e += 256) {
    const int hl = e / (CH * CH), r = e - hl * CH * CH;
    const int64_t src = ((int64_t)(b * FA_HEADS + hg * p.HG + hl)) * CH * CH + r;
    const int dst = (hl * CH + r / CH) * (CH + 1) + r % CH;
    Fs[dst] = F[src]; dFs[dst] = dF[src];
  }
  for (int e = tid; e < nslots * CW; e += 256) {
    const int s = e / CW, cl = e - s * CW;
    int y, x;
    const int n = fa_slot_token(p, s, y, x);
    float d = 0.f, v = 0.f, k = 0.f;
    if (n >= 0) {
      const int hl = cl / CH, i = cl - hl * CH;
      const float* st = stats + ((int64_t)(b * FA_HEADS + hg * p.HG + hl)) * 2 * CH;
      d = dob[(int64_t)n * C + cl];
      v = qb[(int64_t)n * tok + 2 * C + cl];
      k = expf(qb[(int64_t)n * tok + C + cl] - st[i]) / st[CH + i];
    }
    dos[e] = d; vs[e] = v; ks[e] = k;
  }
  __syncthreads();
  if (tid < CW) {
    const int hl = tid / CH, i = tid - hl * CH;
    const float* fr = Fs + (hl * CH + i) * (CH + 1);
    const float* dr = dFs + (hl * CH + i) * (CH + 1);
    float t = 0.f;
    for (int jj = 0; jj < CH; ++jj) t = fmaf(dr[jj], fr[jj], t);
    Ds[tid] = t;
  }
  __syncthreads();
  const int cl = tid % CW, pl = tid / CW;
  if (pl >= p.PL) return;
  const int c = hg * CW + cl, hl = cl / CH, j = cl - hl * CH;
  float w[49], bias;
  int r;
  fa_load_window(p, c, w, bias, r);
  const float* qc = qkv + (int64_t)b * p.N * tok + c;         // this channel's q column; v at + 2C
  const float* doc = dO + (int64_t)b * p.N * C + c;
  const float* Frow = Fs + (hl * CH + j) * (CH + 1);          // F[j][.]
  const float* dFrow = dFs + (hl * CH + j) * (CH + 1);        // dF[j][.]
  const float* dFcol = dFs + hl * CH * (CH + 1) + j;          // dF[.][j]
  for (int s = pl; s < nslots; s += p.PL) {
    int y, x;
    const int n = fa_slot_token(p, s, y, x);
    if (n < 0) continue;
    const float* dor = dos + s * CW + hl * CH;
    const float* vr = vs + s * CW + hl * CH;
    const float* kr = ks + s * CW + hl * CH;
    float dq = 0.f, dks = 0.f, dv = 0.f;
    for (int i = 0; i < CH; ++i) {
      dq = fmaf(dor[i], Frow[i], dq);
      dks = fmaf(dFrow[i], vr[i], dks);
      dv = fmaf(kr[i], dFcol[i * (CH + 1)], dv);
    }
    dq *= p.scale;
    const float dk = kr[j] * (dks - Ds[cl]);
    if (n > 0) {
      const float conv = fa_window_sum<1>(w, r, y, x, p.H, p.W, [&](int yy, int xx) { return qc[(int64_t)(1 + yy * p.W + xx) * tok + 2 * C]; });
      dq = fmaf(dor[j], conv + bias, dq);
      dv += fa_window_sum<-1>(w, r, y, x, p.H, p.W, [&](int yy, int xx) {
        const int64_t m = 1 + yy * p.W + xx;
        return doc[m * C] * qc[m * tok];
      });
    }
    float* o = dqkv + ((int64_t)b * p.N + n) * tok + c;
    o[0] = dq; o[C] = dk; o[2 * C] = dv;
  }
}

// ---------------------------------------------------------------------------------------------------------------- depthwise weight gradients
// partial[(strip * NT + t) * C + c] = sum over the strip's pixels of G[p][c] * V[p + tap t][c], t = NT - 1: sum of G   (NT = (2R+1)^2 + 1)
// G = g1 (* g2 when MUL), all on the image rows of token tensors: element (b, pixel, c) at base + b * sb + (1 + pixel) * st + c.
// HEADS: R = 3 and channel c only owns the window of its head (the rest stays zero).
#define FA_WG_CW 64
template <int R, bool MUL>
__global__ __launch_bounds__(256) void fa_wgrad_kernel(const float* __restrict__ g1, int64_t g1_tok, int64_t g1_b, const float* __restrict__ g2,
                                                       int64_t g2_tok, int64_t g2_b, const float* __restrict__ V, int64_t v_tok, int64_t v_b,
                                                       int H, int W, int C, int CH, int64_t total, int64_t per, float* __restrict__ partial) {
  constexpr int K = 2 * R + 1, NT = K * K + 1;
  __shared__ float red[4][FA_WG_CW];
  const int cl = threadIdx.x % FA_WG_CW, pl = threadIdx.x / FA_WG_CW;
  const int c = blockIdx.y * FA_WG_CW + cl;
  const bool cok = c < C;
  const int r = !cok ? 0 : (MUL ? fa_radius(c / CH) : R);
  float acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0.f;
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = min(total, p0 + per);
  const int HW = H * W;
  if (cok) {
    for (int64_t pp = p0 + pl; pp < p1; pp += 4) {
      const int b = (int)(pp / HW), pix = (int)(pp - (int64_t)b * HW), y = pix / W, x = pix - y * W;
      float g = g1[b * g1_b + (int64_t)(1 + pix) * g1_tok + c];
      if (MUL) g *= g2[b * g2_b + (int64_t)(1 + pix) * g2_tok + c];
      const float* vb = V + b * v_b + c;
#pragma unroll
      for (int dy = -R; dy <= R; ++dy) {
        const int yy = y + dy;
        if (dy < -r || dy > r || (unsigned)yy >= (unsigned)H) continue;
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
          const int xx = x + dx;
          if (dx < -r || dx > r || (unsigned)xx >= (unsigned)W) continue;
          acc[(dy + R) * K + dx + R] = fmaf(g, vb[(int64_t)(1 + yy * W + xx) * v_tok], acc[(dy + R) * K + dx + R]);
        }
      }
      acc[NT - 1] += g;
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {          // the four pixel lanes in lane order, one tap at a time
    red[pl][cl] = acc[t];
    __syncthreads();
    if (pl == 0 && cok) partial[((int64_t)blockIdx.x * NT + t) * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
    __syncthreads();
  }
}
// strips in strip order, in double.  crpe: scatter the 7x7-embedded taps into the three conv_list gradients
__global__ __launch_bounds__(256) void fa_wgrad_finalize_crpe_kernel(const float* __restrict__ partial, int nstrips, int C, int CH, float* dw0,
                                                                     float* dw1, float* dw2, float* db0, float* db1, float* db2) {
  const int i = blockIdx.x * 256 + threadIdx.x;     // over 50 * C: (t, c)
  if (i >= 50 * C) return;
  const int t = i / C, c = i - t * C;
  const int head = c / CH, wi = head < 2 ? 0 : (head < 5 ? 1 : 2), r = wi + 1, k = 2 * r + 1;
  const int lc = c - (wi == 0 ? 0 : (wi == 1 ? 2 : 5)) * CH;
  const int dy = t / 7 - 3, dx = t % 7 - 3;
  if (t < 49 && (dy < -r || dy > r || dx < -r || dx > r)) return;
  double s = 0.0;
  for (int q = 0; q < nstrips; ++q) s += (double)partial[(int64_t)q * 50 * C + i];
  float* dw = wi == 0 ? dw0 : (wi == 1 ? dw1 : dw2);
  float* db = wi == 0 ? db0 : (wi == 1 ? db1 : db2);
  if (t == 49) db[lc] = (float)s;
  else dw[(int64_t)lc * k * k + (dy + r) * k + (dx + r)] = (float)s;
}
__global__ __launch_bounds__(256) void fa_wgrad_finalize_cpe_kernel(const float* __restrict__ partial, int nstrips, int C, float* __restrict__ dw,
                                                                    float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;     // over 10 * C: (t, c)
  if (i >= 10 * C) return;
  const int t = i / C, c = i - t * C;
  double s = 0.0;
  for (int q = 0; q < nstrips; ++q) s += (double)partial[(int64_t)q * 10 * C + i];
  if (t == 9) { if (db) db[c] = (float)s; }
  else if (dw) dw[(int64_t)c * 9 + t] = (float)s;
}
inline void fa_strips(int64_t total, int64_t& per, int& nstrips) {
  per = (total + 255) / 256;
  if (per < 64) per = 64;
  nstrips = (int)((total + per - 1) / per);
}

// ---------------------------------------------------------------------------------------------------------------- position encoding on tokens
// y[b][0] = x[b][0];  y[b][1 + p][c] = x + sum_tap w[c][tap] x[p + SGN * tap] (+ bias): SGN = +1 forward, -1 data gradient (bias = NULL)
#define CPE_TOKS 32
template <int SGN>
__global__ __launch_bounds__(256) void cpe_tok_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ y, int H, int W, int C, int64_t ntok) {
  const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  if (c >= C) return;
  float wr[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wr[t] = w[(int64_t)c * 9 + t];
  const float bv = bias ? bias[c] : 0.f;
  const int N = 1 + H * W;
  const int64_t t0 = (int64_t)blockIdx.x * CPE_TOKS;
  for (int u = pl; u < CPE_TOKS; u += 4) {
    const int64_t t = t0 + u;
    if (t >= ntok) break;
    const int b = (int)(t / N), n = (int)(t - (int64_t)b * N);
    const float* xb = x + (int64_t)b * N * C + c;
    float acc = xb[(int64_t)n * C];
    if (n > 0) {
      const int py = (n - 1) / W, px = (n - 1) - py * W;
      acc += bv;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int yy = py + SGN * dy;
        if ((unsigned)yy >= (unsigned)H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = px + SGN * dx;
          if ((unsigned)xx >= (unsigned)W) continue;
          acc = fmaf(wr[(dy + 1) * 3 + dx + 1], xb[(int64_t)(1 + yy * W + xx) * C], acc);
        }
      }
    }
    y[t * C + c] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int fa_args(FaArgs& a, int B, int H, int W, int Ch, const char* what) {
  ARG_CHECK(B > 0 && H > 0 && W > 0, "%s: bad geometry (B=%d H=%d W=%d)", what, B, H, W);
  ARG_CHECK(Ch == 8 || Ch == 16 || Ch == 32 || Ch == 40 || Ch == 64, "%s: head width %d not in {8, 16, 32, 40, 64}", what, Ch);
  ARG_CHECK((int64_t)H * W < ((int64_t)1 << 22) && (int64_t)B * (1 + (int64_t)H * W) * 24 * Ch < ((int64_t)1 << 40), "%s: tensor too large", what);
  ARG_CHECK(B <= 65535, "%s: batch above the grid limit", what);
  a.B = B; a.H = H; a.W = W; a.N = 1 + H * W; a.CH = Ch; a.C = FA_HEADS * Ch;
  a.HG = FA_HEADS;
  while (a.HG > 1 && a.HG * Ch * (Ch + 1) > FA_FMAX) a.HG >>= 1;
  a.CW = a.HG * Ch;
  a.PL = 256 / a.CW;
  const int P = 2048 / a.CW;
  a.TH = 4; a.TW = P >= 32 ? 8 : 4;
  a.tiles_x = (W + a.TW - 1) / a.TW;
  a.scale = 1.f / sqrtf((float)Ch);
  // the staged blocks fit their LDS arrays
  ARG_CHECK(a.HG * Ch * (Ch + 1) <= FA_FMAX && (a.TH * a.TW + 1) * a.CW <= FA_ROWMAX && a.CW <= 256 && a.PL >= 1, "%s: internal tile plan", what);
  return MMSKIN_OK;
}
inline int fa_nchunk(int N) { return (N + FA_CHUNK - 1) / FA_CHUNK; }

template <bool SOFTMAX>
int fa_reduce(const float* a, int64_t a_tok, int64_t a_b, const float* b, int64_t b_tok, int64_t b_b, float* part, int B, int N, int Ch,
              hipStream_t st) {
  const dim3 grid(B * FA_HEADS, fa_nchunk(N));
  const int nc = fa_nchunk(N);
  switch (Ch) {
    case 8: hipLaunchKernelGGL((fa_reduce_kernel<8, SOFTMAX>), grid, dim3(256), 0, st, a, a_tok, a_b, b, b_tok, b_b, part, N, nc); break;
    case 16: hipLaunchKernelGGL((fa_reduce_kernel<16, SOFTMAX>), grid, dim3(256), 0, st, a, a_tok, a_b, b, b_tok, b_b, part, N, nc); break;
    case 32: hipLaunchKernelGGL((fa_reduce_kernel<32, SOFTMAX>), grid, dim3(256), 0, st, a, a_tok, a_b, b, b_tok, b_b, part, N, nc); break;
    case 40: hipLaunchKernelGGL((fa_reduce_kernel<40, SOFTMAX>), grid, dim3(256), 0, st, a, a_tok, a_b, b, b_tok, b_b, part, N, nc); break;
    default: hipLaunchKernelGGL((fa_reduce_kernel<64, SOFTMAX>), grid, dim3(256), 0, st, a, a_tok, a_b, b, b_tok, b_b, part, N, nc); break;
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

// The scratch of mmskin_factor_attention_*, as float offsets (packed): the reduction partials of both directions, then the backward's dF
// and its position-encoding weight-gradient partials.  mmskin_factor_attention_scratch_floats returns `total`.
struct FaScratch {
  int64_t part = 0, dF, wpart, total;
  FaScratch(int B, int H, int W, int Ch, bool backward) {
    int64_t per; int ns;
    fa_strips((int64_t)B * H * W, per, ns);
    dF = (int64_t)B * FA_HEADS * fa_nchunk(1 + H * W) * fa_part_stride(Ch);
    wpart = dF + (int64_t)B * FA_HEADS * Ch * Ch;
    total = backward ? wpart + (int64_t)ns * 50 * FA_HEADS * Ch : dF;
  }
};

}  // namespace

extern "C" {

int64_t mmskin_factor_attention_scratch_floats(int B, int H, int W, int Ch, int backward) {
  if (B <= 0 || H <= 0 || W <= 0 || Ch <= 0) return 0;
  return FaScratch(B, H, W, Ch, backward != 0).total;
}

int mmskin_factor_attention_forward(const float* qkv, const float* w3, const float* b3, const float* w5, const float* b5, const float* w7,
                                    const float* b7, float* att, float* F, float* stats, float* scratch, int B, int H, int W, int Ch,
                                    void* stream) {
  ARG_CHECK(qkv && w3 && b3 && w5 && b5 && w7 && b7 && att && F && stats && scratch, "factor_attention_forward: null argument");
  ARG_CHECK(((uintptr_t)qkv & 15) == 0, "factor_attention_forward: 16-byte aligned qkv required");
  FaArgs a;
  int rc = fa_args(a, B, H, W, Ch, "factor_attention_forward");
  if (rc) return rc;
  a.w[0] = w3; a.w[1] = w5; a.w[2] = w7; a.bias[0] = b3; a.bias[1] = b5; a.bias[2] = b7;
  const int64_t tok = 3 * (int64_t)a.C, bs = (int64_t)a.N * tok;
  hipStream_t st = ST(stream);
  float* part = scratch + FaScratch(B, H, W, Ch, false).part;
  if ((rc = fa_reduce<true>(qkv + a.C, tok, bs, qkv + 2 * a.C, tok, bs, part, B, a.N, Ch, st))) return rc;
  hipLaunchKernelGGL(fa_combine_fwd_kernel, dim3(B * FA_HEADS), dim3(256), 0, st, part, fa_nchunk(a.N), Ch, F, stats);
  const int tiles = a.tiles_x * ((H + a.TH - 1) / a.TH);
  hipLaunchKernelGGL(fa_apply_fwd_kernel, dim3(tiles, B, FA_HEADS / a.HG), dim3(256), 0, st, qkv, F, att, a);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int mmskin_factor_attention_backward(const float* dO, const float* qkv, const float* w3, const float* b3, const float* w5, const float* b5,
                                     const float* w7, const float* b7, const float* F, const float* stats, float* dqkv, float* dw3,
                                     float* db3, float* dw5, float* db5, float* dw7, float* db7, float* scratch, int B, int H, int W,
                                     int Ch, void* stream) {
  ARG_CHECK(dO && qkv && w3 && b3 && w5 && b5 && w7 && b7 && F && stats && dqkv && dw3 && db3 && dw5 && db5 && dw7 && db7 && scratch,
            "factor_attention_backward: null argument");
  ARG_CHECK(((uintptr_t)qkv & 15) == 0, "factor_attention_backward: 16-byte aligned qkv required");
  FaArgs a;
  int rc = fa_args(a, B, H, W, Ch, "factor_attention_backward");
  if (rc) return rc;
  a.w[0] = w3; a.w[1] = w5; a.w[2] = w7; a.bias[0] = b3; a.bias[1] = b5; a.bias[2] = b7;
  const int C = a.C;
  const int64_t tok = 3 * (int64_t)C, bs = (int64_t)a.N * tok, obs = (int64_t)a.N * C;
  hipStream_t st = ST(stream);
  const FaScratch lay(B, H, W, Ch, true);
  float *part = scratch + lay.part, *dF = scratch + lay.dF, *wpart = scratch + lay.wpart;
  if ((rc = fa_reduce<false>(qkv, tok, bs, dO, C, obs, part, B, a.N, Ch, st))) return rc;          // sum_n q[n]^T dO[n]
  hipLaunchKernelGGL(fa_combine_bwd_kernel, dim3(B * FA_HEADS), dim3(256), 0, st, part, fa_nchunk(a.N), Ch, a.scale, dF);
  int64_t per; int ns;
  const int64_t total = (int64_t)B * H * W;
  fa_strips(total, per, ns);
  hipLaunchKernelGGL((fa_wgrad_kernel<3, true>), dim3(ns, (C + FA_WG_CW - 1) / FA_WG_CW), dim3(256), 0, st, dO, (int64_t)C, obs, qkv, tok, bs,
                     qkv + 2 * C, tok, bs, H, W, C, Ch, total, per, wpart);
  hipLaunchKernelGGL(fa_wgrad_finalize_crpe_kernel, dim3((50 * C + 255) / 256), dim3(256), 0, st, wpart, ns, C, Ch, dw3, dw5, dw7, db3, db5, db7);
  const int tiles = a.tiles_x * ((H + a.TH - 1) / a.TH);
  hipLaunchKernelGGL(fa_apply_bwd_kernel, dim3(tiles, B, FA_HEADS / a.HG), dim3(256), 0, st, dO, qkv, F, dF, stats, dqkv, a);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int64_t mmskin_conv_pos_enc_tokens_scratch_floats(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  int64_t per; int ns;
  fa_strips((int64_t)B * H * W, per, ns);
  return (int64_t)ns * 10 * C;
}

int mmskin_conv_pos_enc_tokens_forward(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int C, void* stream) {
  ARG_CHECK(x && w && b && y && B > 0 && H > 0 && W > 0 && C > 0, "conv_pos_enc_tokens_forward: bad argument");
  ARG_CHECK((int64_t)H * W < ((int64_t)1 << 24), "conv_pos_enc_tokens_forward: grid too large");
  const int64_t ntok = (int64_t)B * (1 + (int64_t)H * W);
  ARG_CHECK((ntok + CPE_TOKS - 1) / CPE_TOKS < ((int64_t)1 << 31) && (C + 63) / 64 <= 65535, "conv_pos_enc_tokens_forward: tensor too large");
  hipLaunchKernelGGL(cpe_tok_kernel<1>, dim3((unsigned)((ntok + CPE_TOKS - 1) / CPE_TOKS), (C + 63) / 64), dim3(256), 0, ST(stream), x, w, b, y, H,
                     W, C, ntok);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int mmskin_conv_pos_enc_tokens_backward(const float* dy, const float* x, const float* w, float* scratch, float* dx, float* dw, float* db, int B,
                                        int H, int W, int C, void* stream) {
  ARG_CHECK(dy && x && w && B > 0 && H > 0 && W > 0 && C > 0, "conv_pos_enc_tokens_backward: bad argument");
  ARG_CHECK((int64_t)H * W < ((int64_t)1 << 24), "conv_pos_enc_tokens_backward: grid too large");
  ARG_CHECK(!(dw || db) || scratch, "conv_pos_enc_tokens_backward: scratch required for dw / db");
  const int N = 1 + H * W;
  const int64_t ntok = (int64_t)B * N;
  ARG_CHECK((ntok + CPE_TOKS - 1) / CPE_TOKS < ((int64_t)1 << 31) && (C + 63) / 64 <= 65535, "conv_pos_enc_tokens_backward: tensor too large");
  hipStream_t st = ST(stream);
  if (dx)
    hipLaunchKernelGGL(cpe_tok_kernel<-1>, dim3((unsigned)((ntok + CPE_TOKS - 1) / CPE_TOKS), (C + 63) / 64), dim3(256), 0, st, dy, w,
                       (const float*)nullptr, dx, H, W, C, ntok);
  if (dw || db) {
    int64_t per; int ns;
    const int64_t total = (int64_t)B * H * W, bs = (int64_t)N * C;
    fa_strips(total, per, ns);
    hipLaunchKernelGGL((fa_wgrad_kernel<1, false>), dim3(ns, (C + FA_WG_CW - 1) / FA_WG_CW), dim3(256), 0, st, dy, (int64_t)C, bs,
                       (const float*)nullptr, (int64_t)0, (int64_t)0, x, (int64_t)C, bs, H, W, C, C, total, per, scratch);
    hipLaunchKernelGGL(fa_wgrad_finalize_cpe_kernel, dim3((10 * C + 255) / 256), dim3(256), 0, st, scratch, ns, C, dw, db);
  }
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

}  // extern "C"
