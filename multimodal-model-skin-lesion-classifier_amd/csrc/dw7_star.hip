// CAFormer SepConv core on gfx950 (timm metaformer.py SepConv: pwconv1 -> StarReLU -> depthwise 7x7 -> pwconv2): the StarReLU and
// the depthwise 7x7 (stride 1, pad 3, no bias) in one kernel each way, on NHWC fp32 activations.  The 1x1 convolutions around it are
// Linear layers over [N*H*W, C] rows (models/hip_caformer.py).
//
// Both kernels stage a tile of 8 x 16 output pixels plus its 3-pixel halo (14 x 22 pixels) for a chunk of 64 channels in LDS
// (78,848 B: two workgroups per CU), one channel per lane and the channel's 49 taps in registers.  A lane computes strips of 8
// horizontally adjacent outputs, reading the 14 staged values a strip needs per kernel row once (12.25 LDS reads per output instead
// of 49).
//   forward : stages act(z) = s relu(z)^2 + b (zero outside the image: the convolution pads the activation), y = dw7(act(z)).
//   backward: stages dy with its halo; per output position q the same 14-value rows serve both
//               g[q]  = sum_tap w[tap] dy[q + 3 - tap]                  (the data gradient of the convolution)
//               dW[tap] += act(z)[q] dy[q + 3 - tap]                     (sum over q of the pixel pairs the tap joins)
//             with act(z)[q] recomputed from z at the lane's own pixels, then dz = g 2 s relu(z), and the StarReLU scalar gradients
//             sum g relu(z)^2, sum g.  Each workgroup walks a fixed set of tiles and keeps its dW / scalar sums in registers; the
//             per-workgroup partials are added by two small kernels in a fixed order, so two calls give bitwise-identical results.
#include "../../include/mmskin.h"
#include "common.h"

namespace {

constexpr int TH = 8, TW = 16;                  // output tile
constexpr int SH = TH + 6, SW = TW + 6;         // staged tile (3-pixel halo)
constexpr int CC = 64;                          // channels per workgroup (one per lane)
constexpr int R = 8;                            // outputs per strip
constexpr int SPW = TH * TW / R / 4;            // strips per wave (4 waves)
constexpr int LDS_BYTES = SH * SW * CC * 4;     // 78,848
constexpr int BWD_TARGET_BLOCKS = 512;          // two resident workgroups per CU on 256 CUs
static_assert(TW == 2 * R, "two strips per tile row");

struct Geo {
  int tx, ty, tiles;                            // tiles across, down, per image
  int64_t ntiles;
  int chunks, G;                                // channel chunks; backward workgroups per chunk
};
inline Geo geo(int N, int H, int W, int C) {
  Geo g;
  g.tx = (W + TW - 1) / TW;
  g.ty = (H + TH - 1) / TH;
  g.tiles = g.tx * g.ty;
  g.ntiles = (int64_t)N * g.tiles;
  g.chunks = (C + CC - 1) / CC;
  int64_t G = (BWD_TARGET_BLOCKS + g.chunks - 1) / g.chunks;
  if (G > g.ntiles) G = g.ntiles;
  g.G = (int)(G < 1 ? 1 : G);
  return g;
}

__device__ __forceinline__ float star(float z, float s, float b) { const float r = fmaxf(z, 0.f); return s * (r * r) + b; }

// lds[p][c] for the SH x SW pixels around tile (y0, x0) of image n, channels [c0, c0 + 64): src (ACT: act(src)), zero outside the
// image and past C.  16 lanes per pixel, one float4 each.
template <bool ACT>
__device__ __forceinline__ void stage(const float* __restrict__ src, int n, int y0, int x0, int c0, int H, int W, int C, float s, float b,
                                      float* __restrict__ lds) {
  const int q = threadIdx.x & 15, c = c0 + q * 4;
#pragma unroll 4
  for (int p = threadIdx.x >> 4; p < SH * SW; p += 16) {
    const int yy = y0 - 3 + p / SW, xx = x0 - 3 + p % SW;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W && c < C) {
      v = *reinterpret_cast<const float4*>(src + (((int64_t)n * H + yy) * W + xx) * C + c);
      if (ACT) v = make_float4(star(v.x, s, b), star(v.y, s, b), star(v.z, s, b), star(v.w, s, b));
    }
    *reinterpret_cast<float4*>(lds + p * CC + q * 4) = v;
  }
}

__global__ __launch_bounds__(256) void dw7_star_fwd_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ sp,
                                                           const float* __restrict__ bp, float* __restrict__ y, int H, int W, int C, int tx,
                                                           int tiles) {
  extern __shared__ float lds[];
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int y0 = (t / tx) * TH, x0 = (t % tx) * TW, c0 = blockIdx.y * CC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = c0 + lane;
  const float s = sp[0], b = bp[0];
  float wr[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) wr[k] = c < C ? w[(int64_t)c * 49 + k] : 0.f;
  stage<true>(z, n, y0, x0, c0, H, W, C, s, b, lds);
  __syncthreads();
  if (c >= C) return;
#pragma unroll 1
  for (int j = 0; j < SPW; ++j) {
    const int strip = wv + 4 * j, row = strip >> 1, col0 = (strip & 1) * R;
    const int yy = y0 + row;
    if (yy >= H || x0 + col0 >= W) continue;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const float* src = lds + ((row + ky) * SW + col0) * CC + lane;
      float in[R + 6];
#pragma unroll
      for (int i = 0; i < R + 6; ++i) in[i] = src[i * CC];
#pragma unroll
      for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(wr[ky * 7 + kx], in[r + kx], acc[r]);
    }
    float* out = y + (((int64_t)n * H + yy) * W + x0 + col0) * C + c;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (x0 + col0 + r < W) out[(int64_t)r * C] = acc[r];
  }
}

// Workgroup (gx, chunk) takes tiles gx, gx + G, ...; writes part_w[gx][tap][C] (its chunk's columns) and part_sb[chunk * G + gx][2].
__global__ __launch_bounds__(256) void dw7_star_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ w,
                                                           const float* __restrict__ sp, const float* __restrict__ bp, float* __restrict__ dz,
                                                           float* __restrict__ part_w, float* __restrict__ part_sb, int H, int W, int C,
                                                           int tx, int tiles, int64_t ntiles) {
  extern __shared__ float lds[];
  const int G = gridDim.x, gx = blockIdx.x, c0 = blockIdx.y * CC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = c0 + lane;
  const float s = sp[0], b = bp[0], s2 = 2.f * s;
  float wr[49], dw[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) { wr[k] = c < C ? w[(int64_t)c * 49 + k] : 0.f; dw[k] = 0.f; }
  float ssum = 0.f, bsum = 0.f;
#pragma unroll 1
  for (int64_t tg = gx; tg < ntiles; tg += G) {
    const int n = (int)(tg / tiles), t = (int)(tg % tiles);
    const int y0 = (t / tx) * TH, x0 = (t % tx) * TW;
    __syncthreads();                            // the previous tile's reads are done
    stage<false>(dy, n, y0, x0, c0, H, W, C, 0.f, 0.f, lds);
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < SPW; ++j) {
      const int strip = wv + 4 * j, row = strip >> 1, col0 = (strip & 1) * R;
      const int yy = y0 + row;
      if (c >= C || yy >= H || x0 + col0 >= W) continue;
      const int64_t pix0 = ((int64_t)n * H + yy) * W + x0 + col0;
      float rz[R], a[R], g[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool ok = x0 + col0 + r < W;
        rz[r] = ok ? fmaxf(z[(pix0 + r) * C + c], 0.f) : 0.f;
        a[r] = ok ? s * (rz[r] * rz[r]) + b : 0.f;
        g[r] = 0.f;
      }
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const float* src = lds + ((row + 6 - ky) * SW + col0) * CC + lane;
        float in[R + 6];
#pragma unroll
        for (int i = 0; i < R + 6; ++i) in[i] = src[i * CC];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            g[r] = fmaf(wr[ky * 7 + kx], in[r + 6 - kx], g[r]);
            dw[ky * 7 + kx] = fmaf(a[r], in[r + 6 - kx], dw[ky * 7 + kx]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (x0 + col0 + r < W) {
          if (dz) dz[(pix0 + r) * C + c] = g[r] * s2 * rz[r];
          ssum = fmaf(g[r], rz[r] * rz[r], ssum);
          bsum += g[r];
        }
      }
    }
  }
  // the four waves' dW meet in LDS (reused), added in a fixed order
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 49; ++k) lds[(wv * 49 + k) * CC + lane] = dw[k];
  __shared__ float red[2][4];
  ssum = wave_sum(ssum); bsum = wave_sum(bsum);
  if (lane == 0) { red[0][wv] = ssum; red[1][wv] = bsum; }
  __syncthreads();
  for (int i = threadIdx.x; i < 49 * CC; i += 256) {
    const int k = i / CC, l = i % CC;
    if (c0 + l < C)
      part_w[((int64_t)gx * 49 + k) * C + c0 + l] = (lds[(0 * 49 + k) * CC + l] + lds[(1 * 49 + k) * CC + l]) +
                                                     (lds[(2 * 49 + k) * CC + l] + lds[(3 * 49 + k) * CC + l]);
  }
  if (threadIdx.x == 0) {
    float* o = part_sb + 2 * ((int64_t)blockIdx.y * G + gx);
    o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// dw[c][tap] = sum_g part_w[g][tap][c], g ascending
__global__ __launch_bounds__(256) void dw7_wgrad_finalize_kernel(const float* __restrict__ part_w, float* __restrict__ dw, int G, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 49 * C) return;
  const int k = i / C, c = i % C;
  float t = 0.f;
  for (int g = 0; g < G; ++g) t += part_w[((int64_t)g * 49 + k) * C + c];
  dw[(int64_t)c * 49 + k] = t;
}

// dsb[0..1] = sums of the nb pairs in part_sb, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void dw7_scalar_finalize_kernel(const float* __restrict__ part_sb, int nb, float* __restrict__ dsb) {
  __shared__ float red[2][4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { a += part_sb[2 * i]; b += part_sb[2 * i + 1]; }
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    dsb[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    dsb[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// The backward's scratch as float offsets (packed): per-group weight-gradient partials, then the (ds, db) pairs per group and chunk.
struct Dw7Scratch {
  int64_t part_w = 0, part_sb, total;
  explicit Dw7Scratch(const Geo& g, int C) {
    part_sb = (int64_t)g.G * 49 * C;
    total = part_sb + 2 * (int64_t)g.G * g.chunks;
  }
};

}  // namespace

extern "C" {

int64_t mmskin_dw7_star_scratch_floats(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return Dw7Scratch(geo(N, H, W, C), C).total;
}

int mmskin_dw7_star_forward(const float* z, const float* w, const float* s, const float* b, float* y, int N, int H, int W, int C,
                            void* stream) {
  ARG_CHECK(z && w && s && b && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "dw7_star_forward: bad argument");
  const Geo g = geo(N, H, W, C);
  ARG_CHECK(g.ntiles <= 0x7fffffff && g.chunks <= 65535, "dw7_star_forward: shape too large");
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)dw7_star_fwd_kernel, LDS_BYTES));
  hipLaunchKernelGGL(dw7_star_fwd_kernel, dim3((unsigned)g.ntiles, g.chunks), dim3(256), LDS_BYTES, ST(stream), z, w, s, b, y, H, W, C,
                     g.tx, g.tiles);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int mmskin_dw7_star_backward(const float* dy, const float* z, const float* w, const float* s, const float* b, float* scratch, float* dz,
                             float* dw, float* dsb, int N, int H, int W, int C, void* stream) {
  ARG_CHECK(dy && z && w && s && b && scratch && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "dw7_star_backward: bad argument");
  const Geo g = geo(N, H, W, C);
  ARG_CHECK(g.chunks <= 65535, "dw7_star_backward: shape too large");
  const Dw7Scratch lay(g, C);
  float *part_w = scratch + lay.part_w, *part_sb = scratch + lay.part_sb;
  HIP_CHECK_RET(opt_in_dynamic_lds((const void*)dw7_star_bwd_kernel, LDS_BYTES));
  hipLaunchKernelGGL(dw7_star_bwd_kernel, dim3(g.G, g.chunks), dim3(256), LDS_BYTES, ST(stream), dy, z, w, s, b, dz, part_w, part_sb, H, W,
                     C, g.tx, g.tiles, g.ntiles);
  HIP_CHECK_RET(hipGetLastError());
  if (dw) {
    hipLaunchKernelGGL(dw7_wgrad_finalize_kernel, dim3(ceil_div(49 * C, 256)), dim3(256), 0, ST(stream), part_w, dw, g.G, C);
    HIP_CHECK_RET(hipGetLastError());
  }
  if (dsb) {
    hipLaunchKernelGGL(dw7_scalar_finalize_kernel, dim3(1), dim3(256), 0, ST(stream), part_sb, g.G * g.chunks, dsb);
    HIP_CHECK_RET(hipGetLastError());
  }
  return MMSKIN_OK;
}

}  // extern "C"
