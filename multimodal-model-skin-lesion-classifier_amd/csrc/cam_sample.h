// Device functions the class-activation-map kernels share (scorecam.hip, gradcam.hip): the bilinear sample of
// torch.nn.Upsample / F.interpolate(mode='bilinear', align_corners=False) from a source tile in LDS, and the workgroup
// min / max.
//
//   src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), l = src - i0,
//   top = f00 + lx * (f01 - f00), bot = f10 + lx * (f11 - f10), value = top + ly * (bot - top)
// The weights 1 - l and l are applied in this difference form because it keeps a constant map exactly constant when every
// operation rounds on its own ((1 - l) * a + l * a is a only when the sum is fused, as torch's own kernels fuse it).
// Whether the multiplies and adds are contracted into FMAs is the including file's choice (scorecam.hip switches it off).
#pragma once
#include "common.h"

// source taps of one destination index along one axis; every index is clamped to [0, in - 1]
__device__ __forceinline__ void axis_tap(int d, float scale, int in, int& i0, int& i1, float& l) {
  float s = ((float)d + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min(max((int)s, 0), in - 1);
  i1 = min(i0 + 1, in - 1);
  l = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// the four LDS offsets and two weights of one output pixel: the same for every channel
struct Tap {
  int a00, a01, a10, a11;
  float lx, ly;
};
__device__ __forceinline__ Tap make_tap(int y, int x, int fh, int fw, float scale_h, float scale_w) {
  int y0, y1, x0, x1;
  Tap t;
  axis_tap(y, scale_h, fh, y0, y1, t.ly);
  axis_tap(x, scale_w, fw, x0, x1, t.lx);
  t.a00 = y0 * fw + x0; t.a01 = y0 * fw + x1; t.a10 = y1 * fw + x0; t.a11 = y1 * fw + x1;
  return t;
}
__device__ __forceinline__ float bilerp(const float* src, const Tap& t) {
  const float f00 = src[t.a00], f10 = src[t.a10];
  const float top = f00 + t.lx * (src[t.a01] - f00);
  const float bot = f10 + t.lx * (src[t.a11] - f10);
  return top + t.ly * (bot - top);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// min / max over the workgroup (at most 4 waves); every thread returns with the result.  red: 8 floats of LDS
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[wave] = mn; red[4 + wave] = mx; }
  __syncthreads();
  mn = red[0]; mx = red[4];
  for (int w = 1; w < nwave; ++w) { mn = fminf(mn, red[w]); mx = fmaxf(mx, red[4 + w]); }
}
