// Score-CAM (interpretability/ScoreCam.py:62-155) without its per-channel host loop: three forward-only kernels around the
// batched masked forwards that mmskin.cam.ScoreCAM drives.
//
//   minmax   per channel, min and max of the bilinearly UPSAMPLED map (not of the source samples: with align_corners=False no
//            output pixel of a 7x7 -> 224x224 upsample lands on a source sample, so the two differ)
//   mask     out[j, ch, y, x] = image[ch, y, x] * cam_j[y, x] for a chunk of channels, cam_j = (up - min) / (max - min)
//   combine  heat = sum_c scores[c] * cam_c in ascending channel order, ReLU, then min-max normalised over the image
//
// The normalised maps are never stored: 1664 maps of 224x224 are 334 MB per explained image against 326 KB of features, and
// recomputing one sample is four LDS reads and about ten flops.  Every kernel keeps its channels' source tiles in LDS and
// interpolates from there.
//
// The upsample is torch.nn.Upsample(size=(H, W), mode='bilinear') (align_corners=False):
//   src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), l = src - i0,
//   top = f00 + lx * (f01 - f00), bot = f10 + lx * (f11 - f10), value = top + ly * (bot - top)
// The weights 1 - l and l are applied in this difference form because it keeps a constant channel exactly constant when
// every operation rounds on its own ((1 - l) * a + l * a is a only when the sum is fused, as torch's own kernels fuse it):
// such a channel is "flat" and must give an all-zero mask (ScoreCam.py:117-121), not its rounding noise stretched to [0, 1].
// tests/scorecam_oracle.py restates exactly this operation order in numpy fp32 and the kernels match it bit for bit, so
// every multiply and add rounds on its own: contraction into FMAs is switched off for this file.
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

#include "cam_sample.h"   // axis_tap / make_tap / bilerp / block_minmax, shared with gradcam.hip; compiled here with contraction off
#include "perturb_tile.h" // tile_pixel / tile_store, shared with rise.hip and faithfulness.hip

namespace {

constexpr int NT = 256;                   // threads per workgroup
constexpr int PPT = 4;                    // mask: pixels per thread (one 16-byte store per colour plane)
constexpr int MASK_G = 8;                 // mask: channels per workgroup (the image tile is read once and reused for them)
constexpr int LDS_FLOATS = 12 * 1024;     // 48 KiB of dynamic LDS per workgroup, the most any of the kernels asks for

// One workgroup per channel.  A wave walks rows, its lanes walk columns: no integer division per pixel.
__global__ __launch_bounds__(NT) void scorecam_minmax_kernel(const float* __restrict__ fmap, int fh, int fw, int H, int W,
                                                             float scale_h, float scale_w, float* __restrict__ minmax) {
  extern __shared__ float lds[];   // fh * fw source values
  __shared__ float red[8];
  const int tid = threadIdx.x, c = blockIdx.x, fhw = fh * fw;
  for (int i = tid; i < fhw; i += NT) lds[i] = fmap[(size_t)c * fhw + i];
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY;
  for (int y = tid >> 6; y < H; y += NT / 64)
    for (int x = tid & 63; x < W; x += 64) {
      const float v = bilerp(lds, make_tap(y, x, fh, fw, scale_h, scale_w));
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  block_minmax(mn, mx, red);
  if (tid == 0) { minmax[2 * c] = mn; minmax[2 * c + 1] = mx; }
}

// grid = (pixel tiles of NT * PPT, groups of G output rows).  A thread fixes its PPT pixels (taps + the three image values)
// once and walks the group's channels; per channel and colour plane it stores once.  The pixels of a thread and the store are
// perturb_tile.h's.  The loads are not: there is one image and no baseline, it is read once for all the group's channels, by
// clamped dwords also under VEC (only `out` must be aligned), and the value is a product, not a blend.  Rows n .. n_pad of the
// chunk are written as zeros.
template <bool VEC>
__global__ __launch_bounds__(NT) void scorecam_mask_kernel(const float* __restrict__ fmap, const float* __restrict__ minmax,
                                                           const float* __restrict__ image, int fh, int fw, int H, int W,
                                                           float scale_h, float scale_w, int c0, int n, int n_pad, int G,
                                                           float* __restrict__ out) {
  extern __shared__ float lds[];   // live * fh * fw source values, then (min, max - min) per channel
  const int tid = threadIdx.x, fhw = fh * fw, HW = H * W;
  const int j0 = blockIdx.y * G, rows = min(G, n_pad - j0), live = max(0, min(rows, n - j0));
  float* mm = lds + G * fhw;
  for (int i = tid; i < live * fhw; i += NT) lds[i] = fmap[(size_t)(c0 + j0) * fhw + i];
  for (int i = tid; i < live; i += NT) {
    const float mn = minmax[2 * (c0 + j0 + i)], mx = minmax[2 * (c0 + j0 + i) + 1];
    mm[2 * i] = mn;
    mm[2 * i + 1] = mx - mn;
  }
  __syncthreads();

  int p[PPT];
  Tap tap[PPT];
  float img[3][PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    p[k] = tile_pixel<VEC, NT, PPT>(blockIdx.x, tid, k);
    const int pc = min(p[k], HW - 1);          // a pixel past the end computes on the last one and is never stored
    const int y = pc / W, x = pc - y * W;
    tap[k] = make_tap(y, x, fh, fw, scale_h, scale_w);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) img[ch][k] = image[(size_t)ch * HW + pc];
  }

  for (int jj = 0; jj < rows; ++jj) {
    const bool is_live = jj < live;
    const float mn = is_live ? mm[2 * jj] : 0.f, range = is_live ? mm[2 * jj + 1] : 0.f;
    float cam[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) cam[k] = range != 0.f ? (bilerp(lds + jj * fhw, tap[k]) - mn) / range : 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float* dst = out + ((size_t)(j0 + jj) * 3 + ch) * HW;
      float v[PPT];
#pragma unroll
      for (int k = 0; k < PPT; ++k) v[k] = is_live ? img[ch][k] * cam[k] : 0.f;
      tile_store<VEC>(dst, 0, p, HW, v);
    }
  }
}

// One pixel per thread; the channels stream through LDS in blocks of CB (source tile, min, max - min, score per channel) and
// are accumulated in ascending order, multiply and add rounded separately.  Writes relu(sum).
__global__ __launch_bounds__(NT) void scorecam_combine_kernel(const float* __restrict__ fmap, const float* __restrict__ minmax,
                                                              const float* __restrict__ scores, int C, int fh, int fw, int H,
                                                              int W, float scale_h, float scale_w, int CB,
                                                              float* __restrict__ heat) {
  extern __shared__ float lds[];   // CB * fh * fw source values, then (min, max - min, score) per channel
  const int tid = threadIdx.x, fhw = fh * fw, HW = H * W;
  float* meta = lds + CB * fhw;
  const int p = blockIdx.x * NT + tid, pc = min(p, HW - 1);
  const int y = pc / W, x = pc - y * W;
  const Tap tap = make_tap(y, x, fh, fw, scale_h, scale_w);
  float acc = 0.f;
  for (int cb = 0; cb < C; cb += CB) {
    const int nc = min(CB, C - cb);
    __syncthreads();
    for (int i = tid; i < nc * fhw; i += NT) lds[i] = fmap[(size_t)cb * fhw + i];
    for (int i = tid; i < nc; i += NT) {
      const float mn = minmax[2 * (cb + i)], mx = minmax[2 * (cb + i) + 1];
      meta[3 * i] = mn;
      meta[3 * i + 1] = mx - mn;
      meta[3 * i + 2] = scores[cb + i];
    }
    __syncthreads();
    for (int i = 0; i < nc; ++i) {
      const float mn = meta[3 * i], range = meta[3 * i + 1], s = meta[3 * i + 2];
      const float cam = range != 0.f ? (bilerp(lds + i * fhw, tap) - mn) / range : 0.f;
      const float term = s * cam;
      acc = acc + term;
    }
  }
  if (p < HW) heat[p] = acc < 0.f ? 0.f : acc;
}

// One workgroup: global min / max of the [H, W] map, then (heat - min) / (max - min) in place.  No zero guard, as in the
// reference (ScoreCam.py:154): a flat combined map comes back as NaN.
__global__ __launch_bounds__(1024) void scorecam_normalise_kernel(float* __restrict__ heat, int HW) {
  __shared__ float red[32];
  const int tid = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < HW; i += 1024) {
    const float v = heat[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((tid & 63) == 0) { red[tid >> 6] = mn; red[16 + (tid >> 6)] = mx; }
  __syncthreads();
  mn = red[0]; mx = red[16];
  for (int w = 1; w < 16; ++w) { mn = fminf(mn, red[w]); mx = fmaxf(mx, red[16 + w]); }
  const float range = mx - mn;
  for (int i = tid; i < HW; i += 1024) heat[i] = (heat[i] - mn) / range;
}

// shape checks shared by the three entry points (before anything is launched)
int check_shape(const char* who, int C, int fh, int fw, int H, int W) {
  ARG_CHECK(C >= 1 && fh >= 1 && fw >= 1 && H >= 1 && W >= 1, "%s: every extent must be >= 1 (C %d, map %dx%d, image %dx%d)", who, C,
            fh, fw, H, W);
  ARG_CHECK(H >= fh && W >= fw, "%s: the image (%dx%d) must be at least as large as the feature map (%dx%d)", who, H, W, fh, fw);
  ARG_CHECK((int64_t)H * W <= (1 << 28) && C <= (1 << 20), "%s: image %dx%d or %d channels out of range", who, H, W, C);
  if ((int64_t)fh * fw + 2 * MASK_G > LDS_FLOATS) {
    mmskin_set_error("%s: a %dx%d feature map does not fit the kernels' LDS tile (%d floats)", who, fh, fw, LDS_FLOATS - 2 * MASK_G);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_scorecam_minmax(const float* fmap, int C, int fh, int fw, int H, int W, float* minmax, void* stream) {
  if (int rc = check_shape("scorecam_minmax", C, fh, fw, H, W)) return rc;
  ARG_CHECK(fmap && minmax, "scorecam_minmax: null argument");
  hipLaunchKernelGGL(scorecam_minmax_kernel, dim3(C), dim3(NT), (size_t)fh * fw * sizeof(float), ST(stream), fmap, fh, fw, H, W,
                     (float)fh / (float)H, (float)fw / (float)W, minmax);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_scorecam_mask(const float* fmap, const float* minmax, const float* image, int C, int fh, int fw, int H, int W,
                                    int c0, int n, int n_pad, float* out, void* stream) {
  if (int rc = check_shape("scorecam_mask", C, fh, fw, H, W)) return rc;
  ARG_CHECK(n >= 1 && n <= n_pad, "scorecam_mask: %d channels do not fit a chunk padded to %d", n, n_pad);
  ARG_CHECK(c0 >= 0 && (int64_t)c0 + n <= C, "scorecam_mask: channels %d .. %d are outside the %d of the feature map", c0, c0 + n, C);
  ARG_CHECK(fmap && minmax && image && out, "scorecam_mask: null argument");
  const int HW = H * W, fhw = fh * fw;
  const int G = min(MASK_G, (LDS_FLOATS - 2 * MASK_G) / fhw);   // >= 1: check_shape bounds fhw
  ARG_CHECK(ceil_div(n_pad, G) <= 65535, "scorecam_mask: a chunk of %d is too large for a %dx%d map", n_pad, fh, fw);
  const dim3 grid(ceil_div(HW, NT * PPT), ceil_div(n_pad, G));
  const size_t lds = (size_t)(G * fhw + 2 * G) * sizeof(float);
  const float sh = (float)fh / (float)H, sw = (float)fw / (float)W;
  const bool vec = HW % PPT == 0 && ((uintptr_t)out % 16) == 0;
  if (vec)
    hipLaunchKernelGGL(scorecam_mask_kernel<true>, grid, dim3(NT), lds, ST(stream), fmap, minmax, image, fh, fw, H, W, sh, sw, c0, n,
                       n_pad, G, out);
  else
    hipLaunchKernelGGL(scorecam_mask_kernel<false>, grid, dim3(NT), lds, ST(stream), fmap, minmax, image, fh, fw, H, W, sh, sw, c0, n,
                       n_pad, G, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_scorecam_combine(const float* fmap, const float* minmax, const float* scores, int C, int fh, int fw, int H,
                                       int W, int channel_block, float* heat, void* stream) {
  if (int rc = check_shape("scorecam_combine", C, fh, fw, H, W)) return rc;
  ARG_CHECK(channel_block >= 0, "scorecam_combine: channel block %d", channel_block);
  ARG_CHECK(fmap && minmax && scores && heat, "scorecam_combine: null argument");
  const int HW = H * W, fhw = fh * fw;
  const int fit = LDS_FLOATS / (fhw + 3);                        // >= 1: check_shape bounds fhw
  const int CB = min(min(channel_block ? channel_block : fit, fit), C);
  hipLaunchKernelGGL(scorecam_combine_kernel, dim3(ceil_div(HW, NT)), dim3(NT), (size_t)CB * (fhw + 3) * sizeof(float), ST(stream),
                     fmap, minmax, scores, C, fh, fw, H, W, (float)fh / (float)H, (float)fw / (float)W, CB, heat);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(scorecam_normalise_kernel, dim3(1), dim3(1024), 0, ST(stream), heat, HW);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
