// Device functions the kernels share that write one chunk of perturbed model inputs [rows, 3, H, W] (rise.hip's apply,
// faithfulness.hip's perturb, scorecam.hip's mask): the pixel tile of a workgroup and the blend.
//
// A workgroup of NT threads owns NT * PPT pixels of one row of the chunk; a thread owns PPT of them, the same in every
// colour plane.  VEC: the PPT pixels are consecutive, base + tid * PPT + k, and the thread moves them as one vector of PPT
// words per plane (the caller launches VEC only where H * W is a multiple of PPT and every plane it touches is aligned to
// that vector); otherwise pixel k is base + k * NT + tid and the accesses are coalesced words.  A pixel past the end of the
// plane is never stored: VEC loads zeros for it (the vector is whole or absent), non-VEC loads the last pixel.
//
// The guarded loads themselves stay written out in rise.hip and faithfulness.hip: taken from here as an inlined function, in
// any of the forms tried (two planes side by side, one plane at a time), they changed the schedule of the four chunk writers
// and cost rise_apply_kernel<false> three VGPRs (profiles/perturb_tile_resources.txt).
//
// NT and PPT are the including file's own constants and arrive as template arguments.  Whether the blend's multiply and add
// are contracted into an FMA is the including file's choice too (all three switch it off before they include this).
#pragma once
#include "common.h"

// pixel k of thread tid in tile number `tile` of the plane
template <bool VEC, int NT, int PPT>
__device__ __forceinline__ int tile_pixel(int tile, int tid, int k) {
  const int base = tile * (NT * PPT);
  return VEC ? base + tid * PPT + k : base + k * NT + tid;
}

// the thread's PPT values into the plane of HW samples that starts `off` samples into dst
template <bool VEC, int PPT>
__device__ __forceinline__ void tile_store(float* dst, size_t off, const int (&p)[PPT], int HW, const float (&v)[PPT]) {
  if (VEC) {
    static_assert(PPT == 4, "VEC moves a thread's pixels as one 4-word vector");
    if (p[0] < HW) *reinterpret_cast<float4*>(dst + off + p[0]) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < PPT; ++k)
      if (p[k] < HW) dst[off + p[k]] = v[k];
  }
}

// b + m * (x - b) in the difference form: x == b comes back exactly, whatever m is (unless it is NaN or infinite)
__device__ __forceinline__ float blend(float b, float x, float m) {
  const float d = x - b;
  const float t = m * d;
  return b + t;
}
