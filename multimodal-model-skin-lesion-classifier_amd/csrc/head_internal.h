// What head.hip and linear.hip share: the library-owned scratch buffer, the two reduction launchers whose kernels live in
// linear.hip, and the launch-grid helpers.
#pragma once
#include "common.h"

// These three cross the two files but not the library's boundary: hidden, so the exported symbol set stays the C ABI plus what it was.
#define HEAD_INTERNAL __attribute__((visibility("hidden")))
// Library-owned scratch for split reductions and bf16 GEMM operands (defined in linear.hip, next to the slot rule).
HEAD_INTERNAL float* head_scratch(size_t bytes, int slot = 0);
// out[c] = sum_r part[r][c] for c < ncols; columns < split go to out0, the rest to out1 (either may be null)
HEAD_INTERNAL int rows_sum(const float* part, int R, int ncols, int split, float* out0, float* out1, hipStream_t st);
// out[0..1] = sums of the nb pairs part[2 i], part[2 i + 1], in a fixed order (the StarReLU scalar gradients)
HEAD_INTERNAL int star_pair_sum(const float* part, int nb, float* out, hipStream_t st);

// 256-thread blocks for a grid-stride loop over n elements.  Pointwise ops: at most 4096 blocks, a few passes per thread
static inline int grid1d(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}
// conversion / pad / un-pad passes over GEMM operands (n > 0 chunks of 8 or 16 bytes): one chunk per thread up to 2^20 blocks
static inline unsigned grid1d_wide(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b > 1048576 ? 1048576 : b);
}
