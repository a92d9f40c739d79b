// What ops.hip and bn.hip share: the element-wise launch grid and the geometry / block reducer of the column-sum producers
// (column_stats, bn_bwd_reduce, slice_stats, the stem's backward sums), which leave the per-workgroup fp32 partial rows that bn.hip's
// finalize kernels reduce.
#pragma once
#include "ops.h"

#define EW_BLOCK 256
static inline int ew_grid(size_t work_items) {
  size_t b = (work_items + EW_BLOCK - 1) / EW_BLOCK;
  // One 16-byte chunk per thread, no grid-stride cap in practice: on MI355X a 2-reads-1-write pass over 1.2 GB ran at
  // 4.9 TB/s with 4 096 workgroups and 5.9 TB/s with 65 536 (scripts/bench/membench.hip) -- many short workgroups
  // keep more loads in flight than few long-running ones.
  if (b > (size_t)1 << 20) b = (size_t)1 << 20;
  if (b < 1) b = 1;
  return (int)b;
}

// ------------------------------------------------------------------ column reduction geometry
struct ColGeom {
  int CPR;   // 16-byte chunks per row
  int CW;    // chunk columns per block
  int RL;    // row lanes per block
  int RB;    // rows per block
  int gx, gy;
};
static inline ColGeom col_geom(size_t rows, int C, int EPC) {
  ColGeom g;
  g.CPR = C / EPC;
  g.CW = g.CPR >= 256 ? 256 : g.CPR;
  g.RL = 256 / g.CW;
  size_t rb = (rows + 1023) / 1024;
  if (rb < (size_t)g.RL * 4) rb = (size_t)g.RL * 4;
  rb = (rb + g.RL - 1) / g.RL * g.RL;
  g.RB = (int)rb;
  g.gx = (int)((rows + rb - 1) / rb);
  g.gy = (g.CPR + g.CW - 1) / g.CW;
  return g;
}

// Reduce NQ per-thread EPC-wide accumulators over the row lanes of a block and write them to
// partial[(blockIdx.x*NQ + q)*C + channel].
template <int EPC, int NQ>
__device__ __forceinline__ void block_col_reduce(float (&acc)[NQ][EPC], int cx, int ry, int CW, int RL,
                                                 int col, int CPR, int C, float* partial, float* red) {
  // red: [NQ][RL][CW*EPC]
  const bool active = ry < RL;
  if (active) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int e = 0; e < EPC; ++e) red[(q * RL + ry) * CW * EPC + cx * EPC + e] = acc[q][e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NQ * CW * EPC; i += blockDim.x) {
    int q = i / (CW * EPC), ce = i - q * CW * EPC;
    int ch = blockIdx.y * CW * EPC + ce;
    if (ch < C) {
      float s = 0.f;
      for (int r = 0; r < RL; ++r) s += red[(q * RL + r) * CW * EPC + ce];
      partial[((size_t)blockIdx.x * NQ + q) * C + ch] = s;
    }
  }
}
