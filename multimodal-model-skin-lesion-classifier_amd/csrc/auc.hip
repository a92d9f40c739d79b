// One-vs-rest AUC of an evaluation pass as exact integer counts: probs [N][C] fp32 (the rows EpochMeter.probs collected) and
// labels int64 [N] in, one int64 block { pos[C], neg[C], wins2[C], nan } out (layout and contract: include/mmskin.h).
//
//   formula    auc[c] = wins2[c] / (2 pos[c] neg[c]) with wins2[c] = sum over (i of class c, j of another class) of
//              2 [p[i][c] > p[j][c]] + [p[i][c] == p[j][c]]: the Mann-Whitney statistic, which is the area under the ROC
//              curve by trapezoids with ties at half weight (sklearn's roc_auc_score).  Everything is an integer, so the result
//              does not depend on the grid or on the order in which the workgroups arrive.
//   pairs      row i is positive for exactly ONE class, y_i, so the thread that owns row i compares p[i][y_i] with
//              p[j][y_i] for every j whose label differs: N^2 compares, not N^2 C.
//   geometry   workgroup (bx, by) owns the 256 rows i of block bx (one per thread) and the j rows of chunk by; the chunks split
//              the j range so that a few thousand workgroups exist at any N.  The j rows are staged tile by tile in LDS with all
//              C columns (a flat, coalesced copy: the rows of a tile are contiguous); the tile height follows from C.  In the
//              compare loop the lanes of a wave read one tile row at their own column y_i: equal columns broadcast, different
//              columns of one row are different banks up to C = 32.  Labels sit beside the tile as int32, -1 for a label
//              outside [0, C), and are read four at a time.
//   totals     a thread's count stays in registers; at the end it goes to its class's 64-bit LDS cell, and the workgroup
//              issues one 64-bit global atomicAdd per class it touched.  The workgroups of block row bx == 0 see every j row
//              exactly once: they also build the class histogram of their chunk (pos, neg = valid rows - pos) and count the
//              NaN entries of the valid rows.
#include "../../include/mmskin.h"
#include "auc_pairs.h"
#include "common.h"

namespace {

constexpr int NT = 256;                  // threads per workgroup = rows i per workgroup
constexpr int TILE_FLOATS = 8192;        // 32 KiB of staged probabilities
constexpr int MAX_TJ = 256;              // tile height for C <= 32
constexpr int MAX_C = 1024;
constexpr int TARGET_WGS = 2048;         // 8 per CU

typedef unsigned long long u64;

// rows of a tile: a multiple of 4 (the compare loop reads four labels at once) with tile_rows(C) * C <= TILE_FLOATS
inline int tile_rows(int C) {
  const int fit = (TILE_FLOATS / C) & ~3;
  return fit < MAX_TJ ? fit : MAX_TJ;    // C = 1024: 8
}

__global__ __launch_bounds__(NT) void ovr_auc_counts_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, int N, int C,
                                                            int TJ, int64_t chunk, u64* __restrict__ out) {
  __shared__ float s_tile[TILE_FLOATS];
  __shared__ __attribute__((aligned(16))) int32_t s_lab[MAX_TJ];
  __shared__ int32_t s_hist[MAX_C];
  __shared__ u64 s_wins[MAX_C];
  __shared__ int32_t s_valid;
  const int tid = threadIdx.x;
  const bool census = blockIdx.x == 0;                             // this workgroup also counts pos / neg / nan of its chunk
  const int64_t jbeg = blockIdx.y * chunk, jend = min(jbeg + chunk, (int64_t)N);   // chunk is a multiple of TJ; jbeg < N by the grid

  for (int c = tid; c < C; c += NT) { s_hist[c] = 0; s_wins[c] = 0; }
  if (tid == 0) s_valid = 0;

  const int64_t i = (int64_t)blockIdx.x * NT + tid;
  int yi = -1;
  float si = 0.f;
  if (i < N) {
    const int64_t y = labels[i];
    if (y >= 0 && y < C) { yi = (int)y; si = probs[i * C + y]; }
  }
  const int col = yi < 0 ? 0 : yi;                                 // a thread without a row reads column 0 and counts nothing

  u64 wins = 0, nans = 0;
  int32_t valid_rows = 0;
  for (int64_t j0 = jbeg; j0 < jend; j0 += TJ) {
    const int rows = (int)min((int64_t)TJ, jend - j0);
    __syncthreads();                                               // the previous tile is consumed (first pass: the cells are zero)
    for (int r = tid; r < TJ; r += NT) {                           // every slot up to TJ: the slots past `rows` hold -1
      int32_t y32 = -1;
      if (r < rows) {
        const int64_t y = labels[j0 + r];
        if (y >= 0 && y < C) {
          y32 = (int32_t)y;
          if (census) { atomicAdd(&s_hist[y32], 1); ++valid_rows; }
        }
      }
      s_lab[r] = y32;
    }
    const float* src = probs + j0 * C;
    const int elems = rows * C;                                    // <= TILE_FLOATS
    for (int e = tid; e < elems; e += NT) s_tile[e] = src[e];
    __syncthreads();
    if (census)
      for (int e = tid; e < elems; e += NT) {
        const float v = s_tile[e];
        if (v != v && s_lab[e / C] >= 0) ++nans;
      }
    if (yi >= 0) {
      int32_t a = 0;                                               // at most 2 * MAX_TJ per tile
      const int rows4 = (rows + 3) & ~3;                           // <= TJ; rows past `rows` carry label -1, whatever the tile holds there
      for (int r = 0; r < rows4; r += 4) {
        const int4 yj = *reinterpret_cast<const int4*>(&s_lab[r]);
        const int32_t ys[4] = {yj.x, yj.y, yj.z, yj.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = s_tile[(r + k) * C + col];               // (r + k) < TJ, col < C: inside TJ * C <= TILE_FLOATS
          const int32_t w = auc_wins2(si, v);                      // a NaN on either side: 0
          a += (ys[k] >= 0 && ys[k] != yi) ? w : 0;
        }
      }
      wins += (u64)a;
    }
  }

  if (yi >= 0 && wins) atomicAdd(&s_wins[yi], wins);
  if (valid_rows) atomicAdd(&s_valid, valid_rows);
  __syncthreads();
  for (int c = tid; c < C; c += NT)
    if (s_wins[c]) atomicAdd(&out[2 * (int64_t)C + c], s_wins[c]);
  if (!census) return;

  const int32_t total = s_valid;                                   // valid rows of the chunk: a negative for every class but their own
  for (int c = tid; c < C; c += NT) {
    const int32_t p = s_hist[c];
    if (p) atomicAdd(&out[c], (u64)p);
    if (total - p) atomicAdd(&out[(int64_t)C + c], (u64)(total - p));
  }
  if (nans) atomicAdd(&out[3 * (int64_t)C], nans);
}

}  // namespace

extern "C" int mmskin_ovr_auc_counts(const float* probs, const int64_t* labels, int64_t N, int C, int64_t* counts, void* stream) {
  ARG_CHECK(C >= 2 && C <= MAX_C, "ovr_auc_counts: %d classes; the kernel holds 2 .. %d", C, MAX_C);
  ARG_CHECK(N >= 1 && N < ((int64_t)1 << 31), "ovr_auc_counts: %lld rows is outside 1 .. 2^31 - 1", (long long)N);
  ARG_CHECK(probs && labels && counts, "ovr_auc_counts: null argument");
  HIP_CHECK_RET(hipMemsetAsync(counts, 0, (3 * (size_t)C + 1) * sizeof(int64_t), ST(stream)));
  const int TJ = tile_rows(C);
  const int64_t iblocks = (N + NT - 1) / NT, tiles = (N + TJ - 1) / TJ;
  int64_t chunks = (TARGET_WGS + iblocks - 1) / iblocks;           // enough chunks for TARGET_WGS workgroups, at most one per tile
  if (chunks > tiles) chunks = tiles;
  const int64_t chunk = (tiles + chunks - 1) / chunks * TJ;        // rows per chunk: whole tiles
  chunks = (N + chunk - 1) / chunk;                                // <= TARGET_WGS: inside the grid's y range
  hipLaunchKernelGGL(ovr_auc_counts_kernel, dim3((unsigned)iblocks, (unsigned)chunks), dim3(NT), 0, ST(stream), probs, labels, (int)N, C, TJ,
                     chunk, (u64*)counts);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
