// One-vs-rest ROC and precision-recall curves of an evaluation pass as exact integers: probs [N][C] fp32 and labels int64 [N] in;
// per class the distinct scores in descending order (thr) with the true- and false-positive counts at each (tp, fp), the number
// of points, pos / neg and the NaN count out; a second entry turns the integers into the fp64 summary (AUC, average precision,
// Youden's point, sensitivity at a specificity, specificity at a sensitivity).  Layout and contract: include/mmskin.h.
//
//   route      counting, no sort.  Every (row i, class c) gets four integers from one tiled pass over the rows j of column c:
//              ge_pos / ge_neg = rows of class c / of another class with s_j >= s_i (the tp and fp at threshold s_i), eq_low = rows
//              with an equal score at a lower index (the row with none represents its tie group), gt = rows with a greater score.
//              Two representatives of one class never share gt, so gt is a slot in [0, N): the representative's row index goes
//              there, and an order-preserving compaction of the occupied slots (count per 1024-slot block, scan of the block
//              counts per class, scan inside the block) yields the distinct scores in descending order.
//   geometry   count kernel: workgroup (bx, by, c) owns the 256 rows i of block bx (one per thread), the rows j of chunk by and
//              class c.  Column c of a j tile (1024 rows) is staged in LDS next to a 0 / 1 flag "label == c"; a row whose label is
//              outside [0, C) is staged as NaN, which compares false everywhere.  In the compare loop every lane of a wave reads
//              the SAME LDS address (four rows per 16-byte read): a broadcast, no bank conflict at any C.  The four counters stay
//              in registers; with one chunk they are stored, with several they meet in 32-bit integer global atomics.
//   census     the workgroups of row block bx == 0 see every (j, c) exactly once: they count pos, neg = valid - pos and the NaN
//              entries of the valid rows (64-bit integer atomics, one per workgroup and cell).
//   exactness  integers and copies of fp32 inputs only, so nothing depends on the grid, the chunking or the arrival order.
#include "../../include/mmskin.h"
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int NT = 256;                  // threads per workgroup of the counting and compaction kernels
constexpr int TJ = 1024;                 // rows of a staged column tile: 4 KiB of scores + 4 KiB of flags
constexpr int MAX_C = 1024;
constexpr int TARGET_WGS = 2048;         // 8 per CU
constexpr int SLOTS = 4;                 // consecutive slots per thread in the compaction
constexpr int SCAN_TILE = NT * SLOTS;    // slots per compaction workgroup
constexpr int SUM_NT = 512;              // threads of the summary workgroup (one per class)
constexpr int MAX_OPS = 1 + 2 * MMSKIN_CURVES_MAX_OPERATING_POINTS;   // Youden + the requested operating points

typedef unsigned long long u64;

struct Scratch {
  int32_t *slot, *ge_pos, *ge_neg, *eq_low, *gt, *block_count;
  size_t bytes;
};

// the one carve: run on a null base it sizes the workspace (mmskin_ovr_curves_scratch_ints)
Scratch carve(void* base, int64_t N, int C) {
  Carver cv(base);
  Scratch s;
  const size_t cells = (size_t)N * (size_t)C, blocks = (size_t)((N + SCAN_TILE - 1) / SCAN_TILE) * (size_t)C;
  s.slot = cv.take<int32_t>(cells);
  s.ge_pos = cv.take<int32_t>(cells);
  s.ge_neg = cv.take<int32_t>(cells);
  s.eq_low = cv.take<int32_t>(cells);
  s.gt = cv.take<int32_t>(cells);
  s.block_count = cv.take<int32_t>(blocks);
  s.bytes = cv.cur;
  return s;
}

bool in_range(int64_t N, int C) { return C >= 2 && C <= MAX_C && N >= 1 && N < ((int64_t)1 << 31); }

__global__ __launch_bounds__(NT) void curve_counts_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, int N, int C,
                                                          int64_t chunk, int single, int32_t* __restrict__ ge_pos,
                                                          int32_t* __restrict__ ge_neg, int32_t* __restrict__ eq_low,
                                                          int32_t* __restrict__ gt, u64* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) float s_val[TJ];
  __shared__ __attribute__((aligned(16))) int32_t s_pos[TJ];
  __shared__ u64 s_census[3];
  const int tid = threadIdx.x, c = blockIdx.z;
  const bool census = blockIdx.x == 0;                             // this workgroup also counts pos / neg / nan of its (chunk, class)
  const int64_t jbeg = blockIdx.y * chunk, jend = min(jbeg + chunk, (int64_t)N);   // chunk is a multiple of TJ; jbeg < N by the grid
  if (tid < 3) s_census[tid] = 0;

  const int64_t i = (int64_t)blockIdx.x * NT + tid;
  float si = NAN;                                                  // a thread without a valid row compares false everywhere
  if (i < N) {
    const int64_t y = labels[i];
    if (y >= 0 && y < C) si = probs[i * C + c];
  }

  int32_t n_ge = 0, n_ge_pos = 0, n_eq = 0, n_eq_low = 0;          // each at most N < 2^31
  uint32_t c_pos = 0, c_valid = 0, c_nan = 0;
  for (int64_t j0 = jbeg; j0 < jend; j0 += TJ) {
    const int rows = (int)min((int64_t)TJ, jend - j0);
    __syncthreads();                                               // the previous tile is consumed
    for (int r = tid; r < TJ; r += NT) {                           // every slot up to TJ: the slots past `rows` hold NaN
      float v = NAN;
      int32_t p = 0;
      if (r < rows) {
        const int64_t y = labels[j0 + r];
        if (y >= 0 && y < C) {
          v = probs[(j0 + r) * C + c];
          p = y == c;
          if (census) { ++c_valid; c_pos += p; c_nan += v != v; }
        }
      }
      s_val[r] = v;
      s_pos[r] = p;
    }
    __syncthreads();
    const int64_t below = i - j0;                                  // the tile rows r < below lie at a lower index than i
    const int lim = below > TJ ? TJ : (below < 0 ? 0 : (int)below);
    const int rows4 = (rows + 3) & ~3;                             // <= TJ
    for (int r = 0; r < rows4; r += 4) {
      const float4 v4 = *reinterpret_cast<const float4*>(&s_val[r]);
      const int4 p4 = *reinterpret_cast<const int4*>(&s_pos[r]);
      const float vs[4] = {v4.x, v4.y, v4.z, v4.w};
      const int32_t ps[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ge = vs[k] >= si, eq = vs[k] == si;             // a NaN on either side: neither
        n_ge += ge;
        n_ge_pos += ge ? ps[k] : 0;
        n_eq += eq;
        n_eq_low += (eq && r + k < lim);
      }
    }
  }

  if (i < N) {
    const int64_t at = (int64_t)c * N + i;
    const int32_t n_ge_neg = n_ge - n_ge_pos, n_gt = n_ge - n_eq;
    if (single) {                                                  // the only chunk: every cell is written, nothing was zeroed
      ge_pos[at] = n_ge_pos; ge_neg[at] = n_ge_neg; eq_low[at] = n_eq_low; gt[at] = n_gt;
    } else {                                                       // partial counts of several chunks meet here
      if (n_ge_pos) atomicAdd(&ge_pos[at], n_ge_pos);
      if (n_ge_neg) atomicAdd(&ge_neg[at], n_ge_neg);
      if (n_eq_low) atomicAdd(&eq_low[at], n_eq_low);
      if (n_gt) atomicAdd(&gt[at], n_gt);
    }
  }
  if (!census) return;                                             // uniform per workgroup
  if (c_pos) atomicAdd(&s_census[0], (u64)c_pos);
  if (c_valid - c_pos) atomicAdd(&s_census[1], (u64)(c_valid - c_pos));
  if (c_nan) atomicAdd(&s_census[2], (u64)c_nan);
  __syncthreads();
  if (tid < 3 && s_census[tid]) atomicAdd(&counts[tid == 0 ? c : (tid == 1 ? C + c : 2 * C)], s_census[tid]);
}

// the representative of every tie group puts its row index + 1 into the slot `gt` of its class (zero = empty)
__global__ __launch_bounds__(NT) void curve_scatter_kernel(int N, const int32_t* __restrict__ ge_pos, const int32_t* __restrict__ ge_neg,
                                                           const int32_t* __restrict__ eq_low, const int32_t* __restrict__ gt,
                                                           int32_t* __restrict__ slot) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)blockIdx.y * N, at = row + i;
  const bool counted = ge_pos[at] + ge_neg[at] > 0;                // a valid row with a score that is no NaN is >= itself
  const int32_t g = gt[at];
  if (counted && eq_low[at] == 0 && g >= 0 && g < N) slot[row + g] = (int32_t)(i + 1);
}

// exclusive scan of one int per thread over the workgroup; `total` = the sum.  s_w: NT / 64 ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int32_t* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                                 // an earlier use of s_w is over
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < w) base += s_w[k];
    total += s_w[k];
  }
  return base + inc - v;
}

__device__ __forceinline__ int load_slots(const int32_t* __restrict__ slot, int64_t row, int64_t p0, int N, int32_t (&mine)[SLOTS]) {
  int n = 0;
#pragma unroll
  for (int q = 0; q < SLOTS; ++q) {
    mine[q] = p0 + q < N ? slot[row + p0 + q] : 0;
    n += mine[q] != 0;
  }
  return n;
}

__global__ __launch_bounds__(NT) void curve_block_count_kernel(int N, int blocks, const int32_t* __restrict__ slot,
                                                               int32_t* __restrict__ block_count) {
  __shared__ int32_t s_w[NT / 64];
  int32_t mine[SLOTS];
  const int n = load_slots(slot, (int64_t)blockIdx.y * N, (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SLOTS, N, mine);
  int total;
  block_exclusive_scan(n, s_w, total);
  if (threadIdx.x == 0) block_count[(int64_t)blockIdx.y * blocks + blockIdx.x] = total;
}

// one workgroup per class: the block counts become their exclusive prefix, the total is n_points[c]
__global__ __launch_bounds__(NT) void curve_block_scan_kernel(int blocks, int32_t* __restrict__ block_count, int32_t* __restrict__ n_points) {
  __shared__ int32_t s_w[NT / 64];
  int32_t* mine = block_count + (int64_t)blockIdx.x * blocks;
  int running = 0;
  for (int b0 = 0; b0 < blocks; b0 += NT) {
    const int b = b0 + threadIdx.x;
    const int v = b < blocks ? mine[b] : 0;
    int total;
    const int before = block_exclusive_scan(v, s_w, total);
    if (b < blocks) mine[b] = running + before;
    running += total;
  }
  if (threadIdx.x == 0) n_points[blockIdx.x] = running;
}

// the occupied slots of a block, in order, go to the points [base, base + count) of their class; every point at or past
// n_points[c] is zeroed by the thread that owns the slot of the same number
__global__ __launch_bounds__(NT) void curve_compact_kernel(const float* __restrict__ probs, int N, int C, int blocks,
                                                           const int32_t* __restrict__ slot, const int32_t* __restrict__ block_base,
                                                           const int32_t* __restrict__ n_points, const int32_t* __restrict__ ge_pos,
                                                           const int32_t* __restrict__ ge_neg, float* __restrict__ thr,
                                                           int32_t* __restrict__ tp, int32_t* __restrict__ fp) {
  __shared__ int32_t s_w[NT / 64];
  const int c = blockIdx.y;
  const int64_t row = (int64_t)c * N, p0 = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SLOTS;
  int32_t mine[SLOTS];
  const int n = load_slots(slot, row, p0, N, mine);
  int total;
  int dst = block_base[(int64_t)c * blocks + blockIdx.x] + block_exclusive_scan(n, s_w, total);
  const int points = n_points[c];
#pragma unroll
  for (int q = 0; q < SLOTS; ++q) {
    if (mine[q] != 0 && dst < N) {                                 // dst < points <= N by the scan
      const int64_t i = (int64_t)mine[q] - 1;
      thr[row + dst] = probs[i * C + c];
      tp[row + dst] = ge_pos[row + i];
      fp[row + dst] = ge_neg[row + i];
      ++dst;
    }
    const int64_t p = p0 + q;
    if (p < N && p >= points) { thr[row + p] = 0.f; tp[row + p] = 0; fp[row + p] = 0; }
  }
}

// ------------------------------------------------------------------------------------------------ the summary
// a candidate point: the larger `a` wins, on equal `a` the smaller index (the first point in threshold-descending order)
struct Best {
  long long a;
  int k;
};
__device__ __forceinline__ void take_better(Best& x, long long a, int k) {
  if (a > x.a || (a == x.a && k < x.k)) { x.a = a; x.k = k; }
}

__global__ __launch_bounds__(SUM_NT) void curve_summary_kernel(const float* __restrict__ thr, const int32_t* __restrict__ tp,
                                                               const int32_t* __restrict__ fp, const int32_t* __restrict__ n_points,
                                                               const int64_t* __restrict__ counts, int N, int C,
                                                               const double* __restrict__ spec, int A, const double* __restrict__ sens,
                                                               int B, double* __restrict__ summary) {
  constexpr int WAVES = SUM_NT / 64;
  __shared__ long long s_a[MAX_OPS][WAVES];
  __shared__ int s_k[MAX_OPS][WAVES];
  __shared__ double s_ap[WAVES];
  __shared__ u64 s_area[WAVES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ops = 1 + A + B, S = 5 + 3 * (A + B);
  double* out = summary + (int64_t)c * S;
  const long long pos = counts[c], neg = counts[C + c];
  if (pos == 0 || neg == 0) {                                      // uniform per workgroup: the curve of this class is undefined
    for (int s = tid; s < S; s += SUM_NT) out[s] = NAN;
    return;
  }
  const double dpos = (double)pos, dneg = (double)neg;
  const int64_t row = (int64_t)c * N;
  int points = n_points[c];
  points = points < 0 ? 0 : (points > N ? N : points);

  double bound[MAX_OPS];                                           // the right-hand side of the admission test of every op
#pragma unroll
  for (int o = 1; o < MAX_OPS; ++o) bound[o] = o <= A ? spec[o - 1] * dneg : (o < ops ? sens[o - 1 - A] * dpos : 0.0);
  Best best[MAX_OPS];
#pragma unroll
  for (int o = 0; o < MAX_OPS; ++o) best[o] = {LLONG_MIN, INT_MAX};
  double ap = 0.0;
  u64 area = 0;
  for (int k = tid; k < points; k += SUM_NT) {
    const long long tpk = tp[row + k], fpk = fp[row + k];
    const long long tpp = k ? tp[row + k - 1] : 0, fpp = k ? fp[row + k - 1] : 0;
    area += (u64)(fpk - fpp) * (u64)(tpk + tpp);
    if (tpk != tpp) ap += ((double)(tpk - tpp) / dpos) * ((double)tpk / (double)(tpk + fpk));
    take_better(best[0], tpk * neg - fpk * pos, k);                // Youden's J as the exact integer numerator over pos neg
#pragma unroll
    for (int o = 1; o < MAX_OPS; ++o) {
      if (o <= A) {
        if ((double)(neg - fpk) >= bound[o]) take_better(best[o], tpk, k);
      } else if (o < ops) {
        if ((double)tpk >= bound[o]) take_better(best[o], -fpk, k);
      }
    }
  }

  // the lanes of a wave by a butterfly, then the waves in order: a fixed order for the one floating-point sum
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    ap += __shfl_xor(ap, d, 64);
    area += __shfl_xor(area, d, 64);
  }
#pragma unroll
  for (int o = 0; o < MAX_OPS; ++o) {
    if (o < ops) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const long long a = __shfl_xor(best[o].a, d, 64);
        const int k = __shfl_xor(best[o].k, d, 64);
        take_better(best[o], a, k);
      }
      if (lane == 0) { s_a[o][w] = best[o].a; s_k[o][w] = best[o].k; }
    }
  }
  if (lane == 0) { s_ap[w] = ap; s_area[w] = area; }
  __syncthreads();

  if (tid == 0) {
    double total = 0.0;
    u64 wins2 = 0;
    for (int v = 0; v < WAVES; ++v) { total += s_ap[v]; wins2 += s_area[v]; }
    out[0] = (double)(long long)wins2 / (2.0 * dpos * dneg);
    out[1] = total;
  }
  if (tid < ops) {
    Best b = {LLONG_MIN, INT_MAX};
    for (int v = 0; v < WAVES; ++v) take_better(b, s_a[tid][v], s_k[tid][v]);
    const bool none = b.k == INT_MAX;
    double value, at, index;
    if (tid == 0) {
      value = none ? NAN : (double)b.a / (dpos * dneg);
      at = none ? NAN : (double)thr[row + b.k];
      index = none ? NAN : (double)b.k;
    } else if (tid <= A) {                                         // no admissible point: the (0, 0) start of the curve
      value = none ? 0.0 : (double)b.a / dpos;
      at = none ? INFINITY : (double)thr[row + b.k];
      index = none ? -1.0 : (double)b.k;
    } else {
      value = none ? NAN : (double)(neg + b.a) / dneg;
      at = none ? NAN : (double)thr[row + b.k];
      index = none ? -1.0 : (double)b.k;
    }
    double* cell = out + 2 + 3 * tid;
    cell[0] = value; cell[1] = at; cell[2] = index;
  }
}

}  // namespace

extern "C" int64_t mmskin_ovr_curves_scratch_ints(int64_t N, int C) {
  if (!in_range(N, C)) return -1;
  return (int64_t)(carve(nullptr, N, C).bytes / sizeof(int32_t));
}

extern "C" int mmskin_ovr_curves_summary_columns(int n_spec, int n_sens) {
  if (n_spec < 0 || n_spec > MMSKIN_CURVES_MAX_OPERATING_POINTS || n_sens < 0 || n_sens > MMSKIN_CURVES_MAX_OPERATING_POINTS) return -1;
  return 5 + 3 * (n_spec + n_sens);
}

extern "C" int mmskin_ovr_curves(const float* probs, const int64_t* labels, int64_t N, int C, int32_t* scratch, float* thr, int32_t* tp,
                                 int32_t* fp, int32_t* n_points, int64_t* counts, void* stream) {
  ARG_CHECK(C >= 2 && C <= MAX_C, "ovr_curves: %d classes; the kernel holds 2 .. %d", C, MAX_C);
  ARG_CHECK(N >= 1 && N < ((int64_t)1 << 31), "ovr_curves: %lld rows is outside 1 .. 2^31 - 1", (long long)N);
  ARG_CHECK(probs && labels && scratch && thr && tp && fp && n_points && counts, "ovr_curves: null argument");
  const Scratch s = carve(scratch, N, C);
  const int64_t iblocks = (N + NT - 1) / NT, tiles = (N + TJ - 1) / TJ, per_chunk = iblocks * C;
  int64_t chunks = (TARGET_WGS + per_chunk - 1) / per_chunk;       // enough chunks for TARGET_WGS workgroups, at most one per tile
  if (chunks > tiles) chunks = tiles;
  const int64_t chunk = (tiles + chunks - 1) / chunks * TJ;        // rows per chunk: whole tiles
  chunks = (N + chunk - 1) / chunk;                                // <= TARGET_WGS: inside the grid's y range
  const int single = chunks == 1;
  // the slots always start empty; the four counters only where several chunks add into them (they follow the slots in the carve)
  const size_t zeroed = (size_t)((unsigned char*)(single ? (void*)s.ge_pos : (void*)s.block_count) - (unsigned char*)scratch);
  HIP_CHECK_RET(hipMemsetAsync(scratch, 0, zeroed, ST(stream)));
  HIP_CHECK_RET(hipMemsetAsync(counts, 0, (2 * (size_t)C + 1) * sizeof(int64_t), ST(stream)));
  hipLaunchKernelGGL(curve_counts_kernel, dim3((unsigned)iblocks, (unsigned)chunks, (unsigned)C), dim3(NT), 0, ST(stream), probs, labels,
                     (int)N, C, chunk, single, s.ge_pos, s.ge_neg, s.eq_low, s.gt, (u64*)counts);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(curve_scatter_kernel, dim3((unsigned)iblocks, (unsigned)C), dim3(NT), 0, ST(stream), (int)N, s.ge_pos, s.ge_neg, s.eq_low,
                     s.gt, s.slot);
  HIP_CHECK_RET(hipGetLastError());
  const int blocks = (int)((N + SCAN_TILE - 1) / SCAN_TILE);
  hipLaunchKernelGGL(curve_block_count_kernel, dim3((unsigned)blocks, (unsigned)C), dim3(NT), 0, ST(stream), (int)N, blocks, s.slot,
                     s.block_count);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(curve_block_scan_kernel, dim3((unsigned)C), dim3(NT), 0, ST(stream), blocks, s.block_count, n_points);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(curve_compact_kernel, dim3((unsigned)blocks, (unsigned)C), dim3(NT), 0, ST(stream), probs, (int)N, C, blocks, s.slot,
                     s.block_count, n_points, s.ge_pos, s.ge_neg, thr, tp, fp);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_ovr_curves_summary(const float* thr, const int32_t* tp, const int32_t* fp, const int32_t* n_points,
                                         const int64_t* counts, int64_t N, int C, const double* specificities, int n_spec,
                                         const double* sensitivities, int n_sens, double* summary, void* stream) {
  ARG_CHECK(C >= 2 && C <= MAX_C, "ovr_curves_summary: %d classes; the kernel holds 2 .. %d", C, MAX_C);
  ARG_CHECK(N >= 1 && N < ((int64_t)1 << 31), "ovr_curves_summary: %lld rows is outside 1 .. 2^31 - 1", (long long)N);
  ARG_CHECK(n_spec >= 0 && n_spec <= MMSKIN_CURVES_MAX_OPERATING_POINTS && n_sens >= 0 && n_sens <= MMSKIN_CURVES_MAX_OPERATING_POINTS,
            "ovr_curves_summary: %d specificities and %d sensitivities; a call holds 0 .. %d operating points of each kind", n_spec, n_sens,
            MMSKIN_CURVES_MAX_OPERATING_POINTS);
  ARG_CHECK(thr && tp && fp && n_points && counts && summary && (specificities || !n_spec) && (sensitivities || !n_sens),
            "ovr_curves_summary: null argument");
  hipLaunchKernelGGL(curve_summary_kernel, dim3((unsigned)C), dim3(SUM_NT), 0, ST(stream), thr, tp, fp, n_points, counts, (int)N, C,
                     specificities, n_spec, sensitivities, n_sens, summary);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
