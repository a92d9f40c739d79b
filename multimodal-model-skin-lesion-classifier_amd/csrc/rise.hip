// RISE saliency (Petsiuk et al., 2018; mmskin.rise.RISE): the image is masked with many random smooth masks, the model runs on
// every masked image, and the masks are averaged with the target-class probability as their weight.  Model-agnostic and
// forward-only, so it explains the encoders the CAM classes cannot hook.  A mask is a pure function of (seed, mask index, pixel),
// stated in include/mmskin.h; every kernel here evaluates it in registers and no mask tensor exists in HBM:
//
//   masks       materialises masks j0 .. j0 + n - 1 (tests, drawing; not on the hot path)
//   apply       one chunk of model inputs [n_pad, 3, H, W]: row r = (image r / n_masks, mask r % n_masks),
//               baseline + m * (image - baseline); the three colour planes of a pixel share one mask evaluation
//   accumulate  after all forwards: the target class and clean probability of every image, the fp64 soft-max weight w[n][j] of
//               every row, the cell table of every mask (80 bytes each, in the workspace), then
//               saliency_sum[n][p] = sum_j w[n][j] m_j(p) and coverage[p] = sum_j m_j(p) in ascending j, fp64, one owner per
//               output element, no atomics: bitwise repeatable.
//
// A mask's state is an "entry" of 20 words: word r <= g holds row r of its (g + 1) x (g + 1) binary cell grid as a bit mask,
// words 17 and 18 its shift (dy, dx).  A pixel needs two row words and four bit tests; the division by the cell size is done
// once per pixel (at shift 0), the shift only adds to the remainder and carries at most one cell.
//
// tests/rise_oracle.py restates every kernel in its operation order, so contraction into FMAs is switched off for this file.
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

#include "perturb_tile.h"   // tile_pixel / tile_store / blend, shared with faithfulness.hip; compiled here with contraction off
#include "target_prob.h"    // pick_target / row_probability / TARGET_MAX_CLASSES, shared with faithfulness.hip

namespace {

constexpr int NT = 256;                   // threads per workgroup
constexpr int PPT = 4;                    // apply: pixels per thread (one 16-byte store per colour plane)
constexpr int MAX_GRID = 16;
constexpr int MAX_CELLS = (MAX_GRID + 1) * (MAX_GRID + 1);
constexpr int ENTRY = 20;                 // words of a mask's entry: MAX_GRID + 1 rows, dy, dx, one of padding
constexpr int E_DY = 17, E_DX = 18;
constexpr int MAX_MASKS = 1 << 20;
constexpr int NI = 4;                     // accumulate: images per workgroup (fp64 accumulators per thread, plus the coverage)
constexpr int MB = 32;                    // accumulate: masks staged in LDS per round

struct Geom {
  int H, W, g, ch, cw;
  uint32_t thr;                           // a cell is on iff the top 24 bits of its word are below thr = round(p1 * 2^24)
  uint64_t key;                           // mix64(seed)
  float den;                              // 4 ch cw: exact in fp32 (at most 4 * 65536)
};

__device__ __forceinline__ uint64_t rise_word(uint64_t key, int j, int q) { return mix64(key ^ ((uint64_t)j * 1024u + (uint64_t)q)); }

// The entry of mask j into s_e[ENTRY], by the whole workgroup: every cell's bit by its own thread, then one thread per word.
// Two barriers; every thread of the workgroup must call it.
__device__ __forceinline__ void stage_entry(const Geom& q, int j, uint8_t* s_bit, uint32_t* s_e, int tid) {
  const int g1 = q.g + 1;
  for (int c = tid; c < g1 * g1; c += NT) s_bit[c] = (uint32_t)(rise_word(q.key, j, c) >> 40) < q.thr ? 1 : 0;
  __syncthreads();
  if (tid < ENTRY) {
    uint32_t v = 0;
    if (tid < g1) {
      for (int c = 0; c < g1; ++c) v |= (uint32_t)s_bit[tid * g1 + c] << c;
    } else if (tid == E_DY) {
      v = (uint32_t)(((rise_word(q.key, j, 1022) >> 32) * (uint64_t)q.ch) >> 32);
    } else if (tid == E_DX) {
      v = (uint32_t)(((rise_word(q.key, j, 1023) >> 32) * (uint64_t)q.cw) >> 32);
    }
    s_e[tid] = v;
  }
  __syncthreads();
}

// One axis of a pixel at shift 0: t = 2 c + 1 - size, i = floor(t / (2 size)) (-1 when t < 0, since t > -2 size), r = t - i * 2 size
struct Axis { int i, r; };
__device__ __forceinline__ Axis axis_of(int c, int size) {
  const int t = 2 * c + 1 - size;
  Axis a;
  a.i = t >= 0 ? t / (2 * size) : -1;
  a.r = t - a.i * 2 * size;
  return a;
}

// m of the pixel (ay, ax) under entry e (LDS or registers): the shift adds 2 d < 2 size to the remainder: at most one carry.
__device__ __forceinline__ float mask_value(const uint32_t* e, Axis ay, Axis ax, const Geom& q) {
  const int ch2 = 2 * q.ch, cw2 = 2 * q.cw;
  int ry = ay.r + 2 * (int)e[E_DY], iy = ay.i;
  if (ry >= ch2) { ry -= ch2; ++iy; }
  int rx = ax.r + 2 * (int)e[E_DX], ix = ax.i;
  if (rx >= cw2) { rx -= cw2; ++ix; }
  const int iy0 = min(max(iy, 0), q.g), iy1 = min(max(iy + 1, 0), q.g);
  const int ix0 = min(max(ix, 0), q.g), ix1 = min(max(ix + 1, 0), q.g);
  const uint32_t r0 = e[iy0], r1 = e[iy1];
  const int g00 = (r0 >> ix0) & 1, g01 = (r0 >> ix1) & 1, g10 = (r1 >> ix0) & 1, g11 = (r1 >> ix1) & 1;
  const int num = (ch2 - ry) * ((cw2 - rx) * g00 + rx * g01) + ry * ((cw2 - rx) * g10 + rx * g11);
  return __fdiv_rn((float)num, q.den);
}

// grid = (blocks of NT pixels, masks)
__global__ __launch_bounds__(NT) void rise_masks_kernel(Geom q, int j0, float* __restrict__ out) {
  __shared__ uint8_t s_bit[MAX_CELLS];
  __shared__ uint32_t s_e[ENTRY];
  const int tid = threadIdx.x, HW = q.H * q.W, p = blockIdx.x * NT + tid;
  stage_entry(q, j0 + (int)blockIdx.y, s_bit, s_e, tid);
  if (p < HW) {
    const int y = p / q.W, x = p - y * q.W;
    out[(size_t)blockIdx.y * HW + p] = mask_value(s_e, axis_of(y, q.ch), axis_of(x, q.cw), q);
  }
}

// grid = (pixel tiles of NT * PPT, rows of the chunk).  The pixels of a thread, the store and the blend are perturb_tile.h's,
// which describes VEC; the guarded loads are written out here (see there).  RISE's own is m: the mask of the row, evaluated
// once per pixel for the three colour planes.  Rows n .. n_pad are zeros.
template <bool VEC>
__global__ __launch_bounds__(NT) void rise_apply_kernel(const float* __restrict__ images, const float* __restrict__ baseline, Geom q,
                                                        int n_masks, int64_t r0, int n, float* __restrict__ out) {
  __shared__ uint8_t s_bit[MAX_CELLS];
  __shared__ uint32_t s_e[ENTRY];
  const int tid = threadIdx.x, row = blockIdx.y, HW = q.H * q.W;
  const bool live = row < n;                                  // the same for the whole workgroup
  int p[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) p[k] = tile_pixel<VEC, NT, PPT>(blockIdx.x, tid, k);
  float* dst = out + (size_t)row * 3 * HW;
  int img = 0;
  float m[PPT] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int64_t r = r0 + row;
    img = (int)(r / n_masks);
    stage_entry(q, (int)(r - (int64_t)img * n_masks), s_bit, s_e, tid);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int pc = min(p[k], HW - 1), y = pc / q.W, x = pc - y * q.W;
      m[k] = mask_value(s_e, axis_of(y, q.ch), axis_of(x, q.cw), q);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[PPT] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float* xs = images + ((size_t)img * 3 + c) * HW;
      const float* bs = baseline + ((size_t)img * 3 + c) * HW;
      float xv[PPT], bv[PPT];
      if (VEC) {
        if (p[0] < HW) {
          const float4 a = *reinterpret_cast<const float4*>(xs + p[0]);
          const float4 b = *reinterpret_cast<const float4*>(bs + p[0]);
          xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
          bv[0] = b.x; bv[1] = b.y; bv[2] = b.z; bv[3] = b.w;
        } else {
#pragma unroll
          for (int k = 0; k < PPT; ++k) { xv[k] = 0.f; bv[k] = 0.f; }
        }
      } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
          const int pc = min(p[k], HW - 1);
          xv[k] = xs[pc];
          bv[k] = bs[pc];
        }
      }
#pragma unroll
      for (int k = 0; k < PPT; ++k) v[k] = blend(bv[k], xv[k], m[k]);
    }
    tile_store<VEC>(dst, (size_t)c * HW, p, HW, v);
  }
}

// One thread per image: the class it is explained on and the probability of that class on the clean image.
__global__ __launch_bounds__(NT) void rise_target_kernel(const float* __restrict__ clean, const int32_t* __restrict__ target_in, int N,
                                                         int K, double* __restrict__ clean_prob, int32_t* __restrict__ target_used) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  const float* l = clean + (size_t)n * K;
  const int t = pick_target(l, K, target_in, n);
  target_used[n] = t;
  clean_prob[n] = row_probability(l, K, t);
}

// One thread per row (n, j) of the image-major row space: w[n][j]
__global__ __launch_bounds__(NT) void rise_weights_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target_used,
                                                          int64_t rows, int n_masks, int K, double* __restrict__ w) {
  const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (r >= rows) return;
  w[r] = row_probability(logits + (size_t)r * K, K, target_used[r / n_masks]);
}

// One workgroup per mask: its entry into the table
__global__ __launch_bounds__(NT) void rise_table_kernel(Geom q, uint32_t* __restrict__ table) {
  __shared__ uint8_t s_bit[MAX_CELLS];
  __shared__ uint32_t s_e[ENTRY];
  const int tid = threadIdx.x, j = blockIdx.x;
  stage_entry(q, j, s_bit, s_e, tid);
  if (tid < ENTRY) table[(size_t)j * ENTRY + tid] = s_e[tid];
}

// grid = (blocks of NT pixels, groups of NI images).  A thread owns one pixel of NI images and walks the masks in ascending j,
// MB at a time through LDS (entries and weights are copied in coalesced; the inner loop reads them at addresses that are the
// same for every lane, or -- the two row words -- differ only where the wave's pixels straddle a cell boundary: broadcasts, no
// bank conflicts).  One mask evaluation feeds NI + 1 fp64 accumulators.  Image group 0 also owns the coverage.
__global__ __launch_bounds__(NT) void rise_accumulate_kernel(const double* __restrict__ w, const uint32_t* __restrict__ table, Geom q,
                                                             int N, int n_masks, double* __restrict__ saliency_sum,
                                                             double* __restrict__ coverage) {
  __shared__ uint32_t s_e[MB * ENTRY];
  __shared__ double s_w[NI][MB];
  const int tid = threadIdx.x, HW = q.H * q.W, p = blockIdx.x * NT + tid, n0 = blockIdx.y * NI;
  const int pc = min(p, HW - 1), y = pc / q.W, x = pc - y * q.W;     // a thread past the end computes on the last pixel, stores nothing
  const Axis ay = axis_of(y, q.ch), ax = axis_of(x, q.cw);
  double acc[NI], cov = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = 0.0;
  for (int j0 = 0; j0 < n_masks; j0 += MB) {
    const int nb = min(MB, n_masks - j0);
    __syncthreads();
    for (int i = tid; i < nb * ENTRY; i += NT) s_e[i] = table[(size_t)j0 * ENTRY + i];
    for (int i = tid; i < NI * MB; i += NT) {
      const int ii = i / MB, b = i - ii * MB;
      s_w[ii][b] = (n0 + ii < N && b < nb) ? w[(size_t)(n0 + ii) * n_masks + j0 + b] : 0.0;
    }
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
      const double m = (double)mask_value(s_e + b * ENTRY, ay, ax, q);
      cov = cov + m;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const double term = s_w[i][b] * m;
        acc[i] = acc[i] + term;
      }
    }
  }
  if (p < HW) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (n0 + i < N) saliency_sum[(size_t)(n0 + i) * HW + p] = acc[i];
    if (blockIdx.y == 0) coverage[p] = cov;
  }
}

// the checks every entry point shares, and the mask geometry
int make_geom(const char* who, uint64_t seed, int grid, double p1, int H, int W, Geom* q) {
  ARG_CHECK(H >= 1 && W >= 1, "%s: every extent must be >= 1 (H = %d, W = %d)", who, H, W);
  ARG_CHECK(grid >= 2 && grid <= MAX_GRID, "%s: grid = %d is outside 2 .. %d", who, grid, MAX_GRID);
  ARG_CHECK(p1 > 0.0 && p1 < 1.0, "%s: p1 = %g is outside (0, 1)", who, p1);
  if ((int64_t)H * W > mmskin_faith_max_pixels()) {
    mmskin_set_error("%s: H * W = %lld pixels per image is above the cap of %d", who, (long long)H * W, mmskin_faith_max_pixels());
    return MMSKIN_ERR_UNSUPPORTED;
  }
  q->H = H; q->W = W; q->g = grid;
  q->ch = ceil_div(H, grid); q->cw = ceil_div(W, grid);
  q->thr = (uint32_t)floor(p1 * 16777216.0 + 0.5);
  q->key = mix64(seed);
  q->den = (float)(4 * q->ch * q->cw);
  return MMSKIN_OK;
}

int check_masks(const char* who, int n_masks) {
  ARG_CHECK(n_masks >= 1, "%s: n_masks = %d must be >= 1", who, n_masks);
  if (n_masks > MAX_MASKS) {
    mmskin_set_error("%s: n_masks = %d is above the cap of %d", who, n_masks, MAX_MASKS);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

struct Workspace { double* w; uint32_t* table; int64_t bytes; };
Workspace carve(void* base, int N, int n_masks) {
  Workspace ws;
  const int64_t w_bytes = (int64_t)N * n_masks * (int64_t)sizeof(double);
  ws.w = (double*)base;
  ws.table = (uint32_t*)((char*)base + w_bytes);
  ws.bytes = w_bytes + (int64_t)n_masks * ENTRY * (int64_t)sizeof(uint32_t);
  return ws;
}

}  // namespace

extern "C" int mmskin_rise_masks(uint64_t seed, int j0, int n, int grid, double p1, int H, int W, float* out, void* stream) {
  Geom q;
  if (int rc = make_geom("rise_masks", seed, grid, p1, H, W, &q)) return rc;
  ARG_CHECK(j0 >= 0 && n >= 1 && n <= 65535, "rise_masks: j0 = %d must be >= 0 and n = %d in 1 .. 65535", j0, n);
  if (int rc = check_masks("rise_masks", j0 > MAX_MASKS - n ? MAX_MASKS + 1 : j0 + n)) return rc;
  ARG_CHECK(out, "rise_masks: null argument");
  hipLaunchKernelGGL(rise_masks_kernel, dim3(ceil_div(H * W, NT), n), dim3(NT), 0, ST(stream), q, j0, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_rise_apply(const float* images, const float* baseline, int N, int H, int W, uint64_t seed, int grid, double p1,
                                 int n_masks, int64_t r0, int n, int n_pad, float* out, void* stream) {
  Geom q;
  if (int rc = make_geom("rise_apply", seed, grid, p1, H, W, &q)) return rc;
  ARG_CHECK(N >= 1 && N <= 65535, "rise_apply: N = %d images is outside 1 .. 65535", N);
  if (int rc = check_masks("rise_apply", n_masks)) return rc;
  ARG_CHECK(n >= 1 && n <= n_pad, "rise_apply: n = %d rows do not fit a chunk of n_pad = %d", n, n_pad);
  ARG_CHECK(n_pad <= 65535, "rise_apply: n_pad = %d is outside 1 .. 65535", n_pad);
  ARG_CHECK(r0 >= 0 && r0 + n <= (int64_t)N * n_masks, "rise_apply: rows r0 = %lld .. r0 + n = %lld are outside the %lld of N * n_masks",
            (long long)r0, (long long)(r0 + n), (long long)N * n_masks);
  ARG_CHECK(images && baseline && out, "rise_apply: null argument");
  const int HW = H * W;
  const dim3 blocks(ceil_div(HW, NT * PPT), n_pad);
  if (HW % PPT == 0 && aligned16(images) && aligned16(baseline) && aligned16(out))
    hipLaunchKernelGGL(rise_apply_kernel<true>, blocks, dim3(NT), 0, ST(stream), images, baseline, q, n_masks, r0, n, out);
  else
    hipLaunchKernelGGL(rise_apply_kernel<false>, blocks, dim3(NT), 0, ST(stream), images, baseline, q, n_masks, r0, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int64_t mmskin_rise_workspace_bytes(int N, int n_masks) {
  if (N < 1 || N > 65535 || n_masks < 1 || n_masks > MAX_MASKS) return -1;
  return carve(nullptr, N, n_masks).bytes;
}

extern "C" int mmskin_rise_accumulate(const float* logits, const int32_t* target, const float* clean_logits, int N, int K, int H, int W,
                                      uint64_t seed, int grid, double p1, int n_masks, double* saliency_sum, double* coverage,
                                      double* clean_prob, int32_t* target_used, void* workspace, void* stream) {
  Geom q;
  if (int rc = make_geom("rise_accumulate", seed, grid, p1, H, W, &q)) return rc;
  ARG_CHECK(N >= 1 && N <= 65535, "rise_accumulate: N = %d images is outside 1 .. 65535", N);
  ARG_CHECK(K >= 1 && K <= TARGET_MAX_CLASSES, "rise_accumulate: K = %d classes is outside 1 .. %d", K, TARGET_MAX_CLASSES);
  if (int rc = check_masks("rise_accumulate", n_masks)) return rc;
  ARG_CHECK(logits && clean_logits && saliency_sum && coverage && clean_prob && target_used && workspace,
            "rise_accumulate: null argument");
  ARG_CHECK(((uintptr_t)workspace % 8) == 0, "rise_accumulate: the workspace must be 8-byte aligned");
  const Workspace ws = carve(workspace, N, n_masks);
  const int64_t rows = (int64_t)N * n_masks;
  hipLaunchKernelGGL(rise_target_kernel, dim3(ceil_div(N, NT)), dim3(NT), 0, ST(stream), clean_logits, target, N, K, clean_prob,
                     target_used);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(rise_weights_kernel, dim3((unsigned)((rows + NT - 1) / NT)), dim3(NT), 0, ST(stream), logits, target_used, rows,
                     n_masks, K, ws.w);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(rise_table_kernel, dim3(n_masks), dim3(NT), 0, ST(stream), q, ws.table);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(rise_accumulate_kernel, dim3(ceil_div(H * W, NT), ceil_div(N, NI)), dim3(NT), 0, ST(stream), ws.w, ws.table, q, N,
                     n_masks, saliency_sum, coverage);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
