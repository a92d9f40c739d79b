// Faithfulness scores of a saliency map (mmskin.faithfulness.CamFaithfulness): deletion and insertion curves (Petsiuk et al.,
// RISE) and average drop / increase in confidence (Chattopadhay et al., Grad-CAM++), batched.  Four forward-only kernels around
// the chunked model forwards, as scorecam.hip is built around Score-CAM's:
//
//   rank     rank[n, p] = #{q : s[n,q] > s[n,p]} + #{q < p : s[n,q] == s[n,p]}: descending saliency, ties by ascending pixel
//            index, -0 == +0, a NaN below every number and NaNs tied among themselves.  Computed as that definition, by pair
//            counting over an order-preserving 32-bit key: every pixel's rank is a sum of integer compares against all pixels
//            of its image, staged through LDS.  No sort network, no scatter, no atomics: the result is a function of the input
//            alone.  H * W = 50176 costs 2.5e9 compare-and-adds per image, tens of microseconds of the chip beside forwards that
//            take milliseconds; the cap of 65536 pixels keeps it there.
//   blur     separable Gaussian with reflect padding, fp32, horizontal then vertical, taps in ascending order, every product and
//            sum rounded on its own.  The taps come from the host (fp64, normalised, rounded to fp32): no device exp.
//   mean     per-plane mean: fp64 partial sums of a fixed stride, a fixed tree, rounded to fp32 once and written over the plane.
//   perturb  one chunk of model inputs [n_pad, 3, H, W]: per row (image, k, mode) a pure select between image and baseline by
//            rank < (k * H * W) / S (deletion, insertion), or b + h * (x - b) with h = saliency clamped to [0, 1] (explanation).
//   curves   soft-max probability of the target class of every row in fp64, trapezoid areas, average drop, increase, and the
//            dataset means, all in a fixed order.
//
// tests/faithfulness_oracle.py restates each kernel in its operation order and the kernels match it bit for bit (curves: to
// 1e-12, the fp64 exp), so contraction into FMAs is switched off for this file.
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

#include "perturb_tile.h"   // tile_pixel / tile_store / blend, shared with rise.hip; compiled here with contraction off
#include "target_prob.h"    // pick_target / row_probability / TARGET_MAX_CLASSES, shared with rise.hip

namespace {

constexpr int NT = 256;                   // threads per workgroup
constexpr int PPT = 4;                    // perturb: pixels per thread (one 16-byte store per colour plane)
constexpr int MAX_PIXELS = 65536;         // rank / perturb: H * W (256 x 256)
constexpr int MAX_STEPS = 1024;           // perturb / curves: S
constexpr int RANK_TILE = 2048;           // rank: keys staged per round, a multiple of NT
constexpr int BLUR_T = 32;                // blur: output tile edge
constexpr int BLUR_MAX_R = 15;            // blur: ksize <= 31
constexpr int BLUR_IN = BLUR_T + 2 * BLUR_MAX_R;

// Descending saliency == descending key.  NaN -> 0, below the key of -inf (0x007fffff); -0 and +0 -> 0x80000000.
__device__ __forceinline__ uint32_t rank_key(float s) {
  const uint32_t u = __float_as_uint(s);
  if (s != s) return 0u;
  if ((u << 1) == 0u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// grid = (blocks of NT pixels p, images).  A thread owns one pixel p and walks every pixel q of its image through LDS tiles;
// the lanes read the same tile words (broadcast), four keys per read.  Tiles and blocks are NT-aligned, so a tile lies wholly
// below the block's pixels (q < p: count key_q >= key_p), wholly above (q > p: count key_q > key_p), or holds them (both rules
// by index).  Slots past the image hold key 0 with q > p: never counted.
__global__ __launch_bounds__(NT) void faith_rank_kernel(const float* __restrict__ sal, int HW, int32_t* __restrict__ rank) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[RANK_TILE];
  const int tid = threadIdx.x, pb = blockIdx.x * NT, p = pb + tid;
  const float* s = sal + (size_t)blockIdx.y * HW;
  const uint32_t kp = rank_key(s[min(p, HW - 1)]);     // a thread past the end computes on the last pixel and stores nothing
  int cnt = 0;
  for (int t0 = 0; t0 < HW; t0 += RANK_TILE) {
    __syncthreads();
    for (int i = tid; i < RANK_TILE; i += NT) tile[i] = t0 + i < HW ? rank_key(s[t0 + i]) : 0u;
    __syncthreads();
    const int lim = min(RANK_TILE, (HW - t0 + 3) & ~3);
    if (t0 + RANK_TILE <= pb) {
#pragma unroll 4
      for (int i = 0; i < lim; i += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(&tile[i]);
        cnt += (int)(k.x >= kp) + (int)(k.y >= kp) + (int)(k.z >= kp) + (int)(k.w >= kp);
      }
    } else if (t0 >= pb + NT) {
#pragma unroll 4
      for (int i = 0; i < lim; i += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(&tile[i]);
        cnt += (int)(k.x > kp) + (int)(k.y > kp) + (int)(k.z > kp) + (int)(k.w > kp);
      }
    } else {
      const int pl = p - t0;                            // the thread's own slot in this tile
#pragma unroll 4
      for (int i = 0; i < lim; i += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(&tile[i]);
        cnt += (int)(k.x > kp || (k.x == kp && i < pl)) + (int)(k.y > kp || (k.y == kp && i + 1 < pl)) +
               (int)(k.z > kp || (k.z == kp && i + 2 < pl)) + (int)(k.w > kp || (k.w == kp && i + 3 < pl));
      }
    }
  }
  if (p < HW) rank[(size_t)blockIdx.y * HW + p] = cnt;
}

struct BlurTaps { float w[2 * BLUR_MAX_R + 1]; };

// index i of an axis of n samples under reflect padding (no edge repeat), for -r <= i <= n - 1 + r with r < n; an index further
// out (a tile row or column past the image, whose outputs are never stored) is clamped into the axis
__device__ __forceinline__ int reflect_index(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// grid = (column tiles, row tiles, planes).  The tile and its halo of r samples are staged in LDS once; the horizontal pass
// writes (BLUR_T + 2 r) rows of BLUR_T sums back to LDS; the vertical pass reads those.
__global__ __launch_bounds__(NT) void faith_blur_kernel(const float* __restrict__ x, int H, int W, BlurTaps taps, int r,
                                                        float* __restrict__ out) {
  __shared__ float s_in[BLUR_IN][BLUR_IN + 1];
  __shared__ float s_h[BLUR_IN][BLUR_T + 1];
  __shared__ float s_w[2 * BLUR_MAX_R + 1];
  const int tid = threadIdx.x, ks = 2 * r + 1, ext = BLUR_T + 2 * r;
  const int x0 = blockIdx.x * BLUR_T, y0 = blockIdx.y * BLUR_T;
  const float* src = x + (size_t)blockIdx.z * H * W;
  if (tid < ks) s_w[tid] = taps.w[tid];
  for (int i = tid; i < ext * ext; i += NT) {
    const int ly = i / ext, lx = i - ly * ext;
    s_in[ly][lx] = src[(size_t)reflect_index(y0 + ly - r, H) * W + reflect_index(x0 + lx - r, W)];
  }
  __syncthreads();
  for (int i = tid; i < ext * BLUR_T; i += NT) {
    const int ly = i / BLUR_T, ox = i - ly * BLUR_T;
    float acc = 0.f;
    for (int t = 0; t < ks; ++t) {
      const float term = s_w[t] * s_in[ly][ox + t];
      acc = acc + term;
    }
    s_h[ly][ox] = acc;
  }
  __syncthreads();
  for (int i = tid; i < BLUR_T * BLUR_T; i += NT) {
    const int oy = i / BLUR_T, ox = i - oy * BLUR_T;
    float acc = 0.f;
    for (int t = 0; t < ks; ++t) {
      const float term = s_w[t] * s_h[oy + t][ox];
      acc = acc + term;
    }
    if (y0 + oy < H && x0 + ox < W) out[(size_t)blockIdx.z * H * W + (size_t)(y0 + oy) * W + x0 + ox] = acc;
  }
}

// fixed-order fp64 sum over a workgroup: red[tid] holds the thread's partial; the tree halves NT; every thread gets the total.
// Not uncertainty.hip's block_sum_f64, which adds wave totals: the orders differ, so the two do not merge bitwise.
__device__ __forceinline__ double block_tree_sum(double* red, int tid) {
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// One workgroup per plane: thread t adds samples t, t + NT, ... in fp64, the partials meet in a fixed tree, and the mean
// (one fp64 division, one rounding to fp32) is written over the whole output plane.
__global__ __launch_bounds__(NT) void faith_mean_kernel(const float* __restrict__ x, int HW, float* __restrict__ out) {
  __shared__ double red[NT];
  const int tid = threadIdx.x;
  const float* src = x + (size_t)blockIdx.x * HW;
  double acc = 0.0;
  for (int i = tid; i < HW; i += NT) acc = acc + (double)src[i];
  red[tid] = acc;
  const float m = (float)(block_tree_sum(red, tid) / (double)HW);
  float* dst = out + (size_t)blockIdx.x * HW;
  for (int i = tid; i < HW; i += NT) dst[i] = m;
}

enum { MODE_DELETION = 0, MODE_INSERTION = 1, MODE_EXPLANATION = 2 };

// grid = (pixel tiles of NT * PPT, rows of the chunk).  The row's (image, k, mode) entry is the same for the whole workgroup and
// is clamped to what exists: a bad entry reads the nearest image, step or mode, never other memory.  The pixels of a
// thread, the store and the blend are perturb_tile.h's, which describes VEC; the guarded loads are written out here (see there).
// This kernel's own: the rank test, which selects, and the clamped saliency that the explanation row blends with.  Rows n ..
// n_pad are zeros.
template <bool VEC>
__global__ __launch_bounds__(NT) void faith_perturb_kernel(const float* __restrict__ images, const float* __restrict__ baseline,
                                                           const int32_t* __restrict__ rank, const float* __restrict__ sal,
                                                           const int32_t* __restrict__ rows, int N, int HW, int S, int n,
                                                           float* __restrict__ out) {
  const int tid = threadIdx.x, j = blockIdx.y;
  int p[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) p[k] = tile_pixel<VEC, NT, PPT>(blockIdx.x, tid, k);
  float* dst = out + (size_t)j * 3 * HW;
  const bool live = j < n;
  int img = 0, mode = MODE_DELETION, count = 0;
  if (live) {
    img = min(max(rows[3 * j], 0), N - 1);
    const int k = min(max(rows[3 * j + 1], 0), S);
    mode = min(max(rows[3 * j + 2], 0), (int)MODE_EXPLANATION);
    count = (int)(((int64_t)k * HW) / S);
  }
  bool take_base[PPT];       // deletion / insertion: the pixel comes from the baseline
  float h[PPT];              // explanation: the saliency clamped to [0, 1] (a NaN clamps to 0)
  if (live) {
    const int32_t* rk = rank + (size_t)img * HW;
    const float* sl = sal + (size_t)img * HW;
    int32_t r[PPT];
    float s[PPT];
    if (VEC) {
      if (p[0] < HW) {
        const int4 rv = *reinterpret_cast<const int4*>(rk + p[0]);
        const float4 sv = *reinterpret_cast<const float4*>(sl + p[0]);
        r[0] = rv.x; r[1] = rv.y; r[2] = rv.z; r[3] = rv.w;
        s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
      } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) { r[k] = 0; s[k] = 0.f; }
      }
    } else {
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int pc = min(p[k], HW - 1);
        r[k] = rk[pc];
        s[k] = sl[pc];
      }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      take_base[k] = (r[k] < count) == (mode == MODE_DELETION);
      h[k] = fminf(fmaxf(s[k], 0.f), 1.f);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[PPT] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float* xs = images + ((size_t)img * 3 + ch) * HW;
      const float* bs = baseline + ((size_t)img * 3 + ch) * HW;
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
      for (int k = 0; k < PPT; ++k) {
        if (mode == MODE_EXPLANATION) {
          v[k] = blend(bv[k], xv[k], h[k]);
        } else {
          v[k] = take_base[k] ? bv[k] : xv[k];
        }
      }
    }
    tile_store<VEC>(dst, (size_t)ch * HW, p, HW, v);
  }
}

// One workgroup per image.  Rows of image n in `logits`: n * P + k deletion step k, n * P + S + 1 + k insertion step k,
// n * P + 2 S + 2 the explanation image, P = 2 S + 3; deletion step 0 is the clean image.  Every thread takes rows t, t + NT,
// ...: the soft-max probability of the target class in fp64 (target_prob.h).
// Three threads of three different waves then form the areas and the two confidence scores, each a serial loop in ascending k.
__global__ __launch_bounds__(NT) void faith_curves_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target_in,
                                                          int N, int S, int C, double* __restrict__ curves,
                                                          double* __restrict__ scalars, int32_t* __restrict__ target_out) {
  __shared__ double s_p[2 * MAX_STEPS + 3];
  __shared__ int s_target;
  const int tid = threadIdx.x, n = blockIdx.x, P = 2 * S + 3;
  const float* rows = logits + (size_t)n * P * C;
  if (tid == 0) {
    const int t = pick_target(rows, C, target_in, n);    // on the clean row
    s_target = t;
    target_out[n] = t;
  }
  __syncthreads();
  const int target = s_target;
  for (int t = tid; t < P; t += NT) s_p[t] = row_probability(rows + (size_t)t * C, C, target);
  __syncthreads();
  for (int t = tid; t < 2 * (S + 1); t += NT) {
    const int which = t / (S + 1), k = t - which * (S + 1);
    curves[((size_t)which * N + n) * (S + 1) + k] = s_p[t];
  }
  if (tid == 0 || tid == 64) {                           // trapezoids over x = k / S: (sum of (c[k] + c[k + 1])) * 0.5 / S
    const double* c = s_p + (tid == 0 ? 0 : S + 1);
    double acc = 0.0;
    for (int k = 0; k < S; ++k) acc = acc + (c[k] + c[k + 1]);
    scalars[(size_t)(tid == 0 ? 0 : 1) * N + n] = acc * 0.5 / (double)S;
  }
  if (tid == 128) {
    const double p = s_p[0], pe = s_p[2 * S + 2];
    scalars[(size_t)2 * N + n] = fmax(0.0, p - pe) / p;
    scalars[(size_t)3 * N + n] = pe > p ? 1.0 : 0.0;
  }
}

// One workgroup: the dataset means of the four per-image scalars, each by strided fp64 partials and the fixed tree.
__global__ __launch_bounds__(NT) void faith_means_kernel(const double* __restrict__ scalars, int N, double* __restrict__ means) {
  __shared__ double red[NT];
  const int tid = threadIdx.x;
  for (int j = 0; j < 4; ++j) {
    double acc = 0.0;
    for (int i = tid; i < N; i += NT) acc = acc + scalars[(size_t)j * N + i];
    __syncthreads();                                     // the previous round's red[0] has been read by every thread
    red[tid] = acc;
    const double total = block_tree_sum(red, tid);
    if (tid == 0) means[j] = total / (double)N;
  }
}

int check_pixels(const char* who, int N, int64_t HW) {
  ARG_CHECK(N >= 1 && HW >= 1, "%s: every extent must be >= 1 (%d images of %lld pixels)", who, N, (long long)HW);
  ARG_CHECK(N <= 65535, "%s: %d images is outside 1 .. 65535", who, N);
  if (HW > MAX_PIXELS) {
    mmskin_set_error("%s: %lld pixels per image is above the cap of %d (256 x 256)", who, (long long)HW, MAX_PIXELS);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int mmskin_faith_max_pixels(void) { return MAX_PIXELS; }

extern "C" int mmskin_faith_rank(const float* saliency, int N, int HW, int32_t* rank, void* stream) {
  if (int rc = check_pixels("faith_rank", N, HW)) return rc;
  ARG_CHECK(saliency && rank, "faith_rank: null argument");
  hipLaunchKernelGGL(faith_rank_kernel, dim3(ceil_div(HW, NT), N), dim3(NT), 0, ST(stream), saliency, HW, rank);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_faith_blur(const float* x, int planes, int H, int W, const float* taps, int ksize, float* out, void* stream) {
  ARG_CHECK(planes >= 1 && H >= 1 && W >= 1, "faith_blur: every extent must be >= 1 (%d planes of %dx%d)", planes, H, W);
  ARG_CHECK(planes <= 65535 && H <= (1 << 16) && W <= (1 << 16), "faith_blur: %d planes of %dx%d out of range", planes, H, W);
  ARG_CHECK(ksize >= 1 && (ksize & 1) == 1 && ksize <= 2 * BLUR_MAX_R + 1, "faith_blur: ksize %d must be odd and at most %d", ksize,
            2 * BLUR_MAX_R + 1);
  ARG_CHECK(ksize / 2 < min(H, W), "faith_blur: reflect padding of %d is undefined on a %dx%d image", ksize / 2, H, W);
  ARG_CHECK(x && taps && out, "faith_blur: null argument");
  BlurTaps t;
  for (int i = 0; i < 2 * BLUR_MAX_R + 1; ++i) t.w[i] = i < ksize ? taps[i] : 0.f;       // taps is HOST memory
  hipLaunchKernelGGL(faith_blur_kernel, dim3(ceil_div(W, BLUR_T), ceil_div(H, BLUR_T), planes), dim3(NT), 0, ST(stream), x, H, W, t,
                     ksize / 2, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_faith_mean(const float* x, int planes, int HW, float* out, void* stream) {
  ARG_CHECK(planes >= 1 && HW >= 1, "faith_mean: every extent must be >= 1 (%d planes of %d samples)", planes, HW);
  ARG_CHECK(HW <= (1 << 28), "faith_mean: %d samples per plane out of range", HW);
  ARG_CHECK(x && out, "faith_mean: null argument");
  hipLaunchKernelGGL(faith_mean_kernel, dim3(planes), dim3(NT), 0, ST(stream), x, HW, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_faith_perturb(const float* images, const float* baseline, const int32_t* rank, const float* saliency,
                                    const int32_t* rows, int N, int H, int W, int S, int n, int n_pad, float* out, void* stream) {
  ARG_CHECK(H >= 1 && W >= 1, "faith_perturb: every extent must be >= 1 (image %dx%d)", H, W);
  if (int rc = check_pixels("faith_perturb", N, (int64_t)H * W)) return rc;
  const int HW = H * W;
  ARG_CHECK(S >= 1 && S <= MAX_STEPS && S <= HW, "faith_perturb: %d steps is outside 1 .. min(%d, H * W = %d)", S, MAX_STEPS, HW);
  ARG_CHECK(n >= 1 && n <= n_pad, "faith_perturb: %d rows do not fit a chunk padded to %d", n, n_pad);
  ARG_CHECK(n_pad <= 65535, "faith_perturb: a chunk of %d is outside 1 .. 65535", n_pad);
  ARG_CHECK(images && baseline && rank && saliency && rows && out, "faith_perturb: null argument");
  const dim3 grid(ceil_div(HW, NT * PPT), n_pad);
  const bool vec = HW % PPT == 0 && aligned16(images) && aligned16(baseline) && aligned16(rank) && aligned16(saliency) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(faith_perturb_kernel<true>, grid, dim3(NT), 0, ST(stream), images, baseline, rank, saliency, rows, N, HW, S, n, out);
  else
    hipLaunchKernelGGL(faith_perturb_kernel<false>, grid, dim3(NT), 0, ST(stream), images, baseline, rank, saliency, rows, N, HW, S, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_faith_curves(const float* logits, const int32_t* target, int N, int S, int C, double* curves, double* scalars,
                                   double* means, int32_t* target_out, void* stream) {
  ARG_CHECK(N >= 1 && C >= 1, "faith_curves: every extent must be >= 1 (%d images, %d classes)", N, C);
  ARG_CHECK(N <= (1 << 20) && C <= TARGET_MAX_CLASSES, "faith_curves: %d images or %d classes out of range", N, C);
  ARG_CHECK(S >= 1 && S <= MAX_STEPS, "faith_curves: %d steps is outside 1 .. %d", S, MAX_STEPS);
  ARG_CHECK(logits && curves && scalars && means && target_out, "faith_curves: null argument");
  hipLaunchKernelGGL(faith_curves_kernel, dim3(N), dim3(NT), 0, ST(stream), logits, target, N, S, C, curves, scalars, target_out);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(faith_means_kernel, dim3(1), dim3(NT), 0, ST(stream), scalars, N, means);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
