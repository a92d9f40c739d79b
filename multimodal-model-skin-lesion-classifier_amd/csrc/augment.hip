// Training-time image augmentation (the train half of the input side): the A.Compose of
// skinLesionDatasets.py:74-113 -- Rotate(45, BORDER_REFLECT), HorizontalFlip, VerticalFlip, GaussianBlur, CoarseDropout,
// HueSaturationValue, RandomBrightnessContrast -- as ONE kernel on the raw uint8 NHWC batch.  The random draws are made on
// the host (mmskin.preprocess.TrainAugment.sample) into one mmskin_augment_params record per sample (include/mmskin.h); the
// kernel is a pure function of (src, table): no atomics, no dependence on launch order.
//
// A workgroup owns a 32x32 output tile.  It gathers the geometric stage (rotate, then the flips as index permutations) for
// the tile plus the blur's halo into LDS, blurs from LDS (horizontal pass to 16 bits, vertical pass per output pixel), runs
// dropout, HSV and brightness/contrast in registers and stores each uint8 once.  The halo is gathered again by the
// neighbouring tiles (1.4x at 7 taps) -- cheaper than a second trip through HBM.
//
// Every stage follows the published algorithm of the OpenCV 8-bit path albumentations calls (fixed-point warpAffine
// INTER_LINEAR, fixed-point GaussianBlur, integer RGB2HSV with 12-bit division tables, float HSV2RGB) and albumentations
// 1.4.18's LUTs.  cv2 and albumentations are not installed in the build container, so this is "parity unpinned" against cv2
// itself, like mmskin_resize_u8; tests/augment_oracle.py restates the same algorithms in numpy and the kernel matches it bit
// for bit.  Wherever a float rounding decides a uint8 (HSV2RGB, the brightness LUT, the float64 coordinate terms) every
// multiply and add rounds on its own: contraction into FMAs is switched off for this file (the one v_fma_f32 left in the ISA is
// the compiler's exact expansion of round_div's integer division).
#include "../../include/mmskin.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;             // output tile edge
constexpr int RMAX = 3;              // largest blur radius (7 taps)
constexpr int GP = TILE + 2 * RMAX;  // LDS pitch of the gathered tile, in pixels
static_assert(sizeof(mmskin_augment_params) == 160, "table record layout is part of the ABI (include/mmskin.h)");

// cv2 borderInterpolate in closed form (the loop form is in the restatement): any index, any length >= 1
__device__ __forceinline__ int reflect(int p, int n) {       // BORDER_REFLECT      fedcba|abcdefgh|hgfedcb
  if ((unsigned)p < (unsigned)n) return p;
  const int period = 2 * n;
  int m = p % period;
  if (m < 0) m += period;
  return m < n ? m : period - 1 - m;
}
__device__ __forceinline__ int reflect101(int p, int n) {    // BORDER_REFLECT_101  gfedcb|abcdefgh|gfedcba
  if ((unsigned)p < (unsigned)n) return p;
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  int m = p % period;
  if (m < 0) m += period;
  return m < n ? m : period - m;
}

// a / b rounded half to even (cvRound of the exact quotient): the entries of cv2's sdiv / hdiv tables
__device__ __forceinline__ int round_div(int a, int b) {
  int q = a / b;
  const int r = a - q * b;
  if (2 * r > b || (2 * r == b && (q & 1))) ++q;
  return q;
}

__device__ __forceinline__ int sat_u8(int v) { return min(max(v, 0), 255); }

// RGB -> HSV (cv2 RGB2HSV_b, H in 0..179) -> shifts (albumentations' LUTs) -> RGB (cv2 HSV2RGB, float32 per-operation rounding)
__device__ __forceinline__ void hue_sat_val(int& r, int& g, int& b, const int* sdiv, const int* hdiv, int hue, int sat, int val) {
  int v = max(max(r, g), b);
  const int diff = v - min(min(r, g), b);
  int s = (diff * sdiv[v] + (1 << 11)) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + (1 << 11)) >> 12;
  if (h < 0) h += 180;
  h = (h + hue) % 180;                       // hue is in [0, 180)
  s = sat_u8(s + sat);
  v = sat_u8(v + val);
  const float vf = (float)v * (1.f / 255.f);
  if (s == 0) {
    r = g = b = sat_u8(__float2int_rn(vf * 255.f));
    return;
  }
  const float sf = (float)s * (1.f / 255.f);
  float hf = (float)h * (6.f / 180.f);
  int sector = (int)floorf(hf);
  hf = hf - (float)sector;
  if ((unsigned)sector >= 6u) { sector = 0; hf = 0.f; }
  const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * hf), t3 = vf * (1.f - sf * (1.f - hf));
  // cv2's sector table {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}} = (b, g, r), written as selects (no indexed registers)
  const float bf = sector < 2 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
  const float gf = sector == 0 ? t3 : (sector < 3 ? t0 : (sector == 3 ? t2 : t1));
  const float rf = (sector == 0 || sector == 5) ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  r = sat_u8(__float2int_rn(rf * 255.f));
  g = sat_u8(__float2int_rn(gf * 255.f));
  b = sat_u8(__float2int_rn(bf * 255.f));
}

__global__ __launch_bounds__(256) void train_augment_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                            const mmskin_augment_params* __restrict__ table,
                                                            uint8_t* __restrict__ dst) {
  __shared__ uint8_t geo[GP * GP * 3];         // geometric stage: tile + halo, interleaved RGB
  __shared__ uint16_t hor[GP * TILE * 3];      // horizontal blur pass: (TILE + 2r) rows x TILE pixels, all 16 bits kept
  __shared__ int col_a[GP], col_b[GP];         // rotate: M0*x, M3*x in 10-bit fixed point; copy: col_a = source column
  __shared__ int row_x[GP], row_y[GP];         // rotate: (M1*y + M2), (M4*y + M5) + rounding; copy: row_y = source row
  __shared__ int sdiv[256], hdiv[256];         // cv2's 12-bit division tables of RGB2HSV

  const int tid = threadIdx.x, n = blockIdx.z;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  const mmskin_augment_params& P = table[n];
  const uint32_t flags = P.flags;
  const bool rot = flags & MMSKIN_AUG_ROTATE;
  const int r = (flags & MMSKIN_AUG_BLUR) ? min(max(P.ksize >> 1, 0), RMAX) : 0;
  const int side = TILE + 2 * r;
  const uint8_t* img = src + (size_t)n * H * W * 3;

  // per-row / per-column terms of the tile (+ halo): blur border (reflect-101 of the DESTINATION index) -> flip -> rotate terms
  if (tid < GP) {
    const int gy = reflect101(y0 - r + tid, H);
    const int yy = (flags & MMSKIN_AUG_VFLIP) ? H - 1 - gy : gy;
    if (rot) {
      row_x[tid] = (int)rint((P.minv[1] * (double)yy + P.minv[2]) * 1024.0) + 16;
      row_y[tid] = (int)rint((P.minv[4] * (double)yy + P.minv[5]) * 1024.0) + 16;
    } else {
      row_y[tid] = yy;
    }
  } else if (tid >= 64 && tid < 64 + GP) {
    const int lx = tid - 64;
    const int gx = reflect101(x0 - r + lx, W);
    const int xx = (flags & MMSKIN_AUG_HFLIP) ? W - 1 - gx : gx;
    if (rot) {
      col_a[lx] = (int)rint(P.minv[0] * (double)xx * 1024.0);
      col_b[lx] = (int)rint(P.minv[3] * (double)xx * 1024.0);
    } else {
      col_a[lx] = xx;
    }
  }
  if (flags & MMSKIN_AUG_HSV) {
    sdiv[tid] = tid ? round_div(255 << 12, tid) : 0;
    hdiv[tid] = tid ? round_div(180 << 12, 6 * tid) : 0;
  }
  __syncthreads();

  // geometric stage into LDS
  for (int i = tid; i < GP * GP; i += 256) {
    const int ly = i / GP, lx = i - ly * GP;
    if (ly >= side || lx >= side) continue;
    uint8_t* out = geo + i * 3;
    if (rot) {
      const int X = (row_x[ly] + col_a[lx]) >> 5, Y = (row_y[ly] + col_b[lx]) >> 5;
      const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
      const int fx = X & 31, fy = Y & 31;
      const int xa = reflect(sx, W), xb = reflect(sx + 1, W), ya = reflect(sy, H), yb = reflect(sy + 1, H);
      const int w00 = 32 * (32 - fy) * (32 - fx), w01 = 32 * (32 - fy) * fx, w10 = 32 * fy * (32 - fx), w11 = 32 * fy * fx;
      const uint8_t* pa = img + ((size_t)ya * W) * 3;
      const uint8_t* pb = img + ((size_t)yb * W) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int acc = w00 * pa[xa * 3 + c] + w01 * pa[xb * 3 + c] + w10 * pb[xa * 3 + c] + w11 * pb[xb * 3 + c];
        out[c] = (uint8_t)((acc + (1 << 14)) >> 15);
      }
    } else {
      const uint8_t* p = img + ((size_t)row_y[ly] * W + col_a[lx]) * 3;
      out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
    }
  }
  __syncthreads();

  const int t0 = P.taps[0], t1 = P.taps[1], t2 = P.taps[2], t3 = P.taps[3];
  if (r > 0) {   // horizontal pass over the interleaved row: neighbours of byte e are e -+ 3j
    for (int i = tid; i < side * TILE * 3; i += 256) {
      const int row = i / (TILE * 3), e = i - row * (TILE * 3);
      const uint8_t* c = geo + row * GP * 3 + r * 3 + e;
      int acc = t0 * c[0] + t1 * (c[-3] + c[3]);
      if (r > 1) acc += t2 * (c[-6] + c[6]);
      if (r > 2) acc += t3 * (c[-9] + c[9]);
      hor[i] = (uint16_t)acc;
    }
    __syncthreads();
  }

  const int n_holes = (flags & MMSKIN_AUG_DROPOUT) ? min(max(P.n_holes, 0), MMSKIN_AUG_MAX_HOLES) : 0;
  const float alpha = P.alpha, beta255 = P.beta255;
#pragma unroll
  for (int q = 0; q < TILE * TILE / 256; ++q) {
    const int p = tid + q * 256, ty = p / TILE, tx = p - ty * TILE;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (r > 0) {   // vertical pass, round half up
        const uint16_t* h = hor + (ty + r) * (TILE * 3) + tx * 3 + c;
        int acc = t0 * h[0] + t1 * (h[-TILE * 3] + h[TILE * 3]);
        if (r > 1) acc += t2 * (h[-2 * TILE * 3] + h[2 * TILE * 3]);
        if (r > 2) acc += t3 * (h[-3 * TILE * 3] + h[3 * TILE * 3]);
        v[c] = (acc + (1 << 15)) >> 16;
      } else {
        v[c] = geo[(ty * GP + tx) * 3 + c];
      }
    }
    for (int k = 0; k < n_holes; ++k)
      if (x >= P.holes[k][0] && x < P.holes[k][2] && y >= P.holes[k][1] && y < P.holes[k][3]) v[0] = v[1] = v[2] = 0;
    if (flags & MMSKIN_AUG_HSV) hue_sat_val(v[0], v[1], v[2], sdiv, hdiv, P.hue, P.sat, P.val);
    uint8_t* out = dst + (((size_t)n * H + y) * W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int o = v[c];
      if (flags & MMSKIN_AUG_BC) o = (int)fminf(fmaxf((float)o * alpha + beta255, 0.f), 255.f);
      out[c] = (uint8_t)o;
    }
  }
}

}  // namespace

extern "C" int mmskin_train_augment_u8(const uint8_t* src_nhwc, int N, int H, int W, const mmskin_augment_params* params_host,
                                       mmskin_augment_params* params_scratch, uint8_t* dst_nhwc, void* stream) {
  ARG_CHECK(src_nhwc && dst_nhwc && params_host && params_scratch, "train_augment_u8: null argument");
  ARG_CHECK(src_nhwc != dst_nhwc, "train_augment_u8: in-place operation is not supported");
  ARG_CHECK(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "train_augment_u8: bad shape %d x %dx%d", N, H, W);
  for (int n = 0; n < N; ++n) {
    const mmskin_augment_params& p = params_host[n];
    ARG_CHECK(p.ksize == 1 || p.ksize == 3 || p.ksize == 5 || p.ksize == 7, "train_augment_u8: sample %d: kernel size %d not in {1, 3, 5, 7}",
              n, p.ksize);
    ARG_CHECK(p.n_holes >= 0 && p.n_holes <= MMSKIN_AUG_MAX_HOLES, "train_augment_u8: sample %d: %d holes, the table holds %d", n,
              p.n_holes, MMSKIN_AUG_MAX_HOLES);
    int sum = p.taps[0];
    for (int j = 1; j < 4; ++j) {
      ARG_CHECK(j <= p.ksize / 2 || p.taps[j] == 0, "train_augment_u8: sample %d: tap %d set beyond kernel size %d", n, j, p.ksize);
      sum += 2 * p.taps[j];
    }
    ARG_CHECK(sum == 256, "train_augment_u8: sample %d: blur taps sum to %d, not 256", n, sum);
    ARG_CHECK(p.hue >= 0 && p.hue < 180, "train_augment_u8: sample %d: hue shift %d not reduced to [0, 180)", n, p.hue);
  }
  // the kernel reads the bytes that were just validated: the upload is part of the call (pageable host memory: the copy has
  // left the host buffer when hipMemcpyAsync returns)
  HIP_CHECK_RET(hipMemcpyAsync(params_scratch, params_host, (size_t)N * sizeof(mmskin_augment_params), hipMemcpyHostToDevice,
                               (hipStream_t)stream));
  hipLaunchKernelGGL(train_augment_kernel, dim3(ceil_div(W, TILE), ceil_div(H, TILE), N), dim3(256), 0, (hipStream_t)stream, src_nhwc, H,
                     W, params_scratch, dst_nhwc);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
