// Grad-CAM and Grad-CAM++ (interpretability/gradcam_atualizado.py:230-306) for R = images x metadata variants rows at once,
// forward only.  The activations A [N, C, fh, fw] at the target layer belong to the image; only d score / d features belongs
// to the row.  On the encoders whose tail from A to the pooled features is diagonal in the channel the gradient at A is
//   g[r, c, i, j] = jac[row_image[r], c, i, j] * dfeat[r, c]
// so the [R, C, fh, fw] gradient tensor is never built: the weight kernel forms g in registers.  With dfeat == NULL, jac is
// that tensor itself, as autograd returns it for any other target layer.
//
//   weights  one (row, channel) pair per sub-wave of 1 / 4 / 16 / 64 lanes (the smallest that covers fh * fw, so a 2x2 map
//            packs 16 pairs into a wave); the lanes stride over the map, sums go through __shfl_xor inside the sub-wave.
//            Grad-CAM: w = mean_ij g.  Grad-CAM++: alpha = g^2 / (2 g^2 + sum_ij(A g^3) + 1e-8), w = sum_ij alpha relu(g):
//            two passes over the pair's fh * fw values (the second one hits L1: a pair is at most a few hundred bytes)
//   raw      raw[r, p] = sum_c w[r, c] * A[row_image[r], c, p].  A workgroup takes PT <= 16 pixels of one row and splits the
//            channels over NT / PT slices; a thread owns (slice, pixel) and keeps four partial sums, so that no partial sum
//            runs over more than C / (4 * NT / PT) terms; the slices are then halved through LDS.  Every step has a fixed
//            order: the result repeats bit for bit.  No atomics
//   cam      relu, (x - min) / (max - min + 1e-8) over the row's fh x fw map (every workgroup recomputes it in LDS: at most
//            MAX_MAP values), then the bilinear upsample of cam_sample.h.  Normalisation BEFORE the upsample: the opposite
//            order from Score-CAM, as in the reference (_normalize, then F.interpolate)
//
// row_image is not trusted: every kernel clamps its entry to [0, N - 1] (as embedding backward clamps its ids).
#include "../../include/mmskin.h"
#include "cam_sample.h"
#include "common.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int PPT = 4;           // cam: output pixels per thread
constexpr int MAX_MAP = 4096;    // fh * fw at most: the cam kernel's LDS tile (16 KiB)
constexpr int RAW_PT = 16;       // raw: pixels per workgroup at most

template <int SW>
__device__ __forceinline__ float sub_sum(float v) {
#pragma unroll
  for (int o = SW / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int clamp_image(const int* __restrict__ row_image, int r, int N) {
  return min(max(row_image[r], 0), N - 1);
}

// grid = ceil(R * C / (NT / SW)).  A sub-wave past the last pair computes the last pair again (the shuffles want every lane)
// and stores nothing.
template <int SW>
__global__ __launch_bounds__(NT) void gradcam_weights_kernel(const float* __restrict__ acts, const float* __restrict__ jac,
                                                             const float* __restrict__ dfeat, const int* __restrict__ row_image,
                                                             int N, int R, int C, int fhw, int mode,
                                                             float* __restrict__ weights) {
  const int lane = threadIdx.x & (SW - 1);
  const int64_t pairs = (int64_t)R * C;
  const int64_t pair = (int64_t)blockIdx.x * (NT / SW) + threadIdx.x / SW;
  const int64_t pc = pair < pairs ? pair : pairs - 1;
  const int r = (int)(pc / C), c = (int)(pc - (int64_t)r * C);
  const int n = clamp_image(row_image, r, N);
  const float* A = acts + ((size_t)n * C + c) * fhw;
  const float* G = jac + ((size_t)(dfeat ? n : r) * C + c) * fhw;
  const float s = dfeat ? dfeat[pc] : 1.f;
  float w;
  if (mode == 0) {
    float sum = 0.f;
    for (int i = lane; i < fhw; i += SW) sum += G[i] * s;
    w = sub_sum<SW>(sum) / (float)fhw;
  } else {
    float t = 0.f;
    for (int i = lane; i < fhw; i += SW) {
      const float g = G[i] * s;
      t += A[i] * (g * g * g);
    }
    t = sub_sum<SW>(t);
    float sum = 0.f;
    for (int i = lane; i < fhw; i += SW) {
      const float g = G[i] * s, g2 = g * g;
      const float alpha = g2 / (2.f * g2 + t + 1e-8f);
      sum += alpha * fmaxf(g, 0.f);
    }
    w = sub_sum<SW>(sum);
  }
  if (lane == 0 && pair < pairs) weights[pair] = w;
}

// grid = (R, ceil(fhw / PT)), PT = 1 << pt_log2 <= RAW_PT.  thread = slice * PT + pixel; slice s takes channels s, s + S, ...
// (S = NT / PT slices), four of them in flight.
__global__ __launch_bounds__(NT) void gradcam_raw_kernel(const float* __restrict__ acts, const float* __restrict__ weights,
                                                         const int* __restrict__ row_image, int N, int C, int fhw, int pt_log2,
                                                         float* __restrict__ raw) {
  __shared__ float part[NT];
  const int tid = threadIdx.x, r = blockIdx.x;
  const int PT = 1 << pt_log2, S = NT >> pt_log2;
  const int pl = tid & (PT - 1), s = tid >> pt_log2;
  const int p = blockIdx.y * PT + pl;
  const int n = clamp_image(row_image, r, N);
  const float* A = acts + (size_t)n * C * fhw + min(p, fhw - 1);
  const float* w = weights + (size_t)r * C;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = s;
  for (; c + 3 * S < C; c += 4 * S) {
    a0 += w[c] * A[(size_t)c * fhw];
    a1 += w[c + S] * A[(size_t)(c + S) * fhw];
    a2 += w[c + 2 * S] * A[(size_t)(c + 2 * S) * fhw];
    a3 += w[c + 3 * S] * A[(size_t)(c + 3 * S) * fhw];
  }
  for (; c < C; c += S) a0 += w[c] * A[(size_t)c * fhw];
  part[tid] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  for (int h = S >> 1; h > 0; h >>= 1) {
    if (s < h) part[tid] += part[tid + (h << pt_log2)];
    __syncthreads();
  }
  if (s == 0 && p < fhw) raw[(size_t)r * fhw + p] = part[pl];
}

// grid = R * tiles, tiles = ceil(H * W / (NT * PPT)); pixel k of a thread is tile + k * NT + tid: coalesced dword stores.
__global__ __launch_bounds__(NT) void gradcam_cam_kernel(const float* __restrict__ raw, int fh, int fw, int H, int W, int tiles,
                                                         float scale_h, float scale_w, float* __restrict__ cam) {
  extern __shared__ float lds[];   // fh * fw values of the row's map
  __shared__ float red[8];
  const int tid = threadIdx.x, fhw = fh * fw, HW = H * W;
  const int r = blockIdx.x / tiles, tile = blockIdx.x - r * tiles;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < fhw; i += NT) {
    const float v = fmaxf(raw[(size_t)r * fhw + i], 0.f);
    lds[i] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, red);
  const float range = mx - mn + 1e-8f;
  for (int i = tid; i < fhw; i += NT) lds[i] = (lds[i] - mn) / range;   // the values this thread wrote itself
  __syncthreads();
  const int base = tile * (NT * PPT);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = base + k * NT + tid;
    if (p < HW) {
      const int y = p / W, x = p - y * W;
      cam[(size_t)r * HW + p] = bilerp(lds, make_tap(y, x, fh, fw, scale_h, scale_w));
    }
  }
}

// shape checks shared by the two entry points (before anything is launched)
int check_shape(const char* who, int N, int R, int C, int fh, int fw) {
  ARG_CHECK(N >= 1 && C >= 1 && fh >= 1 && fw >= 1, "%s: every extent must be >= 1 (N %d, C %d, map %dx%d)", who, N, C, fh, fw);
  ARG_CHECK(R >= 1, "%s: %d rows", who, R);
  ARG_CHECK(N <= (1 << 20) && C <= (1 << 20) && (int64_t)R * C <= (1 << 28), "%s: %d images, %d rows or %d channels out of range",
            who, N, R, C);
  if ((int64_t)fh * fw > MAX_MAP) {
    mmskin_set_error("%s: a %dx%d feature map does not fit the kernels' LDS tile (%d floats)", who, fh, fw, MAX_MAP);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  return MMSKIN_OK;
}

}  // namespace

extern "C" int mmskin_gradcam_weights(const float* acts, const float* jac, const float* dfeat, const int32_t* row_image, int N,
                                      int R, int C, int fh, int fw, int mode, float* weights, void* stream) {
  if (int rc = check_shape("gradcam_weights", N, R, C, fh, fw)) return rc;
  ARG_CHECK(mode == 0 || mode == 1, "gradcam_weights: mode %d is neither 0 (Grad-CAM) nor 1 (Grad-CAM++)", mode);
  ARG_CHECK(acts && jac && row_image && weights, "gradcam_weights: null argument");
  const int fhw = fh * fw;
  const int64_t pairs = (int64_t)R * C;
#define LAUNCH_WEIGHTS(SW)                                                                                                       \
  hipLaunchKernelGGL(gradcam_weights_kernel<SW>, dim3((unsigned)((pairs + NT / SW - 1) / (NT / SW))), dim3(NT), 0, ST(stream), acts, \
                     jac, dfeat, row_image, N, R, C, fhw, mode, weights)
  if (fhw <= 1) LAUNCH_WEIGHTS(1);
  else if (fhw <= 4) LAUNCH_WEIGHTS(4);
  else if (fhw <= 16) LAUNCH_WEIGHTS(16);
  else LAUNCH_WEIGHTS(64);
#undef LAUNCH_WEIGHTS
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_gradcam_map(const float* acts, const float* weights, const int32_t* row_image, int N, int R, int C, int fh,
                                  int fw, int H, int W, float* raw, float* cam, void* stream) {
  if (int rc = check_shape("gradcam_map", N, R, C, fh, fw)) return rc;
  ARG_CHECK(H >= 1 && W >= 1, "gradcam_map: every extent must be >= 1 (image %dx%d)", H, W);
  ARG_CHECK(H >= fh && W >= fw, "gradcam_map: the image (%dx%d) must be at least as large as the feature map (%dx%d)", H, W, fh, fw);
  ARG_CHECK((int64_t)H * W <= (1 << 28), "gradcam_map: image %dx%d out of range", H, W);
  const int fhw = fh * fw, HW = H * W, tiles = ceil_div(HW, NT * PPT);
  ARG_CHECK((int64_t)R * tiles < (1ll << 31), "gradcam_map: %d rows of %dx%d are too many for one launch", R, H, W);
  ARG_CHECK(acts && weights && row_image && raw && cam, "gradcam_map: null argument");
  int pt_log2 = 0;
  while ((1 << pt_log2) < RAW_PT && (1 << pt_log2) < fhw) ++pt_log2;
  hipLaunchKernelGGL(gradcam_raw_kernel, dim3(R, ceil_div(fhw, 1 << pt_log2)), dim3(NT), 0, ST(stream), acts, weights, row_image, N,
                     C, fhw, pt_log2, raw);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(gradcam_cam_kernel, dim3((unsigned)(R * tiles)), dim3(NT), (size_t)fhw * sizeof(float), ST(stream), raw, fh, fw,
                     H, W, tiles, (float)fh / (float)H, (float)fw / (float)W, cam);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}
