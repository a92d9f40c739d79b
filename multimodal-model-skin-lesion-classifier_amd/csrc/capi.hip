// C-ABI glue: error reporting + the op-level convolution / batch-norm / stem entry points.
// These wrap exactly the kernels the backbone plan launches (conv_gemm.hip, wgrad.hip, ops.hip) with
// NCHW fp32 tensors at the boundary, so every kernel can be parity-tested in isolation.
#include <stdarg.h>
#include <string.h>

#include <algorithm>

#include "../../include/mmskin.h"
#include "conv.h"
#include "ops.h"
#include "plan.h"

static thread_local char g_err[1024] = "";

void mmskin_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

__global__ void coef_from_saved_kernel(int C, const float* gamma, const float* beta, const float* mean,
                                       const float* invstd, float* scale, float* shift) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float sc = gamma[c] * invstd[c];
    scale[c] = sc;
    shift[c] = beta[c] - mean[c] * sc;
  }
}

template <typename T>
int stage_one(const float* w, int Cout, int Cin, int taps, bool stem, T* wfwd, T* wdgrad, StageDesc* table_dev,
              hipStream_t st) {
  StageDesc d = {};
  d.src_off = 0; d.fwd_off = 0; d.dgrad_off = 0;
  d.Cout = Cout; d.Cin = Cin; d.taps = taps; d.stem = stem ? 1 : 0;
  HIP_CHECK_RET(hipMemcpyAsync(table_dev, &d, sizeof(d), hipMemcpyHostToDevice, st));
  HIP_CHECK_RET(hipStreamSynchronize(st));  // `d` lives on this stack frame
  if (stem) HIP_CHECK_RET(hipMemsetAsync(wfwd, 0, 64 * 256 * sizeof(T), st));
  return stage_weights<T>(table_dev, 1, Cout * Cin * taps, w, wfwd, wdgrad, wdgrad != nullptr, st);
}

// Op-level workspaces: one layout struct per op family.  Its constructor carves the regions; on a null base it only sizes them, and
// ws_bytes() is how every mmskin_*_workspace_bytes asks.  The size functions take no dtype, so they size with T = float: each take of the
// bf16_t instantiation is no larger and Carver's alignment is monotone, so every bf16 region ends at or before its float counterpart.
template <class Ws, class... A>
int64_t ws_bytes(A... a) { return (int64_t)Ws(nullptr, a...).total; }

// the weight-gradient slab of the shapes the weight-gradient kernels take (the others are rejected at launch and need none)
inline size_t conv_slab_floats(const ConvShape& s) {
  return (s.Cout % 64 == 0 && (s.Cin * s.kh * s.kw) % 64 == 0) ? conv_wgrad_slab_bytes(s) / sizeof(float) : 0;
}

template <typename T>
struct ConvWs {
  StageDesc* table; T *xh, *wf, *yh, *wd, *dxh; WgradSlab slab; size_t total;   // yh: NHWC output (forward) or dy (backward)
  ConvWs(void* ws, const ConvShape& s) {
    Carver c(ws);
    const size_t in = (size_t)s.N * s.H * s.W * s.Cin, wgt = (size_t)s.Cout * s.Cin * s.kh * s.kw;
    table = c.take<StageDesc>(1);
    xh = c.take<T>(in); wf = c.take<T>(wgt); yh = c.take<T>((size_t)s.N * s.OH() * s.OW() * s.Cout);
    wd = c.take<T>(wgt); dxh = c.take<T>(in); slab.floats = conv_slab_floats(s); slab.p = c.take<float>(slab.floats);
    total = c.cur;
  }
};
// the weight-gradient timer writes an fp32 dw, which ConvWs<bf16_t>'s weight regions are too small for
template <typename T>
struct WgradTimeWs {
  T *xh, *yh; float* dw; WgradSlab slab; size_t total;
  WgradTimeWs(void* ws, const ConvShape& s) {
    Carver c(ws);
    xh = c.take<T>((size_t)s.N * s.H * s.W * s.Cin); yh = c.take<T>((size_t)s.N * s.OH() * s.OW() * s.Cout);
    dw = c.take<float>((size_t)s.Cout * s.Cin * s.kh * s.kw); slab.floats = conv_slab_floats(s); slab.p = c.take<float>(slab.floats);
    total = c.cur;
  }
};

template <typename T>
int conv_fwd_op(const float* x, const float* w, float* y, const ConvShape& s, void* ws, hipStream_t st) {
  ConvWs<T> c(ws, s);
  int rc;
  if ((rc = nchw_to_nhwc<T>(x, s.N, s.Cin, s.H, s.W, c.xh, st))) return rc;
  if ((rc = stage_one<T>(w, s.Cout, s.Cin, s.kh * s.kw, false, c.wf, (T*)nullptr, c.table, st))) return rc;
  if ((rc = launch_conv_fwd<T>(s, c.xh, c.wf, c.yh, nullptr, nullptr, st))) return rc;
  return nhwc_to_nchw<T>(c.yh, s.N, s.Cout, s.OH(), s.OW(), y, st);
}

template <typename T>
int conv_bwd_op(const float* dy, const float* x, const float* w, float* dx, float* dw, const ConvShape& s, void* ws,
                hipStream_t st) {
  ConvWs<T> c(ws, s);
  int rc;
  if ((rc = nchw_to_nhwc<T>(dy, s.N, s.Cout, s.OH(), s.OW(), c.yh, st))) return rc;
  if (dx) {
    if ((rc = stage_one<T>(w, s.Cout, s.Cin, s.kh * s.kw, false, c.wf, c.wd, c.table, st))) return rc;
    if ((rc = launch_conv_dgrad<T>(s, c.yh, c.wd, c.dxh, (const T*)nullptr, st))) return rc;
    if ((rc = nhwc_to_nchw<T>(c.dxh, s.N, s.Cin, s.H, s.W, dx, st))) return rc;
  }
  if (dw) {
    if ((rc = nchw_to_nhwc<T>(x, s.N, s.Cin, s.H, s.W, c.xh, st))) return rc;
    if ((rc = launch_conv_wgrad<T>(s, c.yh, c.xh, c.slab, dw, st))) return rc;
  }
  return MMSKIN_OK;
}

// the mmskin_conv_route flags that name an operand (or, EMPTY, the absence of one) of a DgradFuse / FwdFuse: a launch gets the struct when one is set
constexpr int CRD_FUSE_BITS = MMSKIN_CRD_MASK_Y | MMSKIN_CRD_MASK_BITS | MMSKIN_CRD_X | MMSKIN_CRD_SCALE_SHIFT | MMSKIN_CRD_X2 | MMSKIN_CRD_IN2 | MMSKIN_CRD_BIAS |
                              MMSKIN_CRD_ADDEND_S2 | MMSKIN_CRD_PARTIAL | MMSKIN_CRD_EMPTY;
constexpr int CRF_FUSE_BITS = MMSKIN_CRF_BIAS | MMSKIN_CRF_ADDEND | MMSKIN_CRF_RELU | MMSKIN_CRF_GELU | MMSKIN_CRF_OUT_F32 | MMSKIN_CRF_RESIDUAL | MMSKIN_CRF_MASK_OUT |
                              MMSKIN_CRF_MUL;
static_assert(CRD_FUSE_BITS == 0xffc && CRF_FUSE_BITS == 0x3fc, "the masks mmskin_conv_route has always applied");

// ---- the fused epilogues op by op (mmskin_conv2d_dgrad_epilogue / mmskin_conv2d_forward_epilogue): the tensor operands of a DgradFuse /
// FwdFuse arrive NCHW fp32 and are converted into the workspace; mask bytes, per-channel vectors and the fp32 slabs go to the launcher as
// the caller passed them.  Both ask the route first, so a launch the launcher would refuse is refused before anything runs.
struct DgradEpiArgs {
  const float *dy, *w, *addend, *mask_y; const uint8_t* mask_bits; const float *x, *scale, *shift, *x2;
  float *dz, *partial, *partial_b; int* rows_written; int flags;
};
template <typename T>
struct DgradEpiWs {
  StageDesc* table; T *dyh, *wf, *wd, *dzh, *addh, *myh, *xh, *x2h; size_t total;
  DgradEpiWs(void* ws, const ConvShape& s) {
    Carver c(ws);
    const size_t in = (size_t)s.N * s.H * s.W * s.Cin, wgt = (size_t)s.Cout * s.Cin * s.kh * s.kw;
    table = c.take<StageDesc>(1);
    dyh = c.take<T>((size_t)s.N * s.OH() * s.OW() * s.Cout); wf = c.take<T>(wgt); wd = c.take<T>(wgt);
    dzh = c.take<T>(in); addh = c.take<T>(in); myh = c.take<T>(in); xh = c.take<T>(in); x2h = c.take<T>(in);   // addh: the compact addend is smaller
    total = c.cur;
  }
};
template <typename T>
int dgrad_epilogue_op(const DgradEpiArgs& g, const ConvShape& s, void* ws, hipStream_t st) {
  DgradEpiWs<T> c(ws, s);
  const int fl = g.flags;
  const bool in_place = (fl & MMSKIN_CRD_ADDEND_IS_DIN) != 0, s2 = (fl & MMSKIN_CRD_ADDEND_S2) != 0;
  DgradFuse f;
  f.mask_y = (fl & MMSKIN_CRD_MASK_Y) ? c.myh : nullptr; f.mask_bits = g.mask_bits; f.x = (fl & MMSKIN_CRD_X) ? c.xh : nullptr;
  f.scale = g.scale; f.shift = g.shift; f.x2 = (fl & MMSKIN_CRD_X2) ? c.x2h : nullptr; f.partial = g.partial; f.partial_b = g.partial_b; f.addend_s2 = s2;
  DgradFuse* const fp = (fl & CRD_FUSE_BITS) ? &f : nullptr;   // a DgradFuse when a flag names one of its operands, as mmskin_conv_route passes it
  const T* const addend = (fl & MMSKIN_CRD_ADDEND) ? (in_place ? c.dzh : c.addh) : nullptr;
  int rc;
  { ConvGemmArgs a; ConvRoute r; unsigned zero_mask;
    if ((rc = conv_route_dgrad(s, (int)sizeof(T), c.dyh, c.wd, c.dzh, addend, fp, a, zero_mask, r))) return rc; }
  if ((rc = nchw_to_nhwc<T>(g.dy, s.N, s.Cout, s.OH(), s.OW(), c.dyh, st))) return rc;
  if ((rc = stage_one<T>(g.w, s.Cout, s.Cin, s.kh * s.kw, false, c.wf, c.wd, c.table, st))) return rc;
  if (in_place) { if ((rc = nchw_to_nhwc<T>(g.dz, s.N, s.Cin, s.H, s.W, c.dzh, st))) return rc; }
  else if (addend && (rc = nchw_to_nhwc<T>(g.addend, s.N, s.Cin, s2 ? (s.H + 1) / 2 : s.H, s2 ? (s.W + 1) / 2 : s.W, c.addh, st))) return rc;
  if (f.mask_y && (rc = nchw_to_nhwc<T>(g.mask_y, s.N, s.Cin, s.H, s.W, c.myh, st))) return rc;
  if (f.x && (rc = nchw_to_nhwc<T>(g.x, s.N, s.Cin, s.H, s.W, c.xh, st))) return rc;
  if (f.x2 && (rc = nchw_to_nhwc<T>(g.x2, s.N, s.Cin, s.H, s.W, c.x2h, st))) return rc;
  if ((rc = launch_conv_dgrad<T>(s, c.dyh, c.wd, c.dzh, addend, st, fp))) return rc;
  if (g.rows_written) *g.rows_written = f.rows_written;
  return nhwc_to_nchw<T>(c.dzh, s.N, s.Cin, s.H, s.W, g.dz, st);
}

struct FwdEpiArgs {
  const float *x, *w, *mul, *bias, *addend; float *y, *stat_sum, *stat_sq; int* stat_rows; uint8_t* mask_out; int flags;
};
template <typename T>
struct FwdEpiWs {
  StageDesc* table; T *xh, *wf, *yh, *addh; size_t total;
  FwdEpiWs(void* ws, const ConvShape& s) {
    Carver c(ws);
    const size_t out = (size_t)s.N * s.OH() * s.OW() * s.Cout;
    table = c.take<StageDesc>(1);
    xh = c.take<T>((size_t)s.N * s.H * s.W * s.Cin); wf = c.take<T>((size_t)s.Cout * s.Cin * s.kh * s.kw); yh = c.take<T>(out); addh = c.take<T>(out);
    total = c.cur;
  }
};
template <typename T>
int fwd_epilogue_op(const FwdEpiArgs& g, const ConvShape& s, void* ws, hipStream_t st) {
  FwdEpiWs<T> c(ws, s);
  const int fl = g.flags;
  const bool rows_free = (fl & MMSKIN_CRF_ROWS_FREE) != 0;
  FwdFuse f;
  f.bias = g.bias; f.mul = g.mul; f.mask_out = g.mask_out; f.relu = (fl & MMSKIN_CRF_RELU) != 0; f.addend = (fl & MMSKIN_CRF_ADDEND) ? c.addh : nullptr;
  const FwdFuse* const fp = (fl & CRF_FUSE_BITS) ? &f : nullptr;   // a FwdFuse when a flag names one of its operands, as mmskin_conv_route passes it
  T* const out = (fl & MMSKIN_CRF_NO_OUT) ? nullptr : c.yh;
  int rc, rows = 0;
  ConvGemmArgs a; ConvRoute r;
  if ((rc = conv_route_fwd(s, (int)sizeof(T), c.xh, c.wf, out, g.stat_sum, g.stat_sq, fp, rows_free, a, r))) return rc;
  if ((rc = nchw_to_nhwc<T>(g.x, s.N, s.Cin, s.H, s.W, c.xh, st))) return rc;
  if ((rc = stage_one<T>(g.w, s.Cout, s.Cin, s.kh * s.kw, false, c.wf, (T*)nullptr, c.table, st))) return rc;
  if (f.addend && (rc = nchw_to_nhwc<T>(g.addend, s.N, s.Cout, s.OH(), s.OW(), c.addh, st))) return rc;
  if ((rc = launch_conv_fwd<T>(s, c.xh, c.wf, out, g.stat_sum, g.stat_sq, st, fp, rows_free ? &rows : nullptr))) return rc;
  if (g.stat_rows) *g.stat_rows = rows_free ? rows : r.total_mblk;
  return out ? nhwc_to_nchw<T>(c.yh, s.N, s.Cout, s.OH(), s.OW(), g.y, st) : MMSKIN_OK;
}

// Average microseconds per launch of `run` (0 = launched) on stream st: three warm-up launches, then `iters` between an event pair.
// -1.0 when a launch or an event call fails; both events are destroyed on every path.
template <class F>
static double time_launches(F run, int iters, hipStream_t st) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.f;
  bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
  for (int i = 0; ok && i < 3; ++i) ok = run() == 0;
  ok = ok && hipEventRecord(e0, st) == hipSuccess;
  for (int i = 0; ok && i < iters; ++i) ok = run() == 0;
  ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return ok ? (double)ms * 1e3 / iters : -1.0;
}
enum { TIME_FWD, TIME_DGRAD, TIME_WGRAD };
template <typename T>
double conv_time(int op, const ConvShape& s, int iters, void* ws, hipStream_t st) {
  ConvWs<T> c(ws, s);
  WgradTimeWs<T> g(ws, s);
  if (op == TIME_FWD) return time_launches([&] { return launch_conv_fwd<T>(s, c.xh, c.wf, c.yh, nullptr, nullptr, st); }, iters, st);
  if (op == TIME_DGRAD) return time_launches([&] { return launch_conv_dgrad<T>(s, c.yh, c.wd, c.dxh, (const T*)nullptr, st); }, iters, st);
  return time_launches([&] { return launch_conv_wgrad<T>(s, g.yh, g.xh, g.slab, g.dw, st); }, iters, st);
}

template <typename T>
struct BnWs {
  T *xh, *yh, *dxh; float *ssum, *ssq, *partial, *coef, *coefbwd; ColScratch red; size_t total;   // yh: y (forward) or dy (backward)
  BnWs(void* ws, int N, int C, int H, int W) {
    Carver c(ws);
    const size_t rows = (size_t)N * H * W;
    xh = c.take<T>(rows * C); yh = c.take<T>(rows * C); dxh = c.take<T>(rows * C);
    ssum = c.take<float>((size_t)column_stats_rows(rows, C) * C);
    ssq = c.take<float>((size_t)column_stats_rows(rows, C) * C);
    partial = c.take<float>((size_t)bn_bwd_partial_rows(rows, C) * 2 * C);
    coef = c.take<float>(5 * (size_t)C);   // scale | shift, and behind them (backward) cA | cB | cC
    coefbwd = BnCoef(coef, C).mean;           // ... which start where a five-slot block keeps mean
    red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(C) / sizeof(double)), C);
    total = c.cur;
  }
};

template <typename T>
int bn_fwd_op(const float* x, const float* gamma, const float* beta, float* rm, float* rv, float* y, float* save_mean,
              float* save_invstd, int N, int C, int H, int W, float eps, float mom, int relu, void* ws, hipStream_t st) {
  BnWs<T> s(ws, N, C, H, W);
  const size_t rows = (size_t)N * H * W;
  int rc, nr = 0;
  if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
  if ((rc = column_stats<T>(s.xh, rows, C, s.ssum, s.ssq, &nr, st))) return rc;
  const BnCoef k(s.coef, C);
  if ((rc = bn_finalize(s.ssum, s.ssq, nr, C, (double)rows, gamma, beta, eps, mom, rm, rv, k.scale, k.shift, save_mean,
                        save_invstd, s.red, st))) return rc;
  if ((rc = bn_apply<T>(s.xh, nullptr, k.scale, k.shift, nullptr, nullptr, s.yh, rows, C, relu != 0, st))) return rc;
  return nhwc_to_nchw<T>(s.yh, N, C, H, W, y, st);
}

// k.scale | k.shift rebuilt in the op's workspace from the statistics the caller saved, which k.mean / k.invstd then point at
inline int coef_from_saved(BnCoef& k, int C, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                           hipStream_t st) {
  hipLaunchKernelGGL(coef_from_saved_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, C, gamma, beta, save_mean, save_invstd, k.scale, k.shift);
  HIP_CHECK_RET(hipGetLastError());
  k.mean = const_cast<float*>(save_mean); k.invstd = const_cast<float*>(save_invstd);   // read only from here on
  return MMSKIN_OK;
}

template <typename T>
int bn_bwd_op(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
              const float* save_invstd, float* dx, float* dgamma, float* dbeta, int N, int C, int H, int W, int relu,
              void* ws, hipStream_t st) {
  BnWs<T> s(ws, N, C, H, W);
  const size_t rows = (size_t)N * H * W;
  BnCoef k(s.coef, C);
  int rc;
  if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(dy, N, C, H, W, s.yh, st))) return rc;
  if ((rc = coef_from_saved(k, C, gamma, beta, save_mean, save_invstd, st))) return rc;
  if ((rc = bn_backward<T>(s.yh, s.xh, nullptr, relu ? MASK_FROM_X : MASK_NONE, rows, C, k, gamma, dgamma, dbeta, BnBwdCoef(s.coefbwd, C),
                           s.partial, s.red, s.dxh, nullptr, nullptr, 0.0, st))) return rc;
  return nhwc_to_nchw<T>(s.dxh, N, C, H, W, dx, st);
}

template <typename T>
struct StemWs {
  StageDesc* table; T* wv; T* dpool; StemBufs<T> b; size_t total;
  StemWs(void* ws, const StemGeom& g) {
    Carver c(ws);
    table = c.take<StageDesc>(1);
    b.img4 = c.take<T>((size_t)g.N * g.Hp * g.Wp * 4);
    b.wv = wv = c.take<T>(64 * 256);
    b.x0 = c.take<T>(g.rows() * 64);
    b.pool = c.take<T>(g.pooled() * 64);
    b.idx = c.take<uint8_t>(g.pooled() * 64);
    b.ssum = c.take<float>((size_t)stem_conv_stat_rows(g.N, g.OH, g.OW) * 64);
    b.ssq = c.take<float>((size_t)stem_conv_stat_rows(g.N, g.OH, g.OW) * 64);
    b.coef = c.take<float>(7 * 64);   // scale | shift | mean | invstd, and behind them cA | cB | cC
    b.coefbwd = BnCoef(b.coef, 64).gamma;
    dpool = c.take<T>(g.pooled() * 64);
    c.take<T>(g.rows() * 64);   // (a second full-resolution gradient nothing writes: keeps mmskin_stem_workspace_bytes what it was)
    b.dx0 = c.take<T>(g.rows() * 64);
    b.partial = c.take<float>((size_t)bn_bwd_partial_rows(g.rows(), 64) * 2 * 64);
    b.slab.floats = stem_wgrad_slab_bytes(g.N, g.OH, g.OW) / sizeof(float);
    b.slab.p = c.take<float>(b.slab.floats);
    b.dwv = c.take<float>(64 * 256);
    b.red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(64) / sizeof(double)), 64);
    total = c.cur;
  }
};

// pack, stage the weights, then the plans' training forward (batch statistics, no running buffers)
template <typename T>
int stem_fwd_core(StemWs<T>& s, const StemGeom& g, const float* x, const float* w, const float* gamma, const float* beta, float eps,
                  hipStream_t st) {
  int rc;
  if ((rc = stem_pack<T>(x, g.N, g.H, g.W, g.Hp, g.Wp, s.b.img4, st))) return rc;
  if ((rc = stage_one<T>(w, 64, 3, 49, true, s.wv, (T*)nullptr, s.table, st))) return rc;
  StemBn bn;
  bn.gamma = gamma; bn.beta = beta; bn.eps = eps; bn.batch_stats = true;
  return stem_forward<T>(s.b, g, nullptr, nullptr, bn, nullptr, st);
}

template <typename T>
int stem_fwd_op(const float* x, const float* w, const float* gamma, const float* beta, float* y, int N, int H,
                       int W, float eps, void* ws, hipStream_t st) {
  const StemGeom g(N, H, W);
  StemWs<T> s(ws, g);
  int rc;
  if ((rc = stem_fwd_core<T>(s, g, x, w, gamma, beta, eps, st))) return rc;
  return nhwc_to_nchw<T>(s.b.pool, N, 64, g.PH, g.PW, y, st);
}

template <typename T>
int stem_bwd_op(const float* dy, const float* x, const float* w, const float* gamma, const float* beta,
                       float* dw, float* dgamma, float* dbeta, int N, int H, int W, float eps, void* ws, hipStream_t st) {
  const StemGeom g(N, H, W);
  StemWs<T> s(ws, g);
  int rc;
  if ((rc = stem_fwd_core<T>(s, g, x, w, gamma, beta, eps, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(dy, N, 64, g.PH, g.PW, s.dpool, st))) return rc;
  if ((rc = stem_backward<T>(s.b, g, s.dpool, gamma, dgamma, dbeta, stem_sums_pooled(), nullptr, 0.0, st))) return rc;
  return stem_wgrad<T>(s.b, g, dw, nullptr, st);
}

// ---- MBConv family (mbconv.hip's launches, op by op): depthwise k x k, BatchNorm + ReLU6 / SiLU, squeeze-excitation, stochastic depth
template <typename T>
struct DwWs {
  T *xh, *yh, *wst, *dxh; float* partial; size_t total; int OH, OW;
  DwWs(void* ws, int N, int C, int H, int W, int k, int stride) {
    const int pad = k / 2;
    OH = (H + 2 * pad - k) / stride + 1; OW = (W + 2 * pad - k) / stride + 1;
    Carver c(ws);
    xh = c.take<T>((size_t)N * H * W * C);
    yh = c.take<T>((size_t)N * OH * OW * C);
    wst = c.take<T>((size_t)k * k * C);
    dxh = c.take<T>((size_t)N * H * W * C);
    partial = c.take<float>(dwconv3_wgrad_partial_floats(N, H, W, C, stride, k));   // the sizing finish_plan uses
    total = c.cur;
  }
};

template <typename T>
int dw_fwd_op(const float* x, const float* w, float* y, int N, int C, int H, int W, int k, int stride, int Cv, void* ws, hipStream_t st) {
  DwWs<T> s(ws, N, C, H, W, k, stride);
  int rc;
  if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
  if ((rc = dw_stage_weights<T>(w, Cv, C, s.wst, st, k))) return rc;
  if ((rc = dwconv3_fwd<T>(s.xh, s.wst, N, H, W, C, stride, s.yh, st, k))) return rc;
  return nhwc_to_nchw<T>(s.yh, N, C, s.OH, s.OW, y, st);
}

template <typename T>
int dw_bwd_op(const float* dy, const float* x, const float* w, float* dx, float* dw, int N, int C, int H, int W, int k, int stride,
              int Cv, void* ws, hipStream_t st) {
  DwWs<T> s(ws, N, C, H, W, k, stride);
  int rc;
  if ((rc = nchw_to_nhwc<T>(dy, N, C, s.OH, s.OW, s.yh, st))) return rc;
  if (dx) {
    if ((rc = dw_stage_weights<T>(w, Cv, C, s.wst, st, k))) return rc;
    if ((rc = dwconv3_dgrad<T>(s.yh, s.wst, N, H, W, C, stride, s.dxh, st, k))) return rc;
    if ((rc = nhwc_to_nchw<T>(s.dxh, N, C, H, W, dx, st))) return rc;
  }
  if (dw) {
    if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
    if ((rc = dwconv3_wgrad<T>(s.yh, s.xh, N, H, W, C, stride, s.partial, dw, Cv, st, k))) return rc;
  }
  return MMSKIN_OK;
}

template <typename T>
struct BnActWs {
  T *xh, *yh, *rh, *dyh, *dxh, *dzh; float *ssum, *ssq, *tab, *coef, *coefbwd, *partial; ColScratch red; size_t total;
  BnActWs(void* ws, int N, int C, int H, int W) {
    Carver c(ws);
    const size_t rows = (size_t)N * H * W;
    xh = c.take<T>(rows * C); yh = c.take<T>(rows * C); rh = c.take<T>(rows * C);
    dyh = c.take<T>(rows * C); dxh = c.take<T>(rows * C); dzh = c.take<T>(rows * C);
    ssum = c.take<float>((size_t)column_stats_rows(rows, C) * C);
    ssq = c.take<float>((size_t)column_stats_rows(rows, C) * C);
    tab = c.take<float>(2 * (size_t)C);
    coef = c.take<float>(5 * (size_t)C);   // forward: all five slots; backward: scale | shift | cA | cB | cC
    coefbwd = BnCoef(coef, C).mean;
    partial = c.take<float>((size_t)bn_bwd_partial_rows(rows, C) * 2 * C);
    red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(C) / sizeof(double)), C);
    total = c.cur;
  }
};
// act 0 none, 1 ReLU, 2 ReLU6, 3 SiLU -> bn_apply's (relu, cap) and the BatchNorm-backward mask mode (2 / 3: MBPlan::act_cap / act_mask)
inline float act_cap(int act) { return act == 2 ? 6.f : act == 3 ? -1.f : 0.f; }
inline int act_mask(int act) { return act == 1 ? MASK_FROM_Y : act == 2 ? MASK_FROM_Y6 : act == 3 ? MASK_SILU_X : MASK_NONE; }

template <typename T>
int bn_act_fwd_op(const float* x, const float* res, const float* gamma, const float* beta, float* rm, float* rv, float* y, float* save_mean,
                  float* save_invstd, int N, int C, int H, int W, float eps, float mom, int act, void* ws, hipStream_t st) {
  const size_t rows = (size_t)N * H * W;
  BnActWs<T> s(ws, N, C, H, W);
  int rc, nr = 0;
  if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
  if (res && (rc = nchw_to_nhwc<T>(res, N, C, H, W, s.rh, st))) return rc;
  // the plan's sequence behind a depthwise conv: column sums -> statistics table -> coefficient vectors -> apply
  if ((rc = column_stats<T>(s.xh, rows, C, s.ssum, s.ssq, &nr, st))) return rc;
  if ((rc = bn_table_finalize(s.ssum, s.ssq, nr, C, C, (double)rows, s.tab, s.tab + C, s.red, st))) return rc;
  const BnCoef k(s.coef, C);
  if ((rc = bn_coef_from_table(s.tab, s.tab + C, C, C, gamma, beta, eps, mom, (double)rows, rm, rv, true, s.coef, st))) return rc;
  HIP_CHECK_RET(hipMemcpyAsync(save_mean, k.mean, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  HIP_CHECK_RET(hipMemcpyAsync(save_invstd, k.invstd, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  if ((rc = bn_apply<T>(s.xh, res ? s.rh : nullptr, k.scale, k.shift, nullptr, nullptr, s.yh, rows, C, act != 0, st, nullptr, act_cap(act)))) return rc;
  return nhwc_to_nchw<T>(s.yh, N, C, H, W, y, st);
}

template <typename T>
int bn_act_bwd_op(const float* dy, const float* x, const float* y, const float* gamma, const float* beta, const float* save_mean,
                  const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta, int N, int C, int H, int W, int act,
                  void* ws, hipStream_t st) {
  const size_t rows = (size_t)N * H * W;
  BnActWs<T> s(ws, N, C, H, W);
  BnCoef k(s.coef, C);
  int rc;
  if ((rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(y, N, C, H, W, s.yh, st))) return rc;   // the forward's stored y: exact in T, MASK_FROM_Y6 reads it
  if ((rc = nchw_to_nhwc<T>(dy, N, C, H, W, s.dyh, st))) return rc;
  if ((rc = coef_from_saved(k, C, gamma, beta, save_mean, save_invstd, st))) return rc;
  if ((rc = bn_backward<T>(s.dyh, s.xh, s.yh, act_mask(act), rows, C, k, gamma, dgamma, dbeta, BnBwdCoef(s.coefbwd, C), s.partial, s.red,
                           s.dxh, dres ? s.dzh : (T*)nullptr, nullptr, 0.0, st))) return rc;
  if (dres && (rc = nhwc_to_nchw<T>(s.dzh, N, C, H, W, dres, st))) return rc;   // the residual's gradient is the masked dy
  return nhwc_to_nchw<T>(s.dxh, N, C, H, W, dx, st);
}

template <typename T>
struct SeWs {
  T *yh, *yseh, *dyh, *dxh; float *w1p, *w2p, *b2p, *s, *z1, *a1, *z2, *g, *tmp; size_t total;
  SeWs(void* ws, int N, int Cp, int Csq, int HW) {
    Carver c(ws);
    const size_t act = (size_t)N * HW * Cp;
    yh = c.take<T>(act); yseh = c.take<T>(act); dyh = c.take<T>(act); dxh = c.take<T>(act);
    w1p = c.take<float>((size_t)Csq * Cp); w2p = c.take<float>((size_t)Cp * Csq); b2p = c.take<float>(Cp);
    s = c.take<float>((size_t)N * Cp); z1 = c.take<float>((size_t)N * Csq); a1 = c.take<float>((size_t)N * Csq);
    z2 = c.take<float>((size_t)N * Cp); g = c.take<float>((size_t)N * Cp);
    tmp = c.take<float>(se_backward_tmp_floats(N, Cp, Csq));
    total = c.cur;
  }
  SEArgs args(int N, int HW, int C, int Cp, int Csq, const float* b1) const {
    SEArgs a;
    a.N = N; a.HW = HW; a.C = C; a.Cp = Cp; a.Csq = Csq;
    a.w1p = w1p; a.b1 = b1; a.w2p = w2p; a.b2p = b2p;
    a.s = s; a.z1 = z1; a.a1 = a1; a.z2 = z2; a.g = g;
    return a;
  }
};

// y [N][Cp][HW] -> NHWC T, the three padded parameter copies (the plan's staging), then the plan's forward chain
template <typename T>
int se_fwd_core(SeWs<T>& s, const float* y, const float* w1, const float* b1, const float* w2, const float* b2, int N, int C, int Cp,
                int Csq, int HW, hipStream_t st) {
  int rc;
  if ((rc = nchw_to_nhwc<T>(y, N, Cp, HW, 1, s.yh, st))) return rc;
  if ((rc = pad_matrix(w1, Csq, C, Csq, Cp, s.w1p, st))) return rc;
  if ((rc = pad_matrix(w2, C, Csq, Cp, Csq, s.w2p, st))) return rc;
  if ((rc = pad_matrix(b2, 1, C, 1, Cp, s.b2p, st))) return rc;
  return se_forward<T>(s.args(N, HW, C, Cp, Csq, b1), s.yh, s.yseh, nullptr, st);
}

template <typename T>
int se_fwd_op(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* yse, int N, int C, int Cp, int Csq,
              int HW, void* ws, hipStream_t st) {
  SeWs<T> s(ws, N, Cp, Csq, HW);
  int rc;
  if ((rc = se_fwd_core<T>(s, y, w1, b1, w2, b2, N, C, Cp, Csq, HW, st))) return rc;
  return nhwc_to_nchw<T>(s.yseh, N, Cp, HW, 1, yse, st);
}

template <typename T>
int se_bwd_op(const float* dyse, const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* dy, float* dw1,
              float* db1, float* dw2, float* db2, int N, int C, int Cp, int Csq, int HW, void* ws, hipStream_t st) {
  SeWs<T> s(ws, N, Cp, Csq, HW);
  int rc;
  if ((rc = se_fwd_core<T>(s, y, w1, b1, w2, b2, N, C, Cp, Csq, HW, st))) return rc;   // the activations backward reads
  if ((rc = nchw_to_nhwc<T>(dyse, N, Cp, HW, 1, s.dyh, st))) return rc;
  if ((rc = se_backward<T>(s.args(N, HW, C, Cp, Csq, b1), s.dyh, s.yh, s.tmp, dw1, db1, dw2, db2, s.dxh, nullptr, st))) return rc;
  return nhwc_to_nchw<T>(s.dxh, N, Cp, HW, 1, dy, st);
}

// flat [N][per_sample] fp32 <-> T (the converters with H = W = 1 are plain element-type conversions)
template <typename T>
struct SdWs {
  T *ah, *rh, *oh; size_t total;
  SdWs(void* ws, int N, int64_t per) {
    Carver c(ws);
    ah = c.take<T>((size_t)N * per); rh = c.take<T>((size_t)N * per); oh = c.take<T>((size_t)N * per);
    total = c.cur;
  }
};
template <typename T>
int sd_op(const float* a, const float* res, const float* mask, float* out, int N, int64_t per, void* ws, hipStream_t st) {
  SdWs<T> s(ws, N, per);
  int rc;
  if ((rc = nchw_to_nhwc<T>(a, N, (int)per, 1, 1, s.ah, st))) return rc;
  if (res) {
    if ((rc = nchw_to_nhwc<T>(res, N, (int)per, 1, 1, s.rh, st))) return rc;
    if ((rc = sd_residual_add<T>(s.ah, s.rh, mask, N, (size_t)per, s.oh, st))) return rc;
  } else if ((rc = sd_row_scale<T>(s.ah, mask, N, (size_t)per, s.oh, st))) return rc;
  return nhwc_to_nchw<T>(s.oh, N, (int)per, 1, 1, out, st);
}

// algebraic BatchNorm backward of an expanding 1x1 convolution (abn_backward_impl); the slab serves whichever Gram launch mode runs
struct AbnWs {
  bf16_t *gh, *yh, *dyh, *wd; float *bias, *coef, *S, *cs, *gram, *slab; size_t total;
  AbnWs(void* ws, int N, int Cw, int C4, int H, int W) {
    Carver c(ws);
    const size_t M = (size_t)N * H * W;
    gh = c.take<bf16_t>(M * C4); yh = c.take<bf16_t>(M * Cw); dyh = c.take<bf16_t>(M * Cw);
    wd = c.take<bf16_t>((size_t)Cw * (C4 + Cw)); bias = c.take<float>(Cw); coef = c.take<float>(3 * (size_t)C4);
    S = c.take<float>(((size_t)C4 + 256) * Cw); cs = c.take<float>(256); gram = c.take<float>((size_t)256 * Cw);
    size_t sb = 0;
    for (int mode = 0; mode < 3; ++mode) sb = std::max(sb, wgrad_gram_slab_bytes((int)M, mode == 2 ? 0 : C4, Cw, mode));
    slab = c.take<float>(sb / sizeof(float));
    total = c.cur;
  }
};
struct GramStatsWs {
  bf16_t* yh; float *gram, *cs, *slab; size_t total;
  GramStatsWs(void* ws, int N, int Cw, int C4, int H, int W) {
    Carver c(ws);
    const size_t M = (size_t)N * H * W;
    yh = c.take<bf16_t>(M * Cw); gram = c.take<float>((size_t)256 * Cw); cs = c.take<float>(256);
    slab = c.take<float>(wgrad_gram_slab_bytes((int)M, 0, Cw, 2) / sizeof(float));
    total = c.cur;
  }
};

// ---- DenseNet / VGG plan kernels, op by op (densenet.hip's block and transition bodies, vgg.hip's pools)
// several stage descriptors at once (the table lives in the workspace; the host copy must outlive the transfer)
inline int upload_table(const std::vector<StageDesc>& host, StageDesc* dev, hipStream_t st) {
  HIP_CHECK_RET(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(StageDesc), hipMemcpyHostToDevice, st));
  HIP_CHECK_RET(hipStreamSynchronize(st));
  return MMSKIN_OK;
}

// One dense block of L layers on its own: the plan's DBlock with offsets into this carve.  Flat parameters per layer, torchvision order:
// norm1.weight | norm1.bias [Cin], conv1.weight [128][Cin], norm2.weight | norm2.bias [128], conv2.weight [32][128][3][3]; flat buffers
// per layer: norm1.running_mean | running_var [Cin], norm2.running_mean | running_var [128].  es: element size of the compute dtype.
struct DenseBlockWs {
  DBlock b;
  std::vector<StageDesc> table;
  int max_stage_elems = 0;
  int red_C = 0;   // channels the reduction scratch was carved for (bn_reduce_scratch)
  int64_t param_numel = 0, buffer_numel = 0, wf_elems = 0;
  size_t table_off, xh_off, wf_off, wd_off, stat_off, stat_bytes, partial_off, coefbwd_off, defer_off, red_off, slab_off, slab_bytes, sB_off[2], sU_off,
      sA_off[2], sZ_off, rbuf_off, total;
  DenseBlockWs(int N, int C0, int L, int H, int W, size_t es) {
    b.H = H; b.W = W; b.C0 = C0; b.Ctot = C0 + DENSE_GROWTH * L; b.rows = (size_t)N * H * W;
    auto bn = [&](int C) {
      BNRef r;
      r.g_off = param_numel; r.b_off = param_numel + C; param_numel += 2 * C;
      r.rm_off = buffer_numel; r.rv_off = buffer_numel + C; buffer_numel += 2 * C;
      return r;
    };
    int64_t wf = 0, wd = 0;
    for (int i = 0; i < L; ++i) {
      DLayer l = {};
      dense_layer_geom(l, C0, i);
      l.n1 = bn(l.Cin);
      l.w1_off = param_numel; param_numel += (int64_t)DENSE_BOTTLE * l.Cin;
      l.n2 = bn(DENSE_BOTTLE);
      l.w2_off = param_numel; param_numel += (int64_t)DENSE_GROWTH * DENSE_BOTTLE * 9;
      dense_stage_layer(l, table, wf, wd, max_stage_elems);
      b.layers.push_back(l);
    }
    wf_elems = wf;
    size_t cur = 0;
    table_off = carve(cur, table.size() * sizeof(StageDesc));
    xh_off = carve(cur, b.rows * C0 * es);
    wf_off = carve(cur, (size_t)wf * es);
    wd_off = carve(cur, (size_t)wf * es);
    b.cat_off = carve(cur, b.rows * b.Ctot * es);
    b.dcat_off = carve(cur, b.rows * b.Ctot * es);
    b.tab_off = carve(cur, 2 * (size_t)b.Ctot * sizeof(float));
    size_t stat_floats = (size_t)column_stats_rows(b.rows, C0) * 2 * C0, partial = 0, slab = 0, big = b.rows * b.Ctot;
    int maxC = std::max(DENSE_BOTTLE, b.Ctot);
    for (DLayer& l : b.layers) {
      l.t_off = carve(cur, b.rows * l.Cp * es);
      l.a_off = carve(cur, b.rows * DENSE_BOTTLE * es);
      l.u_off = carve(cur, b.rows * DENSE_BOTTLE * es);
      l.coef1_off = carve(cur, 5 * (size_t)l.Cp * sizeof(float));
      l.coef2_off = carve(cur, 4 * (size_t)DENSE_BOTTLE * sizeof(float));
      dense_fold_norm2(l, table);
      dense_layer_needs(N, H, W, b.rows, l, stat_floats, partial, slab);
      big = std::max(big, b.rows * l.Cp);
      maxC = std::max(maxC, l.Cp);
    }
    stat_bytes = align_up(stat_floats * sizeof(float), 256);
    stat_off = carve(cur, 2 * stat_bytes);
    partial_off = carve(cur, partial);
    coefbwd_off = carve(cur, 3 * (size_t)maxC * sizeof(float));
    defer_off = carve(cur, 2 * (size_t)maxC * sizeof(float));
    red_C = maxC;
    red_off = carve(cur, bn_reduce_scratch_bytes(red_C));
    slab_bytes = slab;
    slab_off = carve(cur, slab);
    for (int q = 0; q < 2; ++q) sB_off[q] = carve(cur, b.rows * DENSE_G_PAD * es);
    sU_off = carve(cur, b.rows * DENSE_BOTTLE * es);
    for (int q = 0; q < 2; ++q) sA_off[q] = carve(cur, b.rows * DENSE_BOTTLE * es);
    sZ_off = carve(cur, big * es);
    rbuf_off = carve(cur, (size_t)buffer_numel * sizeof(float));   // the backward entry's forward pass updates these, not the caller's
    total = cur;
  }
  template <typename T>
  DenseRun<T> run(int N, unsigned char* ws, const float* params, float* buffers, float* grads) const {
    DenseRun<T> r;
    r.N = N; r.ws = ws; r.params = params; r.buffers = buffers; r.grads = grads;
    r.wf = reinterpret_cast<T*>(ws + wf_off); r.wd = reinterpret_cast<T*>(ws + wd_off);
    r.stat_sum = reinterpret_cast<float*>(ws + stat_off); r.stat_sq = reinterpret_cast<float*>(ws + stat_off + stat_bytes);
    r.red = bn_reduce_scratch(ws + red_off, red_C);
    for (int q = 0; q < 2; ++q) { r.sBq[q] = reinterpret_cast<T*>(ws + sB_off[q]); r.sAq[q] = reinterpret_cast<T*>(ws + sA_off[q]); }
    r.sU = reinterpret_cast<T*>(ws + sU_off); r.sZ = reinterpret_cast<T*>(ws + sZ_off);
    r.slab = wgrad_slab_at(ws, slab_off, slab_bytes); r.partial = reinterpret_cast<float*>(ws + partial_off);
    r.cA = reinterpret_cast<float*>(ws + coefbwd_off); r.defer = reinterpret_cast<float*>(ws + defer_off);
    return r;
  }
};

// x -> cat prefix, staged weights, the input slice's statistics, then the plan's block body
template <typename T>
int dense_block_fwd_core(DenseBlockWs& w, DenseRun<T>& r, const float* x, int N, bool training, hipStream_t st) {
  unsigned char* ws = r.ws;
  DBlock& b = w.b;
  StageDesc* table = reinterpret_cast<StageDesc*>(ws + w.table_off);
  T* xh = reinterpret_cast<T*>(ws + w.xh_off);
  int rc;
  if ((rc = upload_table(w.table, table, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(x, N, b.C0, b.H, b.W, xh, st))) return rc;
  if ((rc = slice_scatter<T>(xh, b.C0, b.C0, reinterpret_cast<T*>(ws + b.cat_off), b.Ctot, b.rows, st))) return rc;
  if ((rc = stage_weights<T>(table, (int)w.table.size(), w.max_stage_elems, r.params, r.wf, r.wd, training, st, training ? nullptr : r.buffers, 1e-5f))) return rc;
  if (!training && (rc = bn_eval_table(table, (int)w.table.size(), DENSE_BOTTLE, r.params, r.buffers, ws, 1e-5f, st))) return rc;
  if (training && (rc = dense_table_from_slice<T>(r, b, 0, b.C0, st))) return rc;
  return dense_block_forward<T>(r, b, training, st);
}
template <typename T>
int dense_block_fwd_op(const float* x, const float* params, float* buffers, float* cat, float* table_out, int N, int C0, int L, int H, int W,
                       bool training, void* wsp, hipStream_t st) {
  DenseBlockWs w(N, C0, L, H, W, sizeof(T));
  unsigned char* ws = (unsigned char*)wsp;
  DenseRun<T> r = w.run<T>(N, ws, params, buffers, nullptr);
  int rc;
  if ((rc = dense_block_fwd_core<T>(w, r, x, N, training, st))) return rc;
  if (training && table_out) HIP_CHECK_RET(hipMemcpyAsync(table_out, ws + w.b.tab_off, 2 * (size_t)w.b.Ctot * sizeof(float), hipMemcpyDeviceToDevice, st));
  return nhwc_to_nchw<T>(reinterpret_cast<const T*>(ws + w.b.cat_off), N, w.b.Ctot, H, W, cat, st);
}
template <typename T>
int dense_block_bwd_op(const float* dcat, const float* x, const float* params, float* dx, float* grads, int N, int C0, int L, int H, int W,
                       void* wsp, hipStream_t st) {
  DenseBlockWs w(N, C0, L, H, W, sizeof(T));
  unsigned char* ws = (unsigned char*)wsp;
  float* rbuf = reinterpret_cast<float*>(ws + w.rbuf_off);
  DenseRun<T> r = w.run<T>(N, ws, params, rbuf, grads);
  int rc;
  HIP_CHECK_RET(hipMemsetAsync(rbuf, 0, (size_t)w.buffer_numel * sizeof(float), st));
  if ((rc = dense_block_fwd_core<T>(w, r, x, N, true, st))) return rc;   // the activations and coefficients backward reads
  T* dc = reinterpret_cast<T*>(ws + w.b.dcat_off);
  T* xh = reinterpret_cast<T*>(ws + w.xh_off);
  if ((rc = nchw_to_nhwc<T>(dcat, N, w.b.Ctot, H, W, dc, st))) return rc;
  if ((rc = dense_block_backward<T>(r, w.b, st))) return rc;
  if ((rc = slice_pack<T>(dc, w.b.Ctot, C0, C0, w.b.rows, nullptr, nullptr, xh, st))) return rc;
  return nhwc_to_nchw<T>(xh, N, C0, H, W, dx, st);
}

// One transition on its own: block geometry with Ctot = C (the transition reads the whole concatenated activation).  Flat parameters:
// norm.weight | norm.bias [C], conv.weight [C/2][C]; flat buffers: running_mean | running_var [C].
struct DenseTransWs {
  DBlock b;
  DTrans t;
  StageDesc desc;
  int PH, PW;
  int red_C = 0;   // channels the reduction scratch was carved for (bn_reduce_scratch)
  size_t table_off, wf_off, wd_off, sC_off, dst_off, sZ_off, partial_off, coefbwd_off, red_off, slab_off, slab_bytes, rbuf_off, total;
  DenseTransWs(int N, int C, int H, int W, int Cdst, size_t es) {
    b.H = H; b.W = W; b.C0 = C; b.Ctot = C; b.rows = (size_t)N * H * W;
    PH = H / 2; PW = W / 2;
    t = DTrans();
    t.C = C;
    t.n.g_off = 0; t.n.b_off = C; t.n.rm_off = 0; t.n.rv_off = C;
    t.w_off = 2 * (int64_t)C; t.wf = 0; t.wd = 0;
    {
      std::vector<StageDesc> one;
      int64_t wf = 0, wd = 0;
      int max_elems = 0;
      stage_append(one, t.w_off, C / 2, C, 1, C / 2, C, wf, wd, max_elems, t.wf, t.wd);   // as build_dense_plan stages a transition
      desc = one[0];
    }
    const ConvShape ct = {N, H, W, C, C / 2, 1, 1, 1, 0};
    size_t cur = 0;
    table_off = carve(cur, sizeof(StageDesc));
    wf_off = carve(cur, (size_t)C / 2 * C * es);
    wd_off = carve(cur, (size_t)C / 2 * C * es);
    b.cat_off = carve(cur, b.rows * C * es);
    b.dcat_off = carve(cur, b.rows * C * es);
    b.tab_off = carve(cur, 2 * (size_t)C * sizeof(float));
    t.tt_off = carve(cur, b.rows * C * es);
    t.coef_off = carve(cur, 5 * (size_t)C * sizeof(float));
    sC_off = carve(cur, b.rows * (C / 2) * es);
    dst_off = carve(cur, (size_t)N * PH * PW * Cdst * es);
    sZ_off = carve(cur, b.rows * C * es);
    partial_off = carve(cur, dense_partial_bytes(b.rows, C));
    coefbwd_off = carve(cur, 3 * (size_t)C * sizeof(float));
    red_C = C;
    red_off = carve(cur, bn_reduce_scratch_bytes(red_C));
    slab_bytes = conv_wgrad_slab_bytes(ct);
    slab_off = carve(cur, slab_bytes);
    rbuf_off = carve(cur, 2 * (size_t)C * sizeof(float));
    total = cur;
  }
  template <typename T>
  DenseRun<T> run(int N, unsigned char* ws, const float* params, float* buffers, float* grads) const {
    DenseRun<T> r;
    r.N = N; r.ws = ws; r.params = params; r.buffers = buffers; r.grads = grads;
    r.wf = reinterpret_cast<T*>(ws + wf_off); r.wd = reinterpret_cast<T*>(ws + wd_off);
    r.red = bn_reduce_scratch(ws + red_off, red_C);
    r.sZ = reinterpret_cast<T*>(ws + sZ_off); r.sC = reinterpret_cast<T*>(ws + sC_off);
    r.slab = wgrad_slab_at(ws, slab_off, slab_bytes); r.partial = reinterpret_cast<float*>(ws + partial_off);
    r.cA = reinterpret_cast<float*>(ws + coefbwd_off);
    return r;
  }
};
// x and the block's table into the carve, staged weight, the caller's destination rows, then the plan's transition body
template <typename T>
int dense_trans_fwd_core(DenseTransWs& w, DenseRun<T>& r, const float* x, const float* table, const float* dst_in, int N, int Cdst, bool training,
                         hipStream_t st) {
  unsigned char* ws = r.ws;
  StageDesc* tdev = reinterpret_cast<StageDesc*>(ws + w.table_off);
  T* dst = reinterpret_cast<T*>(ws + w.dst_off);
  int rc;
  HIP_CHECK_RET(hipMemcpyAsync(tdev, &w.desc, sizeof(StageDesc), hipMemcpyHostToDevice, st));
  HIP_CHECK_RET(hipStreamSynchronize(st));
  HIP_CHECK_RET(hipMemcpyAsync(ws + w.b.tab_off, table, 2 * (size_t)w.t.C * sizeof(float), hipMemcpyDeviceToDevice, st));
  if ((rc = nchw_to_nhwc<T>(x, N, w.t.C, w.b.H, w.b.W, reinterpret_cast<T*>(ws + w.b.cat_off), st))) return rc;
  if (dst_in && (rc = nchw_to_nhwc<T>(dst_in, N, Cdst, w.PH, w.PW, dst, st))) return rc;
  if ((rc = stage_weights<T>(tdev, 1, w.t.C / 2 * w.t.C, r.params, r.wf, r.wd, true, st))) return rc;
  return dense_transition_forward<T>(r, w.b, w.t, dst, Cdst, training, st);
}
template <typename T>
int dense_trans_fwd_op(const float* x, const float* table, const float* params, float* buffers, float* dst, float* conv_out, int N, int C, int H,
                       int W, int Cdst, bool training, void* wsp, hipStream_t st) {
  DenseTransWs w(N, C, H, W, Cdst, sizeof(T));
  unsigned char* ws = (unsigned char*)wsp;
  DenseRun<T> r = w.run<T>(N, ws, params, buffers, nullptr);
  int rc;
  if ((rc = dense_trans_fwd_core<T>(w, r, x, table, dst, N, Cdst, training, st))) return rc;
  if (conv_out && (rc = nhwc_to_nchw<T>(r.sC, N, C / 2, H, W, conv_out, st))) return rc;   // the stored conv output the pool read
  return nhwc_to_nchw<T>(reinterpret_cast<const T*>(ws + w.dst_off), N, Cdst, w.PH, w.PW, dst, st);
}
template <typename T>
int dense_trans_bwd_op(const float* dnext, const float* x, const float* table, const float* params, float* dx, float* grads, float* dconv_out,
                       int N, int C, int H, int W, int Cdst, void* wsp, hipStream_t st) {
  DenseTransWs w(N, C, H, W, Cdst, sizeof(T));
  unsigned char* ws = (unsigned char*)wsp;
  float* rbuf = reinterpret_cast<float*>(ws + w.rbuf_off);
  DenseRun<T> r = w.run<T>(N, ws, params, rbuf, grads);
  T* dst = reinterpret_cast<T*>(ws + w.dst_off);
  int rc;
  HIP_CHECK_RET(hipMemsetAsync(rbuf, 0, 2 * (size_t)C * sizeof(float), st));
  if ((rc = dense_trans_fwd_core<T>(w, r, x, table, nullptr, N, Cdst, true, st))) return rc;   // tt and the coefficients backward reads
  if ((rc = nchw_to_nhwc<T>(dnext, N, Cdst, w.PH, w.PW, dst, st))) return rc;                  // the next block's dcat, pitch Cdst
  if ((rc = dense_transition_backward<T>(r, w.b, w.t, dst, Cdst, st))) return rc;
  if (dconv_out && (rc = nhwc_to_nchw<T>(r.sC, N, C / 2, H, W, dconv_out, st))) return rc;   // what avgpool2_bwd stored: the conv output's gradient
  return nhwc_to_nchw<T>(reinterpret_cast<const T*>(ws + w.b.dcat_off), N, C, H, W, dx, st);
}

// slice_stats + bn_table_finalize on channels [c0, c0 + C) of a [rows][pitch] matrix (table_from_slice's pair)
template <typename T>
struct SliceStatsWs {
  T* xh; float* stat; ColScratch red; size_t total;
  SliceStatsWs(void* ws, int64_t rows, int pitch, int C) {
    Carver c(ws);
    xh = c.take<T>((size_t)rows * pitch);
    stat = c.take<float>((size_t)column_stats_rows((size_t)rows, C) * 2 * C);
    red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(C) / sizeof(double)), C);
    total = c.cur;
  }
};
template <typename T>
int slice_stats_op(const float* x, int64_t rows, int pitch, int c0, int C, float* mean, float* var, void* ws, hipStream_t st) {
  SliceStatsWs<T> s(ws, rows, pitch, C);
  int rc, nr = 0;
  if ((rc = nchw_to_nhwc<T>(x, (int)rows, pitch, 1, 1, s.xh, st))) return rc;
  if ((rc = slice_stats<T>(s.xh + c0, pitch, C, (size_t)rows, s.stat, s.stat + C, &nr, st))) return rc;
  return bn_table_finalize(s.stat, s.stat + C, nr, 2 * C, C, (double)rows, mean, var, s.red, st);
}

// VGG: 2x2 max-pool of a post-ReLU map with its argmax bytes, and the fused un-pool + ReLU mask
template <typename T>
struct MaxpoolWs {
  T *yh, *ph, *dph, *dzh; uint8_t* idx; size_t total; int PH, PW;
  MaxpoolWs(void* ws, int N, int C, int H, int W) {
    PH = H / 2; PW = W / 2;
    Carver c(ws);
    const size_t rows = (size_t)N * H * W, prows = (size_t)N * PH * PW;
    yh = c.take<T>(rows * C); ph = c.take<T>(prows * C); idx = c.take<uint8_t>(prows * C);
    dph = c.take<T>(prows * C); dzh = c.take<T>(rows * C);
    total = c.cur;
  }
};
template <typename T>
int maxpool_fwd_op(const float* y, float* pooled, uint8_t* idx, int N, int C, int H, int W, void* ws, hipStream_t st) {
  MaxpoolWs<T> s(ws, N, C, H, W);
  int rc;
  if ((rc = nchw_to_nhwc<T>(y, N, C, H, W, s.yh, st))) return rc;
  if ((rc = maxpool2_fwd<T>(s.yh, N, H, W, C, s.ph, s.idx, st))) return rc;
  if (idx) HIP_CHECK_RET(hipMemcpyAsync(idx, s.idx, (size_t)N * s.PH * s.PW * C, hipMemcpyDeviceToDevice, st));
  return pooled ? nhwc_to_nchw<T>(s.ph, N, C, s.PH, s.PW, pooled, st) : MMSKIN_OK;
}
template <typename T>
int maxpool_bwd_op(const float* dpool, const float* y, float* dz, int N, int C, int H, int W, void* ws, hipStream_t st) {
  MaxpoolWs<T> s(ws, N, C, H, W);
  int rc;
  if ((rc = maxpool_fwd_op<T>(y, nullptr, nullptr, N, C, H, W, ws, st))) return rc;   // the argmax bytes backward reads
  if ((rc = nchw_to_nhwc<T>(dpool, N, C, s.PH, s.PW, s.dph, st))) return rc;
  if ((rc = maxpool2_bwd_relu<T>(s.dph, s.idx, s.yh, N, H, W, C, s.dzh, st))) return rc;
  return nhwc_to_nchw<T>(s.dzh, N, C, H, W, dz, st);
}

template <typename T>
struct AdaptivePoolWs {
  T *xh, *dxh; size_t total;
  AdaptivePoolWs(void* ws, int N, int C, int H, int W) {
    Carver c(ws);
    xh = c.take<T>((size_t)N * H * W * C); dxh = c.take<T>((size_t)N * H * W * C);
    total = c.cur;
  }
};
template <typename T>
int adaptive_fwd_op(const float* x, float* out, int N, int C, int H, int W, void* ws, hipStream_t st) {
  AdaptivePoolWs<T> s(ws, N, C, H, W);
  if (int rc = nchw_to_nhwc<T>(x, N, C, H, W, s.xh, st)) return rc;
  return adaptive_avgpool_fwd<T>(s.xh, N, H, W, C, 7, 7, out, st);
}
template <typename T>
int adaptive_bwd_op(const float* dout, float* dx, int N, int C, int H, int W, void* ws, hipStream_t st) {
  AdaptivePoolWs<T> s(ws, N, C, H, W);
  if (int rc = adaptive_avgpool_bwd<T>(dout, N, H, W, C, 7, 7, s.dxh, st)) return rc;
  return nhwc_to_nchw<T>(s.dxh, N, C, H, W, dx, st);
}

// DynamicCNN: GroupNorm(8, C) + ReLU (+ 2x2 max-pool) and its backward, which recomputes the forward's statistics (and argmax bytes) first
template <typename T>
struct GroupNormWs {
  T *yh, *oh, *gh, *dyh; uint8_t* idx; float *mean, *rstd, *sums, *partial, *dg, *db; double* stat; ColScratch red; size_t total; int PH, PW;
  GroupNormWs(void* ws, int N, int C, int H, int W, bool pool) {
    PH = pool ? H / 2 : H; PW = pool ? W / 2 : W;
    Carver c(ws);
    const size_t rows = (size_t)N * H * W, orows = (size_t)N * PH * PW;
    yh = c.take<T>(rows * C); oh = c.take<T>(orows * C); idx = c.take<uint8_t>(pool ? orows * C : 0);
    gh = c.take<T>(orows * C); dyh = c.take<T>(rows * C);
    mean = c.take<float>((size_t)N * 8); rstd = c.take<float>((size_t)N * 8); sums = c.take<float>((size_t)N * 16);
    stat = c.take<double>(gn8_stat_scratch_bytes(N) / sizeof(double));
    partial = c.take<float>(gn8_bwd_partial_bytes(N, C) / sizeof(float));
    dg = c.take<float>(C); db = c.take<float>(C);
    red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(C) / sizeof(double)), C);
    total = c.cur;
  }
};
template <typename T>
int groupnorm_fwd_op(const float* y, const float* gamma, const float* beta, float* out, uint8_t* idx, float* mean, float* rstd, int N, int C, int H,
                     int W, bool pool, float eps, void* ws, hipStream_t st) {
  GroupNormWs<T> s(ws, N, C, H, W, pool);
  int rc;
  if ((rc = nchw_to_nhwc<T>(y, N, C, H, W, s.yh, st))) return rc;
  if ((rc = gn8_stats<T>(s.yh, N, H * W, C, eps, s.stat, s.mean, s.rstd, st))) return rc;
  if (mean) HIP_CHECK_RET(hipMemcpyAsync(mean, s.mean, (size_t)N * 8 * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (rstd) HIP_CHECK_RET(hipMemcpyAsync(rstd, s.rstd, (size_t)N * 8 * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (pool) {
    if ((rc = gn8_relu_pool_apply<T>(s.yh, s.mean, s.rstd, gamma, beta, N, H, W, C, s.oh, s.idx, st))) return rc;
    if (idx) HIP_CHECK_RET(hipMemcpyAsync(idx, s.idx, (size_t)N * s.PH * s.PW * C, hipMemcpyDeviceToDevice, st));
  } else if ((rc = gn8_relu_apply<T>(s.yh, s.mean, s.rstd, gamma, beta, N, H, W, C, s.oh, st))) {
    return rc;
  }
  return out ? nhwc_to_nchw<T>(s.oh, N, C, s.PH, s.PW, out, st) : MMSKIN_OK;
}
template <typename T>
int groupnorm_bwd_op(const float* gout, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta, int N, int C,
                     int H, int W, bool pool, float eps, void* ws, hipStream_t st) {
  GroupNormWs<T> s(ws, N, C, H, W, pool);
  int rc;
  if ((rc = groupnorm_fwd_op<T>(y, gamma, beta, nullptr, nullptr, nullptr, nullptr, N, C, H, W, pool, eps, ws, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(gout, N, C, s.PH, s.PW, s.gh, st))) return rc;
  if ((rc = gn8_relu_backward<T>(s.gh, pool ? s.idx : nullptr, s.yh, s.mean, s.rstd, gamma, beta, N, H, W, C, s.partial, s.sums, s.red,
                                 dgamma ? dgamma : s.dg, dbeta ? dbeta : s.db, s.dyh, st)))
    return rc;
  return nhwc_to_nchw<T>(s.dyh, N, C, H, W, dy, st);
}

// DynamicCNN's tail: GroupNorm(8, C) + ReLU (+ pool) + global average in one kernel pair; no activation, argmax or gradient tensor to carve
template <typename T>
struct GroupNormGapWs {
  T *yh, *dyh; float *mean, *rstd, *sums, *partial, *dg, *db; double* stat; ColScratch red; size_t total;
  GroupNormGapWs(void* ws, int N, int C, int H, int W) {
    Carver c(ws);
    const size_t rows = (size_t)N * H * W;
    yh = c.take<T>(rows * C); dyh = c.take<T>(rows * C);
    mean = c.take<float>((size_t)N * 8); rstd = c.take<float>((size_t)N * 8); sums = c.take<float>((size_t)N * 16);
    stat = c.take<double>(gn8_stat_scratch_bytes(N) / sizeof(double));
    partial = c.take<float>(gn8_bwd_partial_bytes(N, C) / sizeof(float));
    dg = c.take<float>(C); db = c.take<float>(C);
    red = bn_reduce_scratch(c.take<double>(bn_reduce_scratch_bytes(C) / sizeof(double)), C);
    total = c.cur;
  }
};
template <typename T>
int groupnorm_gap_fwd_op(const float* y, const float* gamma, const float* beta, float* feat, float* mean, float* rstd, int N, int C, int H, int W,
                         bool pool, float eps, void* ws, hipStream_t st) {
  GroupNormGapWs<T> s(ws, N, C, H, W);
  int rc;
  if ((rc = nchw_to_nhwc<T>(y, N, C, H, W, s.yh, st))) return rc;
  if ((rc = gn8_stats<T>(s.yh, N, H * W, C, eps, s.stat, s.mean, s.rstd, st))) return rc;
  if (mean) HIP_CHECK_RET(hipMemcpyAsync(mean, s.mean, (size_t)N * 8 * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (rstd) HIP_CHECK_RET(hipMemcpyAsync(rstd, s.rstd, (size_t)N * 8 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return feat ? gn8_relu_gap_apply<T>(s.yh, s.mean, s.rstd, gamma, beta, N, H, W, C, pool, s.partial, feat, st) : MMSKIN_OK;
}
template <typename T>
int groupnorm_gap_bwd_op(const float* dfeat, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta, int N,
                         int C, int H, int W, bool pool, float eps, void* ws, hipStream_t st) {
  GroupNormGapWs<T> s(ws, N, C, H, W);
  int rc;
  if ((rc = groupnorm_gap_fwd_op<T>(y, gamma, beta, nullptr, nullptr, nullptr, N, C, H, W, pool, eps, ws, st))) return rc;
  if ((rc = gn8_relu_gap_backward<T>(dfeat, s.yh, s.mean, s.rstd, gamma, beta, N, H, W, C, pool, s.partial, s.sums, s.red, dgamma ? dgamma : s.dg,
                                     dbeta ? dbeta : s.db, s.dyh, st)))
    return rc;
  return nhwc_to_nchw<T>(s.dyh, N, C, H, W, dy, st);
}

}  // namespace

extern "C" {

const char* mmskin_last_error(void) { return g_err; }
int mmskin_version(void) { return 100; }

int64_t mmskin_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return std::max(ws_bytes<ConvWs<float>>(s), ws_bytes<WgradTimeWs<float>>(s));   // the ops, dgrad_fused and the three timers
}

#define DISPATCH(dtype, call_f32, call_bf16)                            \
  do {                                                                  \
    if ((dtype) == MMSKIN_F32) return call_f32;                         \
    if ((dtype) == MMSKIN_BF16) return call_bf16;                       \
    mmskin_set_error("unknown dtype %d", (dtype));                      \
    return MMSKIN_ERR_ARG;                                              \
  } while (0)

int mmskin_conv2d_forward(const float* x, const float* w, float* y, int N, int Cin, int H, int W, int Cout, int kh,
                          int kw, int stride, int pad, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && w && y && workspace, "conv2d_forward: null argument");
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, conv_fwd_op<float>(x, w, y, s, workspace, st), conv_fwd_op<bf16_t>(x, w, y, s, workspace, st));
}

int mmskin_conv2d_backward(const float* dy, const float* x, const float* w, float* dx, float* dw, int N, int Cin,
                           int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype, void* workspace,
                           void* stream) {
  ARG_CHECK(dy && x && w && workspace, "conv2d_backward: null argument");
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, conv_bwd_op<float>(dy, x, w, dx, dw, s, workspace, st),
           conv_bwd_op<bf16_t>(dy, x, w, dx, dw, s, workspace, st));
}

/* Data gradient with the CONSUMER's BatchNorm-backward prologue fused into the epilogue (DgradFuse, profile 3: what the plan launches
 * for every conv -> BatchNorm -> ReLU unit): dz = dgrad(dy) * (xc * scale + shift > 0), plus the partial sums of dz and dz * xc per
 * row block.  xc [N,Cin,H,W] is the raw BatchNorm input of the unit that produced this conv's input; dz [N,Cin,H,W];
 * partial [rows][2][Cin] (rows <= mmskin_conv2d_dgrad_fused_rows(...)), *rows_written = rows the launch produced. */
int mmskin_conv2d_dgrad_fused_rows(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  const int a = conv_dgrad_partial_rows(s);
  return a > N ? a : N;
}
int mmskin_conv2d_dgrad_fused(const float* dy, const float* w, const float* xc, const float* scale, const float* shift, float* dz,
                              float* partial, int* rows_written, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride,
                              int pad, void* workspace, void* stream) {
  ARG_CHECK(dy && w && xc && scale && shift && dz && partial && rows_written && workspace, "conv2d_dgrad_fused: null argument");
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  hipStream_t st = (hipStream_t)stream;
  typedef bf16_t T;
  ConvWs<T> c(workspace, s);
  int rc;
  if ((rc = nchw_to_nhwc<T>(dy, N, Cout, s.OH(), s.OW(), c.yh, st))) return rc;
  if ((rc = nchw_to_nhwc<T>(xc, N, Cin, H, W, c.xh, st))) return rc;
  if ((rc = stage_one<T>(w, Cout, Cin, kh * kw, false, c.wf, c.wd, c.table, st))) return rc;
  DgradFuse f;
  f.x = c.xh; f.scale = scale; f.shift = shift; f.partial = partial;
  if ((rc = launch_conv_dgrad<T>(s, c.yh, c.wd, c.dxh, (const T*)nullptr, st, &f))) return rc;
  *rows_written = f.rows_written;
  return nhwc_to_nchw<T>(c.dxh, N, Cin, H, W, dz, st);
}

/* The data gradient with any fused epilogue the ResNet plan attaches (DgradFuse; flags = MMSKIN_CRD_* as mmskin_conv_route takes them), and
 * the forward with the light epilogue or the statistics slabs (FwdFuse; MMSKIN_CRF_*): see mmskin.h.  Every flag names an operand that
 * must be there, every operand needs its flag; what the launcher itself refuses is refused before the first launch as well. */
#define OPERAND(who, bit, name, present) \
  ARG_CHECK(((flags & (bit)) != 0) == (present), "%s: flag " #bit " and operand " name " must come together (flags 0x%x)", who, flags)
int64_t mmskin_conv2d_dgrad_epilogue_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return ws_bytes<DgradEpiWs<float>>(s);
}
int mmskin_conv2d_dgrad_epilogue(const float* dy, const float* w, const float* addend, const float* mask_y, const unsigned char* mask_bits,
                                 const float* x, const float* scale, const float* shift, const float* x2, float* dz, float* partial,
                                 float* partial_b, int* rows_written, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride,
                                 int pad, int flags, int dtype, void* workspace, void* stream) {
  const char* const who = "conv2d_dgrad_epilogue";
  const int known = MMSKIN_CRD_ADDEND | MMSKIN_CRD_ADDEND_IS_DIN | MMSKIN_CRD_MASK_Y | MMSKIN_CRD_MASK_BITS | MMSKIN_CRD_X | MMSKIN_CRD_SCALE_SHIFT |
                    MMSKIN_CRD_X2 | MMSKIN_CRD_ADDEND_S2 | MMSKIN_CRD_PARTIAL;
  ARG_CHECK(dy && w && dz && workspace, "%s: null argument", who);
  ARG_CHECK(N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0, "%s: bad shape", who);
  ARG_CHECK(!(flags & ~known), "%s: flags 0x%x: IN2, BIAS and EMPTY are not taken here", who, flags);
  OPERAND(who, MMSKIN_CRD_ADDEND, "addend", addend != nullptr);
  OPERAND(who, MMSKIN_CRD_ADDEND_IS_DIN, "addend == dz", addend == dz);
  ARG_CHECK(!(flags & MMSKIN_CRD_ADDEND_S2) || (flags & (MMSKIN_CRD_ADDEND | MMSKIN_CRD_ADDEND_IS_DIN)) == MMSKIN_CRD_ADDEND,
            "%s: ADDEND_S2 needs an addend of its own (flags 0x%x)", who, flags);
  OPERAND(who, MMSKIN_CRD_MASK_Y, "mask_y", mask_y != nullptr);
  OPERAND(who, MMSKIN_CRD_MASK_BITS, "mask_bits", mask_bits != nullptr);
  OPERAND(who, MMSKIN_CRD_X, "x", x != nullptr);
  OPERAND(who, MMSKIN_CRD_SCALE_SHIFT, "scale", scale != nullptr);
  OPERAND(who, MMSKIN_CRD_SCALE_SHIFT, "shift", shift != nullptr);
  OPERAND(who, MMSKIN_CRD_X2, "x2", x2 != nullptr);
  OPERAND(who, MMSKIN_CRD_X2, "partial_b", partial_b != nullptr);
  OPERAND(who, MMSKIN_CRD_PARTIAL, "partial", partial != nullptr);
  OPERAND(who, MMSKIN_CRD_PARTIAL, "rows_written", rows_written != nullptr);
  ARG_CHECK(!(flags & MMSKIN_CRD_SCALE_SHIFT) || (flags & MMSKIN_CRD_X), "%s: SCALE_SHIFT masks from x: it needs X (flags 0x%x)", who, flags);
  ARG_CHECK(!(flags & MMSKIN_CRD_X2) || ((flags & MMSKIN_CRD_X) && (flags & MMSKIN_CRD_PARTIAL)), "%s: X2 needs X and PARTIAL (flags 0x%x)", who, flags);
  const ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  const DgradEpiArgs g = {dy, w, addend, mask_y, mask_bits, x, scale, shift, x2, dz, partial, partial_b, rows_written, flags};
  DISPATCH(dtype, dgrad_epilogue_op<float>(g, s, workspace, ST(stream)), dgrad_epilogue_op<bf16_t>(g, s, workspace, ST(stream)));
}
int64_t mmskin_conv2d_forward_epilogue_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return ws_bytes<FwdEpiWs<float>>(s);
}
int mmskin_conv2d_forward_epilogue_stat_rows(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  const int a = conv_fwd_stat_rows(s);
  return a > N ? a : N;   // the layer-1 all-taps kernel writes one row per image
}
int mmskin_conv2d_forward_epilogue(const float* x, const float* w, const float* mul, const float* bias, const float* addend, float* y,
                                   float* stat_sum, float* stat_sq, int* stat_rows, unsigned char* mask_out, int N, int Cin, int H, int W,
                                   int Cout, int kh, int kw, int stride, int pad, int flags, int dtype, void* workspace, void* stream) {
  const char* const who = "conv2d_forward_epilogue";
  const int known = MMSKIN_CRF_STATS | MMSKIN_CRF_ROWS_FREE | MMSKIN_CRF_BIAS | MMSKIN_CRF_ADDEND | MMSKIN_CRF_RELU | MMSKIN_CRF_MASK_OUT | MMSKIN_CRF_MUL |
                    MMSKIN_CRF_NO_OUT;
  ARG_CHECK(x && w && workspace, "%s: null argument", who);
  ARG_CHECK(N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0, "%s: bad shape", who);
  ARG_CHECK(!(flags & ~known), "%s: flags 0x%x: GELU, OUT_F32 and RESIDUAL belong to the Linear entry points", who, flags);
  OPERAND(who, MMSKIN_CRF_MUL, "mul", mul != nullptr);
  OPERAND(who, MMSKIN_CRF_BIAS, "bias", bias != nullptr);
  OPERAND(who, MMSKIN_CRF_ADDEND, "addend", addend != nullptr);
  OPERAND(who, MMSKIN_CRF_MASK_OUT, "mask_out", mask_out != nullptr);
  OPERAND(who, MMSKIN_CRF_STATS, "stat_sum", stat_sum != nullptr);
  OPERAND(who, MMSKIN_CRF_STATS, "stat_sq", stat_sq != nullptr);
  OPERAND(who, MMSKIN_CRF_STATS, "stat_rows", stat_rows != nullptr);
  ARG_CHECK(!(flags & (MMSKIN_CRF_ROWS_FREE | MMSKIN_CRF_NO_OUT)) || (flags & MMSKIN_CRF_STATS), "%s: ROWS_FREE and NO_OUT need STATS (flags 0x%x)", who, flags);
  ARG_CHECK(y || (flags & MMSKIN_CRF_NO_OUT), "%s: y required unless NO_OUT", who);
  const ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  const FwdEpiArgs g = {x, w, mul, bias, addend, y, stat_sum, stat_sq, stat_rows, mask_out, flags};
  DISPATCH(dtype, fwd_epilogue_op<float>(g, s, workspace, ST(stream)), fwd_epilogue_op<bf16_t>(g, s, workspace, ST(stream)));
}
#undef OPERAND

/* timing helper: runs the forward conv kernel `iters` times on NHWC buffers already resident in the
 * workspace (contents irrelevant) and returns the average microseconds per launch. */
double mmskin_conv2d_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                          int iters, void* workspace, void* stream) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return dtype == MMSKIN_BF16 ? conv_time<bf16_t>(TIME_FWD, s, iters, workspace, ST(stream)) : conv_time<float>(TIME_FWD, s, iters, workspace, ST(stream));
}

/* same for the data-gradient launch (no fused epilogue; stride-2 layers run as parity classes) */
double mmskin_conv2d_dgrad_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                                int iters, void* workspace, void* stream) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return dtype == MMSKIN_BF16 ? conv_time<bf16_t>(TIME_DGRAD, s, iters, workspace, ST(stream)) : conv_time<float>(TIME_DGRAD, s, iters, workspace, ST(stream));
}

/* Algebraic BatchNorm backward of an expanding 1x1 convolution (abn.hip), op level: g [N,C4,H,W] is the (masked) gradient of the
 * BatchNorm output, y [N,Cw,H,W] the convolution's input, w [C4,Cw] its weight, cA / cB / cC [C4] the BatchNorm-backward coefficients
 * (dz = cA g + cB x + cC, x = conv(y)).  Returns dy = dz W [N,Cw,H,W] and dw = dz^T y [C4,Cw] without forming dz or x. */
int64_t mmskin_abn_workspace_bytes(int N, int Cw, int C4, int H, int W) {
  return std::max(ws_bytes<AbnWs>(N, Cw, C4, H, W), ws_bytes<GramStatsWs>(N, Cw, C4, H, W));   // serves mmskin_conv1x1_gram_stats too
}
static int abn_backward_impl(const float* g, const float* y, const float* w, const float* cA, const float* cB, const float* cC, int N, int Cw,
                             int C4, int H, int W, float* dy, float* dw, void* workspace, hipStream_t st, bool kept_gram) {
  const size_t M = (size_t)N * H * W;
  ARG_CHECK(wgrad_gram_slab_bytes((int)M, C4, Cw) > 0 && (!kept_gram || (wgrad_gram_slab_bytes((int)M, C4, Cw, 1) > 0 && wgrad_gram_slab_bytes((int)M, 0, Cw, 2) > 0)),
            "abn_backward: shape C4=%d Cw=%d unsupported", C4, Cw);
  AbnWs a(workspace, N, Cw, C4, H, W);
  int rc;
  if ((rc = nchw_to_nhwc<bf16_t>(g, N, C4, H, W, a.gh, st))) return rc;
  if ((rc = nchw_to_nhwc<bf16_t>(y, N, Cw, H, W, a.yh, st))) return rc;
  if ((rc = abn_prep(w, cA, cB, cC, C4, Cw, a.wd, a.bias, a.coef, st))) return rc;
  ConvShape s = {N, H, W, Cw, C4, 1, 1, 1, 0};
  DgradFuse f;
  f.in2 = a.yh; f.k2 = Cw; f.bias = a.bias;
  if ((rc = launch_conv_dgrad<bf16_t>(s, a.gh, a.wd, a.dyh, (const bf16_t*)nullptr, st, &f))) return rc;
  if ((rc = nhwc_to_nchw<bf16_t>(a.dyh, N, Cw, H, W, dy, st))) return rc;
  if (kept_gram) {   // the two-pass forward's order: y^T y + colsum(y) first (forward), g^T y alone later
    if ((rc = launch_wgrad_gram(N, H, W, Cw, C4, nullptr, a.yh, a.slab, a.gram, a.cs, st, 2))) return rc;
    if ((rc = launch_wgrad_gram(N, H, W, Cw, C4, a.gh, a.yh, a.slab, a.S, nullptr, st, 1))) return rc;
    return abn_wgrad_finalize(a.S, a.cs, w, a.coef, C4, Cw, dw, st, a.gram);
  }
  if ((rc = launch_wgrad_gram(N, H, W, Cw, C4, a.gh, a.yh, a.slab, a.S, a.cs, st))) return rc;
  return abn_wgrad_finalize(a.S, a.cs, w, a.coef, C4, Cw, dw, st);
}
int mmskin_abn_backward(const float* g, const float* y, const float* w, const float* cA, const float* cB, const float* cC, int N, int Cw,
                        int C4, int H, int W, float* dy, float* dw, void* workspace, void* stream) {
  return abn_backward_impl(g, y, w, cA, cB, cC, N, Cw, C4, H, W, dy, dw, workspace, (hipStream_t)stream, false);
}
/* same result through the two-pass forward's kernels: Gram matrix + column sums of y in their own launch, g^T y alone */
int mmskin_abn_backward_kept_gram(const float* g, const float* y, const float* w, const float* cA, const float* cB, const float* cC, int N,
                                  int Cw, int C4, int H, int W, float* dy, float* dw, void* workspace, void* stream) {
  return abn_backward_impl(g, y, w, cA, cB, cC, N, Cw, C4, H, W, dy, dw, workspace, (hipStream_t)stream, true);
}
/* Per-channel sum and sum of squares of x = conv1x1(y, w) (y [N,Cw,H,W], w [C4,Cw], bf16 operands) WITHOUT forming x: from the Gram
 * matrix y^T y and the column sums of y (abn.hip gram_stats) -- the first pass of the two-pass BatchNorm forward.  Workspace as
 * mmskin_abn_workspace_bytes. */
int mmskin_conv1x1_gram_stats(const float* y, const float* w, int N, int Cw, int C4, int H, int W, float* stat_sum, float* stat_sq,
                              void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ARG_CHECK(wgrad_gram_slab_bytes(N * H * W, 0, Cw, 2) > 0, "conv1x1_gram_stats: Cw=%d unsupported", Cw);
  GramStatsWs a(workspace, N, Cw, C4, H, W);
  int rc;
  if ((rc = nchw_to_nhwc<bf16_t>(y, N, Cw, H, W, a.yh, st))) return rc;
  if ((rc = launch_wgrad_gram(N, H, W, Cw, C4, nullptr, a.yh, a.slab, a.gram, a.cs, st, 2))) return rc;
  return gram_stats(a.gram, a.cs, w, C4, Cw, stat_sum, stat_sq, st);
}

/* same for the weight-gradient kernel (+ its slab reduction) */
double mmskin_conv2d_wgrad_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                                int iters, void* workspace, void* stream) {
  ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  return dtype == MMSKIN_BF16 ? conv_time<bf16_t>(TIME_WGRAD, s, iters, workspace, ST(stream)) : conv_time<float>(TIME_WGRAD, s, iters, workspace, ST(stream));
}

int64_t mmskin_batchnorm_workspace_bytes(int N, int C, int H, int W) {
  return ws_bytes<BnWs<float>>(N, C, H, W);
}

int mmskin_batchnorm_forward(const float* x, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float* y, float* save_mean, float* save_invstd, int N, int C, int H,
                             int W, float eps, float momentum, int relu, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && gamma && beta && y && save_mean && save_invstd && workspace, "batchnorm_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_fwd_op<float>(x, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, N, C, H, W, eps, momentum, relu, workspace, st),
           bn_fwd_op<bf16_t>(x, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, N, C, H, W, eps, momentum, relu, workspace, st));
}

int mmskin_batchnorm_backward(const float* dy, const float* x, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta,
                              int N, int C, int H, int W, int relu, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dy && x && gamma && beta && save_mean && save_invstd && dx && workspace, "batchnorm_backward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_bwd_op<float>(dy, x, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta, N, C, H, W, relu, workspace, st),
           bn_bwd_op<bf16_t>(dy, x, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta, N, C, H, W, relu, workspace, st));
}

int64_t mmskin_stem_workspace_bytes(int N, int H, int W) {
  return ws_bytes<StemWs<float>>(StemGeom(N, H, W));
}

int mmskin_stem_forward(const float* x, const float* w, const float* gamma, const float* beta, float* y, int N, int H,
                        int W, float eps, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && w && gamma && beta && y && workspace, "stem_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, stem_fwd_op<float>(x, w, gamma, beta, y, N, H, W, eps, workspace, st),
           stem_fwd_op<bf16_t>(x, w, gamma, beta, y, N, H, W, eps, workspace, st));
}

int mmskin_stem_backward(const float* dy, const float* x, const float* w, const float* gamma, const float* beta,
                         float* dw, float* dgamma, float* dbeta, int N, int H, int W, float eps, int dtype,
                         void* workspace, void* stream) {
  ARG_CHECK(dy && x && w && gamma && beta && dw && workspace, "stem_backward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, stem_bwd_op<float>(dy, x, w, gamma, beta, dw, dgamma, dbeta, N, H, W, eps, workspace, st),
           stem_bwd_op<bf16_t>(dy, x, w, gamma, beta, dw, dgamma, dbeta, N, H, W, eps, workspace, st));
}

/* fp32 NHWC depthwise 3x3 (stride 1, pad 1) for token-layout models (DaViT's convolutional position encoding):
 * w is the nn.Conv2d(groups = C) weight [C][1][3][3]; w_stage holds 9*C floats; backward also needs
 * mmskin_dwconv3_scratch_floats(...) floats of scratch. */
int64_t mmskin_dwconv3_scratch_floats(int N, int H, int W, int C) { return (int64_t)dwconv3_wgrad_partial_floats(N, H, W, C, 1, 3); }
int mmskin_dwconv3_forward(const float* x, const float* w, float* w_stage, float* y, int N, int H, int W, int C, void* stream) {
  ARG_CHECK(x && w && w_stage && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "dwconv3_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_stage_weights<float>(w, C, C, w_stage, st, 3);
  if (rc) return rc;
  return dwconv3_fwd<float>(x, w_stage, N, H, W, C, 1, y, st, 3);
}
int mmskin_dwconv3_backward(const float* dy, const float* x, const float* w, float* w_stage, float* scratch, float* dx, float* dw,
                            int N, int H, int W, int C, void* stream) {
  ARG_CHECK(dy && x && w && w_stage && scratch && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "dwconv3_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_stage_weights<float>(w, C, C, w_stage, st, 3);
  if (rc) return rc;
  if (dx && (rc = dwconv3_dgrad<float>(dy, w_stage, N, H, W, C, 1, dx, st, 3))) return rc;
  if (dw && (rc = dwconv3_wgrad<float>(dy, x, N, H, W, C, 1, scratch, dw, C, st, 3))) return rc;
  return MMSKIN_OK;
}

/* DaViT's convolutional position encoding in one pass each way (timm davit.py ConvPosEnc.forward: x + proj(x), proj = depthwise 3x3 with
 * bias; loadImageModelClassifier.py:117-131):  y = x + dwconv3(x, w) + b.  Backward: dx = dy + dgrad(dy), dw, and db = sum(dy) from the
 * weight-gradient pass.  Same staging / scratch as mmskin_dwconv3_*. */
int mmskin_conv_pos_enc_forward(const float* x, const float* w, const float* b, float* w_stage, float* y, int N, int H, int W, int C,
                                void* stream) {
  ARG_CHECK(x && w && w_stage && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "conv_pos_enc_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_stage_weights<float>(w, C, C, w_stage, st, 3);
  if (rc) return rc;
  return dwconv3_fwd<float>(x, w_stage, N, H, W, C, 1, y, st, 3, b, true);
}
int mmskin_conv_pos_enc_backward(const float* dy, const float* x, const float* w, float* w_stage, float* scratch, float* dx, float* dw,
                                 float* db, int N, int H, int W, int C, void* stream) {
  ARG_CHECK(dy && x && w && w_stage && scratch && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "conv_pos_enc_backward: bad argument");
  ARG_CHECK(dw || !db, "conv_pos_enc_backward: db is produced by the weight-gradient pass (dw required)");
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_stage_weights<float>(w, C, C, w_stage, st, 3);
  if (rc) return rc;
  if (dx && (rc = dwconv3_dgrad<float>(dy, w_stage, N, H, W, C, 1, dx, st, 3, true))) return rc;
  if (dw && (rc = dwconv3_wgrad<float>(dy, x, N, H, W, C, 1, scratch, dw, C, st, 3, db))) return rc;
  return MMSKIN_OK;
}

/* ---- MBConv family, op by op (MobileNet-V2 / EfficientNet: csrc/mbconv.hip).  NCHW fp32 at the boundary, NHWC `dtype` inside the
 * workspace; every entry launches what the plan launches for the same unit. */
#define DW_ARGS_OK (N > 0 && C > 0 && C % 8 == 0 && H > 0 && W > 0 && (ksize == 3 || ksize == 5) && (stride == 1 || stride == 2) && \
                    c_valid >= 1 && c_valid <= C)
int64_t mmskin_dwconv2d_workspace_bytes(int N, int C, int H, int W, int ksize, int stride) {
  if (!(N > 0 && C > 0 && H > 0 && W > 0 && (ksize == 3 || ksize == 5) && (stride == 1 || stride == 2))) return -1;
  return ws_bytes<DwWs<float>>(N, C, H, W, ksize, stride);
}
int mmskin_dwconv2d_forward(const float* x, const float* w, float* y, int N, int C, int H, int W, int ksize, int stride, int c_valid,
                            int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && w && y && workspace && DW_ARGS_OK, "dwconv2d_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dw_fwd_op<float>(x, w, y, N, C, H, W, ksize, stride, c_valid, workspace, st),
           dw_fwd_op<bf16_t>(x, w, y, N, C, H, W, ksize, stride, c_valid, workspace, st));
}
int mmskin_dwconv2d_backward(const float* dy, const float* x, const float* w, float* dx, float* dw, int N, int C, int H, int W, int ksize,
                             int stride, int c_valid, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dy && x && w && workspace && DW_ARGS_OK, "dwconv2d_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dw_bwd_op<float>(dy, x, w, dx, dw, N, C, H, W, ksize, stride, c_valid, workspace, st),
           dw_bwd_op<bf16_t>(dy, x, w, dx, dw, N, C, H, W, ksize, stride, c_valid, workspace, st));
}
#undef DW_ARGS_OK

int64_t mmskin_batchnorm_act_workspace_bytes(int N, int C, int H, int W) {
  if (!(N > 0 && C > 0 && H > 0 && W > 0)) return -1;
  return ws_bytes<BnActWs<float>>(N, C, H, W);
}
int mmskin_batchnorm_act_forward(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float* y, float* save_mean, float* save_invstd, int N, int C, int H, int W, float eps,
                                 float momentum, int act, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && gamma && beta && running_mean && running_var && y && save_mean && save_invstd && workspace && N > 0 && C > 0 && C % 8 == 0 &&
            H > 0 && W > 0 && act >= 0 && act <= 3, "batchnorm_act_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_act_fwd_op<float>(x, res, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, N, C, H, W, eps, momentum, act, workspace, st),
           bn_act_fwd_op<bf16_t>(x, res, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, N, C, H, W, eps, momentum, act, workspace, st));
}
int mmskin_batchnorm_act_backward(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                                  const float* save_mean, const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta,
                                  int N, int C, int H, int W, int act, int has_residual, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dy && x && y && gamma && beta && save_mean && save_invstd && dx && workspace && N > 0 && C > 0 && C % 8 == 0 && H > 0 && W > 0 &&
            act >= 0 && act <= 3 && (has_residual || !dres), "batchnorm_act_backward: bad argument");
  if (act == 3 && has_residual) {   // MASK_SILU_X recomputes the SiLU argument from x alone; the plan's residual units carry no activation
    mmskin_set_error("batchnorm_act_backward: SiLU behind a residual has no backward kernel");
    return MMSKIN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_act_bwd_op<float>(dy, x, y, gamma, beta, save_mean, save_invstd, dx, dres, dgamma, dbeta, N, C, H, W, act, workspace, st),
           bn_act_bwd_op<bf16_t>(dy, x, y, gamma, beta, save_mean, save_invstd, dx, dres, dgamma, dbeta, N, C, H, W, act, workspace, st));
}

int mmskin_bn_apply_rows(const void* x, const void* res, const float* scale, const float* shift, const float* rscale, const float* rshift,
                         void* y, unsigned char* mask_bits, int64_t rows, int C, int relu, float relu_cap, int dtype, void* stream) {
  ARG_CHECK(x && scale && shift && y && rows > 0 && C > 0 && (!rscale || (res && rshift)), "bn_apply_rows: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_apply<float>((const float*)x, (const float*)res, scale, shift, rscale, rshift, (float*)y, (size_t)rows, C, relu != 0, st, mask_bits, relu_cap),
           bn_apply<bf16_t>((const bf16_t*)x, (const bf16_t*)res, scale, shift, rscale, rshift, (bf16_t*)y, (size_t)rows, C, relu != 0, st, mask_bits, relu_cap));
}
int mmskin_bn_bwd_apply_rows(const void* dy, const void* x, const void* ymask, const float* scale, const float* shift, int mask_mode,
                             const float* cA, const float* cB, const float* cC, void* dx, void* dz, int64_t rows, int C, int dtype,
                             void* stream) {
  ARG_CHECK(dy && x && scale && shift && cA && cB && cC && dx && rows > 0 && C > 0 && mask_mode >= MASK_NONE && mask_mode <= MASK_SILU_X &&
            (ymask || !(mask_mode == MASK_FROM_Y || mask_mode == MASK_FROM_Y6)), "bn_bwd_apply_rows: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           bn_bwd_apply<float>((const float*)dy, (const float*)x, (const float*)ymask, scale, shift, mask_mode, cA, cB, cC, (float*)dx, (float*)dz, (size_t)rows, C, st),
           bn_bwd_apply<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)ymask, scale, shift, mask_mode, cA, cB, cC, (bf16_t*)dx, (bf16_t*)dz, (size_t)rows, C, st));
}

#define SE_ARGS_OK (N > 0 && C > 0 && Cp == pad64(C) && Csq > 0 && HW > 0)
int64_t mmskin_se_workspace_bytes(int N, int Cp, int Csq, int HW) {
  if (!(N > 0 && Cp > 0 && Csq > 0 && HW > 0)) return -1;
  return ws_bytes<SeWs<float>>(N, Cp, Csq, HW);
}
int mmskin_se_forward(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* y_se, int N, int C, int Cp,
                      int Csq, int HW, int dtype, void* workspace, void* stream) {
  ARG_CHECK(y && w1 && b1 && w2 && b2 && y_se && workspace && SE_ARGS_OK, "se_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, se_fwd_op<float>(y, w1, b1, w2, b2, y_se, N, C, Cp, Csq, HW, workspace, st),
           se_fwd_op<bf16_t>(y, w1, b1, w2, b2, y_se, N, C, Cp, Csq, HW, workspace, st));
}
int mmskin_se_backward(const float* dy_se, const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* dy,
                       float* dw1, float* db1, float* dw2, float* db2, int N, int C, int Cp, int Csq, int HW, int dtype, void* workspace,
                       void* stream) {
  ARG_CHECK(dy_se && y && w1 && b1 && w2 && b2 && dy && dw1 && db1 && dw2 && db2 && workspace && SE_ARGS_OK, "se_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, se_bwd_op<float>(dy_se, y, w1, b1, w2, b2, dy, dw1, db1, dw2, db2, N, C, Cp, Csq, HW, workspace, st),
           se_bwd_op<bf16_t>(dy_se, y, w1, b1, w2, b2, dy, dw1, db1, dw2, db2, N, C, Cp, Csq, HW, workspace, st));
}
#undef SE_ARGS_OK

int64_t mmskin_sd_workspace_bytes(int N, int64_t per_sample) {
  if (!(N > 0 && per_sample > 0)) return -1;
  return ws_bytes<SdWs<float>>(N, per_sample);
}
int mmskin_sd_forward(const float* branch, const float* res, const float* mask, float* y, int N, int64_t per_sample, int dtype,
                      void* workspace, void* stream) {
  ARG_CHECK(branch && res && mask && y && workspace && N > 0 && per_sample > 0 && per_sample % 8 == 0 && per_sample < (1ll << 31),
            "sd_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, sd_op<float>(branch, res, mask, y, N, per_sample, workspace, st), sd_op<bf16_t>(branch, res, mask, y, N, per_sample, workspace, st));
}
int mmskin_sd_backward(const float* dy, const float* mask, float* out, int N, int64_t per_sample, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dy && mask && out && workspace && N > 0 && per_sample > 0 && per_sample % 8 == 0 && per_sample < (1ll << 31),
            "sd_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, sd_op<float>(dy, nullptr, mask, out, N, per_sample, workspace, st), sd_op<bf16_t>(dy, nullptr, mask, out, N, per_sample, workspace, st));
}

/* ---- DenseNet / VGG plan kernels, op by op (csrc/densenet.hip, csrc/vgg.hip).  Same conventions as the MBConv entries; the dense-block
 * and transition entries call the functions the plan calls (dense_block_forward / _backward, dense_transition_forward / _backward), with
 * the weight-gradient GEMMs on the caller's stream as in a profiled plan run.  The backward entries run the training forward first. */
#define DENSE_BLOCK_OK (N > 0 && C0 > 0 && C0 % 32 == 0 && L >= 1 && L <= 64 && H > 0 && W > 0)
int64_t mmskin_dense_block_workspace_bytes(int N, int C0, int L, int H, int W) {
  if (!DENSE_BLOCK_OK) return -1;
  return (int64_t)DenseBlockWs(N, C0, L, H, W, sizeof(float)).total;
}
int64_t mmskin_dense_block_param_numel(int C0, int L) {
  if (!(C0 > 0 && C0 % 32 == 0 && L >= 1 && L <= 64)) return -1;
  return DenseBlockWs(1, C0, L, 1, 1, sizeof(float)).param_numel;
}
int mmskin_dense_block_forward(const float* x, const float* params, float* buffers, float* cat, float* table, int N, int C0, int L, int H, int W,
                               int training, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && params && buffers && cat && workspace && DENSE_BLOCK_OK, "dense_block_forward: bad argument (C0 = %d must be a multiple of 32)", C0);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dense_block_fwd_op<float>(x, params, buffers, cat, table, N, C0, L, H, W, training != 0, workspace, st),
           dense_block_fwd_op<bf16_t>(x, params, buffers, cat, table, N, C0, L, H, W, training != 0, workspace, st));
}
int mmskin_dense_block_backward(const float* dcat, const float* x, const float* params, float* dx, float* grads, int N, int C0, int L, int H,
                                int W, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dcat && x && params && dx && grads && workspace && DENSE_BLOCK_OK, "dense_block_backward: bad argument (C0 = %d must be a multiple of 32)", C0);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dense_block_bwd_op<float>(dcat, x, params, dx, grads, N, C0, L, H, W, workspace, st),
           dense_block_bwd_op<bf16_t>(dcat, x, params, dx, grads, N, C0, L, H, W, workspace, st));
}
#undef DENSE_BLOCK_OK

#define DENSE_TRANS_OK (N > 0 && C > 0 && C % 128 == 0 && H >= 2 && W >= 2 && Cdst >= C / 2 && Cdst % 8 == 0)
int64_t mmskin_dense_transition_workspace_bytes(int N, int C, int H, int W, int Cdst) {
  if (!DENSE_TRANS_OK) return -1;
  return (int64_t)DenseTransWs(N, C, H, W, Cdst, sizeof(float)).total;
}
int mmskin_dense_transition_forward(const float* x, const float* table, const float* params, float* buffers, float* dst, float* conv_out, int N,
                                    int C, int H, int W, int Cdst, int training, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && table && params && buffers && dst && workspace && DENSE_TRANS_OK,
            "dense_transition_forward: bad argument (C = %d a multiple of 128, map %dx%d at least 2x2, pitch %d >= C/2)", C, H, W, Cdst);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dense_trans_fwd_op<float>(x, table, params, buffers, dst, conv_out, N, C, H, W, Cdst, training != 0, workspace, st),
           dense_trans_fwd_op<bf16_t>(x, table, params, buffers, dst, conv_out, N, C, H, W, Cdst, training != 0, workspace, st));
}
int mmskin_dense_transition_backward(const float* dnext, const float* x, const float* table, const float* params, float* dx, float* grads,
                                     float* dconv_out, int N, int C, int H, int W, int Cdst, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dnext && x && table && params && dx && grads && workspace && DENSE_TRANS_OK,
            "dense_transition_backward: bad argument (C = %d a multiple of 128, map %dx%d at least 2x2, pitch %d >= C/2)", C, H, W, Cdst);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, dense_trans_bwd_op<float>(dnext, x, table, params, dx, grads, dconv_out, N, C, H, W, Cdst, workspace, st),
           dense_trans_bwd_op<bf16_t>(dnext, x, table, params, dx, grads, dconv_out, N, C, H, W, Cdst, workspace, st));
}
#undef DENSE_TRANS_OK

#define SLICE_OK (rows > 0 && rows < (1ll << 31) && rows * pitch < (1ll << 31) && C > 0 && C % 8 == 0 && pitch % 8 == 0 && c0 >= 0 && c0 % 8 == 0 && c0 + C <= pitch)
int64_t mmskin_col_reduce_scratch_doubles(int64_t cols_total) { return cols_total < 0 ? -1 : (int64_t)col_reduce_scratch_doubles((size_t)cols_total); }
int mmskin_col_reduce_scratch_check(int slabs, int nrows, int cols_total, int64_t doubles) {
  return col_reduce_scratch_check(slabs, nrows, cols_total, doubles < 0 ? 0 : (size_t)doubles);
}
// the launch geometry of a convolution as the plans run it: the 7x7 / stride 2 stem and the 3-channel 3x3 first conv through their virtual forms
static bool wgrad_export_geom(const ConvShape& s, WgradArgs& g) {
  if (s.Cin == 3 && s.Cout == 64 && s.kh == 7 && s.kw == 7 && s.stride == 2 && s.pad == 3) {
    const StemGeom sg(s.N, s.H, s.W);
    g = wgrad_geom_stem(sg.N, sg.OH, sg.OW, sg.Hp, sg.Wp);
    return true;
  }
  if (s.Cin == 3 && s.Cout == 64 && s.kh == 3 && s.kw == 3 && s.pad == 1 && (s.stride == 1 || s.stride == 2)) {
    g = wgrad_geom_first(FirstGeom(s.N, s.H, s.W, s.stride));
    return true;
  }
  g = wgrad_geom_conv(s);
  return false;
}
static int wgrad_export_plan(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, WgradArgs& g, WgradPlan& pl) {
  ARG_CHECK(N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && (elem_bytes == 2 || elem_bytes == 4),
            "conv_wgrad_plan: bad argument");
  const ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  const bool virt = wgrad_export_geom(s, g);
  ARG_CHECK(wgrad_plan(g, virt ? nullptr : &s, elem_bytes, pl), "conv_wgrad_plan: no weight-gradient kernel takes Cout=%d Ktot=%d", g.Cout, g.Ktot);
  return MMSKIN_OK;
}
int mmskin_conv_wgrad_plan(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, int64_t out[8]) {
  static_assert(WG_STAGED == MMSKIN_WG_STAGED && WG_TAPS3 == MMSKIN_WG_TAPS3 && WG_RING == MMSKIN_WG_RING && WG_RING3 == MMSKIN_WG_RING3 &&
                WGR_DIRECT == MMSKIN_WGR_DIRECT && WGR_LANES == MMSKIN_WGR_LANES, "mmskin.h documents the WgradPlan values");
  WgradArgs g;
  WgradPlan pl;
  ARG_CHECK(out, "conv_wgrad_plan: out required");
  if (int rc = wgrad_export_plan(N, Cin, H, W, Cout, kh, kw, stride, pad, elem_bytes, g, pl)) return rc;
  const int64_t v[8] = {pl.family, pl.tile_o, pl.tile_k, pl.variant, pl.nsplit, pl.per_split, pl.reduce, (int64_t)pl.slab_floats};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return MMSKIN_OK;
}
int mmskin_conv_wgrad_slab_check(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, int64_t capacity_floats) {
  WgradArgs g;
  WgradPlan pl;
  if (int rc = wgrad_export_plan(N, Cin, H, W, Cout, kh, kw, stride, pad, elem_bytes, g, pl)) return rc;
  return wgrad_slab_check(g, pl, capacity_floats < 0 ? 0 : (size_t)capacity_floats);
}
int mmskin_conv_route(int op, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, int flags, int64_t out[9]) {
  static_assert(CG_TILE128 == MMSKIN_CG_TILE128 && CG_BIG256 == MMSKIN_CG_BIG256 && CG_PIPE == MMSKIN_CG_PIPE && CG_C64 == MMSKIN_CG_C64 &&
                CG_STEM7 == MMSKIN_CG_STEM7, "mmskin.h documents the ConvRoute values");
  ARG_CHECK(out && op >= 0 && op <= 3 && N > 0 && H > 0 && W > 0 && (elem_bytes == 2 || elem_bytes == 4), "conv_route: bad argument");
  ARG_CHECK(op >= 2 || (Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0), "conv_route: bad argument");
  // the route only asks whether an operand is there: one address stands for every operand a flag names
  static float operand[1];
  void* const set = operand;
  auto on = [&](int bit) -> float* { return (flags & bit) ? operand : nullptr; };
  const ConvShape s = {N, H, W, Cin, Cout, kh, kw, stride, pad};
  ConvGemmArgs a;
  ConvRoute r;
  int rc = MMSKIN_OK;
  if (op == 1) {
    DgradFuse f;
    f.mask_y = on(MMSKIN_CRD_MASK_Y); f.mask_bits = reinterpret_cast<const uint8_t*>(on(MMSKIN_CRD_MASK_BITS)); f.x = on(MMSKIN_CRD_X);
    f.scale = f.shift = on(MMSKIN_CRD_SCALE_SHIFT); f.x2 = on(MMSKIN_CRD_X2); f.in2 = on(MMSKIN_CRD_IN2); f.k2 = (flags >> 16) & 0xffff;
    f.bias = on(MMSKIN_CRD_BIAS); f.addend_s2 = (flags & MMSKIN_CRD_ADDEND_S2) != 0; f.partial = f.partial_b = on(MMSKIN_CRD_PARTIAL);
    static float other[1];   // din; the addend is this or its own buffer
    unsigned zero_mask;
    rc = conv_route_dgrad(s, elem_bytes, set, set, other, (flags & MMSKIN_CRD_ADDEND) ? ((flags & MMSKIN_CRD_ADDEND_IS_DIN) ? other : operand) : nullptr,
                          (flags & CRD_FUSE_BITS) ? &f : nullptr, a, zero_mask, r);
  } else {
    FwdFuse f;
    f.bias = on(MMSKIN_CRF_BIAS); f.addend = on(MMSKIN_CRF_ADDEND); f.relu = (flags & MMSKIN_CRF_RELU) != 0; f.gelu = (flags & MMSKIN_CRF_GELU) != 0;
    f.out_f32 = on(MMSKIN_CRF_OUT_F32); f.gamma = f.res_f32 = on(MMSKIN_CRF_RESIDUAL); f.mul = on(MMSKIN_CRF_MUL);
    f.mask_out = reinterpret_cast<uint8_t*>(on(MMSKIN_CRF_MASK_OUT));
    float* const stats = on(MMSKIN_CRF_STATS);
    if (op == 0) {
      rc = conv_route_fwd(s, elem_bytes, set, set, (flags & MMSKIN_CRF_NO_OUT) ? nullptr : set, stats, stats, (flags & CRF_FUSE_BITS) ? &f : nullptr,
                          (flags & MMSKIN_CRF_ROWS_FREE) != 0, a, r);
    } else if (op == 2) {   // the 7x7 / stride 2 stem of an N x 3 x H x W batch, in the geometry the plans run
      const StemGeom sg(N, H, W);
      a = conv_geom_stem(sg.N, sg.OH, sg.OW, sg.Hp, sg.Wp);
      a.in = a.w = set; a.out = set; a.stat_sum = a.stat_sq = stats;
      rc = conv_route_stem(a, elem_bytes, sg.Hp, sg.Wp, r);
    } else {                // the 3-channel 3x3 / pad 1 first conv (stride 1 | 2); flags: statistics, bias, addend, relu
      ARG_CHECK(stride == 1 || stride == 2, "conv_route: first conv stride");
      a = conv_geom_first(FirstGeom(N, H, W, stride));
      a.in = a.w = set; a.out = set; a.stat_sum = a.stat_sq = stats;
      a.ep_bias = f.bias; a.addend = f.addend; a.ep_relu = f.relu ? 1 : 0;
      rc = conv_gemm_route(a, elem_bytes, r) ? MMSKIN_OK : MMSKIN_ERR_ARG;
    }
  }
  if (rc) return rc;
  const int64_t v[9] = {r.family, r.bm, r.step, r.bn, r.nst, r.epi, r.group_m, r.total_mblk, r.nblk_n};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return MMSKIN_OK;
}
int64_t mmskin_slice_stats_workspace_bytes(int64_t rows, int pitch, int c0, int C) {
  if (!SLICE_OK) return -1;
  return ws_bytes<SliceStatsWs<float>>(rows, pitch, C);
}
int mmskin_slice_stats(const float* x, int64_t rows, int pitch, int c0, int C, float* mean, float* var, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && mean && var && workspace && SLICE_OK, "slice_stats: bad argument (C = %d, c0 = %d, pitch = %d: multiples of 8, c0 + C <= pitch)", C, c0, pitch);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, slice_stats_op<float>(x, rows, pitch, c0, C, mean, var, workspace, st),
           slice_stats_op<bf16_t>(x, rows, pitch, c0, C, mean, var, workspace, st));
}
#undef SLICE_OK

#define POOL2_OK (N > 0 && C > 0 && C % 8 == 0 && H >= 2 && W >= 2)
int64_t mmskin_maxpool2_relu_workspace_bytes(int N, int C, int H, int W) {
  if (!POOL2_OK) return -1;
  return ws_bytes<MaxpoolWs<float>>(N, C, H, W);
}
/* idx: the argmax tap (0..3, row-major inside the window) of every pooled element, in the kernel's layout [N][H/2][W/2][C] */
int mmskin_maxpool2_relu_forward(const float* y, float* pooled, unsigned char* idx, int N, int C, int H, int W, int dtype, void* workspace,
                                 void* stream) {
  ARG_CHECK(y && pooled && idx && workspace && POOL2_OK, "maxpool2_relu_forward: bad argument (C = %d a multiple of 8, map %dx%d at least 2x2)", C, H, W);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, maxpool_fwd_op<float>(y, pooled, idx, N, C, H, W, workspace, st), maxpool_fwd_op<bf16_t>(y, pooled, idx, N, C, H, W, workspace, st));
}
int mmskin_maxpool2_relu_backward(const float* dpool, const float* y, float* dz, int N, int C, int H, int W, int dtype, void* workspace,
                                  void* stream) {
  ARG_CHECK(dpool && y && dz && workspace && POOL2_OK, "maxpool2_relu_backward: bad argument (C = %d a multiple of 8, map %dx%d at least 2x2)", C, H, W);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, maxpool_bwd_op<float>(dpool, y, dz, N, C, H, W, workspace, st), maxpool_bwd_op<bf16_t>(dpool, y, dz, N, C, H, W, workspace, st));
}
#undef POOL2_OK

#define APOOL_OK (N > 0 && C > 0 && H > 0 && W > 0)
int64_t mmskin_adaptive_avgpool_workspace_bytes(int N, int C, int H, int W) {
  if (!APOOL_OK) return -1;
  return ws_bytes<AdaptivePoolWs<float>>(N, C, H, W);
}
/* AdaptiveAvgPool2d(7): x [N][C][H][W] -> out [N][C][7][7] (fp32, as the plan writes its features), and its backward */
int mmskin_adaptive_avgpool_forward(const float* x, float* out, int N, int C, int H, int W, int dtype, void* workspace, void* stream) {
  ARG_CHECK(x && out && workspace && APOOL_OK, "adaptive_avgpool_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, adaptive_fwd_op<float>(x, out, N, C, H, W, workspace, st), adaptive_fwd_op<bf16_t>(x, out, N, C, H, W, workspace, st));
}
int mmskin_adaptive_avgpool_backward(const float* dout, float* dx, int N, int C, int H, int W, int dtype, void* workspace, void* stream) {
  ARG_CHECK(dout && dx && workspace && APOOL_OK, "adaptive_avgpool_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, adaptive_bwd_op<float>(dout, dx, N, C, H, W, workspace, st), adaptive_bwd_op<bf16_t>(dout, dx, N, C, H, W, workspace, st));
}
#undef APOOL_OK

int64_t mmskin_groupnorm8_relu_workspace_bytes(int N, int C, int H, int W, int groups, int pool) {
  if (gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_workspace_bytes")) return -1;
  return ws_bytes<GroupNormWs<float>>(N, C, H, W, pool != 0);
}
int mmskin_groupnorm8_relu_forward(const float* y, const float* gamma, const float* beta, float* out, unsigned char* idx, float* mean, float* rstd,
                                   int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace, void* stream) {
  if (int rc = gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_forward")) return rc;
  ARG_CHECK(y && gamma && beta && out && workspace && (!pool || idx), "groupnorm8_relu_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, groupnorm_fwd_op<float>(y, gamma, beta, out, idx, mean, rstd, N, C, H, W, pool != 0, eps, workspace, st),
           groupnorm_fwd_op<bf16_t>(y, gamma, beta, out, idx, mean, rstd, N, C, H, W, pool != 0, eps, workspace, st));
}
int mmskin_groupnorm8_relu_backward(const float* gout, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta,
                                    int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace, void* stream) {
  if (int rc = gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_backward")) return rc;
  ARG_CHECK(gout && y && gamma && beta && dy && workspace, "groupnorm8_relu_backward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, groupnorm_bwd_op<float>(gout, y, gamma, beta, dy, dgamma, dbeta, N, C, H, W, pool != 0, eps, workspace, st),
           groupnorm_bwd_op<bf16_t>(gout, y, gamma, beta, dy, dgamma, dbeta, N, C, H, W, pool != 0, eps, workspace, st));
}

int64_t mmskin_groupnorm8_relu_gap_workspace_bytes(int N, int C, int H, int W, int groups, int pool) {
  if (gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_gap_workspace_bytes")) return -1;
  return ws_bytes<GroupNormGapWs<float>>(N, C, H, W);
}
int mmskin_groupnorm8_relu_gap_forward(const float* y, const float* gamma, const float* beta, float* feat, float* mean, float* rstd, int N, int C,
                                       int H, int W, int groups, int pool, float eps, int dtype, void* workspace, void* stream) {
  if (int rc = gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_gap_forward")) return rc;
  ARG_CHECK(y && gamma && beta && feat && workspace, "groupnorm8_relu_gap_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, groupnorm_gap_fwd_op<float>(y, gamma, beta, feat, mean, rstd, N, C, H, W, pool != 0, eps, workspace, st),
           groupnorm_gap_fwd_op<bf16_t>(y, gamma, beta, feat, mean, rstd, N, C, H, W, pool != 0, eps, workspace, st));
}
int mmskin_groupnorm8_relu_gap_backward(const float* dfeat, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma,
                                        float* dbeta, int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace,
                                        void* stream) {
  if (int rc = gn8_check(N, C, H, W, groups, pool != 0, "groupnorm8_relu_gap_backward")) return rc;
  ARG_CHECK(dfeat && y && gamma && beta && dy && workspace, "groupnorm8_relu_gap_backward: null argument");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype, groupnorm_gap_bwd_op<float>(dfeat, y, gamma, beta, dy, dgamma, dbeta, N, C, H, W, pool != 0, eps, workspace, st),
           groupnorm_gap_bwd_op<bf16_t>(dfeat, y, gamma, beta, dy, dgamma, dbeta, N, C, H, W, pool != 0, eps, workspace, st));
}

}  // extern "C"
