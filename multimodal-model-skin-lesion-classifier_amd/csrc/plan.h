// Shared scaffolding of the image-encoder plan executors (backbone.hip: ResNet, densenet.hip: DenseNet, vgg.hip: VGG,
// mbconv.hip: MobileNet-V2 / EfficientNet, dynamic_cnn.hip: the NAS DynamicCNN trunk).
// A plan is built once per (architecture, batch, H, W, dtype): it fixes the flat parameter / buffer
// layout (torchvision named_parameters() order), the workspace carve-up and the launch sequence, so
// that one C-ABI call runs a whole forward or backward on the caller's stream.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "conv.h"
#include "ops.h"

struct TensorInfo {
  std::string name;
  int64_t offset, numel;
  int ndim;
  int64_t shape[4];
};

enum KClass { K_CONV_FWD = 0, K_CONV_DGRAD, K_WGRAD, K_BN_FWD, K_BN_BWD, K_STAGE, K_STEM_MISC, K_NCLASS };

// Optional per-kernel-class timing with HIP events recorded on the launch stream (bench.py's live
// roofline).  Off by default: the timed region of a benchmark never pays for it.
struct Profiler {
  bool on = false;
  std::vector<hipEvent_t> pool;
  std::vector<int> cls;       // class of event pair i (events 2i, 2i+1)
  size_t used = 0;
  double flops[K_NCLASS] = {0};
  double bytes[K_NCLASS] = {0};
  hipEvent_t get() {
    if (used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
    return pool[used++];
  }
  void begin(int c, hipStream_t st) { if (on) { cls.push_back(c); (void)hipEventRecord(get(), st); } }
  void end(hipStream_t st) { if (on) (void)hipEventRecord(get(), st); }
  void reset() { used = 0; cls.clear(); for (int i = 0; i < K_NCLASS; ++i) { flops[i] = 0; bytes[i] = 0; } }
};

// Weight-gradient GEMMs only feed the optimizer, so they run on a second HIP stream beside the
// dgrad -> BN-backward chain of the main stream (fills launch tails and latency-bound phases).
// A slot stands for one operand buffer the main stream writes and a side-stream launch reads: the hand-off is run(), and the
// main stream calls acquire() before it writes that buffer again.
struct SideStream {
  hipStream_t s = nullptr;
  struct Slot {
    hipEvent_t ready = nullptr;   // main: the buffer holds a fresh operand
    hipEvent_t done = nullptr;    // side: the launch reading the buffer has finished
    bool done_valid = false;
  };
  std::vector<Slot> slots;
  hipEvent_t f_ready = nullptr, f_done = nullptr;      // forward: block input ready / downsample branch finished
  hipEvent_t f_staged = nullptr;                       // forward: weights of the residual stages staged (beside the stem)
  int init(int nslots) {
    if (s) return MMSKIN_OK;
    HIP_CHECK_RET(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));   // normal priority: high / low measured no different
    slots.resize(nslots);
    for (Slot& x : slots) {
      HIP_CHECK_RET(hipEventCreateWithFlags(&x.ready, hipEventDisableTiming));
      HIP_CHECK_RET(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
    }
    HIP_CHECK_RET(hipEventCreateWithFlags(&f_ready, hipEventDisableTiming));
    HIP_CHECK_RET(hipEventCreateWithFlags(&f_done, hipEventDisableTiming));
    HIP_CHECK_RET(hipEventCreateWithFlags(&f_staged, hipEventDisableTiming));
    return MMSKIN_OK;
  }
  void destroy() {
    if (!s) return;
    for (Slot& x : slots) {
      if (x.ready) (void)hipEventDestroy(x.ready);
      if (x.done) (void)hipEventDestroy(x.done);
    }
    if (f_ready) (void)hipEventDestroy(f_ready);
    if (f_done) (void)hipEventDestroy(f_done);
    if (f_staged) (void)hipEventDestroy(f_staged);
    (void)hipStreamDestroy(s);
    s = nullptr;
  }
  void begin_backward() { for (Slot& x : slots) x.done_valid = false; }   // nothing of the previous backward is pending
  // main may overwrite the slot's buffer only after the side-stream launch that reads it has finished
  int acquire(int slot, hipStream_t main, bool use_side) {
    if (use_side && slots[slot].done_valid) HIP_CHECK_RET(hipStreamWaitEvent(main, slots[slot].done, 0));
    return MMSKIN_OK;
  }
  // launch(stream) reads the slot's buffer: on the side stream behind everything main has enqueued so far, or (use_side off: the
  // profiled path) on main itself
  template <class F>
  int run(int slot, hipStream_t main, bool use_side, F launch) {
    if (!use_side) return launch(main);
    Slot& x = slots[slot];
    HIP_CHECK_RET(hipEventRecord(x.ready, main));
    HIP_CHECK_RET(hipStreamWaitEvent(s, x.ready, 0));
    if (int rc = launch(s)) return rc;
    HIP_CHECK_RET(hipEventRecord(x.done, s));
    x.done_valid = true;
    return MMSKIN_OK;
  }
};

struct PlanBase {
  Profiler prof;
  SideStream side;
  int N = 0, H = 0, W = 0, dtype = 0;
  int feat_dim = 0;
  int out_h = 1, out_w = 1;   // spatial size of the output (1x1 = pooled features; >1 for feature-map plans)
  std::vector<TensorInfo> params, buffers;
  int64_t param_numel = 0, buffer_numel = 0;
  StageDesc* table_dev = nullptr;
  std::vector<StageDesc> table_host;
  int max_stage_elems = 0;
  size_t ws_bytes = 0;
  size_t esz() const { return dtype == 1 ? 2 : 4; }

  // Gradient segments: contiguous ranges of the flat gradient arena in the order backward COMPLETES them,
  // each with an event pair (main stream: BN gamma/beta gradients; side stream: weight gradients), so the caller can
  // start the data-parallel all-reduce of a finished range while the rest of backward is still running.
  struct GradSegment {
    int64_t offset = 0, numel = 0;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    bool side_valid = false;
  };
  std::vector<GradSegment> segments;
  int segment_done(int i, hipStream_t st, bool use_side) {   // called by backward once segment i is fully enqueued
    GradSegment& g = segments[i];
    if (!g.ev_main) {
      HIP_CHECK_RET(hipEventCreateWithFlags(&g.ev_main, hipEventDisableTiming));
      HIP_CHECK_RET(hipEventCreateWithFlags(&g.ev_side, hipEventDisableTiming));
    }
    HIP_CHECK_RET(hipEventRecord(g.ev_main, st));
    g.side_valid = use_side;
    if (use_side) HIP_CHECK_RET(hipEventRecord(g.ev_side, side.s));
    return MMSKIN_OK;
  }
  int segment_wait(int i, hipStream_t waiter) {
    GradSegment& g = segments[i];
    if (!g.ev_main) return MMSKIN_ERR_ARG;   // no backward has run yet
    HIP_CHECK_RET(hipStreamWaitEvent(waiter, g.ev_main, 0));
    if (g.side_valid) HIP_CHECK_RET(hipStreamWaitEvent(waiter, g.ev_side, 0));
    return MMSKIN_OK;
  }

  virtual ~PlanBase() {
    if (table_dev) (void)hipFree(table_dev);
    for (GradSegment& g : segments)
      if (g.ev_main) { (void)hipEventDestroy(g.ev_main); (void)hipEventDestroy(g.ev_side); }
    side.destroy();
  }
  // image: fp32 NCHW, or (norm6 != nullptr) uint8 NHWC normalised on the fly with the 6 host floats mean rgb | std rgb
  virtual int forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                      float* features, bool training, hipStream_t st) = 0;
  virtual int backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) = 0;
  // Grad-CAM support: the raw output of the network's last nn.Conv2d and d(features)/d(that output)
  // for an eval-mode forward that kept raw conv outputs (option "keep_raw_eval"); plans without it: unsupported
  bool keep_raw_eval = false;
  // Serving: option "reuse_staged" = the caller vouches that parameters and BatchNorm buffers are unchanged
  // since the previous folded eval forward on this workspace, so the staged (BN-folded) weights and the coefficient
  // table already in it are reused instead of rebuilt.  Plans that do not implement it simply restage.
  bool reuse_staged = false;
  const void* staged_eval_ws = nullptr;
  virtual int last_conv_shape(int*, int*, int*) const { return MMSKIN_ERR_UNSUPPORTED; }
  virtual int last_conv_export(const unsigned char*, float*, hipStream_t) { return MMSKIN_ERR_UNSUPPORTED; }
  virtual int last_conv_grad(const float*, const unsigned char*, float*, hipStream_t) { return MMSKIN_ERR_UNSUPPORTED; }
  // per-step device pointers handed in by the host (e.g. "sd_mask": stochastic-depth keep/scale factors)
  virtual int set_pointer(const char*, const void*) { return MMSKIN_ERR_UNSUPPORTED; }
  // per-unit introspection (tests / diagnostics); plans without it report zero units
  virtual int num_units() const { return 0; }
  virtual int unit_info(int, std::string*, int64_t*) const { return MMSKIN_ERR_UNSUPPORTED; }
  virtual int unit_flags(int, int*) const { return MMSKIN_ERR_UNSUPPORTED; }   // MMSKIN_UNIT_* bits: the plan's decisions for one unit

  int ensure_table() {   // uploaded on the first forward (create() needs no GPU)
    if (table_dev) return MMSKIN_OK;
    HIP_CHECK_RET(hipMalloc((void**)&table_dev, table_host.size() * sizeof(StageDesc)));
    HIP_CHECK_RET(hipMemcpy(table_dev, table_host.data(), table_host.size() * sizeof(StageDesc),
                            hipMemcpyHostToDevice));
    return MMSKIN_OK;
  }
};

static inline int64_t add_tensor(std::vector<TensorInfo>& v, int64_t& total, const std::string& name,
                                 std::initializer_list<int64_t> shape) {
  TensorInfo t;
  t.name = name;
  t.offset = total;
  t.ndim = (int)shape.size();
  t.numel = 1;
  int i = 0;
  for (int64_t d : shape) { t.shape[i++] = d; t.numel *= d; }
  for (; i < 4; ++i) t.shape[i] = 1;
  total += t.numel;
  v.push_back(t);
  return t.offset;
}

// One BatchNorm2d's flat offsets: weight, bias (params) and running_mean, running_var (buffers), in torchvision's order.
struct BNRef {
  int64_t g_off, b_off, rm_off, rv_off;
};

static inline BNRef add_bn(PlanBase& p, const std::string& name, int C) {
  BNRef r;
  r.g_off = add_tensor(p.params, p.param_numel, name + ".weight", {C});
  r.b_off = add_tensor(p.params, p.param_numel, name + ".bias", {C});
  r.rm_off = add_tensor(p.buffers, p.buffer_numel, name + ".running_mean", {C});
  r.rv_off = add_tensor(p.buffers, p.buffer_numel, name + ".running_var", {C});
  return r;
}

static inline size_t carve(size_t& cursor, size_t bytes) {
  size_t o = cursor;
  cursor = align_up(cursor + bytes, 256);
  return o;
}

// One staged weight [Cout][Cin][taps] appended to `table` (every plan's stage table and the op-level carves of capi.hip).  wf / wd: the
// running element cursors of the forward / data-gradient staging buffers, the weight's own offsets returned in wf_off / wd_off.
// Cop / Cip: the staged (zero-padded) dims, 0 = as Cout / Cin.
inline void stage_append(std::vector<StageDesc>& table, int64_t src, int Cout, int Cin, int taps, int Cop, int Cip, int64_t& wf, int64_t& wd,
                         int& max_stage_elems, int64_t& wf_off, int64_t& wd_off) {
  StageDesc d = {};
  d.src_off = src; d.Cout = Cout; d.Cin = Cin; d.taps = taps; d.Cout_pad = Cop; d.Cin_pad = Cip;
  wf_off = wf; wd_off = wd;
  d.fwd_off = wf; d.dgrad_off = wd;
  const int64_t n = (int64_t)(Cop ? Cop : Cout) * (Cip ? Cip : Cin) * taps;
  wf += n; wd += n;
  if (n > max_stage_elems) max_stage_elems = (int)n;
  table.push_back(d);
}

// The body of every plan factory (create() needs no GPU): a Plan for (N, H, W, dtype) that build(plan) fills; nullptr and *rc on failure
template <class Plan, class Build>
PlanBase* make_plan(int N, int H, int W, int dtype, int* rc, Build build) {
  Plan* p = new Plan();
  p->N = N; p->H = H; p->W = W; p->dtype = dtype;
  *rc = build(*p);
  if (*rc) { delete p; return nullptr; }
  return p;
}
// f(T()) for the plan's element type: the forward / backward overrides call their templates through it
template <class F>
int by_dtype(int dtype, F f) { return dtype == 1 ? f(bf16_t()) : f(float()); }

// One profiler event pair around `call_` on stream `st`, its FLOPs / bytes added to class cls_; returns from the enclosing function
// (which has `int rc` and `hipStream_t st`) when the call fails.  prof_ may be null (op-level callers).
#define PROF_AT(prof_, cls_, flops_, bytes_, call_)            \
  do {                                                        \
    Profiler* pr_ = (prof_);                                  \
    if (pr_) pr_->begin((cls_), st);                          \
    rc = (call_);                                             \
    if (pr_) pr_->end(st);                                    \
    if (pr_ && pr_->on) { pr_->flops[(cls_)] += (flops_); pr_->bytes[(cls_)] += (bytes_); } \
    if (rc) return rc;                                        \
  } while (0)
#define PROF(cls_, flops_, bytes_, call_) PROF_AT(&p.prof, cls_, flops_, bytes_, call_)
// The same pair around a group of launches: opened here, closed when the scope is left on any path.
struct ProfScope {
  Profiler* pr;
  hipStream_t st;
  ProfScope(Profiler* prof, int cls, hipStream_t stream, double flops, double bytes) : pr(prof), st(stream) {
    if (!pr) return;
    pr->begin(cls, st);
    if (pr->on) { pr->flops[cls] += flops; pr->bytes[cls] += bytes; }
  }
  ~ProfScope() { if (pr) pr->end(st); }
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
};

static inline double conv_flops(const ConvShape& s) {
  return 2.0 * s.N * s.OH() * s.OW() * (double)s.Cout * s.Cin * s.kh * s.kw;
}
// algorithmic HBM bytes of one conv GEMM pass: input once, output once, weights once, plus `extra`
// input-shaped tensors read by a fused dgrad epilogue (addend, mask source, BN inputs)
static inline double conv_bytes(const ConvShape& s, size_t es, int extra_in_shaped = 0) {
  double in = (double)s.N * s.H * s.W * s.Cin, out = (double)s.N * s.OH() * s.OW() * s.Cout;
  return (in * (1 + extra_in_shaped) + out) * es + (double)s.Cout * s.Cin * s.kh * s.kw * es;
}

// ---- BatchNorm coefficient blocks.  Forward: scale | shift | mean | invstd | gamma, C floats each, written by bn_finalize (the first
// four), bn_eval_coeffs / bn_eval_table (the first two) or bn_coef_from_table (all five: gamma is the copy zero-padded to C channels).
// A view over a block of only two or four slots simply does not touch the later members.
struct BnCoef {
  float *scale, *shift, *mean, *invstd, *gamma;
  BnCoef(float* base, int C) : scale(base), shift(scale + C), mean(shift + C), invstd(mean + C), gamma(invstd + C) {}
};
// Backward: dx = cA * dz + cB * x + cC, written by bn_bwd_finalize
struct BnBwdCoef {
  float *cA, *cB, *cC;
  BnBwdCoef(float* base, int C) : cA(base), cB(cA + C), cC(cB + C) {}
};

// BatchNorm backward when the masked gradient dz already exists and its partial sums (sum dz, sum dz * x) came from the epilogue of the
// launch that wrote it: finalize (gamma / beta gradients for channels < n_grad, and c) + one apply pass dx = cA dz + cB x + cC.
// dx == nullptr: finalize only.  accumulate_bc / sum_dz_x: as bn_bwd_finalize.  One profiler pair (prof may be null) with the
// caller's byte count.
template <typename T>
int bn_backward_from_sums(const T* dz, const T* x, const float* partial, int nrows, size_t rows, int C, const BnCoef& k, const float* gamma,
                          float* dgamma, float* dbeta, const BnBwdCoef& c, ColScratch red, T* dx, Profiler* prof, double prof_bytes,
                          hipStream_t st, int n_grad = -1, bool accumulate_bc = false, const float* sum_dz_x = nullptr) {
  ProfScope scope(prof, K_BN_BWD, st, 0.0, prof_bytes);
  if (int rc = bn_bwd_finalize(partial, nrows, C, (double)rows, gamma, k.mean, k.invstd, dgamma, dbeta, c.cA, c.cB, c.cC, red, st, n_grad,
                               accumulate_bc, sum_dz_x)) return rc;
  if (!dx) return MMSKIN_OK;
  return bn_bwd_apply<T>(dz, x, nullptr, k.scale, k.shift, MASK_NONE, c.cA, c.cB, c.cC, dx, nullptr, rows, C, st);
}
// BatchNorm (+ activation mask `mode` from x or ymask) backward from dy: reduce -> finalize -> apply; fills dx and, when given, dz (the
// masked dy).  One profiler pair with the caller's byte count.
template <typename T>
int bn_backward(const T* dy, const T* x, const T* ymask, int mode, size_t rows, int C, const BnCoef& k, const float* gamma, float* dgamma,
                float* dbeta, const BnBwdCoef& c, float* partial, ColScratch red, T* dx, T* dz, Profiler* prof, double prof_bytes,
                hipStream_t st, int n_grad = -1) {
  ProfScope scope(prof, K_BN_BWD, st, 0.0, prof_bytes);
  int nr = 0;
  if (int rc = bn_bwd_reduce<T>(dy, x, ymask, k.scale, k.shift, mode, rows, C, partial, &nr, st)) return rc;
  if (int rc = bn_bwd_finalize(partial, nr, C, (double)rows, gamma, k.mean, k.invstd, dgamma, dbeta, c.cA, c.cB, c.cC, red, st, n_grad)) return rc;
  return bn_bwd_apply<T>(dy, x, ymask, k.scale, k.shift, mode, c.cA, c.cB, c.cC, dx, dz, rows, C, st);
}

// ---- the 7x7 / stride 2 stem of ResNet and DenseNet: conv -> BatchNorm -> ReLU -> max-pool 3x3 / stride 2, 64 channels
struct StemGeom {
  int N, H, W;
  int OH, OW;   // conv output
  int Hp, Wp;   // zero-padded NHWC4 image the conv kernels read (stem_pack): 3 px top / left border, even width
  int PH, PW;   // pooled output
  StemGeom(int n = 0, int h = 0, int w = 0) : N(n), H(h), W(w) {
    OH = (H + 6 - 7) / 2 + 1; OW = (W + 6 - 7) / 2 + 1;
    Hp = 2 * OH + 8; Wp = 2 * OW + 8;
    if (Hp < H + 6) Hp = H + 6;
    if (Wp < W + 6) Wp = W + 6;
    Wp = (Wp + 1) / 2 * 2;
    PH = pool3s2_out(OH); PW = pool3s2_out(OW);
  }
  size_t rows() const { return (size_t)N * OH * OW; }
  size_t pooled() const { return (size_t)N * PH * PW; }
  ConvShape conv() const { return ConvShape{N, H, W, 3, 64, 7, 7, 2, 3}; }
};
// The stem's buffers: the plans fill it from their workspace offsets, the op-level entry points from their carve.
template <typename T>
struct StemBufs {
  T* img4 = nullptr;         // packed image [N][Hp][Wp][4]
  const T* wv = nullptr;     // staged weights (64 x 256, zero padding taps)
  T* x0 = nullptr;           // raw conv output [rows][64]
  T* pool = nullptr;         // pooled activation [pooled][64]
  uint8_t* idx = nullptr;    // argmax tap of every pooled element
  float* coef = nullptr;     // BnCoef block (4 slots)
  float *ssum = nullptr, *ssq = nullptr;   // batch-statistics slabs of the conv epilogue
  ColScratch red;            // reduction scratch of the finalize kernels
  // backward
  float* coefbwd = nullptr;  // BnBwdCoef block
  float* partial = nullptr;  // BatchNorm-backward partial sums
  T* dx0 = nullptr;          // gradient of the raw conv output [rows][64]
  WgradSlab slab = {};       // weight-gradient slab with the floats carved for it
  float* dwv = nullptr;      // the gradient in the staged (64 x 256) layout
};
// Where the stem's BatchNorm coefficients come from
struct StemBn {
  const float *gamma = nullptr, *beta = nullptr;   // both null: coef already holds scale | shift (folded eval: bn_eval_table wrote them)
  float *rm = nullptr, *rv = nullptr;              // running statistics: updated (batch_stats; may be null) or read
  float eps = 1e-5f, mom = 0.1f;
  bool batch_stats = false;                        // training: statistics of this batch from the conv epilogue
};
// image: fp32 NCHW, uint8 NHWC with norm6 (PlanBase::forward), or null when b.img4 is packed already
template <typename T>
int stem_forward(const StemBufs<T>& b, const StemGeom& g, const void* image, const float* norm6, const StemBn& bn, Profiler* prof,
                 hipStream_t st) {
  int rc, stat_rows = 0;
  if (image && norm6) PROF_AT(prof, K_STEM_MISC, 0.0, 0.0, stem_pack_u8<T>((const uint8_t*)image, g.N, g.H, g.W, g.Hp, g.Wp, norm6, b.img4, st));
  else if (image) PROF_AT(prof, K_STEM_MISC, 0.0, 0.0, stem_pack<T>((const float*)image, g.N, g.H, g.W, g.Hp, g.Wp, b.img4, st));
  const ConvShape s = g.conv();
  const BnCoef k(b.coef, 64);
  PROF_AT(prof, K_CONV_FWD, conv_flops(s), conv_bytes(s, sizeof(T)),
          launch_stem_conv_fwd<T>(g.N, g.OH, g.OW, g.Hp, g.Wp, b.img4, b.wv, b.x0, bn.batch_stats ? b.ssum : nullptr,
                                  bn.batch_stats ? b.ssq : nullptr, st, &stat_rows));
  if (bn.batch_stats)
    PROF_AT(prof, K_BN_FWD, 0.0, 0.0, bn_finalize(b.ssum, b.ssq, stat_rows, 64, (double)g.rows(), bn.gamma, bn.beta, bn.eps, bn.mom, bn.rm, bn.rv,
                                                  k.scale, k.shift, k.mean, k.invstd, b.red, st));
  else if (bn.gamma)
    PROF_AT(prof, K_BN_FWD, 0.0, 0.0, bn_eval_coeffs(64, bn.gamma, bn.beta, bn.rm, bn.rv, bn.eps, k.scale, k.shift, st));
  // one pass over the largest activation: BatchNorm + ReLU + max-pool
  PROF_AT(prof, K_STEM_MISC, 0.0, 0.0, stem_bn_relu_pool<T>(b.x0, k.scale, k.shift, g.N, g.OH, g.OW, 64, b.pool, b.idx, st));
  return MMSKIN_OK;
}
// dpool (gradient of the pooled activation) -> b.dx0 and dgamma / dbeta: max-pool + ReLU + BatchNorm backward without materialising the
// full-resolution pooled gradient.  sums_pooled (callers: stem_sums_pooled()): the partial sums come from the pooled tensors alone
// instead of the conv output and the routed gradient.  One profiler pair with the caller's byte count.
template <typename T>
int stem_backward(const StemBufs<T>& b, const StemGeom& g, const T* dpool, const float* gamma, float* dgamma, float* dbeta, bool sums_pooled,
                  Profiler* prof, double prof_bytes, hipStream_t st) {
  const BnCoef k(b.coef, 64);
  const BnBwdCoef c(b.coefbwd, 64);
  ProfScope scope(prof, K_BN_BWD, st, 0.0, prof_bytes);
  int rc, nr = 0;
  if (sums_pooled) rc = stem_pool_bwd_sums<T>(dpool, b.pool, b.idx, b.x0, k.scale, k.shift, g.N, g.OH, g.OW, 64, b.partial, &nr, st);
  else rc = stem_pool_bn_bwd_reduce<T>(dpool, b.idx, b.x0, k.scale, k.shift, g.N, g.OH, g.OW, 64, b.partial, &nr, st);
  if (rc) return rc;
  if ((rc = bn_backward_from_sums<T>(nullptr, nullptr, b.partial, nr, g.rows(), 64, k, gamma, dgamma, dbeta, c, b.red, nullptr, nullptr, 0.0, st)))
    return rc;
  return stem_pool_bn_bwd_apply<T>(dpool, b.idx, b.x0, k.scale, k.shift, c.cA, c.cB, c.cC, g.N, g.OH, g.OW, 64, b.dx0, st);
}
// b.dx0, b.img4 -> dw [64][3][7][7], on the stream the caller picks (SideStream::run: it needs the slab)
template <typename T>
int stem_wgrad(const StemBufs<T>& b, const StemGeom& g, float* dw, Profiler* prof, hipStream_t st) {
  int rc;
  PROF_AT(prof, K_WGRAD, conv_flops(g.conv()), 0.0, launch_stem_conv_wgrad<T>(g.N, g.OH, g.OW, g.Hp, g.Wp, b.dx0, b.img4, b.slab, b.dwv, st));
  return stem_wgrad_unpack(b.dwv, dw, st);
}

// ---- the 3-channel 3x3 first conv of VGG, DynamicCNN (stride 1), MobileNet-V2 and EfficientNet (stride 2): FirstGeom in conv.h
template <typename T>
struct FirstBufs {
  T* img8 = nullptr;      // packed image [N][Hp][Wp][8]
  T* wv = nullptr;        // staged weights [64][128]: slot 0 of the plan's forward staging buffer
  T* out = nullptr;       // conv output [rows][64]
  WgradSlab slab = {};    // weight-gradient slab with the floats carved for it
  float* dwv = nullptr;   // the gradient in the staged layout
};
// Where a plan keeps them (byte offsets into its workspace).  The image is the front of the workspace, dwv sits where the plan calls
// dwv(); the staged weights are the first FirstGeom::WV_ELEMS elements of the forward staging buffer, so the plan's stage_append cursor
// starts there.
struct FirstCarve {
  size_t off_img8 = 0, off_dwv = 0;
  // returns the first conv's weight-gradient slab bytes: the seed of the plan's slab maximum
  size_t image(size_t& cur, const FirstGeom& g, size_t es) { off_img8 = carve(cur, g.img8_elems() * es); return first3_wgrad_slab_bytes(g); }
  void dwv(size_t& cur) { off_dwv = carve(cur, FirstGeom::WV_ELEMS * sizeof(float)); }
  template <typename T>
  FirstBufs<T> bufs(unsigned char* ws, T* wv, T* out, WgradSlab slab = {}) const {
    return FirstBufs<T>{reinterpret_cast<T*>(ws + off_img8), wv, out, slab, reinterpret_cast<float*>(ws + off_dwv)};
  }
};
// image (as PlanBase::forward takes it) -> b.out: stage w [cout][3][3][3] (null: b.wv is staged already), pack, conv.  fuse: optional
// bias / ReLU epilogue; ssum / ssq: optional batch-statistics slabs; flops_scale: the share of the 64-column GEMM the caller's profile counts
template <typename T>
int first_conv_forward(const FirstBufs<T>& b, const FirstGeom& g, const void* image, const float* norm6, const float* w, const FwdFuse* fuse,
                       float* ssum, float* ssq, Profiler* prof, hipStream_t st, double flops_scale = 1.0) {
  int rc;
  if (w) PROF_AT(prof, K_STAGE, 0.0, 0.0, first3_stage<T>(w, b.wv, st));
  PROF_AT(prof, K_STEM_MISC, 0.0, 0.0, pack_nhwc8<T>(image, norm6, g.N, g.H, g.W, g.Hp, g.Wp, b.img8, st));
  PROF_AT(prof, K_CONV_FWD, conv_flops(g.conv()) * flops_scale, conv_bytes(g.conv(), sizeof(T)),
          launch_first3_conv_fwd<T>(g, b.img8, b.wv, b.out, fuse, st, ssum, ssq));
  return MMSKIN_OK;
}
// dy (gradient of b.out), b.img8 -> dw [cout][3][3][3]
template <typename T>
int first_conv_wgrad(const FirstBufs<T>& b, const FirstGeom& g, const T* dy, float* dw, int cout, Profiler* prof, hipStream_t st,
                     double flops_scale = 1.0) {
  int rc;
  PROF_AT(prof, K_WGRAD, conv_flops(g.conv()) * flops_scale, 0.0, launch_first3_conv_wgrad<T>(g, dy, b.img8, b.slab, b.dwv, st));
  return first3_wgrad_unpack(b.dwv, dw, st, cout);
}

// ---- squeeze-excitation (mbconv.hip): the chain the MBConv plan runs behind a depthwise unit, shared with the op-level entry
// points mmskin_se_* so that a test of the chain runs the plan's own launches.  Channels are padded to Cp = pad64(C).
struct SEArgs {
  int N, HW, C, Cp, Csq;
  const float* w1p;   // fc1 weight padded to [Csq][Cp]
  const float* b1;    // fc1 bias [Csq]
  const float* w2p;   // fc2 weight padded to [Cp][Csq]
  const float* b2p;   // fc2 bias padded to [Cp]
  float *s, *z1, *a1, *z2, *g;   // fp32 activations kept for backward: [N][Cp], [N][Csq], [N][Csq], [N][Cp], [N][Cp]
};
// floats of backward temporaries: dgate / dz2 / ds [N][Cp] x3, da1 / dz1 [N][Csq] x2, dW1p, dW2p, db2p (+ [N][Csq] slack)
static inline size_t se_backward_tmp_floats(int N, int Cp, int Csq) {
  return (size_t)3 * N * Cp + (size_t)2 * N * Csq + (size_t)2 * Csq * Cp + Cp + (size_t)N * Csq;
}
// yse = y * sigmoid(fc2(silu(fc1(mean_hw y))))          (prof may be null)
template <typename T>
int se_forward(const SEArgs& a, const T* y, T* yse, Profiler* prof, hipStream_t st);
// dyse -> dy = dyse * g + ds / HW, and the unpadded parameter gradients dW1 [Csq][C], db1 [Csq], dW2 [C][Csq], db2 [C]
template <typename T>
int se_backward(const SEArgs& a, const T* dyse, const T* y, float* tmp, float* dW1, float* db1, float* dW2, float* db2, T* dy,
                Profiler* prof, hipStream_t st);

// ---- DenseNet (densenet.hip): one dense block and one transition, shared with the op-level entry points mmskin_dense_* so that a
// test of a block runs the plan's own launches.  Offsets are bytes into the workspace (activations, coefficients), elements into the
// flat parameter / buffer / gradient arrays (BNRef, w*_off) and elements into the staged-weight buffers (wf*, wd*).
constexpr int DENSE_GROWTH = 32, DENSE_BOTTLE = 128, DENSE_G_PAD = 64;
struct DLayer {
  int Cin, Cp;
  BNRef n1, n2;
  int64_t w1_off, w2_off;        // flat param offsets
  int64_t wf1, wd1, wf2, wd2;    // staged element offsets
  size_t t_off, a_off, u_off;    // saved activations (bytes)
  size_t coef1_off, coef2_off;   // floats: 5*Cp | 4*128
  int tab1;                      // stage-table index of conv1 (norm2 folds into it for inference)
};
struct DBlock {
  int H, W, C0, Ctot;
  size_t rows;
  std::vector<DLayer> layers;
  size_t cat_off, dcat_off, tab_off;   // tab: mean[Ctot] | var[Ctot]
};
struct DTrans {
  int C;
  BNRef n;
  int64_t w_off, wf, wd;
  size_t tt_off, coef_off;   // coef: 5*C floats
};
// The geometry every carve of a dense layer shares (build_dense_plan and the op-level carves of capi.hip call these, so they cannot drift):
inline void dense_layer_geom(DLayer& l, int c0, int i) {   // layer i of a block whose input has c0 channels; operands padded to 64
  l.Cin = c0 + DENSE_GROWTH * i;
  l.Cp = (l.Cin + 63) / 64 * 64;
}
inline void dense_stage_layer(DLayer& l, std::vector<StageDesc>& table, int64_t& wf, int64_t& wd, int& max_stage_elems) {
  l.tab1 = (int)table.size();
  stage_append(table, l.w1_off, DENSE_BOTTLE, l.Cin, 1, DENSE_BOTTLE, l.Cp, wf, wd, max_stage_elems, l.wf1, l.wd1);
  stage_append(table, l.w2_off, DENSE_GROWTH, DENSE_BOTTLE, 9, DENSE_G_PAD, DENSE_BOTTLE, wf, wd, max_stage_elems, l.wf2, l.wd2);
}
// inference: conv1 carries norm2's scale, its epilogue adds shift + ReLU (coef2_off must be carved)
inline void dense_fold_norm2(const DLayer& l, std::vector<StageDesc>& table) {
  StageDesc& d = table[l.tab1];
  d.has_bn = 1;
  d.bn_g_off = l.n2.g_off; d.bn_b_off = l.n2.b_off; d.bn_rm_off = l.n2.rm_off; d.bn_rv_off = l.n2.rv_off;
  d.coef_off = (int64_t)l.coef2_off;
}
// bytes of BatchNorm-backward partial sums for `rows` rows of C channels: the stand-alone reduce's rows or a fused dgrad epilogue's
inline size_t dense_partial_bytes(size_t rows, int C) {
  size_t a = (size_t)bn_bwd_partial_rows(rows, C) * 2 * C * sizeof(float);
  size_t b = ((rows + 127) / 128 + 4) * 2 * (size_t)C * sizeof(float);
  return a > b ? a : b;
}
// what one layer asks of the shared scratch regions: statistics floats, partial bytes, weight-gradient slab bytes (maxima kept)
inline void dense_layer_needs(int N, int H, int W, size_t rows, const DLayer& l, size_t& stat_floats, size_t& partial_bytes, size_t& slab) {
  ConvShape c1 = {N, H, W, l.Cp, DENSE_BOTTLE, 1, 1, 1, 0}, c2 = {N, H, W, DENSE_BOTTLE, DENSE_G_PAD, 3, 3, 1, 1};
  auto up = [](size_t& m, size_t v) { if (v > m) m = v; };
  up(stat_floats, (size_t)conv_fwd_stat_rows(c1) * DENSE_BOTTLE);
  up(stat_floats, (size_t)conv_fwd_stat_rows(c2) * DENSE_G_PAD);
  up(partial_bytes, dense_partial_bytes(rows, l.Cp));
  up(partial_bytes, dense_partial_bytes(rows, DENSE_BOTTLE));
  up(slab, conv_wgrad_slab_bytes(c1));
  up(slab, conv_wgrad_slab_bytes(c2));
}
// What a block / transition runs on: the plan fills it from its workspace offsets, the op-level entry points from their carve.
template <typename T>
struct DenseRun {
  int N = 0;
  Profiler* prof = nullptr;        // may be null (op-level callers)
  unsigned char* ws = nullptr;
  const float* params = nullptr;
  float* buffers = nullptr;        // running statistics (forward)
  float* grads = nullptr;          // backward
  T *wf = nullptr, *wd = nullptr;  // staged weights
  float *stat_sum = nullptr, *stat_sq = nullptr;   // batch-statistics slabs
  ColScratch red;                  // reduction scratch of the finalize kernels
  T* sBq[2] = {nullptr, nullptr};  // conv2 output / gradient, padded to 64 channels (forward uses [0]); alternate between layers
  T* sAq[2] = {nullptr, nullptr};  // gradient of conv1's output
  T *sU = nullptr, *sZ = nullptr, *sC = nullptr;   // gradient of u; of the padded prefix t; the transition conv's output / its gradient
  WgradSlab slab = {};
  float *partial = nullptr, *cA = nullptr, *defer = nullptr;
  SideStream* side = nullptr;      // null: the weight-gradient GEMMs run on the caller's stream
  bool use_side = false;
  int layer_no = 0;                // layers seen by this backward (picks the alternating operand buffers)
};
// batch statistics of cat channels [c0, c0+C) of block b -> its mean/var table
template <typename T>
int dense_table_from_slice(DenseRun<T>& r, const DBlock& b, int c0, int C, hipStream_t st);
// every layer of block b on the block input already in cat[:, :C0] (training: its table entries written too)
template <typename T>
int dense_block_forward(DenseRun<T>& r, DBlock& b, bool training, hipStream_t st);
// norm -> relu -> conv 1x1 (C -> C/2) -> avgpool 2x2 of block b's cat into the channel prefix of dst rows of dst_pitch channels
template <typename T>
int dense_transition_forward(DenseRun<T>& r, DBlock& b, DTrans& t, T* dst, int dst_pitch, bool training, hipStream_t st);
// dcat of block b (whole concatenated output's gradient) -> parameter gradients, dcat[:, :C0] = gradient of the block input
template <typename T>
int dense_block_backward(DenseRun<T>& r, DBlock& b, hipStream_t st);
// gradient of the next block's cat prefix (rows of pitch_next channels) -> the whole of block pb's dcat, and the transition's gradients
template <typename T>
int dense_transition_backward(DenseRun<T>& r, DBlock& pb, DTrans& tr, const T* dcat_next, int pitch_next, hipStream_t st);

// plan factories (create() needs no GPU); return nullptr and set *rc on failure
PlanBase* make_resnet_plan(int arch, int N, int H, int W, int dtype, int* rc);
PlanBase* make_densenet_plan(int N, int H, int W, int dtype, bool feature_map, int* rc);
PlanBase* make_vgg_plan(int N, int H, int W, int dtype, int* rc);
PlanBase* make_dynamic_cnn_plan(const char* arch, int N, int H, int W, int dtype, int* rc);   // arch: the dynamic-cnn/... string (mmskin.h)
PlanBase* make_mobilenet_plan(int N, int H, int W, int dtype, int* rc);
PlanBase* make_efficientnet_plan(int variant, int N, int H, int W, int dtype, int* rc);
