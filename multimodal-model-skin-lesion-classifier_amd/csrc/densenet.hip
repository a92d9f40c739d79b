// DenseNet-169 image-encoder plan executor (torchvision layout: growth 32, blocks 6/12/32/32,
// bn_size 4, 64 stem features, 1664 output features).  Replaces `self.image_encoder(image)` of the
// reference for cnn_model_name == "densenet169" (loadImageModelClassifier.py:84-92 builds
// torchvision's densenet169 and drops its classifier) with the same kernels the ResNet plan uses.
//
// Data layout.  Each dense block owns ONE concatenated activation `cat` [rows][Ctot] (NHWC, compute
// dtype): layer i reads channels [0, Cin_i) and appends its 32 new channels at [Cin_i, Cin_i+32), so
// torch.cat never copies.  BatchNorm statistics of a cat channel are computed once, when the channel
// is written (conv2 epilogue partial sums / one slice_stats pass), into a per-block mean/var table
// every consumer (norm1 of later layers, the transition norm, norm5) reads.  The GEMM kernels want
// compact operands whose channel count is a multiple of 64, so norm1+ReLU writes a compact,
// zero-padded copy t_i [rows][Cp_i] (also what the weight-gradient GEMM needs later), and conv2 runs
// with its 32 output channels padded to 64 (zero weight rows) into a temp that is scattered into cat.
// Backward keeps ONE gradient buffer dcat per block; every layer accumulates its BN-backward result
// into the channel prefix it consumed.
#include "plan.h"

namespace {

constexpr int GROWTH = DENSE_GROWTH, BOTTLE = DENSE_BOTTLE, G_PAD = DENSE_G_PAD;

struct DensePlan : PlanBase {
  bool fmap = false;   // "densenet169-features": output = norm5 feature map [N][C][H/32][W/32] fp32 (MDNet), no ReLU / pool
  StemGeom sg;
  // stem
  int64_t w0_off; BNRef n0; int64_t wf0;
  size_t x0_off, coef0_off, off_pool, off_idx, off_img4;
  std::vector<DBlock> blocks;
  DTrans trans[3];
  BNRef n5; size_t coef5_off, y5_off;
  size_t off_wf, off_wd, off_stat, off_partial, off_coefbwd, off_defer, off_dwv, off_red, off_slab, slab_bytes;
  int red_C = 0;   // channels the reduction scratch was carved for (bn_reduce_scratch)
  size_t off_sB, off_sB2, off_sU, off_sA, off_sA2, off_sX, off_sZ, off_sC;
  size_t stat_bytes = 0;
  // weight-gradient GEMMs on the side stream (SideStream slots): 0/1 = conv2 operand (sB) of even/odd layers, 2/3 = conv1
  // operand (sA) of even/odd layers, 4 = transition operand (sC)
  static constexpr int SIDE_SLOTS = 5;

  int forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
              float* features, bool training, hipStream_t st) override;
  int backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) override;
};

int build_dense_plan(DensePlan& p) {
  const int depths[4] = {6, 12, 32, 32};
  // ---- parameters in torchvision's named_parameters() order (MDNet holds densenet.features itself: no prefix)
  const std::string pre = p.fmap ? "" : "features.";
  p.w0_off = add_tensor(p.params, p.param_numel, pre + "conv0.weight", {64, 3, 7, 7});
  p.n0 = add_bn(p, pre + "norm0", 64);
  p.sg = StemGeom(p.N, p.H, p.W);
  int c = 64, h = p.sg.PH, w = p.sg.PW;
  for (int bi = 0; bi < 4; ++bi) {
    ARG_CHECK(h >= 1 && w >= 1, "densenet169: input %dx%d too small", p.H, p.W);
    DBlock b;
    b.H = h; b.W = w; b.C0 = c; b.Ctot = c + GROWTH * depths[bi];
    b.rows = (size_t)p.N * h * w;
    for (int i = 0; i < depths[bi]; ++i) {
      DLayer l;
      dense_layer_geom(l, c, i);
      std::string base = pre + "denseblock" + std::to_string(bi + 1) + ".denselayer" + std::to_string(i + 1);
      l.n1 = add_bn(p, base + ".norm1", l.Cin);
      l.w1_off = add_tensor(p.params, p.param_numel, base + ".conv1.weight", {BOTTLE, l.Cin, 1, 1});
      l.n2 = add_bn(p, base + ".norm2", BOTTLE);
      l.w2_off = add_tensor(p.params, p.param_numel, base + ".conv2.weight", {GROWTH, BOTTLE, 3, 3});
      b.layers.push_back(l);
    }
    c = b.Ctot;
    p.blocks.push_back(b);
    if (bi < 3) {
      DTrans& t = p.trans[bi];
      std::string base = pre + "transition" + std::to_string(bi + 1);
      t.C = c;
      t.n = add_bn(p, base + ".norm", c);
      t.w_off = add_tensor(p.params, p.param_numel, base + ".conv.weight", {c / 2, c, 1, 1});
      c /= 2; h /= 2; w /= 2;
    }
  }
  p.n5 = add_bn(p, pre + "norm5", c);
  p.feat_dim = c;
  if (p.fmap) { p.out_h = h; p.out_w = w; }

  // ---- staged weights + stage table (stem first: its slot needs zeroed padding taps)
  int64_t wf = 0, wd = 0;
  auto stage = [&](int64_t src, int Cout, int Cin, int taps, int Cop, int Cip, int64_t& wf_off, int64_t& wd_off) {
    stage_append(p.table_host, src, Cout, Cin, taps, Cop, Cip, wf, wd, p.max_stage_elems, wf_off, wd_off);
  };
  {
    StageDesc d = {};
    d.src_off = p.w0_off; d.Cout = 64; d.Cin = 3; d.taps = 49; d.stem = 1; d.fwd_off = 0;
    p.wf0 = 0; wf = 64 * 256;
    p.max_stage_elems = 64 * 3 * 49;
    p.table_host.push_back(d);
  }
  for (DBlock& b : p.blocks)
    for (DLayer& l : b.layers) dense_stage_layer(l, p.table_host, wf, wd, p.max_stage_elems);
  for (int i = 0; i < 3; ++i) stage(p.trans[i].w_off, p.trans[i].C / 2, p.trans[i].C, 1, p.trans[i].C / 2, p.trans[i].C, p.trans[i].wf, p.trans[i].wd);

  // ---- workspace
  const size_t es = p.esz();
  size_t cur = 0;
  p.off_img4 = carve(cur, (size_t)p.N * p.sg.Hp * p.sg.Wp * 4 * es);
  p.off_wf = carve(cur, (size_t)wf * es);
  p.off_wd = carve(cur, (size_t)wd * es);
  const size_t rows0 = p.sg.rows();
  p.x0_off = carve(cur, rows0 * 64 * es);
  p.coef0_off = carve(cur, 4 * 64 * sizeof(float));
  p.off_pool = carve(cur, p.sg.pooled() * 64 * es);
  p.off_idx = carve(cur, p.sg.pooled() * 64);

  size_t stat_floats = (size_t)stem_conv_stat_rows(p.N, p.sg.OH, p.sg.OW) * 64;
  size_t partial_bytes = (size_t)bn_bwd_partial_rows(rows0, 64) * 2 * 64 * sizeof(float);
  size_t slab = stem_wgrad_slab_bytes(p.N, p.sg.OH, p.sg.OW);
  size_t small_elems = 0, big_elems = rows0 * 64;
  int maxC = BOTTLE;
  auto need_stat = [&](size_t floats) { if (floats > stat_floats) stat_floats = floats; };
  auto need_partial = [&](size_t rows, int C) {
    size_t a = dense_partial_bytes(rows, C);
    if (a > partial_bytes) partial_bytes = a;
    if (C > maxC) maxC = C;
  };
  auto need_slab = [&](const ConvShape& s) { size_t v = conv_wgrad_slab_bytes(s); if (v > slab) slab = v; };
  for (int bi = 0; bi < 4; ++bi) {
    DBlock& b = p.blocks[bi];
    b.cat_off = carve(cur, b.rows * b.Ctot * es);
    b.dcat_off = carve(cur, b.rows * b.Ctot * es);
    b.tab_off = carve(cur, 2 * (size_t)b.Ctot * sizeof(float));
    need_stat((size_t)column_stats_rows(b.rows, b.C0) * 2 * b.C0);
    if (b.rows * BOTTLE > small_elems) small_elems = b.rows * BOTTLE;
    for (DLayer& l : b.layers) {
      l.t_off = carve(cur, b.rows * l.Cp * es);
      l.a_off = carve(cur, b.rows * BOTTLE * es);
      l.u_off = carve(cur, b.rows * BOTTLE * es);
      l.coef1_off = carve(cur, 5 * (size_t)l.Cp * sizeof(float));
      l.coef2_off = carve(cur, 4 * (size_t)BOTTLE * sizeof(float));
      dense_fold_norm2(l, p.table_host);
      dense_layer_needs(p.N, b.H, b.W, b.rows, l, stat_floats, partial_bytes, slab);
      if (l.Cp > maxC) maxC = l.Cp;
      if (b.rows * l.Cp > big_elems) big_elems = b.rows * l.Cp;
    }
    if (b.rows * b.Ctot > big_elems) big_elems = b.rows * b.Ctot;
    if (bi < 3) {
      DTrans& t = p.trans[bi];
      t.tt_off = carve(cur, b.rows * t.C * es);
      t.coef_off = carve(cur, 5 * (size_t)t.C * sizeof(float));
      ConvShape ct = {p.N, b.H, b.W, t.C, t.C / 2, 1, 1, 1, 0};
      need_partial(b.rows, t.C);
      need_slab(ct);
    }
  }
  DBlock& lb = p.blocks[3];
  p.coef5_off = carve(cur, 5 * (size_t)lb.Ctot * sizeof(float));
  p.y5_off = carve(cur, lb.rows * lb.Ctot * es);
  need_partial(lb.rows, lb.Ctot);
  if (rows0 * 64 > big_elems) big_elems = rows0 * 64;   // stem backward: full-resolution dy / dx
  p.stat_bytes = align_up(stat_floats * sizeof(float), 256);
  p.off_stat = carve(cur, 2 * p.stat_bytes);
  p.off_partial = carve(cur, partial_bytes);
  p.off_coefbwd = carve(cur, 3 * (size_t)maxC * sizeof(float));
  p.off_defer = carve(cur, 2 * (size_t)maxC * sizeof(float));   // per block: running sums of the consumers' cB / cC (backward)
  p.off_dwv = carve(cur, 64 * 256 * sizeof(float));
  p.red_C = maxC;
  p.off_red = carve(cur, bn_reduce_scratch_bytes(p.red_C));
  p.slab_bytes = slab;
  p.off_slab = carve(cur, slab);
  p.off_sB = carve(cur, p.blocks[0].rows * G_PAD * es);
  p.off_sB2 = carve(cur, p.blocks[0].rows * G_PAD * es);
  p.off_sU = carve(cur, small_elems * es);
  p.off_sA = carve(cur, small_elems * es);
  p.off_sA2 = carve(cur, small_elems * es);
  p.off_sX = carve(cur, big_elems * es);
  p.off_sZ = carve(cur, big_elems * es);
  p.off_sC = carve(cur, big_elems * es);
  p.ws_bytes = cur;
  return MMSKIN_OK;
}

template <typename T>
StemBufs<T> stem_bufs(const DensePlan& p, unsigned char* ws) {
  StemBufs<T> b;
  b.img4 = reinterpret_cast<T*>(ws + p.off_img4);
  b.wv = reinterpret_cast<const T*>(ws + p.off_wf) + p.wf0;
  b.x0 = reinterpret_cast<T*>(ws + p.x0_off);
  b.pool = reinterpret_cast<T*>(ws + p.off_pool);
  b.idx = ws + p.off_idx;
  b.coef = reinterpret_cast<float*>(ws + p.coef0_off);
  b.ssum = reinterpret_cast<float*>(ws + p.off_stat);
  b.ssq = reinterpret_cast<float*>(ws + p.off_stat + p.stat_bytes);
  b.red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  b.coefbwd = reinterpret_cast<float*>(ws + p.off_coefbwd);
  b.partial = reinterpret_cast<float*>(ws + p.off_partial);
  b.dx0 = reinterpret_cast<T*>(ws + p.off_sX);
  b.slab = wgrad_slab_at(ws, p.off_slab, p.slab_bytes);
  b.dwv = reinterpret_cast<float*>(ws + p.off_dwv);
  return b;
}

template <typename T>
DenseRun<T> dense_run(DensePlan& p, const float* params, float* buffers, float* grads, unsigned char* ws) {
  DenseRun<T> r;
  r.N = p.N; r.prof = &p.prof; r.ws = ws; r.params = params; r.buffers = buffers; r.grads = grads;
  r.wf = reinterpret_cast<T*>(ws + p.off_wf);
  r.wd = reinterpret_cast<T*>(ws + p.off_wd);
  r.stat_sum = reinterpret_cast<float*>(ws + p.off_stat);
  r.stat_sq = reinterpret_cast<float*>(ws + p.off_stat + p.stat_bytes);
  r.red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  r.sBq[0] = reinterpret_cast<T*>(ws + p.off_sB); r.sBq[1] = reinterpret_cast<T*>(ws + p.off_sB2);
  r.sAq[0] = reinterpret_cast<T*>(ws + p.off_sA); r.sAq[1] = reinterpret_cast<T*>(ws + p.off_sA2);
  r.sU = reinterpret_cast<T*>(ws + p.off_sU);
  r.sZ = reinterpret_cast<T*>(ws + p.off_sZ);
  r.sC = reinterpret_cast<T*>(ws + p.off_sC);
  r.slab = wgrad_slab_at(ws, p.off_slab, p.slab_bytes);
  r.partial = reinterpret_cast<float*>(ws + p.off_partial);
  r.cA = reinterpret_cast<float*>(ws + p.off_coefbwd);
  r.defer = reinterpret_cast<float*>(ws + p.off_defer);
  return r;
}

}  // namespace

template <typename T>
int dense_table_from_slice(DenseRun<T>& r, const DBlock& b, int c0, int C, hipStream_t st) {
  float* tab = reinterpret_cast<float*>(r.ws + b.tab_off);
  int nr = 0, rc;
  ProfScope scope(r.prof, K_BN_FWD, st, 0.0, (double)b.rows * C * sizeof(T));
  if ((rc = slice_stats<T>(reinterpret_cast<const T*>(r.ws + b.cat_off) + c0, b.Ctot, C, b.rows, r.stat_sum, r.stat_sum + C, &nr, st))) return rc;
  return bn_table_finalize(r.stat_sum, r.stat_sum + C, nr, 2 * C, C, (double)b.rows, tab + c0, tab + b.Ctot + c0, r.red, st);
}

template <typename T>
int dense_block_forward(DenseRun<T>& r, DBlock& b, bool training, hipStream_t st) {
  const float eps = 1e-5f, mom = 0.1f;
  unsigned char* ws = r.ws;
  const float* params = r.params;
  float* buffers = r.buffers;
  T* wf = r.wf;
  float *stat_sum = r.stat_sum, *stat_sq = r.stat_sq;
  const ColScratch red = r.red;
  T* sB = r.sBq[0];
  int rc;
  T* cat = reinterpret_cast<T*>(ws + b.cat_off);
  float* tab = reinterpret_cast<float*>(ws + b.tab_off);
  const double count = (double)b.rows;
  for (DLayer& l : b.layers) {
    const BnCoef k1(reinterpret_cast<float*>(ws + l.coef1_off), l.Cp), k2(reinterpret_cast<float*>(ws + l.coef2_off), BOTTLE);
    T* t = reinterpret_cast<T*>(ws + l.t_off);
    T* a = reinterpret_cast<T*>(ws + l.a_off);
    T* u = reinterpret_cast<T*>(ws + l.u_off);
    // norm1 + relu over the channel prefix -> compact padded operand
    PROF_AT(r.prof, K_BN_FWD, 0.0, 0.0, bn_coef_from_table(tab, tab + b.Ctot, l.Cin, l.Cp, params + l.n1.g_off, params + l.n1.b_off, eps, mom,
                       count, buffers + l.n1.rm_off, buffers + l.n1.rv_off, training, k1.scale, st));
    PROF_AT(r.prof, K_BN_FWD, 0.0, (double)b.rows * (l.Cin + l.Cp) * sizeof(T),
         slice_pack<T>(cat, b.Ctot, l.Cin, l.Cp, b.rows, k1.scale, k1.shift, t, st));
    // conv1 1x1 -> norm2 -> relu
    ConvShape c1 = {r.N, b.H, b.W, l.Cp, BOTTLE, 1, 1, 1, 0};
    if (!training) {   // norm2 folded: u = relu(conv1'(t) + shift2) straight from the conv epilogue
      FwdFuse f; f.bias = k2.shift; f.relu = true;
      PROF_AT(r.prof, K_CONV_FWD, conv_flops(c1), conv_bytes(c1, sizeof(T)), launch_conv_fwd<T>(c1, t, wf + l.wf1, u, nullptr, nullptr, st, &f));
    } else {
    PROF_AT(r.prof, K_CONV_FWD, conv_flops(c1), conv_bytes(c1, sizeof(T)),
         launch_conv_fwd<T>(c1, t, wf + l.wf1, a, training ? stat_sum : nullptr, training ? stat_sq : nullptr, st));
    }
    if (training) {
      PROF_AT(r.prof, K_BN_FWD, 0.0, 0.0, bn_finalize(stat_sum, stat_sq, conv_fwd_stat_rows(c1), BOTTLE, count, params + l.n2.g_off, params + l.n2.b_off, eps, mom,
                       buffers + l.n2.rm_off, buffers + l.n2.rv_off, k2.scale, k2.shift, k2.mean, k2.invstd, red, st));
      PROF_AT(r.prof, K_BN_FWD, 0.0, 2.0 * b.rows * BOTTLE * sizeof(T),
           bn_apply<T>(a, nullptr, k2.scale, k2.shift, nullptr, nullptr, u, b.rows, BOTTLE, true, st));
    }
    // conv2 3x3 (32 outputs padded to 64) -> new cat channels + their batch statistics
    ConvShape c2 = {r.N, b.H, b.W, BOTTLE, G_PAD, 3, 3, 1, 1};
    PROF_AT(r.prof, K_CONV_FWD, conv_flops(c2) / 2, conv_bytes(c2, sizeof(T)),
         launch_conv_fwd<T>(c2, u, wf + l.wf2, sB, training ? stat_sum : nullptr, training ? stat_sq : nullptr, st));
    PROF_AT(r.prof, K_BN_FWD, 0.0, 2.0 * b.rows * GROWTH * sizeof(T), slice_scatter<T>(sB, G_PAD, GROWTH, cat + l.Cin, b.Ctot, b.rows, st));
    if (training)
      PROF_AT(r.prof, K_BN_FWD, 0.0, 0.0, bn_table_finalize(stat_sum, stat_sq, conv_fwd_stat_rows(c2), G_PAD, GROWTH, count, tab + l.Cin, tab + b.Ctot + l.Cin, red, st));
  }
  return MMSKIN_OK;
}

template <typename T>
int dense_transition_forward(DenseRun<T>& r, DBlock& b, DTrans& t, T* dst, int dst_pitch, bool training, hipStream_t st) {
  const float eps = 1e-5f, mom = 0.1f;
  unsigned char* ws = r.ws;
  const T* cat = reinterpret_cast<const T*>(ws + b.cat_off);
  float* tab = reinterpret_cast<float*>(ws + b.tab_off);
  const double count = (double)b.rows;
  int rc;
  const BnCoef k(reinterpret_cast<float*>(ws + t.coef_off), t.C);
  T* tt = reinterpret_cast<T*>(ws + t.tt_off);
  PROF_AT(r.prof, K_BN_FWD, 0.0, 0.0, bn_coef_from_table(tab, tab + b.Ctot, t.C, t.C, r.params + t.n.g_off, r.params + t.n.b_off, eps, mom, count,
                     r.buffers + t.n.rm_off, r.buffers + t.n.rv_off, training, k.scale, st));
  PROF_AT(r.prof, K_BN_FWD, 0.0, 2.0 * b.rows * t.C * sizeof(T), bn_apply<T>(cat, nullptr, k.scale, k.shift, nullptr, nullptr, tt, b.rows, t.C, true, st));
  ConvShape ct = {r.N, b.H, b.W, t.C, t.C / 2, 1, 1, 1, 0};
  PROF_AT(r.prof, K_CONV_FWD, conv_flops(ct), conv_bytes(ct, sizeof(T)), launch_conv_fwd<T>(ct, tt, r.wf + t.wf, r.sC, nullptr, nullptr, st));
  PROF_AT(r.prof, K_STEM_MISC, 0.0, 0.0, avgpool2_fwd<T>(r.sC, r.N, b.H, b.W, t.C / 2, dst, dst_pitch, st));
  return MMSKIN_OK;
}

// Weight-gradient GEMMs only feed the optimizer: they run on the side stream beside the dgrad -> BN-backward
// chain (one slab, the side stream is in order).  Operand buffers alternate between consecutive layers; the main
// stream re-acquires a buffer (waits for the wgrad that read it) before overwriting it.
template <typename T>
static int dense_acquire(DenseRun<T>& r, int slot, hipStream_t st) { return r.side ? r.side->acquire(slot, st, r.use_side) : MMSKIN_OK; }
template <typename T>
static int dense_wgrad_async(DenseRun<T>& r, int slot, const ConvShape& cs, double flops, const T* dout, const T* in, float* dw, int cov, int civ,
                             hipStream_t st) {
  auto launch = [&](hipStream_t wst) {
    ProfScope scope(r.prof, K_WGRAD, wst, flops, conv_bytes(cs, sizeof(T)));
    return launch_conv_wgrad<T>(cs, dout, in, r.slab, dw, wst, cov, civ);
  };
  return r.side ? r.side->run(slot, st, r.use_side, launch) : launch(st);
}

// Every later layer of a block adds cA*g + cB*x + cC to the channel prefix it consumed, and x (the concatenated activation) is the
// same tensor for all of them: the x / constant terms are summed as COEFFICIENTS (sB, sC: bn_bwd_finalize adds into them) and
// applied once, when a channel's gradient is consumed (its own layer's slice, or the block input at the block's end) -- the
// per-layer pass then reads g and read-modify-writes dcat only (3 passes over the prefix instead of 4).
template <typename T>
int dense_block_backward(DenseRun<T>& r, DBlock& b, hipStream_t st) {
  unsigned char* ws = r.ws;
  const float* params = r.params;
  float* grads = r.grads;
  T* wd = r.wd;
  float *partial = r.partial, *cA = r.cA;
  const ColScratch red = r.red;
  T *sU = r.sU, *sZ = r.sZ;
  int rc;
  float* sB_ = r.defer;
  const T* cat = reinterpret_cast<const T*>(ws + b.cat_off);
  T* dcat = reinterpret_cast<T*>(ws + b.dcat_off);
  const double count = (double)b.rows;
  float* sC_ = sB_ + b.Ctot;
  HIP_CHECK_RET(hipMemsetAsync(sB_, 0, 2 * (size_t)b.Ctot * sizeof(float), st));
  for (int li = (int)b.layers.size() - 1; li >= 0; --li) {
    DLayer& l = b.layers[li];
    const BnCoef k1(reinterpret_cast<float*>(ws + l.coef1_off), l.Cp), k2(reinterpret_cast<float*>(ws + l.coef2_off), BOTTLE);
    const T* t = reinterpret_cast<const T*>(ws + l.t_off);
    const T* a = reinterpret_cast<const T*>(ws + l.a_off);
    const T* u = reinterpret_cast<const T*>(ws + l.u_off);
    ConvShape c1 = {r.N, b.H, b.W, l.Cp, BOTTLE, 1, 1, 1, 0}, c2 = {r.N, b.H, b.W, BOTTLE, G_PAD, 3, 3, 1, 1};
    const int q = r.layer_no++ & 1;
    T* sB = r.sBq[q];
    T* sA = r.sAq[q];
    // gradient of this layer's 32 output channels, padded to the GEMM's 64
    if ((rc = dense_acquire(r, q, st))) return rc;
    PROF_AT(r.prof, K_BN_BWD, 0.0, 3.0 * b.rows * GROWTH * sizeof(T),
         slice_pack_deferred<T>(dcat + l.Cin, cat + l.Cin, b.Ctot, GROWTH, G_PAD, b.rows, sB_ + l.Cin, sC_ + l.Cin, sB, st));
    // conv2: weight gradient (first 32 rows are real) and data gradient with norm2's mask + sums fused
    if ((rc = dense_wgrad_async<T>(r, q, c2, conv_flops(c2) / 2, sB, u, grads + l.w2_off, GROWTH, 0, st))) return rc;
    DgradFuse f2;
    f2.x = a; f2.scale = k2.scale; f2.shift = k2.shift; f2.partial = partial;
    PROF_AT(r.prof, K_CONV_DGRAD, conv_flops(c2) / 2, conv_bytes(c2, sizeof(T), 1), launch_conv_dgrad<T>(c2, sB, wd + l.wd2, sU, (const T*)nullptr, st, &f2));
    if ((rc = dense_acquire(r, 2 + q, st))) return rc;
    if ((rc = bn_backward_from_sums<T>(sU, a, partial, f2.rows_written, b.rows, BOTTLE, k2, params + l.n2.g_off, grads + l.n2.g_off,
                                       grads + l.n2.b_off, BnBwdCoef(cA, BOTTLE), red, sA, r.prof, 3.0 * b.rows * BOTTLE * sizeof(T), st)))
      return rc;
    // conv1: weight gradient, padded input channels dropped by the reduction
    if ((rc = dense_wgrad_async<T>(r, 2 + q, c1, conv_flops(c1), sA, t, grads + l.w1_off, 0, l.Cin, st))) return rc;
    // conv1 data gradient with norm1's mask + sums fused: the epilogue reads the raw channel prefix straight from
    // cat (row pitch Ctot); padded channels [Cin, Cp) have scale = shift = 0, so their mask is false
    DgradFuse f1;
    f1.x = cat; f1.x_pitch = b.Ctot; f1.scale = k1.scale; f1.shift = k1.shift; f1.partial = partial;
    PROF_AT(r.prof, K_CONV_DGRAD, conv_flops(c1), conv_bytes(c1, sizeof(T), 1), launch_conv_dgrad<T>(c1, sA, wd + l.wd1, sZ, (const T*)nullptr, st, &f1));
    {
      // norm1: cB / cC are added to the block's running sums (padded channels [Cin, Cp) have gamma = 0: they add zeros), and the
      // apply pass is the scaled accumulation into dcat -- a finalize of its own, not bn_backward_from_sums
      ProfScope scope(r.prof, K_BN_BWD, st, 0.0, 3.0 * b.rows * l.Cin * sizeof(T));
      if ((rc = bn_bwd_finalize(partial, f1.rows_written, l.Cp, count, k1.gamma, k1.mean, k1.invstd, grads + l.n1.g_off, grads + l.n1.b_off,
                                cA, sB_, sC_, red, st, l.Cin, true))) return rc;
      if ((rc = slice_accumulate_scaled<T>(dcat, b.Ctot, l.Cin, sZ, l.Cp, cA, b.rows, st))) return rc;
    }
  }
  // the block-input channels [0, C0): every layer of the block consumed them
  PROF_AT(r.prof, K_BN_BWD, 0.0, 3.0 * b.rows * b.C0 * sizeof(T), slice_affine_inplace<T>(dcat, cat, b.Ctot, b.C0, b.rows, sB_, sC_, st));
  return MMSKIN_OK;
}

// avgpool <- conv 1x1 <- relu <- norm; writes the whole of the previous block's dcat
template <typename T>
int dense_transition_backward(DenseRun<T>& r, DBlock& pb, DTrans& tr, const T* dcat_next, int pitch_next, hipStream_t st) {
  unsigned char* ws = r.ws;
  T *sZ = r.sZ, *sC = r.sC;
  int rc;
  const BnCoef k(reinterpret_cast<float*>(ws + tr.coef_off), tr.C);
  const T* tt = reinterpret_cast<const T*>(ws + tr.tt_off);
  const T* pcat = reinterpret_cast<const T*>(ws + pb.cat_off);
  ConvShape ct = {r.N, pb.H, pb.W, tr.C, tr.C / 2, 1, 1, 1, 0};
  if ((rc = dense_acquire(r, 4, st))) return rc;
  PROF_AT(r.prof, K_STEM_MISC, 0.0, 0.0, avgpool2_bwd<T>(dcat_next, pitch_next, r.N, pb.H, pb.W, tr.C / 2, sC, st));
  if ((rc = dense_wgrad_async<T>(r, 4, ct, conv_flops(ct), sC, tt, r.grads + tr.w_off, 0, 0, st))) return rc;
  DgradFuse f;
  f.x = pcat; f.scale = k.scale; f.shift = k.shift; f.partial = r.partial;
  PROF_AT(r.prof, K_CONV_DGRAD, conv_flops(ct), conv_bytes(ct, sizeof(T), 1), launch_conv_dgrad<T>(ct, sC, r.wd + tr.wd, sZ, (const T*)nullptr, st, &f));
  return bn_backward_from_sums<T>(sZ, pcat, r.partial, f.rows_written, pb.rows, tr.C, k, r.params + tr.n.g_off, r.grads + tr.n.g_off,
                                  r.grads + tr.n.b_off, BnBwdCoef(r.cA, tr.C), r.red, reinterpret_cast<T*>(ws + pb.dcat_off), r.prof,
                                  3.0 * pb.rows * tr.C * sizeof(T), st);
}

#define INST_DENSE(T)                                                                                     \
  template int dense_table_from_slice<T>(DenseRun<T>&, const DBlock&, int, int, hipStream_t);             \
  template int dense_block_forward<T>(DenseRun<T>&, DBlock&, bool, hipStream_t);                          \
  template int dense_transition_forward<T>(DenseRun<T>&, DBlock&, DTrans&, T*, int, bool, hipStream_t);   \
  template int dense_block_backward<T>(DenseRun<T>&, DBlock&, hipStream_t);                               \
  template int dense_transition_backward<T>(DenseRun<T>&, DBlock&, DTrans&, const T*, int, hipStream_t);
INST_DENSE(float)
INST_DENSE(bf16_t)
#undef INST_DENSE

namespace {

template <typename T>
int dense_forward(DensePlan& p, const void* image, const float* norm6, const float* params, float* buffers,
                  unsigned char* ws, float* features, bool training, hipStream_t st) {
  const float eps = 1e-5f, mom = 0.1f;
  DenseRun<T> r = dense_run<T>(p, params, buffers, nullptr, ws);
  int rc;
  if ((rc = p.ensure_table())) return rc;
  HIP_CHECK_RET(hipMemsetAsync(r.wf + p.wf0, 0, 64 * 256 * sizeof(T), st));
  PROF(K_STAGE, 0.0, 0.0, stage_weights<T>(p.table_dev, (int)p.table_host.size(), p.max_stage_elems, params, r.wf, r.wd, training, st,
                                           training ? nullptr : buffers, eps));
  if (!training) PROF(K_BN_FWD, 0.0, 0.0, bn_eval_table(p.table_dev, (int)p.table_host.size(), BOTTLE, params, buffers, ws, eps, st));

  // ---- stem: conv0 (7x7 s2) -> norm0 -> relu -> maxpool 3x3 s2
  StemBn bn0;
  bn0.gamma = params + p.n0.g_off; bn0.beta = params + p.n0.b_off; bn0.rm = buffers + p.n0.rm_off; bn0.rv = buffers + p.n0.rv_off;
  bn0.eps = eps; bn0.mom = mom; bn0.batch_stats = training;
  if ((rc = stem_forward<T>(stem_bufs<T>(p, ws), p.sg, image, norm6, bn0, &p.prof, st))) return rc;
  const T* pool = reinterpret_cast<const T*>(ws + p.off_pool);
  {
    DBlock& b = p.blocks[0];
    PROF(K_STEM_MISC, 0.0, 0.0, slice_scatter<T>(pool, 64, 64, reinterpret_cast<T*>(ws + b.cat_off), b.Ctot, b.rows, st));
    if (training && (rc = dense_table_from_slice<T>(r, b, 0, 64, st))) return rc;
  }

  for (int bi = 0; bi < 4; ++bi) {
    DBlock& b = p.blocks[bi];
    if ((rc = dense_block_forward<T>(r, b, training, st))) return rc;
    if (bi < 3) {
      // transition into the next block's cat prefix
      DTrans& t = p.trans[bi];
      DBlock& nb = p.blocks[bi + 1];
      if ((rc = dense_transition_forward<T>(r, b, t, reinterpret_cast<T*>(ws + nb.cat_off), nb.Ctot, training, st))) return rc;
      if (training && (rc = dense_table_from_slice<T>(r, nb, 0, t.C / 2, st))) return rc;
    }
  }
  // ---- norm5 -> relu -> global average pool
  DBlock& lb = p.blocks[3];
  const int C5 = lb.Ctot;
  const BnCoef k5(reinterpret_cast<float*>(ws + p.coef5_off), C5);
  float* tab = reinterpret_cast<float*>(ws + lb.tab_off);
  T* y5 = reinterpret_cast<T*>(ws + p.y5_off);
  PROF(K_BN_FWD, 0.0, 0.0, bn_coef_from_table(tab, tab + C5, C5, C5, params + p.n5.g_off, params + p.n5.b_off, eps, mom, (double)lb.rows,
                     buffers + p.n5.rm_off, buffers + p.n5.rv_off, training, k5.scale, st));
  PROF(K_BN_FWD, 0.0, 2.0 * lb.rows * C5 * sizeof(T),
       bn_apply<T>(reinterpret_cast<const T*>(ws + lb.cat_off), nullptr, k5.scale, k5.shift, nullptr, nullptr, y5, lb.rows, C5, !p.fmap, st));
  if (p.fmap) return nhwc_to_nchw<T>(y5, p.N, C5, lb.H, lb.W, features, st);
  return avgpool_fwd<T>(y5, p.N, lb.H * lb.W, C5, features, st);
}

template <typename T>
int dense_backward(DensePlan& p, const float* dfeat, const float* params, unsigned char* ws, float* grads,
                   hipStream_t st) {
  DenseRun<T> r = dense_run<T>(p, params, nullptr, grads, ws);
  int rc;

  // the weight-gradient GEMMs run on the side stream unless the profiler is on
  const bool use_side = !p.prof.on;
  if (use_side && (rc = p.side.init(DensePlan::SIDE_SLOTS))) return rc;
  p.side.begin_backward();
  r.side = &p.side; r.use_side = use_side;

  // ---- global average pool <- relu <- norm5: writes the whole of dcat4
  {
    DBlock& lb = p.blocks[3];
    const int C5 = lb.Ctot;
    const T* x = reinterpret_cast<const T*>(ws + lb.cat_off);
    const T* y5 = reinterpret_cast<const T*>(ws + p.y5_off);
    if (p.fmap) rc = nchw_to_nhwc<T>(dfeat, p.N, C5, lb.H, lb.W, r.sZ, st);
    else rc = avgpool_bwd<T>(dfeat, p.N, lb.H * lb.W, C5, r.sZ, st);
    if (rc) return rc;
    // (profiler: norm5's bytes are not counted -- an omission, kept)
    if ((rc = bn_backward<T>(r.sZ, x, y5, p.fmap ? MASK_NONE : MASK_FROM_Y, lb.rows, C5, BnCoef(reinterpret_cast<float*>(ws + p.coef5_off), C5),
                             params + p.n5.g_off, grads + p.n5.g_off, grads + p.n5.b_off, BnBwdCoef(r.cA, C5), r.partial, r.red,
                             reinterpret_cast<T*>(ws + lb.dcat_off), nullptr, &p.prof, 0.0, st))) return rc;
  }

  for (int bi = 3; bi >= 0; --bi) {
    DBlock& b = p.blocks[bi];
    if ((rc = dense_block_backward<T>(r, b, st))) return rc;
    if (bi > 0 && (rc = dense_transition_backward<T>(r, p.blocks[bi - 1], p.trans[bi - 1], reinterpret_cast<const T*>(ws + b.dcat_off), b.Ctot, st)))
      return rc;
  }

  // join: the stem reuses the slab and scratch buffers the side stream has been working on
  for (int i = 0; i < DensePlan::SIDE_SLOTS; ++i)
    if ((rc = p.side.acquire(i, st, use_side))) return rc;

  // ---- stem: maxpool <- relu <- norm0 <- conv0
  {
    T* sB = r.sBq[0];
    DBlock& b = p.blocks[0];
    const StemBufs<T> sb = stem_bufs<T>(p, ws);   // dx0 = sX
    PROF(K_STEM_MISC, 0.0, 0.0, slice_pack<T>(reinterpret_cast<const T*>(ws + b.dcat_off), b.Ctot, 64, 64, b.rows, nullptr, nullptr, sB, st));
    // sums_pooled = false: the routed form whatever stem_sums_pooled() says -- inherited behaviour, not a decision.
    // (profiler: the stem's BatchNorm-backward bytes are not counted -- an omission, kept)
    if ((rc = stem_backward<T>(sb, p.sg, sB, params + p.n0.g_off, grads + p.n0.g_off, grads + p.n0.b_off, false, &p.prof, 0.0, st))) return rc;
    return stem_wgrad<T>(sb, p.sg, grads + p.w0_off, &p.prof, st);
  }
}

int DensePlan::forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                       float* features, bool training, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return dense_forward<decltype(t)>(*this, image, norm6, params, buffers, ws, features, training, st); });
}
int DensePlan::backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return dense_backward<decltype(t)>(*this, dfeat, params, ws, grads, st); });
}

}  // namespace

PlanBase* make_densenet_plan(int N, int H, int W, int dtype, bool feature_map, int* rc) {
  return make_plan<DensePlan>(N, H, W, dtype, rc, [feature_map](DensePlan& p) { p.fmap = feature_map; return build_dense_plan(p); });
}
