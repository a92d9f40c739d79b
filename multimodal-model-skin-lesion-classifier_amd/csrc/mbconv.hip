// Inverted-residual (MBConv) image-encoder plan executor for MobileNet-V2 and EfficientNet-B0 / B7 (torchvision
// layouts: 3x3/2 stem, inverted-residual stages, 1x1 head, global average pool; `classifier = Identity`).  Replaces
// `self.image_encoder(image)` for cnn_model_name == "mobilenet-v2" / "efficientnet-b0" / "efficientnet-b7"
// (loadImageModelClassifier.py:96-112).
//
// The 1x1 convolutions (97 % of MobileNet-V2's MACs) run on the implicit-GEMM kernels; every activation is kept NHWC
// with its channel count padded to a multiple of 64 (zero weights / zero BatchNorm gain on the padding, so padded
// channels stay exactly zero) and the weight-gradient reductions drop the padding.  The 3x3 / 5x5 depthwise
// convolutions are HBM-bound elementwise-style kernels (ops.hip: dwconv3_*).  BatchNorm uses the shared
// statistics-table kernels (batch statistics from the conv epilogue / one column pass).
//
// The two networks differ in data only, which their builders set: the activation after the BatchNorm (ReLU6 or SiLU:
// the clamp / SiLU variants of the BatchNorm apply and backward kernels), the depthwise kernel sizes, the BatchNorm
// eps / momentum, squeeze-excitation behind every depthwise unit (EfficientNet: global average pool -> two small fp32
// Linear layers on the head GEMM -> per-(sample, channel) gate) and row-mode stochastic depth on the residual
// branches (EfficientNet: the per-sample keep/scale mask is handed in by the host each training step).
#include <math.h>

#include "plan.h"
#include "../../include/mmskin.h"

namespace {

enum UKind { U_FIRST = 0, U_PW = 1, U_DW = 2 };
enum Act { ACT_RELU6, ACT_SILU };

struct SEBlock {   // squeeze-excitation behind a depthwise unit
  int C, Cp, Csq;
  int64_t w1_off, b1_off, w2_off, b2_off;            // flat params: fc1 [Csq][C], fc2 [C][Csq]
  size_t w1p_off, w2p_off, b2p_off;                  // padded fp32 copies (bytes in ws): [Csq][Cp], [Cp][Csq], [Cp]
  size_t s_off, z1_off, a1_off, z2_off, g_off;       // fp32 activations [N][Cp] / [N][Csq]
  size_t yse_off;                                     // gated activation (T) -- the project conv's input
};

struct MBUnit {
  int kind, ksize;
  int Cin, Cout, Cinp, Coutp;   // real / padded channels
  int H, W, stride, OH, OW;     // input and output spatial size
  bool act;                     // the plan's activation after the BatchNorm
  bool res_last;                // last unit of a block with a residual connection: y = bn(x) + block input
  bool res_first;               // first unit of such a block: its data gradient adds the residual branch's gradient
  int se;                       // index into ses (depthwise units) or -1
  int sd;                       // row of the stochastic-depth mask (res_last units) or -1
  int64_t w_off;
  BNRef bn;
  int64_t wf, wd;               // staged weights (element offsets; depthwise: [k*k][Cp] inside the forward buffer)
  size_t x_off, y_off, coef_off;
  size_t in_off;                // input activation (bytes); block input for res_last's residual = res_off
  size_t res_off;
};

inline int make_divisible(double v, int divisor = 8) {
  int nv = (int)(v + divisor / 2.0) / divisor * divisor;
  if (nv < divisor) nv = divisor;
  if (nv < 0.9 * v) nv += divisor;
  return nv;
}

struct MBPlan : PlanBase {
  Act act = ACT_RELU6;
  float eps = 1e-5f, mom = 0.1f;
  std::vector<MBUnit> units;
  std::vector<SEBlock> ses;
  int n_sd = 0;                     // residual blocks with stochastic depth; 0: the plan takes no "sd_mask"
  const float* sd_mask = nullptr;   // [n_sd][N] keep/scale factors for this training step (null: no stochastic depth)
  int stemC;
  FirstGeom fg;                     // the stride-2 first conv (3 -> stemC <= 64) and its padded NHWC8 image
  FirstCarve first;
  size_t off_wf, off_wd, off_stat, off_tab, off_partial, off_coefbwd, off_red, off_slab, slab_bytes, off_dwpart, off_setmp = 0, off_g[4];
  int red_C = 0;   // channels the reduction scratch was carved for (bn_reduce_scratch)
  size_t stat_bytes = 0;

  // the activation's bn_apply cap and BatchNorm-backward mask mode
  float act_cap() const { return act == ACT_RELU6 ? 6.f : -1.f; }
  int act_mask() const { return act == ACT_RELU6 ? MASK_FROM_Y6 : MASK_SILU_X; }

  int set_pointer(const char* key, const void* ptr) override {
    if (!n_sd) return PlanBase::set_pointer(key, ptr);
    if (!strcmp(key, "sd_mask")) { sd_mask = reinterpret_cast<const float*>(ptr); return MMSKIN_OK; }
    return MMSKIN_ERR_ARG;
  }
  int forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
              float* features, bool training, hipStream_t st) override;
  int backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) override;
  int num_units() const override { return (int)units.size(); }
  int unit_info(int index, std::string* name, int64_t* info12) const override;
};

// The twelve fields of the ResNet plan's unit_info; channel counts are the real (unpadded) ones, the two plan-wide offsets are
// this plan's analogues: the unit's input activation and the first gradient buffer.
int MBPlan::unit_info(int index, std::string* name, int64_t* info12) const {
  const MBUnit& u = units[index];
  for (const TensorInfo& t : params)
    if (t.offset == u.w_off && name) *name = t.name;
  const int64_t v[12] = {(int64_t)u.x_off, (int64_t)u.y_off, (int64_t)u.coef_off, (int64_t)N * u.OH * u.OW, u.Cout,
                         u.OH, u.OW, u.Cin, u.H, u.W, (int64_t)u.in_off, (int64_t)off_g[0]};
  for (int i = 0; i < 12; ++i) info12[i] = v[i];
  return MMSKIN_OK;
}

// Registers one conv + BatchNorm unit (torchvision named_parameters() order); returns its index.
int add_unit(MBPlan& p, int kind, const std::string& conv_name, const std::string& bn_name, int cin, int cout, int h,
             int w, int stride, int ksize, bool act) {
  MBUnit u = {};
  u.kind = kind; u.ksize = ksize; u.Cin = cin; u.Cout = cout; u.Cinp = kind == U_FIRST ? 3 : pad64(cin); u.Coutp = pad64(cout);
  u.H = h; u.W = w; u.stride = stride; u.se = -1; u.sd = -1;
  const int pad = ksize / 2;
  u.OH = kind == U_PW ? h : (h + 2 * pad - ksize) / stride + 1;
  u.OW = kind == U_PW ? w : (w + 2 * pad - ksize) / stride + 1;
  u.act = act;
  if (kind == U_DW) u.w_off = add_tensor(p.params, p.param_numel, conv_name + ".weight", {cout, 1, ksize, ksize});
  else u.w_off = add_tensor(p.params, p.param_numel, conv_name + ".weight", {cout, cin, kind == U_FIRST ? 3 : 1, kind == U_FIRST ? 3 : 1});
  u.bn = add_bn(p, bn_name, cout);
  p.units.push_back(u);
  return (int)p.units.size() - 1;
}

// Staged-weight table and workspace carve-up, once the builder has registered every unit.
int finish_plan(MBPlan& p, const char* arch) {
  p.fg = FirstGeom(p.N, p.H, p.W, p.units[0].stride);
  if (int rc = p.fg.check(arch)) return rc;

  // ---- staged weights
  int64_t wf = FirstGeom::WV_ELEMS, wd = 0;   // slot 0: first conv's virtual operand
  for (size_t i = 1; i < p.units.size(); ++i) {
    MBUnit& u = p.units[i];
    if (u.kind == U_DW) { u.wf = wf; wf += (int64_t)u.ksize * u.ksize * u.Coutp; continue; }
    stage_append(p.table_host, u.w_off, u.Cout, u.Cin, 1, u.Coutp, u.Cinp, wf, wd, p.max_stage_elems, u.wf, u.wd);
  }

  // ---- workspace
  const size_t es = p.esz();
  size_t cur = 0, maxact = 0, stat_floats = 0, partial = 0, dwpart = 0, setmp = 0, slab = p.first.image(cur, p.fg, es);
  p.off_wf = carve(cur, (size_t)wf * es);
  p.off_wd = carve(cur, (size_t)(wd > 0 ? wd : 1) * es);
  int maxCp = 64;
  size_t prev_y = 0, block_in = 0;
  for (size_t i = 0; i < p.units.size(); ++i) {
    MBUnit& u = p.units[i];
    const size_t rows = (size_t)p.N * u.OH * u.OW, in_rows = (size_t)p.N * u.H * u.W;
    u.in_off = prev_y;
    if (u.res_first) block_in = prev_y;
    if (u.res_last) u.res_off = block_in;
    u.x_off = carve(cur, rows * u.Coutp * es);
    u.y_off = carve(cur, rows * u.Coutp * es);
    u.coef_off = carve(cur, 5 * (size_t)u.Coutp * sizeof(float));
    prev_y = u.y_off;
    if (u.se >= 0) {
      SEBlock& se = p.ses[u.se];
      se.yse_off = carve(cur, rows * u.Coutp * es);
      se.w1p_off = carve(cur, (size_t)se.Csq * se.Cp * 4);
      se.w2p_off = carve(cur, (size_t)se.Cp * se.Csq * 4);
      se.b2p_off = carve(cur, (size_t)se.Cp * 4);
      se.s_off = carve(cur, (size_t)p.N * se.Cp * 4);
      se.z1_off = carve(cur, (size_t)p.N * se.Csq * 4);
      se.a1_off = carve(cur, (size_t)p.N * se.Csq * 4);
      se.z2_off = carve(cur, (size_t)p.N * se.Cp * 4);
      se.g_off = carve(cur, (size_t)p.N * se.Cp * 4);
      prev_y = se.yse_off;
      // backward temporaries: dgate/dz2 [N][Cp] x2, da1/dz1 [N][Csq] x2, ds [N][Cp], dW1p, dW2p, db2p
      size_t t = se_backward_tmp_floats(p.N, se.Cp, se.Csq);
      if (t > setmp) setmp = t;
    }
    if (rows * u.Coutp > maxact) maxact = rows * u.Coutp;
    if (u.kind != U_FIRST && in_rows * u.Cinp > maxact) maxact = in_rows * u.Cinp;
    size_t sf = u.kind == U_DW ? (size_t)column_stats_rows(rows, u.Coutp) * u.Coutp : (size_t)((rows + 127) / 128) * u.Coutp;
    if (sf > stat_floats) stat_floats = sf;
    size_t pb = (size_t)bn_bwd_partial_rows(rows, u.Coutp) * 2 * u.Coutp * sizeof(float);
    if (pb > partial) partial = pb;
    if (u.Coutp > maxCp) maxCp = u.Coutp;
    if (u.kind == U_PW) {
      ConvShape s = {p.N, u.H, u.W, u.Cinp, u.Coutp, 1, 1, 1, 0};
      size_t sb = conv_wgrad_slab_bytes(s);
      if (sb > slab) slab = sb;
    }
    if (u.kind == U_DW) {
      size_t f = dwconv3_wgrad_partial_floats(p.N, u.H, u.W, u.Coutp, u.stride, u.ksize);
      if (f > dwpart) dwpart = f;
    }
  }
  p.stat_bytes = align_up(stat_floats * sizeof(float), 256);
  p.off_stat = carve(cur, 2 * p.stat_bytes);
  p.off_tab = carve(cur, 2 * (size_t)maxCp * sizeof(float));
  p.off_partial = carve(cur, partial);
  p.off_coefbwd = carve(cur, 3 * (size_t)maxCp * sizeof(float));
  p.red_C = maxCp;
  p.off_red = carve(cur, bn_reduce_scratch_bytes(p.red_C));
  p.slab_bytes = slab;
  p.off_slab = carve(cur, slab);
  p.first.dwv(cur);
  p.off_dwpart = carve(cur, (dwpart > 0 ? dwpart : 1) * sizeof(float));
  if (setmp) p.off_setmp = carve(cur, setmp * sizeof(float));
  for (int i = 0; i < 4; ++i) p.off_g[i] = carve(cur, maxact * es);
  p.ws_bytes = cur;
  return MMSKIN_OK;
}

int build_mobilenet_v2(MBPlan& p) {
  p.act = ACT_RELU6;
  p.stemC = 32;
  int h = p.H, w = p.W;
  {
    const int i = add_unit(p, U_FIRST, "features.0.0", "features.0.1", 3, p.stemC, h, w, 2, 3, true);
    h = p.units[i].OH; w = p.units[i].OW;
  }
  // expansion, out, layers, stride  (torchvision mobilenet_v2)
  const int cfg[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
  int cin = p.stemC, fi = 1;
  for (const auto& c : cfg) {
    for (int i = 0; i < c[2]; ++i, ++fi) {
      const int t = c[0], oup = c[1], stride = i == 0 ? c[3] : 1, hidden = cin * t;
      const bool res = stride == 1 && cin == oup;
      const std::string base = "features." + std::to_string(fi) + ".conv.";
      const size_t first = p.units.size();
      int k = 0;
      if (t != 1) { add_unit(p, U_PW, base + "0.0", base + "0.1", cin, hidden, h, w, 1, 1, true); k = 1; }
      const int di = add_unit(p, U_DW, base + std::to_string(k) + ".0", base + std::to_string(k) + ".1", hidden, hidden, h, w, stride, 3, true);
      h = p.units[di].OH; w = p.units[di].OW;
      const int pi = add_unit(p, U_PW, base + std::to_string(k + 1), base + std::to_string(k + 2), hidden, oup, h, w, 1, 1, false);
      if (res) { p.units[first].res_first = true; p.units[pi].res_last = true; }
      ARG_CHECK(h >= 1 && w >= 1, "mobilenet-v2: input %dx%d too small", p.H, p.W);
      cin = oup;
    }
  }
  add_unit(p, U_PW, "features.18.0", "features.18.1", cin, 1280, h, w, 1, 1, true);
  p.feat_dim = 1280;
  return finish_plan(p, "mobilenet-v2");
}

int build_efficientnet(MBPlan& p, int variant) {   // variant 0 = B0, 7 = B7
  const double width = variant == 7 ? 2.0 : 1.0, depth = variant == 7 ? 3.1 : 1.0;
  if (variant == 7) { p.eps = 1e-3f; p.mom = 0.01f; }   // torchvision: BatchNorm2d(eps=0.001, momentum=0.01) for B5-B7
  p.act = ACT_SILU;
  auto adj = [&](int c) { return make_divisible(c * width); };
  int h = p.H, w = p.W;
  p.stemC = adj(32);
  ARG_CHECK(p.stemC <= 64, "efficientnet: stem width %d", p.stemC);
  {
    const int i = add_unit(p, U_FIRST, "features.0.0", "features.0.1", 3, p.stemC, h, w, 2, 3, true);
    h = p.units[i].OH; w = p.units[i].OW;
  }
  // expand, kernel, stride, in, out, layers  (torchvision _efficientnet_conf)
  const int cfg[7][6] = {{1, 3, 1, 32, 16, 1}, {6, 3, 2, 16, 24, 2}, {6, 5, 2, 24, 40, 2}, {6, 3, 2, 40, 80, 3},
                         {6, 5, 1, 80, 112, 3}, {6, 5, 2, 112, 192, 4}, {6, 3, 1, 192, 320, 1}};
  int last_out = 0;
  for (int si = 0; si < 7; ++si) {
    const int layers = (int)ceil(cfg[si][5] * depth);
    for (int li = 0; li < layers; ++li) {
      const int expand = cfg[si][0], ks = cfg[si][1];
      const int cout = adj(cfg[si][4]);
      const int cin = li == 0 ? adj(cfg[si][3]) : cout;
      const int stride = li == 0 ? cfg[si][2] : 1;
      const int hidden = make_divisible((double)cin * expand);
      const bool res = stride == 1 && cin == cout;
      const std::string base = "features." + std::to_string(si + 1) + "." + std::to_string(li) + ".block.";
      const size_t first = p.units.size();
      int k = 0;
      if (hidden != cin) { add_unit(p, U_PW, base + "0.0", base + "0.1", cin, hidden, h, w, 1, 1, true); k = 1; }
      const int di = add_unit(p, U_DW, base + std::to_string(k) + ".0", base + std::to_string(k) + ".1", hidden, hidden, h, w, stride, ks, true);
      h = p.units[di].OH; w = p.units[di].OW;
      SEBlock se = {};
      se.C = hidden; se.Cp = pad64(hidden); se.Csq = cin / 4 > 1 ? cin / 4 : 1;
      const std::string sn = base + std::to_string(k + 1);
      se.w1_off = add_tensor(p.params, p.param_numel, sn + ".fc1.weight", {se.Csq, hidden, 1, 1});
      se.b1_off = add_tensor(p.params, p.param_numel, sn + ".fc1.bias", {se.Csq});
      se.w2_off = add_tensor(p.params, p.param_numel, sn + ".fc2.weight", {hidden, se.Csq, 1, 1});
      se.b2_off = add_tensor(p.params, p.param_numel, sn + ".fc2.bias", {hidden});
      p.units[di].se = (int)p.ses.size();
      p.ses.push_back(se);
      const int pi = add_unit(p, U_PW, base + std::to_string(k + 2) + ".0", base + std::to_string(k + 2) + ".1", hidden, cout, h, w, 1, 1, false);
      if (res) { p.units[first].res_first = true; p.units[pi].res_last = true; p.units[pi].sd = p.n_sd++; }
      ARG_CHECK(h >= 1 && w >= 1, "efficientnet: input %dx%d too small", p.H, p.W);
      last_out = cout;
    }
  }
  const int headC = 4 * last_out;
  add_unit(p, U_PW, "features.8.0", "features.8.1", last_out, headC, h, w, 1, 1, true);
  p.feat_dim = headC;
  ARG_CHECK(headC % 64 == 0, "efficientnet: head width %d", headC);
  return finish_plan(p, "efficientnet");
}

inline SEArgs se_args(const MBPlan& p, const SEBlock& se, unsigned char* ws, const float* params, int HW) {
  SEArgs a;
  a.N = p.N; a.HW = HW; a.C = se.C; a.Cp = se.Cp; a.Csq = se.Csq;
  a.w1p = reinterpret_cast<const float*>(ws + se.w1p_off); a.b1 = params + se.b1_off;
  a.w2p = reinterpret_cast<const float*>(ws + se.w2p_off); a.b2p = reinterpret_cast<const float*>(ws + se.b2p_off);
  a.s = reinterpret_cast<float*>(ws + se.s_off); a.z1 = reinterpret_cast<float*>(ws + se.z1_off);
  a.a1 = reinterpret_cast<float*>(ws + se.a1_off); a.z2 = reinterpret_cast<float*>(ws + se.z2_off);
  a.g = reinterpret_cast<float*>(ws + se.g_off);
  return a;
}

template <typename T>
int mb_forward(MBPlan& p, const void* image, const float* norm6, const float* params, float* buffers,
               unsigned char* ws, float* features, bool training, hipStream_t st) {
  const float eps = p.eps, mom = p.mom, cap = p.act_cap();
  T* wf = reinterpret_cast<T*>(ws + p.off_wf);
  T* wd = reinterpret_cast<T*>(ws + p.off_wd);
  float* stat_sum = reinterpret_cast<float*>(ws + p.off_stat);
  float* stat_sq = reinterpret_cast<float*>(ws + p.off_stat + p.stat_bytes);
  float* tab = reinterpret_cast<float*>(ws + p.off_tab);
  const ColScratch red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  const float* sd = training ? p.sd_mask : nullptr;
  int rc;
  if ((rc = p.ensure_table())) return rc;
  PROF(K_STAGE, 0.0, 0.0, stage_weights<T>(p.table_dev, (int)p.table_host.size(), p.max_stage_elems, params, wf, wd, training, st));
  PROF(K_STAGE, 0.0, 0.0, first3_stage<T>(params + p.units[0].w_off, wf, st, p.stemC));
  for (MBUnit& u : p.units)
    if (u.kind == U_DW) PROF(K_STAGE, 0.0, 0.0, dw_stage_weights<T>(params + u.w_off, u.Cout, u.Coutp, wf + u.wf, st, u.ksize));
  for (SEBlock& se : p.ses) {
    PROF(K_STAGE, 0.0, 0.0, pad_matrix(params + se.w1_off, se.Csq, se.C, se.Csq, se.Cp, reinterpret_cast<float*>(ws + se.w1p_off), st));
    PROF(K_STAGE, 0.0, 0.0, pad_matrix(params + se.w2_off, se.C, se.Csq, se.Cp, se.Csq, reinterpret_cast<float*>(ws + se.w2p_off), st));
    PROF(K_STAGE, 0.0, 0.0, pad_matrix(params + se.b2_off, 1, se.C, 1, se.Cp, reinterpret_cast<float*>(ws + se.b2p_off), st));
  }

  for (MBUnit& u : p.units) {
    const size_t rows = (size_t)p.N * u.OH * u.OW;
    const T* in = reinterpret_cast<const T*>(ws + u.in_off);
    T* x = reinterpret_cast<T*>(ws + u.x_off);
    T* y = reinterpret_cast<T*>(ws + u.y_off);
    const int Cp = u.Coutp;
    const BnCoef k(reinterpret_cast<float*>(ws + u.coef_off), Cp);
    int nrows = 0;
    if (u.kind == U_FIRST) {   // weights staged above (null here); the profile counts half the 64-column GEMM
      if ((rc = first_conv_forward<T>(p.first.bufs<T>(ws, wf, x), p.fg, image, norm6, nullptr, nullptr, training ? stat_sum : nullptr,
                                      training ? stat_sq : nullptr, &p.prof, st, 0.5))) return rc;
      nrows = (int)((rows + 127) / 128);
    } else if (u.kind == U_PW) {
      ConvShape s = {p.N, u.H, u.W, u.Cinp, u.Coutp, 1, 1, 1, 0};
      PROF(K_CONV_FWD, conv_flops(s), conv_bytes(s, sizeof(T)),
           launch_conv_fwd<T>(s, in, wf + u.wf, x, training ? stat_sum : nullptr, training ? stat_sq : nullptr, st));
      nrows = conv_fwd_stat_rows(s);
    } else {
      PROF(K_CONV_FWD, 2.0 * u.ksize * u.ksize * rows * Cp, (double)((size_t)p.N * u.H * u.W + rows) * Cp * sizeof(T),
           dwconv3_fwd<T>(in, wf + u.wf, p.N, u.H, u.W, Cp, u.stride, x, st, u.ksize));
      if (training) PROF(K_BN_FWD, 0.0, (double)rows * Cp * sizeof(T), column_stats<T>(x, rows, Cp, stat_sum, stat_sq, &nrows, st));
    }
    if (training)
      PROF(K_BN_FWD, 0.0, 0.0, bn_table_finalize(stat_sum, stat_sq, nrows, Cp, Cp, (double)rows, tab, tab + Cp, red, st));
    PROF(K_BN_FWD, 0.0, 0.0, bn_coef_from_table(tab, tab + Cp, u.Cout, Cp, params + u.bn.g_off, params + u.bn.b_off, eps, mom,
                       (double)rows, buffers + u.bn.rm_off, buffers + u.bn.rv_off, training, k.scale, st));
    const T* res = u.res_last ? reinterpret_cast<const T*>(ws + u.res_off) : nullptr;
    if (res && sd) {   // stochastic depth: y = bn(x) * mask[n] + block input
      PROF(K_BN_FWD, 0.0, 2.0 * rows * Cp * sizeof(T), bn_apply<T>(x, nullptr, k.scale, k.shift, nullptr, nullptr, y, rows, Cp, false, st));
      PROF(K_BN_FWD, 0.0, 3.0 * rows * Cp * sizeof(T),
           sd_residual_add<T>(y, res, sd + (size_t)u.sd * p.N, p.N, (size_t)u.OH * u.OW * Cp, y, st));
    } else {
      PROF(K_BN_FWD, 0.0, (res ? 3.0 : 2.0) * rows * Cp * sizeof(T),
           bn_apply<T>(x, res, k.scale, k.shift, nullptr, nullptr, y, rows, Cp, u.act, st, nullptr, cap));
    }
    if (u.se >= 0) {   // squeeze-excitation on the depthwise output
      SEBlock& se = p.ses[u.se];
      if ((rc = se_forward<T>(se_args(p, se, ws, params, u.OH * u.OW), y, reinterpret_cast<T*>(ws + se.yse_off), &p.prof, st))) return rc;
    }
  }
  MBUnit& last = p.units.back();
  return avgpool_fwd<T>(reinterpret_cast<const T*>(ws + last.y_off), p.N, last.OH * last.OW, last.Coutp, features, st);
}

template <typename T>
int mb_backward(MBPlan& p, const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  T* wf = reinterpret_cast<T*>(ws + p.off_wf);
  T* wd = reinterpret_cast<T*>(ws + p.off_wd);
  const WgradSlab slab = wgrad_slab_at(ws, p.off_slab, p.slab_bytes);
  float* partial = reinterpret_cast<float*>(ws + p.off_partial);
  float* cA = reinterpret_cast<float*>(ws + p.off_coefbwd);
  const ColScratch red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  float* setmp = reinterpret_cast<float*>(ws + p.off_setmp);
  const float* sd = p.sd_mask;
  const int act_mask = p.act_mask();
  T* B[4];
  for (int i = 0; i < 4; ++i) B[i] = reinterpret_cast<T*>(ws + p.off_g[i]);
  int rc, cur = 0, reserved = -1;
  auto take = [&](int a, int b) { for (int i = 0; i < 4; ++i) if (i != a && i != b && i != reserved) return i; return -1; };
  MBUnit& last = p.units.back();
  if ((rc = avgpool_bwd<T>(dfeat, p.N, last.OH * last.OW, last.Coutp, B[cur], st))) return rc;

  for (int ui = (int)p.units.size() - 1; ui >= 0; --ui) {
    MBUnit& u = p.units[ui];
    const size_t rows = (size_t)p.N * u.OH * u.OW;
    const int Cp = u.Coutp, HW = u.OH * u.OW;
    const T* x = reinterpret_cast<const T*>(ws + u.x_off);
    const T* y = reinterpret_cast<const T*>(ws + u.y_off);
    const T* in = reinterpret_cast<const T*>(ws + u.in_off);
    if (u.se >= 0) {
      // ---- squeeze-excitation backward: B[cur] = d(y_se) -> d(y_dw) = dyse * g + ds / HW
      SEBlock& se = p.ses[u.se];
      const int nb = take(cur, -1);
      if ((rc = se_backward<T>(se_args(p, se, ws, params, HW), B[cur], y, setmp, grads + se.w1_off, grads + se.b1_off, grads + se.w2_off,
                               grads + se.b2_off, B[nb], &p.prof, st))) return rc;
      cur = nb;
    }
    if (u.res_last) {
      reserved = cur;   // this gradient is also the residual branch's: keep it until the block's first unit
      if (sd) {         // branch gradient = dy * mask[n]
        const int nb = take(cur, -1);
        PROF(K_BN_BWD, 0.0, 2.0 * rows * Cp * sizeof(T), sd_row_scale<T>(B[cur], sd + (size_t)u.sd * p.N, p.N, (size_t)HW * Cp, B[nb], st));
        cur = nb;
      }
    }
    // ---- BatchNorm (+ activation) backward: dy -> dx
    const int a = take(cur, -1);
    const BnCoef k(reinterpret_cast<float*>(ws + u.coef_off), Cp);   // gamma: the copy zero-padded to Cp channels
    if ((rc = bn_backward<T>(B[cur], x, y, u.act ? act_mask : MASK_NONE, rows, Cp, k, k.gamma, grads + u.bn.g_off, grads + u.bn.b_off,
                             BnBwdCoef(cA, Cp), partial, red, B[a], nullptr, &p.prof, 6.0 * rows * Cp * sizeof(T), st, u.Cout))) return rc;
    const T* dx = B[a];
    // ---- convolution backward
    if (u.kind == U_FIRST) return first_conv_wgrad<T>(p.first.bufs<T>(ws, nullptr, nullptr, slab), p.fg, dx, grads + u.w_off, p.stemC, &p.prof, st, 0.5);
    int b;
    if (u.kind == U_PW) {
      ConvShape s = {p.N, u.H, u.W, u.Cinp, u.Coutp, 1, 1, 1, 0};
      PROF(K_WGRAD, conv_flops(s), conv_bytes(s, sizeof(T)), launch_conv_wgrad<T>(s, dx, in, slab, grads + u.w_off, st, u.Cout, u.Cin));
      if (u.res_first) {   // add the residual branch's gradient in the epilogue, in place on the buffer that holds it
        b = reserved;
        PROF(K_CONV_DGRAD, conv_flops(s), conv_bytes(s, sizeof(T), 1), launch_conv_dgrad<T>(s, dx, wd + u.wd, B[b], B[b], st));
        reserved = -1;
      } else {
        b = take(a, -1);
        PROF(K_CONV_DGRAD, conv_flops(s), conv_bytes(s, sizeof(T)), launch_conv_dgrad<T>(s, dx, wd + u.wd, B[b], (const T*)nullptr, st));
      }
    } else {
      b = take(a, -1);
      PROF(K_WGRAD, 2.0 * u.ksize * u.ksize * rows * Cp, 0.0,
           dwconv3_wgrad<T>(dx, in, p.N, u.H, u.W, Cp, u.stride, reinterpret_cast<float*>(ws + p.off_dwpart), grads + u.w_off, u.Cout, st, u.ksize));
      PROF(K_CONV_DGRAD, 2.0 * u.ksize * u.ksize * rows * Cp, 0.0, dwconv3_dgrad<T>(dx, wf + u.wf, p.N, u.H, u.W, Cp, u.stride, B[b], st, u.ksize));
      if (u.res_first) {   // block whose first unit is the depthwise conv (expand ratio 1, B7 stage 1): add the residual gradient
        PROF(K_CONV_DGRAD, 0.0, 0.0, ew_add<T>(B[b], B[reserved], B[reserved], (size_t)p.N * u.H * u.W * Cp, st));
        b = reserved;
        reserved = -1;
      }
    }
    cur = b;
  }
  return MMSKIN_OK;
}

int MBPlan::forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                    float* features, bool training, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return mb_forward<decltype(t)>(*this, image, norm6, params, buffers, ws, features, training, st); });
}
int MBPlan::backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return mb_backward<decltype(t)>(*this, dfeat, params, ws, grads, st); });
}

}  // namespace

template <typename T>
int se_forward(const SEArgs& a, const T* y, T* yse, Profiler* prof, hipStream_t st) {
  const int cls = K_BN_FWD;
  const size_t rows = (size_t)a.N * a.HW;
  int rc;
  if ((rc = gap_reduce<T>(y, nullptr, a.N, a.HW, a.Cp, 1.f / (float)a.HW, a.s, st))) return rc;
  if ((rc = mmskin_linear_forward(a.s, a.w1p, a.b1, a.z1, a.N, a.Cp, a.Csq, 0, st))) return rc;
  if ((rc = ew_act_fwd(a.z1, a.a1, (int64_t)a.N * a.Csq, 0, st))) return rc;
  if ((rc = mmskin_linear_forward(a.a1, a.w2p, a.b2p, a.z2, a.N, a.Csq, a.Cp, 0, st))) return rc;
  if ((rc = ew_act_fwd(a.z2, a.g, (int64_t)a.N * a.Cp, 1, st))) return rc;
  PROF_AT(prof, cls, 0.0, 2.0 * rows * a.Cp * sizeof(T), se_scale_fwd<T>(y, a.g, a.N, a.HW, a.Cp, yse, st));
  return MMSKIN_OK;
}

template <typename T>
int se_backward(const SEArgs& a, const T* dyse, const T* y, float* tmp, float* dW1, float* db1, float* dW2, float* db2, T* dy,
                Profiler* prof, hipStream_t st) {
  const int cls = K_BN_BWD;
  const size_t rows = (size_t)a.N * a.HW;
  const int N = a.N, Cp = a.Cp, Csq = a.Csq;
  int rc;
  float* t = tmp;
  float* dgate = t; t += (size_t)N * Cp;
  float* dz2 = t; t += (size_t)N * Cp;
  float* ds = t; t += (size_t)N * Cp;
  float* da1 = t; t += (size_t)N * Csq;
  float* dz1 = t; t += (size_t)N * Csq;
  float* dw1p = t; t += (size_t)Csq * Cp;
  float* dw2p = t; t += (size_t)Cp * Csq;
  float* db2p = t; t += Cp;
  if ((rc = gap_reduce<T>(dyse, y, N, a.HW, Cp, 1.f, dgate, st))) return rc;
  if ((rc = ew_act_bwd(dgate, a.z2, dz2, (int64_t)N * Cp, 1, st))) return rc;
  if ((rc = mmskin_linear_backward(dz2, a.a1, a.w2p, nullptr, nullptr, da1, dw2p, db2p, N, Csq, Cp, st))) return rc;
  if ((rc = ew_act_bwd(da1, a.z1, dz1, (int64_t)N * Csq, 0, st))) return rc;
  if ((rc = mmskin_linear_backward(dz1, a.s, a.w1p, nullptr, nullptr, ds, dw1p, db1, N, Cp, Csq, st))) return rc;
  HIP_CHECK_RET(hipMemcpy2DAsync(dW1, (size_t)a.C * 4, dw1p, (size_t)Cp * 4, (size_t)a.C * 4, Csq, hipMemcpyDeviceToDevice, st));
  HIP_CHECK_RET(hipMemcpyAsync(dW2, dw2p, (size_t)a.C * Csq * 4, hipMemcpyDeviceToDevice, st));
  HIP_CHECK_RET(hipMemcpyAsync(db2, db2p, (size_t)a.C * 4, hipMemcpyDeviceToDevice, st));
  PROF_AT(prof, cls, 0.0, 2.0 * rows * Cp * sizeof(T), se_dx<T>(dyse, a.g, ds, N, a.HW, Cp, dy, st));
  return MMSKIN_OK;
}
template int se_forward<float>(const SEArgs&, const float*, float*, Profiler*, hipStream_t);
template int se_forward<bf16_t>(const SEArgs&, const bf16_t*, bf16_t*, Profiler*, hipStream_t);
template int se_backward<float>(const SEArgs&, const float*, const float*, float*, float*, float*, float*, float*, float*, Profiler*, hipStream_t);
template int se_backward<bf16_t>(const SEArgs&, const bf16_t*, const bf16_t*, float*, float*, float*, float*, float*, bf16_t*, Profiler*, hipStream_t);

PlanBase* make_mobilenet_plan(int N, int H, int W, int dtype, int* rc) {
  return make_plan<MBPlan>(N, H, W, dtype, rc, build_mobilenet_v2);
}
PlanBase* make_efficientnet_plan(int variant, int N, int H, int W, int dtype, int* rc) {
  return make_plan<MBPlan>(N, H, W, dtype, rc, [variant](MBPlan& p) { return build_efficientnet(p, variant); });
}
