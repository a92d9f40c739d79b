// ResNet image-encoder plan executor (resnet-18 / resnet-50, torchvision v1.5 layout).
//
// One C-ABI call runs the whole backbone forward (or backward) by launching the gfx950 kernels of
// conv_gemm.hip / wgrad.hip / ops.hip back to back on the caller's stream: no Python per layer, no
// allocation, graph-capturable.  Replaces `self.image_encoder(image)` of the reference
// (multimodalIntraInterModal.py:167; factory loadImageModelClassifier.py:65-75) and its autograd
// backward.  Parameters stay fp32 masters in one flat buffer laid out in torchvision's
// named_parameters() order; they are re-staged to the compute dtype (K-contiguous GEMM operands) at
// the start of every forward.
#include <algorithm>

#include "plan.h"
#include "../../include/mmskin.h"

namespace {

struct Unit {  // conv + batch-norm
  ConvShape s;
  bool stem = false;
  int64_t w_off, g_off, b_off;   // flat param offsets
  int64_t rm_off, rv_off;        // flat buffer offsets
  int64_t wf_off, wd_off;        // staged weight element offsets
  size_t x_off;                  // raw conv output (bytes in workspace)
  size_t y_off = 0;              // post-activation output (bytes); for the last unit of a block = block output (stem: none, its output is the pooled map)
  size_t coef_off;               // floats: scale, shift, mean, invstd (4*Cout)
  bool abn = false;              // algebraic BatchNorm backward (abn.hip): expanding 1x1 conv3 of a bottleneck, bf16 plans
  size_t gram_off = 0;           // two-pass unit with Gram statistics: y^T y [128][Cin] + colsum(y) [Cin] of its input, forward -> backward
  bool fwd2p = false;            // ... and its raw output x never stored: two-pass forward (statistics, then conv + BatchNorm + residual + ReLU in the
                                 // epilogue), BatchNorm-backward x sums from the weight-gradient GEMM (blocks without a downsample branch)
  size_t abn_coef_off = 0;       // this unit's copy of cA | cB | cC (3*Cout floats) for the weight-gradient stream
  size_t rows() const { return (size_t)s.N * s.OH() * s.OW(); }
};

struct Block {
  std::vector<int> units;
  int ds = -1;
  size_t mask_off = 0;   // 1-bit ReLU mask of the block output (one byte per 16-byte chunk)
  size_t in_off;   // block input activation (bytes)
  int in_C, in_H, in_W;
  int seg_done = -1;   // gradient segment that is complete once this block's backward has been enqueued
  bool ds_compact = false;   // stride-2 1x1 downsample in front of a 1x1 / stride 1 conv1: its data gradient is computed on the pixels the
                             // convolution read only, and conv1's data gradient adds it at the even pixels (knob MMSKIN_DS_COMPACT, default on)
};

// Side-stream slots of backward: one per gradient buffer that the main stream writes and a weight-gradient launch on the side stream
// reads (SideStream::run hands the buffer over, SideStream::acquire comes before the main stream writes it again).  BwdBufs below
// says which buffer each slot guards.
enum SideSlot { SLOT_DX0 = 0, SLOT_DX1, SLOT_DS, SLOT_G0, SLOT_G1, SIDE_SLOTS };

struct Plan : PlanBase {
  int arch;
  StemGeom sg;
  std::vector<Unit> units;
  std::vector<Block> blocks;
  int64_t staged_elems = 0;
  // workspace layout (bytes)
  size_t off_img4, off_wf, off_wd, off_stat, off_pool, off_idx, off_scratch[7], off_slab, slab_bytes, off_partial,
      off_coefbwd, off_dwv, off_red, off_partial_b, off_stat_b, off_red_b;
  int red_C = 0;   // channels both reduction scratches were carved for (bn_reduce_scratch)
  size_t off_abn_wd = 0, off_abn_bias = 0, off_abn_S = 0, off_abn_cs = 0;   // algebraic BatchNorm backward scratch
  size_t off_abn_wd2 = 0, off_abn_bias2 = 0;                                 // ... of a stride-1 downsample convolution (its folded weights live beside conv3's)
  size_t off_abn_sgx = 0, off_abn_slab2 = 0, off_abn_S2 = 0, off_abn_cs2 = 0;   // two-pass units: main-stream weight-gradient scratch
  size_t maxact_bytes = 0, stat_bytes = 0;

  int forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
              float* features, bool training, hipStream_t st) override;
  int backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) override;
  int last_conv_shape(int* C, int* OH, int* OW) const override;
  int last_conv_export(const unsigned char* ws, float* x_nchw, hipStream_t st) override;
  int last_conv_grad(const float* dfeat, const unsigned char* ws, float* dx_nchw, hipStream_t st) override;
  int num_units() const override { return (int)units.size(); }
  int unit_info(int index, std::string* name, int64_t* info12) const override;
  int unit_flags(int index, int* flags) const override;
};

int add_unit(Plan& p, const std::string& conv_name, const std::string& bn_name, ConvShape s) {
  Unit u;
  u.s = s;
  u.w_off = add_tensor(p.params, p.param_numel, conv_name + ".weight", {s.Cout, s.Cin, s.kh, s.kw});
  u.g_off = add_tensor(p.params, p.param_numel, bn_name + ".weight", {s.Cout});
  u.b_off = add_tensor(p.params, p.param_numel, bn_name + ".bias", {s.Cout});
  u.rm_off = add_tensor(p.buffers, p.buffer_numel, bn_name + ".running_mean", {s.Cout});
  u.rv_off = add_tensor(p.buffers, p.buffer_numel, bn_name + ".running_var", {s.Cout});
  p.units.push_back(u);
  return (int)p.units.size() - 1;
}

int build_plan(Plan& p) {
  const bool bottleneck = p.arch == 50;
  const int depths18[4] = {2, 2, 2, 2}, depths50[4] = {3, 4, 6, 3};
  const int* depths = bottleneck ? depths50 : depths18;
  const int expansion = bottleneck ? 4 : 1;
  // stem
  p.sg = StemGeom(p.N, p.H, p.W);
  int u0 = add_unit(p, "conv1", "bn1", p.sg.conv());
  p.units[u0].stem = true;
  int cin = 64, h = p.sg.PH, w = p.sg.PW;
  const int widths[4] = {64, 128, 256, 512};
  std::vector<int64_t> seg_starts;   // first parameter of layer2, layer3, layer4
  for (int li = 0; li < 4; ++li) {
    for (int b = 0; b < depths[li]; ++b) {
      const int stride = (b == 0 && li > 0) ? 2 : 1;
      const int width = widths[li], cout = width * expansion;
      std::string base = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      Block blk;
      blk.in_C = cin; blk.in_H = h; blk.in_W = w;
      if (bottleneck) {
        blk.units.push_back(add_unit(p, base + ".conv1", base + ".bn1", {p.N, h, w, cin, width, 1, 1, 1, 0}));
        blk.units.push_back(add_unit(p, base + ".conv2", base + ".bn2", {p.N, h, w, width, width, 3, 3, stride, 1}));
        int h2 = (h + 2 - 3) / stride + 1, w2 = (w + 2 - 3) / stride + 1;
        blk.units.push_back(add_unit(p, base + ".conv3", base + ".bn3", {p.N, h2, w2, width, cout, 1, 1, 1, 0}));
      } else {
        blk.units.push_back(add_unit(p, base + ".conv1", base + ".bn1", {p.N, h, w, cin, width, 3, 3, stride, 1}));
        int h2 = (h + 2 - 3) / stride + 1, w2 = (w + 2 - 3) / stride + 1;
        blk.units.push_back(add_unit(p, base + ".conv2", base + ".bn2", {p.N, h2, w2, width, cout, 3, 3, 1, 1}));
      }
      if (stride != 1 || cin != cout)
        blk.ds = add_unit(p, base + ".downsample.0", base + ".downsample.1", {p.N, h, w, cin, cout, 1, 1, stride, 0});
      static const bool ds_compact_on = env_knob("MMSKIN_DS_COMPACT", 1) != 0;
      const ConvShape& c1 = p.units[blk.units[0]].s;   // conv1's data gradient adds the compact gradient in its fused epilogue; the first block has none
      blk.ds_compact = ds_compact_on && blk.ds >= 0 && !p.blocks.empty() && stride == 2 && c1.kh == 1 && c1.stride == 1;
      if (b == 0 && li > 0) {   // layerN's parameters start here: everything from this offset on completes first in backward
        blk.seg_done = 3 - li;
        seg_starts.push_back(p.units[blk.units[0]].w_off);
      }
      p.blocks.push_back(blk);
      cin = cout;
      h = (h + 2 - 3) / stride + 1;
      w = (w + 2 - 3) / stride + 1;
    }
  }
  p.feat_dim = cin;
  {   // gradient segments in backward completion order: layer4, layer3, layer2, layer1 + stem
    int64_t end = p.param_numel;
    for (int i = 2; i >= 0; --i) {
      PlanBase::GradSegment g;
      g.offset = seg_starts[i]; g.numel = end - seg_starts[i];
      p.segments.push_back(g);
      end = seg_starts[i];
    }
    PlanBase::GradSegment g;
    g.offset = 0; g.numel = end;
    p.segments.push_back(g);
  }

  // ---- staged weights + stage table
  std::vector<StageDesc> table;
  int64_t wf = 0, wd = 0;
  for (Unit& u : p.units) {
    if (!u.stem) { stage_append(table, u.w_off, u.s.Cout, u.s.Cin, u.s.kh * u.s.kw, 0, 0, wf, wd, p.max_stage_elems, u.wf_off, u.wd_off); continue; }
    StageDesc d = {};   // the stem row: a 64 x 256 forward slot (virtual [64][8][32]) and no data-gradient slot
    d.src_off = u.w_off; d.Cout = u.s.Cout; d.Cin = u.s.Cin; d.taps = u.s.kh * u.s.kw; d.stem = 1;
    u.wf_off = d.fwd_off = wf; u.wd_off = d.dgrad_off = wd;
    wf += 64 * 256;
    if (d.Cout * d.Cin * d.taps > p.max_stage_elems) p.max_stage_elems = d.Cout * d.Cin * d.taps;
    table.push_back(d);
  }
  p.staged_elems = wf;
  p.table_host = table;  // uploaded by ensure_table() on the first forward (create() needs no GPU)

  // ---- workspace layout
  const size_t es = p.esz();
  size_t cur = 0;
  p.off_img4 = carve(cur, (size_t)p.N * p.sg.Hp * p.sg.Wp * 4 * es);
  p.off_wf = carve(cur, (size_t)wf * es);
  p.off_wd = carve(cur, (size_t)wd * es);
  size_t stat_rows_max = 0, maxact = 0, slab_max = stem_wgrad_slab_bytes(p.N, p.sg.OH, p.sg.OW), partial_max = 0;
  int maxC = 64;
  for (Unit& u : p.units) {
    size_t rows = u.rows();
    size_t sr = (size_t)ceil_div((int)rows, 128) * u.s.Cout;
    if (sr > stat_rows_max) stat_rows_max = sr;
    if (rows * u.s.Cout > maxact) maxact = rows * u.s.Cout;
    if ((size_t)u.s.N * u.s.H * u.s.W * u.s.Cin > maxact && !u.stem) maxact = (size_t)u.s.N * u.s.H * u.s.W * u.s.Cin;
    if (!u.stem) { size_t sb = conv_wgrad_slab_bytes(u.s); if (sb > slab_max) slab_max = sb; }
    size_t pr = (size_t)bn_bwd_partial_rows(rows, u.s.Cout) * 2 * u.s.Cout * sizeof(float);
    if (pr > partial_max) partial_max = pr;
    // partial rows written by a dgrad epilogue that produces this unit's output-shaped gradient
    pr = ((rows + 127) / 128 + 4) * 2 * u.s.Cout * sizeof(float);
    if (pr > partial_max) partial_max = pr;
    if (u.s.Cout > maxC) maxC = u.s.Cout;
  }
  p.stat_bytes = stat_rows_max * sizeof(float);
  p.off_stat = carve(cur, 2 * p.stat_bytes);
  p.off_stat_b = carve(cur, 2 * p.stat_bytes);   // downsample branch (runs on the side stream)
  p.maxact_bytes = maxact * es;
  for (Unit& u : p.units) {
    u.coef_off = carve(cur, 4 * (size_t)u.s.Cout * sizeof(float));
    u.x_off = carve(cur, u.rows() * u.s.Cout * es);
  }
  for (size_t i = 0; i < p.units.size(); ++i) {   // BatchNorm behind every conv: inference folding / eval coefficients
    StageDesc& d = p.table_host[i];
    const Unit& u = p.units[i];
    d.has_bn = 1;
    d.bn_g_off = u.g_off; d.bn_b_off = u.b_off; d.bn_rm_off = u.rm_off; d.bn_rv_off = u.rv_off;
    d.coef_off = (int64_t)u.coef_off;
  }
  p.off_pool = carve(cur, p.sg.pooled() * 64 * es);
  p.off_idx = carve(cur, p.sg.pooled() * 64);
  // post-activation outputs
  size_t prev = p.off_pool;
  for (Block& b : p.blocks) {
    b.in_off = prev;
    for (int ui : b.units) {
      Unit& u = p.units[ui];
      u.y_off = carve(cur, u.rows() * u.s.Cout * es);
    }
    prev = p.units[b.units.back()].y_off;
    Unit& bl = p.units[b.units.back()];
    b.mask_off = carve(cur, bl.rows() * bl.s.Cout * es / 16);
  }
  for (int i = 0; i < 7; ++i) p.off_scratch[i] = carve(cur, p.maxact_bytes);
  {   // algebraic BatchNorm backward of the bottlenecks' expanding 1x1 convolutions (bf16 plans), up to abn_maxc input channels:
      // the data gradient of wider layers belongs to the pipelined kernel
    constexpr int abn_maxc = 128;
    size_t wd_max = 0, s_max = 0;
    int cw_max = 0;
    std::vector<int> cand;
    for (Block& b : p.blocks) { cand.push_back(b.units.back()); if (b.ds >= 0) cand.push_back(b.ds); }
    for (int ui : cand) {
      Unit& u = p.units[ui];
      WgradRingPlan rp;
      if (p.dtype != 1 || !bottleneck || u.s.kh != 1 || u.s.stride != 1 || u.s.Cin > abn_maxc || !abn_accepts(u.s.Cout, u.s.Cin) ||
          !wgrad_gram_plan((int)u.rows(), u.s.Cout, u.s.Cin, rp) || rp.gram_tiles != 1)
        continue;
      u.abn = true;
      u.abn_coef_off = carve(cur, 3 * (size_t)u.s.Cout * sizeof(float));
      const size_t sb = wgrad_gram_slab_bytes((int)u.rows(), u.s.Cout, u.s.Cin);
      if (sb > slab_max) slab_max = sb;
      const size_t wdb = (size_t)u.s.Cin * (u.s.Cout + u.s.Cin) * 2, sf = ((size_t)u.s.Cout + 64 * rp.wo) * u.s.Cin * sizeof(float);
      if (wdb > wd_max) wd_max = wdb;
      if (sf > s_max) s_max = sf;
      if (u.s.Cin > cw_max) cw_max = u.s.Cin;
    }
    if (wd_max) {
      p.off_abn_wd = carve(cur, wd_max);
      p.off_abn_bias = carve(cur, (size_t)cw_max * sizeof(float));
      p.off_abn_S = carve(cur, s_max);
      p.off_abn_cs = carve(cur, (size_t)cw_max * sizeof(float));
      p.off_abn_wd2 = carve(cur, wd_max);
      p.off_abn_bias2 = carve(cur, (size_t)cw_max * sizeof(float));
      size_t slab2 = 0;
      for (Block& b : p.blocks) {
        Unit& u = p.units[b.units.back()];
        // never in the last block: its gradient arrives from the average pool with no sums, so its BatchNorm backward runs from dy
        // and reads the raw output a two-pass unit does not store (today no unit there is algebraic either: 512 input channels)
        if (!u.abn || b.ds >= 0 || &b == &p.blocks.back()) continue;
        u.fwd2p = true;
        size_t sb = wgrad_gram_slab_bytes((int)u.rows(), u.s.Cout, u.s.Cin);
        if (sb > slab2) slab2 = sb;
        // the first pass is not the convolution again but the Gram matrix of its INPUT (gram_stats, abn.hip); the backward pass
        // reuses that matrix and runs g^T y alone
        WgradRingPlan rg;
        if (wgrad_gram_plan((int)u.rows(), 0, u.s.Cin, rg, 2) && rg.gram_tiles == 1 &&
            wgrad_gram_slab_bytes((int)u.rows(), u.s.Cout, u.s.Cin, 1)) {
          u.gram_off = carve(cur, ((size_t)128 + 1) * u.s.Cin * sizeof(float));
          sb = wgrad_gram_slab_bytes((int)u.rows(), 0, u.s.Cin, 2);
          if (sb > slab2) slab2 = sb;
          sb = wgrad_gram_slab_bytes((int)u.rows(), u.s.Cout, u.s.Cin, 1);
          if (sb > slab2) slab2 = sb;
        }
      }
      if (slab2) {
        p.off_abn_sgx = carve(cur, 1024 * sizeof(float));
        p.off_abn_slab2 = carve(cur, slab2);
        p.off_abn_S2 = carve(cur, s_max);
        p.off_abn_cs2 = carve(cur, (size_t)cw_max * sizeof(float));
      }
    }
  }
  p.slab_bytes = slab_max;
  p.off_slab = carve(cur, slab_max);
  p.off_partial = carve(cur, partial_max);
  p.off_partial_b = carve(cur, partial_max);
  p.off_coefbwd = carve(cur, 3 * (size_t)maxC * sizeof(float));
  p.off_dwv = carve(cur, 64 * 256 * sizeof(float));
  p.red_C = maxC;
  p.off_red = carve(cur, bn_reduce_scratch_bytes(p.red_C));
  p.off_red_b = carve(cur, bn_reduce_scratch_bytes(p.red_C));
  p.ws_bytes = cur;
  return MMSKIN_OK;
}

// Backward's gradient buffers by role.  Each is one of the plan's seven scratch regions of maxact_bytes (the largest activation).
//   role      region  slot        written by the main stream                          read by
//   G[0 / 1]  0 / 1   SLOT_G0/1   pool backward; conv1's data gradient (a block reads  main: the block below; side: the algebraic weight
//                                 one and writes the other)                            gradient of its conv3 / downsample (g itself)
//   dX[0 / 1] 2 / 6   SLOT_DX0/1  a unit's BatchNorm backward, alternating per unit    main: its data gradient; side: its weight gradient
//   dXd       5       SLOT_DS     the downsample branch's BatchNorm backward           main / side: the branch's two gradients
//   dY        3       -           data gradient of units 1.. (masked, sums taken)      main: BatchNorm backward of the unit below
//   dZ        4       -           BatchNorm backward from dy (last block)              main: conv1's data gradient (residual addend)
// Region 3 has three roles and no slot.  Inside the block loop only the main stream touches it, and each role is consumed before
// the next is written: dY goes from unit i's data gradient to unit i-1's BatchNorm backward; ds_addend (the compact stride-2
// downsample gradient) is written after the block's last dY was consumed and read by conv1's data gradient right behind it;
// stem_dx0 is written after the last block, and the stem's weight gradient that reads it is handed over and joined through
// SLOT_DX0 (the dX pair is idle by then) before backward returns.
template <typename T>
struct SlotBuf {
  T* p;
  int slot;
};
template <typename T>
struct BwdBufs {
  SlotBuf<T> G[2], dX[2], dXd;
  T *dY, *dZ, *ds_addend, *stem_dx0;
  BwdBufs(const Plan& p, unsigned char* ws) {
    auto region = [&](int i) { return reinterpret_cast<T*>(ws + p.off_scratch[i]); };
    G[0] = {region(0), SLOT_G0}; G[1] = {region(1), SLOT_G1};
    dX[0] = {region(2), SLOT_DX0}; dX[1] = {region(6), SLOT_DX1};
    dXd = {region(5), SLOT_DS};
    dY = ds_addend = stem_dx0 = region(3);
    dZ = region(4);
  }
};

template <typename T>
StemBufs<T> stem_bufs(const Plan& p, unsigned char* ws) {
  const Unit& u0 = p.units[0];
  StemBufs<T> b;
  b.img4 = reinterpret_cast<T*>(ws + p.off_img4);
  b.wv = reinterpret_cast<const T*>(ws + p.off_wf) + u0.wf_off;
  b.x0 = reinterpret_cast<T*>(ws + u0.x_off);
  b.pool = reinterpret_cast<T*>(ws + p.off_pool);
  b.idx = ws + p.off_idx;
  b.coef = reinterpret_cast<float*>(ws + u0.coef_off);
  b.ssum = reinterpret_cast<float*>(ws + p.off_stat);
  b.ssq = reinterpret_cast<float*>(ws + p.off_stat + p.stat_bytes);
  b.red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  b.coefbwd = reinterpret_cast<float*>(ws + p.off_coefbwd);
  b.partial = reinterpret_cast<float*>(ws + p.off_partial);
  b.dx0 = BwdBufs<T>(p, ws).stem_dx0;
  b.slab = wgrad_slab_at(ws, p.off_slab, p.slab_bytes);
  b.dwv = reinterpret_cast<float*>(ws + p.off_dwv);
  return b;
}

// Inference: eval-mode BatchNorm is folded into the convolutions -- the staged weights carry gamma/sqrt(var+eps)
// (stage_weights above), the conv epilogue adds the shift, the residual and the ReLU, so no BatchNorm pass and
// no raw conv output exists (loadImageModelClassifier.py backbones under model.eval(): model_metrics.py:50-62).
template <typename T>
int forward_eval(Plan& p, const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                 float* features, hipStream_t st, bool reuse_table) {
  const float eps = 1e-5f;
  T* wf = reinterpret_cast<T*>(ws + p.off_wf);
  int rc;
  if (!reuse_table) PROF(K_BN_FWD, 0.0, 0.0, bn_eval_table(p.table_dev, (int)p.units.size(), p.red_C, params, buffers, ws, eps, st));
  auto shift_of = [&](const Unit& u) { return BnCoef(reinterpret_cast<float*>(ws + u.coef_off), u.s.Cout).shift; };
  // stem: the 7x7 conv keeps its own BN + ReLU + max-pool kernel; its coefficients are in the table above
  if ((rc = stem_forward<T>(stem_bufs<T>(p, ws), p.sg, image, norm6, StemBn(), &p.prof, st))) return rc;
  for (Block& b : p.blocks) {
    const T* in = reinterpret_cast<const T*>(ws + b.in_off);
    const T* cur = in;
    const int nu = (int)b.units.size();
    const T* skip = in;
    if (b.ds >= 0) {
      Unit& d = p.units[b.ds];
      FwdFuse f; f.bias = shift_of(d);
      T* xd = reinterpret_cast<T*>(ws + d.x_off);
      PROF(K_CONV_FWD, conv_flops(d.s), conv_bytes(d.s, sizeof(T)), launch_conv_fwd<T>(d.s, in, wf + d.wf_off, xd, nullptr, nullptr, st, &f));
      skip = xd;
    }
    for (int i = 0; i < nu; ++i) {
      Unit& u = p.units[b.units[i]];
      T* y = reinterpret_cast<T*>(ws + u.y_off);
      FwdFuse f; f.bias = shift_of(u); f.relu = true;
      if (i + 1 == nu) f.addend = skip;
      PROF(K_CONV_FWD, conv_flops(u.s), conv_bytes(u.s, sizeof(T), 0), launch_conv_fwd<T>(u.s, cur, wf + u.wf_off, y, nullptr, nullptr, st, &f));
      cur = y;
    }
  }
  Unit& last = p.units[p.blocks.back().units.back()];
  return avgpool_fwd<T>(reinterpret_cast<const T*>(ws + last.y_off), p.N, last.s.OH() * last.s.OW(), last.s.Cout, features, st);
}

// g^T in, in^T in and colsum(in) of a 1x1 / stride 1 unit (launch_wgrad_gram; mode as there).  This is the one launch of the algebraic
// path that exists for bf16 only, and build_plan sets Unit::abn / fwd2p / gram_off on bf16 plans only: the one place that says so.
template <typename T>
int wgrad_gram(const ConvShape& s, const T* g, const T* in, float* slab, float* s_out, float* colsum_out, hipStream_t st, int mode = 0) {
  if constexpr (sizeof(T) == 2) return launch_wgrad_gram(s.N, s.OH(), s.OW(), s.Cin, s.Cout, g, in, slab, s_out, colsum_out, st, mode);
  else return MMSKIN_ERR_UNSUPPORTED;
}

template <typename T>
int forward_impl(Plan& p, const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                 float* features, bool training, hipStream_t st) {
  const float eps = 1e-5f, mom = 0.1f;
  T* wf = reinterpret_cast<T*>(ws + p.off_wf);
  T* wd = reinterpret_cast<T*>(ws + p.off_wd);
  float* stat_sum = reinterpret_cast<float*>(ws + p.off_stat);
  float* stat_sq = reinterpret_cast<float*>(ws + p.off_stat + p.stat_bytes);
  int rc;
  if ((rc = p.ensure_table())) return rc;
  const bool folded_eval = !training && !p.keep_raw_eval;
  const bool reuse = folded_eval && p.reuse_staged && p.staged_eval_ws == ws;
  p.staged_eval_ws = folded_eval ? ws : nullptr;
  // stage weights (stem region needs zeros in its padding taps)
  if (!reuse) HIP_CHECK_RET(hipMemsetAsync(wf + p.units[0].wf_off, 0, 64 * 256 * sizeof(T), st));
  const bool use_side = !p.prof.on;
  if (use_side && (rc = p.side.init(SIDE_SLOTS))) return rc;
  const bool stage_aside = use_side && training;   // the stem only needs its own weights: the other layers are staged beside it
  const float* fold = (training || p.keep_raw_eval) ? nullptr : buffers;
  if (stage_aside) {
    if ((rc = stage_weights<T>(p.table_dev, 1, p.max_stage_elems, params, wf, wd, training, st, fold, eps))) return rc;
    HIP_CHECK_RET(hipEventRecord(p.side.f_ready, st));
    HIP_CHECK_RET(hipStreamWaitEvent(p.side.s, p.side.f_ready, 0));
    if ((rc = stage_weights<T>(p.table_dev + 1, (int)p.units.size() - 1, p.max_stage_elems, params, wf, wd, training, p.side.s,
                               fold, eps))) return rc;
    HIP_CHECK_RET(hipEventRecord(p.side.f_staged, p.side.s));
  } else if (!reuse) {
    PROF(K_STAGE, 0.0, 0.0, stage_weights<T>(p.table_dev, (int)p.units.size(), p.max_stage_elems, params, wf, wd, training, st, fold, eps));
  }
  if (folded_eval) return forward_eval<T>(p, image, norm6, params, buffers, ws, features, st, reuse);

  auto bn_coeffs_on = [&](Unit& u, int stat_rows, float* ssum, float* ssq, ColScratch red, hipStream_t s2) -> int {
    const int C = u.s.Cout;
    const BnCoef k(reinterpret_cast<float*>(ws + u.coef_off), C);
    ProfScope scope(&p.prof, K_BN_FWD, s2, 0.0, 0.0);
    if (training)
      return bn_finalize(ssum, ssq, stat_rows, C, (double)u.rows(), params + u.g_off, params + u.b_off, eps,
                         mom, buffers + u.rm_off, buffers + u.rv_off, k.scale, k.shift, k.mean, k.invstd, red, s2);
    return bn_eval_coeffs(C, params + u.g_off, params + u.b_off, buffers + u.rm_off, buffers + u.rv_off, eps, k.scale, k.shift, s2);
  };
  auto bn_coeffs = [&](Unit& u, int stat_rows) -> int {
    return bn_coeffs_on(u, stat_rows, stat_sum, stat_sq, bn_reduce_scratch(ws + p.off_red, p.red_C), st);
  };
  float* stat_b_sum = reinterpret_cast<float*>(ws + p.off_stat_b);
  float* stat_b_sq = reinterpret_cast<float*>(ws + p.off_stat_b + p.stat_bytes);

  // ---- stem
  Unit& u0 = p.units[0];
  StemBn bn0;
  bn0.gamma = params + u0.g_off; bn0.beta = params + u0.b_off; bn0.rm = buffers + u0.rm_off; bn0.rv = buffers + u0.rv_off;
  bn0.eps = eps; bn0.mom = mom; bn0.batch_stats = training;
  if ((rc = stem_forward<T>(stem_bufs<T>(p, ws), p.sg, image, norm6, bn0, &p.prof, st))) return rc;

  // ---- residual stages
  if (stage_aside) HIP_CHECK_RET(hipStreamWaitEvent(st, p.side.f_staged, 0));
  for (Block& b : p.blocks) {
    const T* in = reinterpret_cast<const T*>(ws + b.in_off);
    const T* cur = in;
    const int nu = (int)b.units.size();
    if (b.ds >= 0) {
      // the downsample conv + its BN statistics only meet the main branch at the block's final BN-apply:
      // they run on the side stream (own stat slab / reduction scratch) beside conv1..conv3
      Unit& d = p.units[b.ds];
      const hipStream_t dst = use_side ? p.side.s : st;   // (the profiled path has no side stream: main stream, main scratch)
      float* dsum = use_side ? stat_b_sum : stat_sum;
      float* dsq = use_side ? stat_b_sq : stat_sq;
      if (use_side) {
        HIP_CHECK_RET(hipEventRecord(p.side.f_ready, st));
        HIP_CHECK_RET(hipStreamWaitEvent(dst, p.side.f_ready, 0));
      }
      int nrows_d = 0;
      {
        ProfScope scope(&p.prof, K_CONV_FWD, dst, conv_flops(d.s), conv_bytes(d.s, sizeof(T)));
        if ((rc = launch_conv_fwd<T>(d.s, in, wf + d.wf_off, reinterpret_cast<T*>(ws + d.x_off), training ? dsum : nullptr,
                                     training ? dsq : nullptr, dst, nullptr, &nrows_d))) return rc;
      }
      if ((rc = bn_coeffs_on(d, nrows_d, dsum, dsq, bn_reduce_scratch(ws + (use_side ? p.off_red_b : p.off_red), p.red_C), dst))) return rc;
      if (use_side) HIP_CHECK_RET(hipEventRecord(p.side.f_done, dst));
    }
    for (int i = 0; i < nu; ++i) {
      Unit& u = p.units[b.units[i]];
      T* x = reinterpret_cast<T*>(ws + u.x_off);
      T* y = reinterpret_cast<T*>(ws + u.y_off);
      int nrows_u = 0;   // statistics row blocks this launch wrote (the launcher picks the tile height)
      const bool two_pass = training && u.fwd2p;   // (a block's final unit)
      const bool gram_pass = two_pass && u.gram_off != 0;
      if (gram_pass) {
        float* gm = reinterpret_cast<float*>(ws + u.gram_off);
        float* gcs = gm + (size_t)128 * u.s.Cin;
        PROF(K_BN_FWD, 0.0, (double)u.rows() * u.s.Cin * sizeof(T),
             wgrad_gram<T>(u.s, nullptr, cur, reinterpret_cast<float*>(ws + p.off_abn_slab2), gm, gcs, st, 2));
        const BnCoef kq(reinterpret_cast<float*>(ws + u.coef_off), u.s.Cout);
        PROF(K_BN_FWD, 0.0, 0.0, gram_stats_finalize(gm, gcs, params + u.w_off, u.s.Cout, u.s.Cin, (double)u.rows(), params + u.g_off, params + u.b_off, eps, mom,
                                                     buffers + u.rm_off, buffers + u.rv_off, kq.scale, kq.shift, kq.mean, kq.invstd, st));
        nrows_u = -1;   // coefficients done
      } else {
        PROF(K_CONV_FWD, conv_flops(u.s), conv_bytes(u.s, sizeof(T)),
             launch_conv_fwd<T>(u.s, cur, wf + u.wf_off, two_pass ? (T*)nullptr : x, training ? stat_sum : nullptr,
                                training ? stat_sq : nullptr, st, nullptr, &nrows_u));
      }
      if (nrows_u >= 0 && (rc = bn_coeffs(u, nrows_u))) return rc;
      const int C = u.s.Cout;
      const BnCoef k(reinterpret_cast<float*>(ws + u.coef_off), C);
      if (two_pass) {
        // second pass: the conv again with scale * acc + shift + identity + ReLU (+ the mask byte) in its epilogue -- the raw output
        // (the block's widest tensor) is neither written nor read: 2T + 2t bytes instead of 4T + t, and the normalisation multiplies the
        // fp32 accumulator, not a bf16-rounded copy of it
        FwdFuse f2; f2.mul = k.scale; f2.bias = k.shift; f2.addend = in; f2.relu = true; f2.mask_out = ws + b.mask_off;
        // (class accounting: the recomputed MACs are overhead, not algorithmic work -- the layer's FLOPs were counted with the first pass)
        PROF(K_CONV_FWD, gram_pass ? conv_flops(u.s) : 0.0, conv_bytes(u.s, sizeof(T), 0) + (double)u.rows() * C * sizeof(T), launch_conv_fwd<T>(u.s, cur, wf + u.wf_off, y, nullptr, nullptr, st, &f2));
      } else if (i + 1 < nu) {
        PROF(K_BN_FWD, 0.0, 2.0 * u.rows() * C * sizeof(T), bn_apply<T>(x, nullptr, k.scale, k.shift, nullptr, nullptr, y, u.rows(), C, true, st));
      } else if (b.ds >= 0) {
        Unit& d = p.units[b.ds];
        const BnCoef kd(reinterpret_cast<float*>(ws + d.coef_off), C);
        if (use_side) HIP_CHECK_RET(hipStreamWaitEvent(st, p.side.f_done, 0));
        PROF(K_BN_FWD, 0.0, 3.0 * u.rows() * C * sizeof(T),
             bn_apply<T>(x, reinterpret_cast<const T*>(ws + d.x_off), k.scale, k.shift, kd.scale, kd.shift, y, u.rows(), C, true, st,
                         training ? ws + b.mask_off : nullptr));
      } else {
        PROF(K_BN_FWD, 0.0, 3.0 * u.rows() * C * sizeof(T),
             bn_apply<T>(x, in, k.scale, k.shift, nullptr, nullptr, y, u.rows(), C, true, st, training ? ws + b.mask_off : nullptr));
      }
      cur = y;
    }
  }
  Unit& last = p.units[p.blocks.back().units.back()];
  return avgpool_fwd<T>(reinterpret_cast<const T*>(ws + last.y_off), p.N, last.s.OH() * last.s.OW(), last.s.Cout,
                        features, st);
}

// ------------------------------------------------------------------------------------------ backward
// The gradient of a block's output, as the step that finished the block above hands it to the block below.
//   masked_with_sums: dz is already multiplied by the block's ReLU mask (Block::mask_off bits), and conv1's data gradient of the block
//   above, which wrote it, left the BatchNorm-backward partial sums of the block's final unit in `partial` (sum dz, sum dz * x against
//   that unit's raw output x; a two-pass unit has no x and takes the second sum from its weight-gradient GEMM instead) and of its
//   downsample branch in `partial_b` (against the branch's raw output), sum_rows rows each.
//   Otherwise dz is the plain gradient dy: the last block's, which arrives from the average pool.
template <typename T>
struct BlockGrad {
  SlotBuf<T> dz;
  bool masked_with_sums;
  int sum_rows;
};

// The folded data-gradient weights [cA (.) W ; Q] and bias r that abn_prep writes and the algebraic data gradient reads: one set for a
// block's conv3, one for a stride-1 downsample convolution (both are live between the block's tail and its block-input step).
enum AbnSet { ABN_CONV3, ABN_DS };

template <typename T>
struct ResNetBackward {
  Plan& p;
  const float* params;
  unsigned char* ws;
  float* grads;
  hipStream_t st;
  const bool use_side;   // weight gradients on the side stream (off on the profiled path)
  const BwdBufs<T> B;
  const WgradSlab slab;
  const ColScratch red;
  int dxi = 0;           // which of B.dX holds the current dX

  ResNetBackward(Plan& plan, const float* params_, unsigned char* ws_, float* grads_, hipStream_t st_)
      : p(plan), params(params_), ws(ws_), grads(grads_), st(st_), use_side(!plan.prof.on), B(plan, ws_),
        slab(wgrad_slab_at(ws_, plan.off_slab, plan.slab_bytes)), red(bn_reduce_scratch(ws_ + plan.off_red, plan.red_C)) {}

  template <typename U>
  U* at(size_t off) const { return reinterpret_cast<U*>(ws + off); }
  T* wd(const Unit& u) const { return at<T>(p.off_wd) + u.wd_off; }
  float* partial() const { return at<float>(p.off_partial); }
  float* partial_b() const { return at<float>(p.off_partial_b); }
  BnCoef coef_of(const Unit& u) const { return BnCoef(at<float>(u.coef_off), u.s.Cout); }
  BnBwdCoef bwd_coef(const Unit& u) const { return BnBwdCoef(at<float>(p.off_coefbwd), u.s.Cout); }
  const T* x_of(const Unit& u) const { return at<const T>(u.x_off); }
  const T* input_of(const Block& b, int i) const { return at<const T>(i == 0 ? b.in_off : p.units[b.units[i - 1]].y_off); }
  const SlotBuf<T>& dX() const { return B.dX[dxi]; }
  bool algebraic(const Unit& u, const BlockGrad<T>& bg) const { return u.abn && bg.masked_with_sums; }
  int acquire(int slot) { return p.side.acquire(slot, st, use_side); }
  int next_dX() {   // the next dX goes to the other buffer of the pair: the weight gradient handed the current one may still be reading it
    dxi ^= 1;
    return acquire(dX().slot);
  }

  // ---- BatchNorm backward of unit u, three forms
  // from dy: reduce -> finalize -> apply with the ReLU mask taken from the block output y; fills dx and, when given, dz (the masked dy)
  int bn_from_dy(Unit& u, const T* dy, const T* y, T* dx, T* dz) {
    return bn_backward<T>(dy, x_of(u), y, MASK_FROM_Y, u.rows(), u.s.Cout, coef_of(u), params + u.g_off, grads + u.g_off, grads + u.b_off,
                          bwd_coef(u), partial(), red, dx, dz, &p.prof, 7.0 * u.rows() * u.s.Cout * sizeof(T), st);
  }
  // from sums: dz is masked already and the data gradient that wrote it left its partial sums: finalize + one apply pass.
  // dx == nullptr: finalize only (gamma / beta gradients and cA, cB, cC); sum_dz_x: the second sum from elsewhere (two-pass units)
  int bn_from_sums(Unit& u, const T* dz, const float* part, int nrows, T* dx, const float* sum_dz_x = nullptr) {
    return bn_backward_from_sums<T>(dz, x_of(u), part, nrows, u.rows(), u.s.Cout, coef_of(u), params + u.g_off, grads + u.g_off,
                                    grads + u.b_off, bwd_coef(u), red, dx, &p.prof, dx ? 3.0 * u.rows() * u.s.Cout * sizeof(T) : 0.0, st, -1,
                                    false, sum_dz_x);
  }
  // algebraic (abn.hip): finalize without the apply pass, then fold cA, cB, cC into data-gradient weights of buffer set k; u keeps a
  // copy of the coefficients for its weight gradient.  A two-pass unit stored no x: its g^T y runs first, on this stream (the sum of
  // g x is W . (g^T y) row by row), and its weight gradient is finished here from the same product.
  int bn_algebraic(Unit& u, const BlockGrad<T>& bg, const float* part, AbnSet k, const T* uin) {
    int rc;
    const T* g = bg.dz.p;
    float* S2 = at<float>(p.off_abn_S2);
    float* coef_copy = at<float>(u.abn_coef_off);
    const float* sgx = nullptr;
    if (u.fwd2p) {
      PROF(K_WGRAD, conv_flops(u.s), conv_bytes(u.s, sizeof(T)),
           wgrad_gram<T>(u.s, g, uin, at<float>(p.off_abn_slab2), S2, at<float>(p.off_abn_cs2), st, u.gram_off ? 1 : 0));
      if ((rc = abn_sgx(S2, params + u.w_off, u.s.Cout, u.s.Cin, at<float>(p.off_abn_sgx), st))) return rc;
      sgx = at<float>(p.off_abn_sgx);
    }
    if ((rc = bn_from_sums(u, g, part, bg.sum_rows, nullptr, sgx))) return rc;
    const BnBwdCoef c = bwd_coef(u);
    if ((rc = abn_prep(params + u.w_off, c.cA, c.cB, c.cC, u.s.Cout, u.s.Cin, at<bf16_t>(k == ABN_DS ? p.off_abn_wd2 : p.off_abn_wd),
                       at<float>(k == ABN_DS ? p.off_abn_bias2 : p.off_abn_bias), coef_copy, st))) return rc;
    if (!u.fwd2p) return MMSKIN_OK;
    const float* gkept = u.gram_off ? at<const float>(u.gram_off) : nullptr;   // y^T y | colsum(y) from the forward pass
    return abn_wgrad_finalize(S2, gkept ? gkept + (size_t)128 * u.s.Cin : at<const float>(p.off_abn_cs2), params + u.w_off, coef_copy, u.s.Cout,
                              u.s.Cin, grads + u.w_off, st, gkept);
  }
  // ... and its data gradient din = [g | y] [cA (.) W ; Q] + r from set k: no dz in memory.  f: the epilogue of the unit below, if any
  int dgrad_algebraic(const Unit& u, AbnSet k, const T* g, const T* uin, T* din, DgradFuse& f, int extra_in_shaped) {
    int rc;
    f.in2 = uin; f.k2 = u.s.Cin; f.bias = at<const float>(k == ABN_DS ? p.off_abn_bias2 : p.off_abn_bias);
    PROF(K_CONV_DGRAD, conv_flops(u.s), conv_bytes(u.s, sizeof(T), extra_in_shaped),
         launch_conv_dgrad<T>(u.s, g, at<const T>(k == ABN_DS ? p.off_abn_wd2 : p.off_abn_wd), din, (const T*)nullptr, st, &f));
    return MMSKIN_OK;
  }

  // ---- weight gradients: handed to the side stream with the buffer they read
  int wgrad_async(Unit& u, const SlotBuf<T>& dx, const T* uin) {
    return p.side.run(dx.slot, st, use_side, [&](hipStream_t wst) {
      ProfScope scope(&p.prof, K_WGRAD, wst, conv_flops(u.s), conv_bytes(u.s, sizeof(T)));
      return launch_conv_wgrad<T>(u.s, dx.p, uin, slab, grads + u.w_off, wst);
    });
  }
  // algebraic: dW = cA (.) (g^T y) + cB (.) (W (y^T y)) + cC (x) colsum(y), reading the block-output gradient g itself
  int wgrad_abn_async(Unit& u, const SlotBuf<T>& g, const T* uin) {
    return p.side.run(g.slot, st, use_side, [&](hipStream_t wst) {
      float* S_out = at<float>(p.off_abn_S);
      float* cs_out = at<float>(p.off_abn_cs);
      ProfScope scope(&p.prof, K_WGRAD, wst, conv_flops(u.s), conv_bytes(u.s, sizeof(T)));
      if (int r = wgrad_gram<T>(u.s, g.p, uin, slab.p, S_out, cs_out, wst)) return r;
      return abn_wgrad_finalize(S_out, cs_out, params + u.w_off, at<const float>(u.abn_coef_off), u.s.Cout, u.s.Cin, grads + u.w_off, wst);
    });
  }
  int wgrad_of(const Block& b, int i, const BlockGrad<T>& bg) {   // unit i of the block, from the current dX
    Unit& u = p.units[b.units[i]];
    if (!algebraic(u, bg)) return wgrad_async(u, dX(), input_of(b, i));
    return u.fwd2p ? MMSKIN_OK : wgrad_abn_async(u, bg.dz, input_of(b, i));   // (two-pass units: finished in bn_algebraic)
  }

  // ---- the three steps of a block
  // tail: BatchNorm backward of the block's final unit (dx into the next dX, or algebraic set ABN_CONV3) and of its downsample branch
  // (B.dXd, or ABN_DS).  *dz_final: the masked gradient of the block output, the residual addend of a block without a branch.
  int tail(const Block& b, const BlockGrad<T>& bg, const T** dz_final) {
    int rc;
    const int nu = (int)b.units.size();
    Unit& ul = p.units[b.units[nu - 1]];
    Unit* d = b.ds >= 0 ? &p.units[b.ds] : nullptr;
    if ((rc = next_dX())) return rc;
    if (d && (rc = acquire(B.dXd.slot))) return rc;
    if (!bg.masked_with_sums) {
      ARG_CHECK(!ul.fwd2p, "backbone_backward: a two-pass unit stores no raw output, its BatchNorm backward cannot start from dy");
      const T* out = at<const T>(ul.y_off);
      *dz_final = B.dZ;
      if ((rc = bn_from_dy(ul, bg.dz.p, out, dX().p, d ? nullptr : B.dZ))) return rc;
      return d ? bn_from_dy(*d, bg.dz.p, out, B.dXd.p, nullptr) : MMSKIN_OK;
    }
    *dz_final = bg.dz.p;
    if (ul.abn) rc = bn_algebraic(ul, bg, partial(), ABN_CONV3, input_of(b, nu - 1));
    else rc = bn_from_sums(ul, bg.dz.p, partial(), bg.sum_rows, dX().p);
    if (rc || !d) return rc;
    if (d->abn) return bn_algebraic(*d, bg, partial_b(), ABN_DS, nullptr);
    return bn_from_sums(*d, bg.dz.p, partial_b(), bg.sum_rows, B.dXd.p);
  }

  // unit i > 0: its weight gradient is handed off, its data gradient writes the gradient of unit i-1's ReLU output into B.dY -- the
  // epilogue applies that ReLU's mask and takes unit i-1's BatchNorm-backward sums -- and unit i-1's BatchNorm backward makes the next dX
  int unit(const Block& b, int i, const BlockGrad<T>& bg) {
    int rc;
    Unit& u = p.units[b.units[i]];
    Unit& up = p.units[b.units[i - 1]];
    if ((rc = wgrad_of(b, i, bg))) return rc;
    DgradFuse f;
    f.x = ws + up.x_off; f.scale = coef_of(up).scale; f.shift = coef_of(up).shift; f.partial = partial();
    if (algebraic(u, bg)) {
      if ((rc = dgrad_algebraic(u, ABN_CONV3, bg.dz.p, input_of(b, i), B.dY, f, 1))) return rc;
    } else {
      PROF(K_CONV_DGRAD, conv_flops(u.s), conv_bytes(u.s, sizeof(T), 1), launch_conv_dgrad<T>(u.s, dX().p, wd(u), B.dY, (const T*)nullptr, st, &f));
    }
    if ((rc = next_dX())) return rc;
    return bn_from_sums(up, B.dY, partial(), f.rows_written, dX().p);
  }

  // block input: the downsample branch's data gradient (algebraic, compact stride-2 or dense) and conv1's on top of it -- or on top of
  // dz_final -- into gin, with the mask and the BatchNorm-backward sums of the block below in its epilogue.  Returns what that block takes.
  int block_input(int bi, const BlockGrad<T>& bg, const T* dz_final, const SlotBuf<T>& gin, BlockGrad<T>* below) {
    int rc;
    const Block& b = p.blocks[bi];
    Unit& u = p.units[b.units[0]];
    const T* in = input_of(b, 0);
    if ((rc = wgrad_of(b, 0, bg))) return rc;
    if ((rc = acquire(gin.slot))) return rc;   // an algebraic weight gradient of the block above may still be reading it
    const T* addend = dz_final;
    if (b.ds >= 0) {
      Unit& d = p.units[b.ds];
      addend = b.ds_compact ? B.ds_addend : gin.p;   // conv1's data gradient accumulates on top (in place unless the branch's gradient is compact)
      if (algebraic(d, bg)) {   // stride-1 downsample convolution, as conv3
        if ((rc = wgrad_abn_async(d, bg.dz, in))) return rc;
        DgradFuse fd;
        if ((rc = dgrad_algebraic(d, ABN_DS, bg.dz.p, in, gin.p, fd, 0))) return rc;
      } else {
        if ((rc = wgrad_async(d, B.dXd, in))) return rc;
        // Stride-2 1x1 downsample: its data gradient lives on the even pixels only.  Compact: the dense GEMM over the pixels the
        // convolution read (a 1x1 / stride 1 launch on the OH x OW grid) into B.ds_addend, and conv1's data gradient adds it at the even
        // pixels in its epilogue: no zero fill of the other three quarters (154 + 77 + 38 MB written, then read back as the addend).
        ConvShape dc = d.s;
        if (b.ds_compact) { dc.H = d.s.OH(); dc.W = d.s.OW(); dc.stride = 1; }
        PROF(K_CONV_DGRAD, conv_flops(d.s), conv_bytes(d.s, sizeof(T)),
             launch_conv_dgrad<T>(dc, B.dXd.p, wd(d), b.ds_compact ? B.ds_addend : gin.p, (const T*)nullptr, st));
      }
    }
    DgradFuse f;
    DgradFuse* fp = nullptr;
    if (bi > 0) {   // gin is the gradient of the block below's output: fuse that block's mask and final BatchNorm-backward sums
      const Block& pb = p.blocks[bi - 1];
      const Unit& pu = p.units[pb.units.back()];
      f.mask_bits = ws + pb.mask_off; f.x = pu.fwd2p ? nullptr : ws + pu.x_off; f.partial = partial();   // two-pass unit: no raw output to take sums against
      if (pb.ds >= 0) { f.x2 = ws + p.units[pb.ds].x_off; f.partial_b = partial_b(); }
      f.addend_s2 = b.ds_compact;
      fp = &f;
    }
    PROF(K_CONV_DGRAD, conv_flops(u.s), conv_bytes(u.s, sizeof(T), 1 + (fp ? (f.x2 ? 3 : 2) : 0)),
         launch_conv_dgrad<T>(u.s, dX().p, wd(u), gin.p, addend, st, fp));
    *below = BlockGrad<T>{gin, fp != nullptr, f.rows_written};
    return MMSKIN_OK;
  }

  // the stem: g = gradient of the pooled activation.  Its BatchNorm backward touches none of the buffers the side stream's
  // weight-gradient GEMMs are still reading (dX ring, forward activations) or writing (slab), so it runs on the main stream BESIDE the
  // tail of layer1's weight gradients; the stem's own needs the slab and queues behind them on the side stream.
  int stem(const T* g) {
    int rc;
    Unit& u0 = p.units[0];
    const StemBufs<T> sb = stem_bufs<T>(p, ws);
    if ((rc = stem_backward<T>(sb, p.sg, g, params + u0.g_off, grads + u0.g_off, grads + u0.b_off, stem_sums_pooled(), &p.prof,
                               3.5 * u0.rows() * 64 * sizeof(T), st))) return rc;
    if ((rc = p.side.run(SLOT_DX0, st, use_side, [&](hipStream_t wst) { return stem_wgrad<T>(sb, p.sg, grads + u0.w_off, &p.prof, wst); }))) return rc;
    return acquire(SLOT_DX0);   // final join: everything the side stream was given has finished before backward's last event
  }

  int run(const float* dfeat) {
    int rc;
    const Unit& last = p.units[p.blocks.back().units.back()];
    BlockGrad<T> bg = {B.G[0], false, 0};
    if ((rc = avgpool_bwd<T>(dfeat, p.N, last.s.OH() * last.s.OW(), last.s.Cout, bg.dz.p, st))) return rc;
    if (use_side && (rc = p.side.init(SIDE_SLOTS))) return rc;
    p.side.begin_backward();
    int gi = 0;   // B.G[gi] holds the gradient of the current block's output
    for (int bi = (int)p.blocks.size() - 1; bi >= 0; --bi) {
      const Block& b = p.blocks[bi];
      const T* dz_final;
      if ((rc = tail(b, bg, &dz_final))) return rc;
      for (int i = (int)b.units.size() - 1; i > 0; --i)
        if ((rc = unit(b, i, bg))) return rc;
      BlockGrad<T> below;
      if ((rc = block_input(bi, bg, dz_final, B.G[gi ^= 1], &below))) return rc;
      bg = below;
      if (b.seg_done >= 0 && (rc = p.segment_done(b.seg_done, st, use_side))) return rc;
    }
    if ((rc = stem(bg.dz.p))) return rc;
    return p.segment_done((int)p.segments.size() - 1, st, false);
  }
};

int Plan::forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                  float* features, bool training, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return forward_impl<decltype(t)>(*this, image, norm6, params, buffers, ws, features, training, st); });
}
int Plan::backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return ResNetBackward<decltype(t)>(*this, params, ws, grads, st).run(dfeat); });
}
// torchvision's last nn.Conv2d in module order is the final block's last conv (layerN.k.conv3 / conv2)
int Plan::last_conv_shape(int* C, int* OH, int* OW) const {
  const Unit& u = units[blocks.back().units.back()];
  *C = u.s.Cout; *OH = u.s.OH(); *OW = u.s.OW();
  return MMSKIN_OK;
}
int Plan::last_conv_export(const unsigned char* ws, float* x_nchw, hipStream_t st) {
  const Unit& u = units[blocks.back().units.back()];
  if (dtype == 1) return nhwc_to_nchw<bf16_t>(reinterpret_cast<const bf16_t*>(ws + u.x_off), N, u.s.Cout, u.s.OH(), u.s.OW(), x_nchw, st);
  return nhwc_to_nchw<float>(reinterpret_cast<const float*>(ws + u.x_off), N, u.s.Cout, u.s.OH(), u.s.OW(), x_nchw, st);
}
int Plan::last_conv_grad(const float* dfeat, const unsigned char* ws, float* dx_nchw, hipStream_t st) {
  const Unit& u = units[blocks.back().units.back()];
  const float* scale = reinterpret_cast<const float*>(ws + u.coef_off);
  const int HW = u.s.OH() * u.s.OW();
  if (dtype == 1) return gap_relu_bn_grad<bf16_t>(dfeat, reinterpret_cast<const bf16_t*>(ws + u.y_off), scale, N, HW, u.s.Cout, dx_nchw, st);
  return gap_relu_bn_grad<float>(dfeat, reinterpret_cast<const float*>(ws + u.y_off), scale, N, HW, u.s.Cout, dx_nchw, st);
}
int Plan::unit_info(int index, std::string* name, int64_t* info12) const {
  const Unit& u = units[index];
  // the conv weight is the unit's first parameter; find its name through the param table
  for (const TensorInfo& t : params)
    if (t.offset == u.w_off && name) *name = t.name;
  const int64_t v[12] = {(int64_t)u.x_off, (int64_t)u.y_off, (int64_t)u.coef_off, (int64_t)u.rows(), u.s.Cout,
                         u.s.OH(), u.s.OW(), u.s.Cin, u.s.H, u.s.W, (int64_t)off_pool, (int64_t)off_scratch[0]};
  for (int i = 0; i < 12; ++i) info12[i] = v[i];
  return MMSKIN_OK;
}

int Plan::unit_flags(int index, int* flags) const {
  const Unit& u = units[index];
  int f = (u.abn ? MMSKIN_UNIT_ABN : 0) | (u.fwd2p ? MMSKIN_UNIT_FWD2P : 0) | (u.gram_off ? MMSKIN_UNIT_GRAM : 0);
  for (const Block& b : blocks) {
    if (b.ds != index && std::find(b.units.begin(), b.units.end(), index) == b.units.end()) continue;
    if (&b == &blocks.back()) f |= MMSKIN_UNIT_LAST_BLOCK;
    if (b.ds == index) f |= MMSKIN_UNIT_DS | (b.ds_compact ? MMSKIN_UNIT_DS_COMPACT : 0);
  }
  *flags = f;
  return MMSKIN_OK;
}

}  // namespace

PlanBase* make_resnet_plan(int arch, int N, int H, int W, int dtype, int* rc) {
  return make_plan<Plan>(N, H, W, dtype, rc, [arch](Plan& p) { p.arch = arch; return build_plan(p); });
}

// ------------------------------------------------------------------------------------------ C ABI

struct mmskin_backbone { PlanBase* plan = nullptr; };

extern "C" {

int mmskin_backbone_create(const char* arch, int batch, int height, int width, int dtype, mmskin_backbone_t* out) {
  ARG_CHECK(arch && out, "backbone_create: null argument");
  int a = 0;
  if (!strcmp(arch, "resnet-18")) a = 18;
  else if (!strcmp(arch, "resnet-50")) a = 50;
  else if (!strcmp(arch, "densenet169")) a = 169;
  else if (!strcmp(arch, "densenet169-features")) a = 1690;   // norm5 feature map, no ReLU / pool (MDNet)
  else if (!strcmp(arch, "vgg16-features")) a = 16;           // vgg16().features + avgpool -> [N][512][7][7]
  else if (!strcmp(arch, "mobilenet-v2")) a = 2;
  else if (!strcmp(arch, "efficientnet-b0")) a = 100;
  else if (!strcmp(arch, "efficientnet-b7")) a = 107;
  else if (!strncmp(arch, "dynamic-cnn/", 12)) a = 3;         // configured NAS trunk: the string carries filters / layers / pooling / kernel
  else { mmskin_set_error("backbone_create: Backbone '%s' has no HIP plan", arch); return MMSKIN_ERR_UNSUPPORTED; }
  ARG_CHECK(batch > 0 && height >= 32 && width >= 32, "backbone_create: bad shape %dx%dx%d", batch, height, width);
  ARG_CHECK(dtype == MMSKIN_F32 || dtype == MMSKIN_BF16, "backbone_create: dtype %d", dtype);
  int rc = MMSKIN_OK;
  PlanBase* p = (a == 169 || a == 1690) ? make_densenet_plan(batch, height, width, dtype, a == 1690, &rc)
                : a == 16               ? make_vgg_plan(batch, height, width, dtype, &rc)
                : a == 3                ? make_dynamic_cnn_plan(arch, batch, height, width, dtype, &rc)
                : a == 2                ? make_mobilenet_plan(batch, height, width, dtype, &rc)
                : a >= 100              ? make_efficientnet_plan(a - 100, batch, height, width, dtype, &rc)
                                        : make_resnet_plan(a, batch, height, width, dtype, &rc);
  if (!p) return rc ? rc : MMSKIN_ERR_ARG;
  mmskin_backbone* h = new mmskin_backbone();
  h->plan = p;
  *out = h;
  return MMSKIN_OK;
}

void mmskin_backbone_destroy(mmskin_backbone_t h) {
  if (!h) return;
  delete h->plan;
  delete h;
}

int mmskin_backbone_num_tensors(mmskin_backbone_t h, int kind) {
  return (int)(kind == 0 ? h->plan->params.size() : h->plan->buffers.size());
}

int mmskin_backbone_tensor_info(mmskin_backbone_t h, int kind, int index, char* name, int name_cap,
                                int64_t* offset, int64_t* numel, int* ndim, int64_t* shape4) {
  const std::vector<TensorInfo>& v = kind == 0 ? h->plan->params : h->plan->buffers;
  ARG_CHECK(index >= 0 && index < (int)v.size(), "tensor_info: index %d out of range", index);
  const TensorInfo& t = v[index];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (ndim) *ndim = t.ndim;
  if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
  return MMSKIN_OK;
}

int64_t mmskin_backbone_param_numel(mmskin_backbone_t h) { return h->plan->param_numel; }
int64_t mmskin_backbone_buffer_numel(mmskin_backbone_t h) { return h->plan->buffer_numel; }
int64_t mmskin_backbone_workspace_bytes(mmskin_backbone_t h) { return (int64_t)h->plan->ws_bytes; }
int mmskin_backbone_feature_dim(mmskin_backbone_t h) { return h->plan->feat_dim; }
int mmskin_backbone_feature_hw(mmskin_backbone_t h, int* out_h, int* out_w) {
  ARG_CHECK(h && out_h && out_w, "backbone_feature_hw: null argument");
  *out_h = h->plan->out_h; *out_w = h->plan->out_w;
  return MMSKIN_OK;
}

int mmskin_backbone_profile_enable(mmskin_backbone_t h, int on) {
  h->plan->prof.on = on != 0;
  h->plan->prof.reset();
  return MMSKIN_OK;
}

int mmskin_backbone_profile_read(mmskin_backbone_t h, double* ms7, double* flops7, double* bytes7, int64_t* launches7) {
  Profiler& pr = h->plan->prof;
  HIP_CHECK_RET(hipDeviceSynchronize());
  for (int c = 0; c < K_NCLASS; ++c) { ms7[c] = 0; flops7[c] = pr.flops[c]; bytes7[c] = pr.bytes[c]; launches7[c] = 0; }
  for (size_t i = 0; i < pr.cls.size(); ++i) {
    float ms = 0.f;
    HIP_CHECK_RET(hipEventElapsedTime(&ms, pr.pool[2 * i], pr.pool[2 * i + 1]));
    ms7[pr.cls[i]] += ms;
    launches7[pr.cls[i]] += 1;
  }
  pr.reset();
  return MMSKIN_OK;
}

int mmskin_backbone_num_units(mmskin_backbone_t h) { return h->plan->num_units(); }

int mmskin_backbone_unit_info(mmskin_backbone_t h, int index, char* name, int name_cap, int64_t* info12) {
  ARG_CHECK(index >= 0 && index < h->plan->num_units(), "unit_info: index %d out of range", index);
  std::string nm;
  int rc = h->plan->unit_info(index, &nm, info12);
  if (rc) return rc;
  if (name && name_cap > 0) { strncpy(name, nm.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  return MMSKIN_OK;
}

int mmskin_backbone_unit_flags(mmskin_backbone_t h, int index, int* flags) {
  ARG_CHECK(h && flags, "backbone_unit_flags: null argument");
  if (h->plan->num_units() == 0) { mmskin_set_error("backbone_unit_flags: this plan reports no units"); return MMSKIN_ERR_UNSUPPORTED; }
  ARG_CHECK(index >= 0 && index < h->plan->num_units(), "backbone_unit_flags: index %d out of range", index);
  int rc = h->plan->unit_flags(index, flags);
  if (rc == MMSKIN_ERR_UNSUPPORTED) mmskin_set_error("backbone_unit_flags: this plan exports no unit flags");
  return rc;
}

int mmskin_backbone_forward(mmskin_backbone_t h, const float* image_nchw, const float* params, float* buffers,
                            void* workspace, float* features, int training, void* stream) {
  ARG_CHECK(h && image_nchw && params && (buffers || h->plan->buffer_numel == 0) && workspace && features, "backbone_forward: null argument");
  return h->plan->forward(image_nchw, nullptr, params, buffers, (unsigned char*)workspace, features, training != 0,
                          (hipStream_t)stream);
}

int mmskin_backbone_forward_u8(mmskin_backbone_t h, const uint8_t* image_nhwc, const float* mean_std6, const float* params,
                               float* buffers, void* workspace, float* features, int training, void* stream) {
  ARG_CHECK(h && image_nhwc && mean_std6 && params && (buffers || h->plan->buffer_numel == 0) && workspace && features, "backbone_forward_u8: null argument");
  return h->plan->forward(image_nhwc, mean_std6, params, buffers, (unsigned char*)workspace, features, training != 0,
                          (hipStream_t)stream);
}

int mmskin_backbone_set_option(mmskin_backbone_t h, const char* key, int value) {
  ARG_CHECK(h && key, "backbone_set_option: null argument");
  if (!strcmp(key, "keep_raw_eval")) { h->plan->keep_raw_eval = value != 0; return MMSKIN_OK; }
  if (!strcmp(key, "reuse_staged")) { h->plan->reuse_staged = value != 0; return MMSKIN_OK; }
  mmskin_set_error("backbone_set_option: unknown option '%s'", key);
  return MMSKIN_ERR_ARG;
}
int mmskin_backbone_num_grad_segments(mmskin_backbone_t h, int* count) {
  ARG_CHECK(h && count, "backbone_num_grad_segments: null argument");
  *count = (int)h->plan->segments.size();   // 0: this plan reports no segments (all-reduce the arena after backward)
  return MMSKIN_OK;
}
int mmskin_backbone_grad_segment(mmskin_backbone_t h, int index, int64_t* offset, int64_t* numel) {
  ARG_CHECK(h && offset && numel, "backbone_grad_segment: null argument");
  ARG_CHECK(index >= 0 && index < (int)h->plan->segments.size(), "backbone_grad_segment: index %d", index);
  *offset = h->plan->segments[index].offset;
  *numel = h->plan->segments[index].numel;
  return MMSKIN_OK;
}
int mmskin_backbone_wait_grad_segment(mmskin_backbone_t h, int index, void* stream) {
  ARG_CHECK(h, "backbone_wait_grad_segment: null argument");
  ARG_CHECK(index >= 0 && index < (int)h->plan->segments.size(), "backbone_wait_grad_segment: index %d", index);
  int rc = h->plan->segment_wait(index, (hipStream_t)stream);
  if (rc == MMSKIN_ERR_ARG) mmskin_set_error("backbone_wait_grad_segment: no backward has been enqueued on this plan yet");
  return rc;
}
int mmskin_backbone_set_pointer(mmskin_backbone_t h, const char* key, const void* device_ptr) {
  ARG_CHECK(h && key, "backbone_set_pointer: null argument");
  int rc = h->plan->set_pointer(key, device_ptr);
  if (rc) mmskin_set_error("backbone_set_pointer: '%s' is not a pointer this plan takes", key);
  return rc;
}
int mmskin_backbone_last_conv_shape(mmskin_backbone_t h, int* C, int* OH, int* OW) {
  ARG_CHECK(h && C && OH && OW, "backbone_last_conv_shape: null argument");
  int rc = h->plan->last_conv_shape(C, OH, OW);
  if (rc == MMSKIN_ERR_UNSUPPORTED) mmskin_set_error("backbone_last_conv_*: this plan has no Grad-CAM export");
  return rc;
}
int mmskin_backbone_last_conv_export(mmskin_backbone_t h, const void* workspace, float* x_nchw, void* stream) {
  ARG_CHECK(h && workspace && x_nchw, "backbone_last_conv_export: null argument");
  ARG_CHECK(h->plan->keep_raw_eval, "backbone_last_conv_export: set option keep_raw_eval before the forward");
  int rc = h->plan->last_conv_export((const unsigned char*)workspace, x_nchw, (hipStream_t)stream);
  if (rc == MMSKIN_ERR_UNSUPPORTED) mmskin_set_error("backbone_last_conv_*: this plan has no Grad-CAM export");
  return rc;
}
int mmskin_backbone_last_conv_grad(mmskin_backbone_t h, const float* dfeatures, const void* workspace, float* dx_nchw,
                                   void* stream) {
  ARG_CHECK(h && dfeatures && workspace && dx_nchw, "backbone_last_conv_grad: null argument");
  int rc = h->plan->last_conv_grad(dfeatures, (const unsigned char*)workspace, dx_nchw, (hipStream_t)stream);
  if (rc == MMSKIN_ERR_UNSUPPORTED) mmskin_set_error("backbone_last_conv_*: this plan has no Grad-CAM export");
  return rc;
}

int mmskin_backbone_backward(mmskin_backbone_t h, const float* dfeatures, const float* params, void* workspace,
                             float* param_grads, void* stream) {
  ARG_CHECK(h && dfeatures && params && workspace && param_grads, "backbone_backward: null argument");
  return h->plan->backward(dfeatures, params, (unsigned char*)workspace, param_grads, (hipStream_t)stream);
}

}  // extern "C"
