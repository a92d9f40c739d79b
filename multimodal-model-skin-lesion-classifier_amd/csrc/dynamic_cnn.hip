// NAS DynamicCNN trunk plan executor (dynamicMultimodalmodel.py of the reference, `conv_block` + `global_pool`):
// [Conv2d(3x3, pad 1, no bias) -> GroupNorm(8, C) -> ReLU] x layers_per_block per entry of `filters`, MaxPool2d(2, 2) after each block when
// use_pooling, then AdaptiveAvgPool2d(1).  Output: [N][filters.back()] fp32.  The configuration travels in the arch string
// (dynamic-cnn/64-128-256/l2/p1/k3, grammar in include/mmskin.h).
//
// Per layer, forward: the conv writes its raw output y (no epilogue: no bias, and the ReLU follows the normalisation), gn8_stats leaves
// mean / rstd [N][8], and one apply pass writes z -- or, for a block's last layer under pooling, only the pooled tensor and its argmax bytes.
// y, mean and rstd are kept for the backward; the un-pooled z of a pooled layer never exists.  The LAST layer's activation has one consumer,
// the global average, so gn8_relu_gap_apply reduces it straight to the features and gn8_relu_gap_backward forms its gradient in registers:
// that layer stores y alone.  Backward per layer: GroupNorm + ReLU (+ pool) backward -> dy, dgamma, dbeta; weight gradient against the
// layer's input; plain data gradient (the ReLU mask belongs to the GroupNorm backward of the layer below).  The first layer is the virtual
// 3-channel first conv over the packed NHWC8 image (FirstGeom) and has no data gradient.
#include "plan.h"

namespace {

struct DcLayer {
  int Cin, Cout, H, W;        // input = output spatial size (3x3 s1 p1)
  bool pool;                  // MaxPool2d(2, 2) follows this layer
  int64_t w_off, g_off, b_off;   // flat params: conv weight, GroupNorm weight / bias
  int64_t wf, wd;             // staged
  size_t y_off;               // raw conv output, NHWC (bytes)
  size_t a_off, idx_off;      // stored activation (z, or the pooled tensor + argmax bytes); not carved for the fused tail
  size_t stat_off;            // mean [N][8] | rstd [N][8] floats
};

struct DynamicCnnPlan : PlanBase {
  std::vector<int> filters;
  int layers_per_block = 0, ksize = 0;
  bool pooling = false, fused_tail = true;
  std::vector<DcLayer> layers;
  FirstGeom fg;               // the first conv (3 -> 64) and its padded NHWC8 image
  FirstCarve first;
  int fH, fW;                 // spatial size the global average sees
  size_t off_wf, off_wd, off_gnstat, off_partial, off_sums, off_red, off_slab, slab_bytes, off_g[2];
  int red_C;                  // channels the reduction scratch at off_red was carved for

  int forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
              float* features, bool training, hipStream_t st) override;
  int backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) override;
};

// dynamic-cnn/<f0>-<f1>-...-<fn>/l<L>/p<0|1>/k<K>[/t<0|1>]; false on any other spelling
bool parse_arch(const char* arch, DynamicCnnPlan& p) {
  const char* s = arch;
  if (strncmp(s, "dynamic-cnn/", 12)) return false;
  s += 12;
  auto number = [&s](int& v) {
    if (*s < '0' || *s > '9') return false;
    long n = 0;
    int digits = 0;
    while (*s >= '0' && *s <= '9' && digits < 7) { n = n * 10 + (*s - '0'); ++s; ++digits; }
    if (*s >= '0' && *s <= '9') return false;
    v = (int)n;
    return true;
  };
  while (*s != '/') {   // an empty list is legal spelling; build refuses it
    int f;
    if (!number(f)) return false;
    p.filters.push_back(f);
    if (*s == '-') { ++s; if (*s == '/') return false; }
    else if (*s != '/') return false;
  }
  int pool = 0, tail = 1;
  if (strncmp(s, "/l", 2)) return false;
  s += 2;
  if (!number(p.layers_per_block)) return false;
  if (strncmp(s, "/p", 2)) return false;
  s += 2;
  if (!number(pool) || pool > 1) return false;
  if (strncmp(s, "/k", 2)) return false;
  s += 2;
  if (!number(p.ksize)) return false;
  if (!strncmp(s, "/t", 2)) {
    s += 2;
    if (!number(tail) || tail > 1) return false;
  }
  p.pooling = pool != 0;
  p.fused_tail = tail != 0;
  return *s == 0;
}

int build_dynamic_cnn_plan(DynamicCnnPlan& p, const char* arch) {
  ARG_CHECK(parse_arch(arch, p), "dynamic-cnn: cannot read '%s' (dynamic-cnn/<f0>-<f1>-...-<fn>/l<layers>/p<0|1>/k<kernel>)", arch);
  ARG_CHECK(!p.filters.empty(), "dynamic-cnn: filters is empty");
  ARG_CHECK(p.layers_per_block >= 1, "dynamic-cnn: layers_per_block = %d, at least 1", p.layers_per_block);
  if (p.ksize != 3) {
    mmskin_set_error("dynamic-cnn: kernel_size = %d is not supported (3 only: a 5x5 tap class exceeds the conv kernels' tap table)", p.ksize);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  for (int f : p.filters)
    if (int rc = gn8_check(p.N, f, p.H, p.W, 8, false, "dynamic-cnn: filters")) return rc;
  if (p.filters[0] != 64) {
    mmskin_set_error("dynamic-cnn: filters[0] = %d is not supported (the first conv's virtual operand is [64][4][32])", p.filters[0]);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  p.fg = FirstGeom(p.N, p.H, p.W, 1);
  if (int rc = p.fg.check("dynamic-cnn")) return rc;

  int cin = 3, h = p.H, w = p.W, idx = 0;
  for (int f : p.filters) {
    for (int l = 0; l < p.layers_per_block; ++l) {
      DcLayer c = {};
      c.Cin = cin; c.Cout = f; c.H = h; c.W = w;
      c.pool = p.pooling && l == p.layers_per_block - 1;
      const std::string conv = std::to_string(idx), gn = std::to_string(idx + 1);   // indices inside the reference's conv_block Sequential
      c.w_off = add_tensor(p.params, p.param_numel, conv + ".weight", {f, cin, 3, 3});
      c.g_off = add_tensor(p.params, p.param_numel, gn + ".weight", {f});
      c.b_off = add_tensor(p.params, p.param_numel, gn + ".bias", {f});
      p.layers.push_back(c);
      cin = f;
      idx += 3;   // conv, GroupNorm, ReLU
    }
    if (p.pooling) {
      ARG_CHECK(h >= 2 && w >= 2, "dynamic-cnn: use_pooling: the map is %dx%d in front of pool %d of a %dx%d input", h, w, idx, p.H, p.W);
      h /= 2; w /= 2;
      ++idx;
    }
  }
  p.fH = h; p.fW = w;
  p.feat_dim = p.filters.back(); p.out_h = 1; p.out_w = 1;

  int64_t wf = FirstGeom::WV_ELEMS, wd = 0;   // slot 0 of wf: the first conv's virtual operand
  for (size_t i = 1; i < p.layers.size(); ++i) {
    DcLayer& c = p.layers[i];
    stage_append(p.table_host, c.w_off, c.Cout, c.Cin, 9, 0, 0, wf, wd, p.max_stage_elems, c.wf, c.wd);
  }

  // the one carve: sizes and lays out the workspace
  const size_t es = p.esz();
  size_t cur = 0, maxact = 0, partial = 0, slab = p.first.image(cur, p.fg, es);
  p.off_wf = carve(cur, (size_t)wf * es);
  p.off_wd = carve(cur, (size_t)wd * es);
  int maxC = 64;
  for (size_t i = 0; i < p.layers.size(); ++i) {
    DcLayer& c = p.layers[i];
    const size_t rows = (size_t)p.N * c.H * c.W;
    c.y_off = carve(cur, rows * c.Cout * es);
    c.stat_off = carve(cur, (size_t)p.N * 16 * sizeof(float));
    if (!(p.fused_tail && i + 1 == p.layers.size())) {
      const size_t arow = c.pool ? (size_t)p.N * (c.H / 2) * (c.W / 2) : rows;
      c.a_off = carve(cur, arow * c.Cout * es);
      if (c.pool) c.idx_off = carve(cur, arow * c.Cout);
    }
    if (rows * c.Cout > maxact) maxact = rows * c.Cout;
    const size_t pr = gn8_bwd_partial_bytes(p.N, c.Cout);
    if (pr > partial) partial = pr;
    if (c.Cout > maxC) maxC = c.Cout;
    if (i > 0) {
      ConvShape s = {p.N, c.H, c.W, c.Cin, c.Cout, 3, 3, 1, 1};
      const size_t sb = conv_wgrad_slab_bytes(s);
      if (sb > slab) slab = sb;
    }
  }
  p.off_gnstat = carve(cur, gn8_stat_scratch_bytes(p.N));
  p.off_partial = carve(cur, partial);
  p.off_sums = carve(cur, (size_t)p.N * 16 * sizeof(float));
  p.red_C = maxC;
  p.off_red = carve(cur, bn_reduce_scratch_bytes(p.red_C));   // the column reducer's scratch for the widest 2 * C
  p.slab_bytes = slab;
  p.off_slab = carve(cur, slab);
  p.first.dwv(cur);
  p.off_g[0] = carve(cur, maxact * es);
  p.off_g[1] = carve(cur, maxact * es);
  p.ws_bytes = cur;
  return MMSKIN_OK;
}

// algorithmic bytes of the GroupNorm passes of one layer: in_elems of y, out_elems of the stored activation
double gn_fwd_bytes(size_t in_elems, size_t out_elems, bool idx, size_t es) { return (2.0 * in_elems + out_elems) * es + (idx ? (double)out_elems : 0.0); }
double gn_bwd_bytes(size_t in_elems, size_t g_elems, bool idx, size_t es) {
  return (3.0 * in_elems + 2.0 * g_elems) * es + (idx ? 2.0 * g_elems : 0.0);
}

template <typename T>
int dynamic_cnn_forward(DynamicCnnPlan& p, const void* image, const float* norm6, const float* params, unsigned char* ws, float* features,
                        hipStream_t st) {
  T* wf = reinterpret_cast<T*>(ws + p.off_wf);
  T* wd = reinterpret_cast<T*>(ws + p.off_wd);
  double* gnstat = reinterpret_cast<double*>(ws + p.off_gnstat);
  float* partial = reinterpret_cast<float*>(ws + p.off_partial);
  int rc;
  if (!p.table_host.empty()) {
    if ((rc = p.ensure_table())) return rc;
    PROF(K_STAGE, 0.0, 0.0, stage_weights<T>(p.table_dev, (int)p.table_host.size(), p.max_stage_elems, params, wf, wd, true, st));
  }
  const T* cur = nullptr;
  for (size_t i = 0; i < p.layers.size(); ++i) {
    DcLayer& c = p.layers[i];
    T* y = reinterpret_cast<T*>(ws + c.y_off);
    float* mean = reinterpret_cast<float*>(ws + c.stat_off);
    float* rstd = mean + (size_t)p.N * 8;
    const float *gamma = params + c.g_off, *beta = params + c.b_off;
    const size_t in_elems = (size_t)p.N * c.H * c.W * c.Cout;
    ConvShape s = {p.N, c.H, c.W, c.Cin, c.Cout, 3, 3, 1, 1};
    if (i == 0) {
      if ((rc = first_conv_forward<T>(p.first.bufs<T>(ws, wf, y), p.fg, image, norm6, params + c.w_off, nullptr, nullptr, nullptr, &p.prof, st))) return rc;
    } else {
      PROF(K_CONV_FWD, conv_flops(s), conv_bytes(s, sizeof(T)), launch_conv_fwd<T>(s, cur, wf + c.wf, y, nullptr, nullptr, st));
    }
    PROF(K_BN_FWD, 0.0, 0.0, gn8_stats<T>(y, p.N, c.H * c.W, c.Cout, 1e-5f, gnstat, mean, rstd, st));
    if (p.fused_tail && i + 1 == p.layers.size()) {
      PROF(K_BN_FWD, 0.0, gn_fwd_bytes(in_elems, 0, false, sizeof(T)),
           gn8_relu_gap_apply<T>(y, mean, rstd, gamma, beta, p.N, c.H, c.W, c.Cout, c.pool, partial, features, st));
      return MMSKIN_OK;
    }
    T* a = reinterpret_cast<T*>(ws + c.a_off);
    if (c.pool) {
      PROF(K_BN_FWD, 0.0, gn_fwd_bytes(in_elems, in_elems / 4, true, sizeof(T)),
           gn8_relu_pool_apply<T>(y, mean, rstd, gamma, beta, p.N, c.H, c.W, c.Cout, a, ws + c.idx_off, st));
    } else {
      PROF(K_BN_FWD, 0.0, gn_fwd_bytes(in_elems, in_elems, false, sizeof(T)),
           gn8_relu_apply<T>(y, mean, rstd, gamma, beta, p.N, c.H, c.W, c.Cout, a, st));
    }
    cur = a;
  }
  // the un-fused tail ("/t0"): the global average as a launch of its own over the stored activation
  PROF(K_STEM_MISC, 0.0, 0.0, avgpool_fwd<T>(cur, p.N, p.fH * p.fW, p.feat_dim, features, st));
  return MMSKIN_OK;
}

template <typename T>
int dynamic_cnn_backward(DynamicCnnPlan& p, const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  T* wd = reinterpret_cast<T*>(ws + p.off_wd);
  const WgradSlab slab = wgrad_slab_at(ws, p.off_slab, p.slab_bytes);
  float* partial = reinterpret_cast<float*>(ws + p.off_partial);
  float* sums = reinterpret_cast<float*>(ws + p.off_sums);
  const ColScratch red = bn_reduce_scratch(ws + p.off_red, p.red_C);
  T* G[2] = {reinterpret_cast<T*>(ws + p.off_g[0]), reinterpret_cast<T*>(ws + p.off_g[1])};
  int rc, gi = 0;   // G[gi]: the gradient at the layer's stored activation (not used by the fused tail)
  if (!p.fused_tail) PROF(K_STEM_MISC, 0.0, 0.0, avgpool_bwd<T>(dfeat, p.N, p.fH * p.fW, p.feat_dim, G[gi], st));
  for (int i = (int)p.layers.size() - 1; i >= 0; --i) {
    DcLayer& c = p.layers[i];
    const T* y = reinterpret_cast<const T*>(ws + c.y_off);
    const float* mean = reinterpret_cast<const float*>(ws + c.stat_off);
    const float* rstd = mean + (size_t)p.N * 8;
    const float *gamma = params + c.g_off, *beta = params + c.b_off;
    const size_t in_elems = (size_t)p.N * c.H * c.W * c.Cout;
    T* dy = G[gi ^ 1];
    if (p.fused_tail && i + 1 == (int)p.layers.size()) {
      PROF(K_BN_BWD, 0.0, gn_bwd_bytes(in_elems, 0, false, sizeof(T)),
           gn8_relu_gap_backward<T>(dfeat, y, mean, rstd, gamma, beta, p.N, c.H, c.W, c.Cout, c.pool, partial, sums, red, grads + c.g_off,
                                    grads + c.b_off, dy, st));
    } else {
      PROF(K_BN_BWD, 0.0, gn_bwd_bytes(in_elems, c.pool ? in_elems / 4 : in_elems, c.pool, sizeof(T)),
           gn8_relu_backward<T>(G[gi], c.pool ? ws + c.idx_off : nullptr, y, mean, rstd, gamma, beta, p.N, c.H, c.W, c.Cout, partial, sums, red,
                                grads + c.g_off, grads + c.b_off, dy, st));
    }
    gi ^= 1;
    ConvShape s = {p.N, c.H, c.W, c.Cin, c.Cout, 3, 3, 1, 1};
    if (i == 0) return first_conv_wgrad<T>(p.first.bufs<T>(ws, nullptr, nullptr, slab), p.fg, dy, grads + c.w_off, FirstGeom::COUT, &p.prof, st);
    const T* in = reinterpret_cast<const T*>(ws + p.layers[i - 1].a_off);
    PROF(K_WGRAD, conv_flops(s), conv_bytes(s, sizeof(T)), launch_conv_wgrad<T>(s, dy, in, slab, grads + c.w_off, st));
    // plain data gradient: the ReLU mask (and the pool) of the layer below are undone by its own GroupNorm backward
    PROF(K_CONV_DGRAD, conv_flops(s), conv_bytes(s, sizeof(T)), launch_conv_dgrad<T>(s, dy, wd + c.wd, G[gi ^ 1], (const T*)nullptr, st));
    gi ^= 1;
  }
  return MMSKIN_OK;
}

int DynamicCnnPlan::forward(const void* image, const float* norm6, const float* params, float* buffers, unsigned char* ws,
                            float* features, bool training, hipStream_t st) {
  (void)buffers; (void)training;   // GroupNorm keeps no running statistics: train and eval run the same kernels
  return by_dtype(dtype, [&](auto t) { return dynamic_cnn_forward<decltype(t)>(*this, image, norm6, params, ws, features, st); });
}
int DynamicCnnPlan::backward(const float* dfeat, const float* params, unsigned char* ws, float* grads, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) { return dynamic_cnn_backward<decltype(t)>(*this, dfeat, params, ws, grads, st); });
}

}  // namespace

PlanBase* make_dynamic_cnn_plan(const char* arch, int N, int H, int W, int dtype, int* rc) {
  return make_plan<DynamicCnnPlan>(N, H, W, dtype, rc, [arch](DynamicCnnPlan& p) { return build_dynamic_cnn_plan(p, arch); });
}
