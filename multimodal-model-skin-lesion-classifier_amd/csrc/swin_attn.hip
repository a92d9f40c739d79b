// Shifted-window attention of the Swin Transformer encoders (timm swin_transformer.py SwinTransformerBlock._attn + WindowAttention),
// gfx950, fp32, forward and backward, on the image-major packed qkv [B, Hp, Wp, 3, H, Dh] a fused qkv Linear writes; the output
// [B, Hp, Wp, H, Dh] is what the projection reads.  One WAVE per (window, head), the structure of attention_rows_* in head.hip: lane i owns
// query row i, key / value rows come through wave-uniform (scalar) loads, the backward recomputes the probabilities from the saved row
// log-sum-exp.  What timm composes around the attention lives in the kernels' index arithmetic instead:
//
//   cyclic shift     window (wy, wx), row (r, c) of the ROLLED image is token ((wy ws + r + shift_y) mod Hp, (wx ws + c + shift_x) mod Wp) of the
//                    un-rolled activation.  q / k / v are read there and o, dq, dk, dv written there: neither torch.roll, nor
//                    window_partition / window_reverse exists as a copy.  A window's first token never wraps (wy ws + shift < Hp); only the
//                    walk over the rows / columns of the last window row / column does, one compare and subtract per step.
//   position bias    logit_ij += table[(r_i - r_j + ws - 1)(2 ws - 1) + (c_i - c_j + ws - 1)][h].  The head's column of the table
//                    ((2 ws - 1)^2 <= 225 floats) sits in wave-private LDS; lane i reads entry e_i - (r_j (2 ws - 1) + c_j), e_i its own constant.
//   mask             logit_ij -= 100 when tokens i and j carry different region ids; the ids are timm's three slices per axis,
//                    [0, Hp - ws), [Hp - ws, Hp - shift), [Hp - shift, Hp), evaluated on the rolled coordinates.  No mask or index tensor is
//                    loaded.  An axis with shift 0 gives every token of a window the same id on that axis: no wrap and no mask there
//                    (timm shifts per axis: an axis no longer than the window is not shifted, _calc_window_shift).
//
// Backward: dS_ij = p_ij (f_ij dO_i . v_j - dO_i . o_i) is the gradient of logit_ij (f: dropout factor); dq = scale dS k, dk = scale dS^T q,
// dv = P'^T dO as in attention_rows_bwd_kernel, through the wave's LDS tiles.  The table gradient is the sum of dS_ij over every pair with
// the same relative position: lane e sums the pairs of entry e from the wave's dS tile in (r_j, c_j) order and writes
// partial[window][e][h]; the fp64 column reducer (bias_grad_finalize) adds the windows.  No floating-point atomics: bitwise repeatable.
#include "../../include/mmskin.h"
#include <stdlib.h>

#include "ops.h"

namespace {

struct SwinArgs {
  int64_t qs_tok, qs_head;     // element strides of q / k / v (and dq / dk / dv) between tokens / heads
  int64_t os_tok, os_head;     // of o (and dO)
  int nunits, H, ws, L, T1, T, Tpad, shy, shx, nwy, nwx, Hp, Wp;     // units = windows x heads; L = ws^2; T1 = 2 ws - 1, T = T1^2 table rows
  float scale, drop_p;
  uint64_t seed, offset;
};

// token index (in the un-rolled image-major activation) of row (r, c) of the window whose first token is (ty0, tx0)
__device__ __forceinline__ int64_t swin_tok(const SwinArgs& p, int64_t img_tok, int ty0, int tx0, int r, int c) {
  int ty = ty0 + r, tx = tx0 + c;
  ty -= ty >= p.Hp ? p.Hp : 0;
  tx -= tx >= p.Wp ? p.Wp : 0;
  return img_tok + (int64_t)ty * p.Wp + tx;
}
// region id of rolled coordinate (y, x): timm's img_mask slices (0, -ws), (-ws, -shift), (-shift, None) per axis
__device__ __forceinline__ int swin_region(const SwinArgs& p, int y, int x) {
  const int ry = y < p.Hp - p.ws ? 0 : (y < p.Hp - p.shy ? 1 : 2);
  const int rx = x < p.Wp - p.ws ? 0 : (x < p.Wp - p.shx ? 1 : 2);
  return ry * 3 + rx;
}
#define SWIN_STEP(r, c) do { if (++c == p.ws) { c = 0; ++r; } } while (0)

// what a wave knows about its (window, head) and a lane about its row
struct SwinUnit {
  int h, y0, x0, ty0, tx0, rid, eb;
  int64_t img_tok, tok;
};
__device__ __forceinline__ SwinUnit swin_unit(const SwinArgs& p, int unit, int row) {
  SwinUnit u;
  const int win = unit / p.H, nw = p.nwy * p.nwx, img = win / nw, w = win - img * nw, wy = w / p.nwx, wx = w - wy * p.nwx;
  u.h = unit - win * p.H;
  u.y0 = wy * p.ws; u.x0 = wx * p.ws;
  u.ty0 = u.y0 + p.shy; u.tx0 = u.x0 + p.shx;            // < Hp, Wp: shifts < ws
  u.img_tok = (int64_t)img * p.Hp * p.Wp;
  const int r = row / p.ws, c = row - r * p.ws;
  u.tok = swin_tok(p, u.img_tok, u.ty0, u.tx0, r, c);
  u.rid = swin_region(p, u.y0 + r, u.x0 + c);
  u.eb = (r + p.ws - 1) * p.T1 + c + p.ws - 1;          // table row of (i, j) = eb - (r_j T1 + c_j)
  return u;
}
__device__ __forceinline__ void swin_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (pointers are separate __restrict__ kernel parameters and the loops over the OTHER token are rolled, for the reasons given at
// attention_rows_fwd_kernel: the no-alias guarantee keeps the uniform key / value reads scalar, the rolled loop keeps them in registers)
template <int DH>
__global__ __launch_bounds__(256) void swin_attn_fwd_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                            const float* __restrict__ gv, const float* __restrict__ gtab,
                                                            float* __restrict__ gout, float* __restrict__ glse, const SwinArgs p) {
  extern __shared__ float swin_lds[];                        // per wave: bias column [Tpad] | S [L][64]
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int unit = blockIdx.x * 4 + wave;                    // wave-uniform
  if (unit >= p.nunits) return;
  const int lane = threadIdx.x & 63;
  const int L = p.L;
  float* tb = swin_lds + (size_t)wave * (p.Tpad + L * 64);
  float* Ss = tb + p.Tpad + lane;
  const bool act = lane < L;
  const int row = act ? lane : 0;                            // idle lanes shadow row 0; nothing of theirs is stored
  const SwinUnit u = swin_unit(p, unit, row);
  const int64_t hq = u.h * p.qs_head;
  for (int e = lane; e < p.T; e += 64) tb[e] = gtab[(int64_t)e * p.H + u.h];
  const float* __restrict__ qrow = gq + u.tok * p.qs_tok + hq;
  float qv[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(qrow + d);
    qv[d] = t.x * p.scale; qv[d + 1] = t.y * p.scale; qv[d + 2] = t.z * p.scale; qv[d + 3] = t.w * p.scale;
  }
  swin_wave_sync();
  float mx = -INFINITY;
  int jr = 0, jc = 0;
#pragma unroll 1
  for (int j = 0; j < L; ++j) {
    const float* __restrict__ kr = gk + swin_tok(p, u.img_tok, u.ty0, u.tx0, jr, jc) * p.qs_tok + hq;     // uniform address: scalar loads
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) a = fmaf(qv[d], kr[d], a);
    a += tb[u.eb - (jr * p.T1 + jc)];
    if (u.rid != swin_region(p, u.y0 + jr, u.x0 + jc)) a -= 100.f;
    Ss[j * 64] = a;
    mx = fmaxf(mx, a);
    SWIN_STEP(jr, jc);
  }
  const float keep_scale = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const AttnDropKey dkey = attn_drop_key(p.seed, p.offset, p.drop_p);
  float ov[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) ov[d] = 0.f;
  float sum = 0.f;
  jr = 0; jc = 0;
#pragma unroll 1
  for (int j = 0; j < L; ++j) {
    const float* __restrict__ vr = gv + swin_tok(p, u.img_tok, u.ty0, u.tx0, jr, jc) * p.qs_tok + hq;
    float e = expf(Ss[j * 64] - mx);
    sum += e;                                                // the softmax denominator counts dropped probabilities too
    if (p.drop_p > 0.f) e = attn_keep(dkey, attn_row_base((uint64_t)unit * L + row, (L + 1) >> 1), j) ? e * keep_scale : 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) ov[d] = fmaf(e, vr[d], ov[d]);
    SWIN_STEP(jr, jc);
  }
  const float inv = 1.f / sum;
  if (act) {
    if (glse) glse[(int64_t)unit * L + lane] = mx + logf(sum);
    float* __restrict__ orow = gout + u.tok * p.os_tok + u.h * p.os_head;
#pragma unroll
    for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(orow + d) = make_float4(ov[d] * inv, ov[d + 1] * inv, ov[d + 2] * inv, ov[d + 3] * inv);
  }
}

template <int DH>
__global__ __launch_bounds__(256) void swin_attn_bwd_kernel(const float* __restrict__ gq, const float* __restrict__ gk,
                                                            const float* __restrict__ gv, const float* __restrict__ gtab,
                                                            const float* __restrict__ go, const float* __restrict__ gdO,
                                                            const float* __restrict__ glse, float* __restrict__ gdq,
                                                            float* __restrict__ gdk, float* __restrict__ gdv,
                                                            float* __restrict__ gpart, const SwinArgs p) {
  extern __shared__ float swin_lds[];                        // per wave: bias column [Tpad] | dS [L][L+1] | P' [L][L+1]
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int unit = blockIdx.x * 4 + wave;
  if (unit >= p.nunits) return;
  const int lane = threadIdx.x & 63;
  const int L = p.L, LP = L + 1;
  float* tb = swin_lds + (size_t)wave * (p.Tpad + 2 * L * LP);
  float* dSs = tb + p.Tpad;
  float* Pps = dSs + L * LP;
  const bool act = lane < L;
  const int row = act ? lane : 0;
  const SwinUnit u = swin_unit(p, unit, row);
  const int64_t hq = u.h * p.qs_head, ho = u.h * p.os_head;
  for (int e = lane; e < p.T; e += 64) tb[e] = gtab[(int64_t)e * p.H + u.h];
  swin_wave_sync();
  {
    // ---- phase A: lane i = query row i.  p_ij from the saved row log-sum-exp, dP'_ij = dO_i . v_j, delta_i = dO_i . o_i,
    // dS_ij = p_ij (f_ij dP'_ij - delta_i): the gradient of logit_ij, BEFORE the scale factor (the table gradient sums it as it is);
    // dq_i = scale sum_j dS_ij k_j
    const float* __restrict__ qrow = gq + u.tok * p.qs_tok + hq;
    const float* __restrict__ dorow = gdO + u.tok * p.os_tok + ho;
    const float* __restrict__ orow = go + u.tok * p.os_tok + ho;
    float qv[DH], gvv[DH], acc[DH];
    float delta = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const float4 t = *reinterpret_cast<const float4*>(qrow + d);
      qv[d] = t.x * p.scale; qv[d + 1] = t.y * p.scale; qv[d + 2] = t.z * p.scale; qv[d + 3] = t.w * p.scale;
      const float4 g = *reinterpret_cast<const float4*>(dorow + d);
      gvv[d] = g.x; gvv[d + 1] = g.y; gvv[d + 2] = g.z; gvv[d + 3] = g.w;
      const float4 w = *reinterpret_cast<const float4*>(orow + d);
      delta = fmaf(g.x, w.x, fmaf(g.y, w.y, fmaf(g.z, w.z, fmaf(g.w, w.w, delta))));
      acc[d] = 0.f; acc[d + 1] = 0.f; acc[d + 2] = 0.f; acc[d + 3] = 0.f;
    }
    const float lse = glse[(int64_t)unit * L + row];
    const float keep_scale = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
    const AttnDropKey dkey = attn_drop_key(p.seed, p.offset, p.drop_p);
    int jr = 0, jc = 0;
#pragma unroll 1
    for (int j = 0; j < L; ++j) {
      const int64_t jt = swin_tok(p, u.img_tok, u.ty0, u.tx0, jr, jc) * p.qs_tok + hq;
      const float* __restrict__ kr = gk + jt;
      const float* __restrict__ vr = gv + jt;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) { a = fmaf(qv[d], kr[d], a); c = fmaf(gvv[d], vr[d], c); }
      a += tb[u.eb - (jr * p.T1 + jc)];
      if (u.rid != swin_region(p, u.y0 + jr, u.x0 + jc)) a -= 100.f;
      const float pj = expf(a - lse);
      float f = 1.f;
      if (p.drop_p > 0.f) f = attn_keep(dkey, attn_row_base((uint64_t)unit * L + row, (L + 1) >> 1), j) ? keep_scale : 0.f;
      const float ds = pj * (f * c - delta);
      if (act) { dSs[lane * LP + j] = ds; Pps[lane * LP + j] = pj * f; }
#pragma unroll
      for (int d = 0; d < DH; ++d) acc[d] = fmaf(ds, kr[d], acc[d]);
      SWIN_STEP(jr, jc);
    }
    if (act) {
      float* __restrict__ dqrow = gdq + u.tok * p.qs_tok + hq;
#pragma unroll
      for (int d = 0; d < DH; d += 4)
        *reinterpret_cast<float4*>(dqrow + d) = make_float4(acc[d] * p.scale, acc[d + 1] * p.scale, acc[d + 2] * p.scale, acc[d + 3] * p.scale);
    }
  }
  // ---- phase B: lane j = key row j.  dk_j = scale sum_i dS_ij q_i, dv_j = sum_i P'_ij dO_i  (columns of the wave's LDS tiles)
  swin_wave_sync();
  {
    float ak[DH], av[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) { ak[d] = 0.f; av[d] = 0.f; }
    int ir = 0, ic = 0;
#pragma unroll 1
    for (int i = 0; i < L; ++i) {
      const float dsi = dSs[i * LP + row], ppi = Pps[i * LP + row];
      const int64_t it = swin_tok(p, u.img_tok, u.ty0, u.tx0, ir, ic);
      const float* __restrict__ qr = gq + it * p.qs_tok + hq;       // uniform: scalar loads
      const float* __restrict__ gr = gdO + it * p.os_tok + ho;
#pragma unroll
      for (int d = 0; d < DH; ++d) { ak[d] = fmaf(dsi, qr[d], ak[d]); av[d] = fmaf(ppi, gr[d], av[d]); }
      SWIN_STEP(ir, ic);
    }
    if (act) {
      float* __restrict__ dkrow = gdk + u.tok * p.qs_tok + hq;
      float* __restrict__ dvrow = gdv + u.tok * p.qs_tok + hq;
#pragma unroll
      for (int d = 0; d < DH; d += 4) {
        *reinterpret_cast<float4*>(dkrow + d) = make_float4(ak[d] * p.scale, ak[d + 1] * p.scale, ak[d + 2] * p.scale, ak[d + 3] * p.scale);
        *reinterpret_cast<float4*>(dvrow + d) = make_float4(av[d], av[d + 1], av[d + 2], av[d + 3]);
      }
    }
  }
  // ---- phase C: lane e = table row e = (dy + ws - 1) T1 + (dx + ws - 1).  Its pairs are i = (r_j + dy, c_j + dx) for every key (r_j, c_j)
  // that keeps i inside the window; each (i, j) of the dS tile belongs to exactly one e.  Summed in (r_j, c_j) order.
  if (gpart) {
    const int ws = p.ws;
    float* __restrict__ prow = gpart + (int64_t)(unit / p.H) * p.T * p.H + u.h;
    for (int e = lane; e < p.T; e += 64) {
      const int ey = e / p.T1, dy = ey - (ws - 1), dx = e - ey * p.T1 - (ws - 1);
      const int r0 = dy < 0 ? -dy : 0, r1 = dy > 0 ? ws - dy : ws, c0 = dx < 0 ? -dx : 0, c1 = dx > 0 ? ws - dx : ws;
      float s = 0.f;
      for (int rj = r0; rj < r1; ++rj)
        for (int cj = c0; cj < c1; ++cj) s += dSs[((rj + dy) * ws + cj + dx) * LP + rj * ws + cj];
      prow[(int64_t)e * p.H] = s;
    }
  }
}

// The backward's workspace: the per-window partial table gradients [B nwy nwx][T][H] and the scratch of the fp64 column reducer over them.
struct SwinWorkspace {
  float* partial;
  ColScratch red;
  size_t bytes;
  SwinWorkspace(void* base, int64_t nwin, int T, int H) {
    Carver cv(base);
    partial = cv.take<float>((size_t)nwin * T * H);
    red.doubles = col_reduce_scratch_doubles((size_t)T * H);
    red.p = cv.take<double>(red.doubles);
    bytes = cv.cur;
  }
};

int swin_geometry_ok(int B, int Hp, int Wp, int ws, int H, const char* what) {
  ARG_CHECK(B > 0 && Hp > 0 && Wp > 0 && H > 0 && ws > 0, "%s: bad shape (B=%d Hp=%d Wp=%d H=%d ws=%d)", what, B, Hp, Wp, H, ws);
  ARG_CHECK(ws * ws <= 64, "%s: needs ws*ws <= 64 (ws=%d)", what, ws);
  ARG_CHECK(Hp % ws == 0 && Wp % ws == 0, "%s: token grid %d x %d is not a multiple of the window %d", what, Hp, Wp, ws);
  ARG_CHECK((int64_t)B * (Hp / ws) * (Wp / ws) * H < (int64_t)1 << 30, "%s: too many windows", what);
  return MMSKIN_OK;
}

int swin_args(SwinArgs& a, int B, int Hp, int Wp, int ws, int shift_y, int shift_x, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head,
              float scale, float drop_p, uint64_t seed, uint64_t offset, const char* what) {
  if (int rc = swin_geometry_ok(B, Hp, Wp, ws, H, what)) return rc;
  ARG_CHECK(Dh == 32 || Dh == 64, "%s: needs Dh 32 or 64 (Dh=%d)", what, Dh);
  ARG_CHECK(shift_y >= 0 && shift_y < ws && shift_x >= 0 && shift_x < ws, "%s: shift (%d, %d) outside [0, %d)", what, shift_y, shift_x, ws);
  ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "%s: dropout %f", what, (double)drop_p);
  ARG_CHECK(q_tok > 0 && q_head > 0 && o_tok > 0 && o_head > 0 && q_tok % 4 == 0 && q_head % 4 == 0 && o_tok % 4 == 0 && o_head % 4 == 0,
            "%s: strides must be positive and keep rows 16-byte aligned", what);
  a.qs_tok = q_tok; a.qs_head = q_head; a.os_tok = o_tok; a.os_head = o_head;
  a.nwy = Hp / ws; a.nwx = Wp / ws; a.Hp = Hp; a.Wp = Wp;
  a.nunits = B * a.nwy * a.nwx * H; a.H = H; a.ws = ws; a.L = ws * ws; a.T1 = 2 * ws - 1; a.T = a.T1 * a.T1; a.Tpad = (a.T + 7) & ~7;
  a.shy = shift_y; a.shx = shift_x; a.scale = scale; a.drop_p = drop_p; a.seed = seed; a.offset = offset;
  return MMSKIN_OK;
}

}  // namespace

extern "C" {

int64_t mmskin_swin_attention_workspace_bytes(int B, int Hp, int Wp, int ws, int H) {
  if (swin_geometry_ok(B, Hp, Wp, ws, H, "swin_attention_workspace_bytes")) return -1;
  return (int64_t)SwinWorkspace(nullptr, (int64_t)B * (Hp / ws) * (Wp / ws), (2 * ws - 1) * (2 * ws - 1), H).bytes;
}

int mmskin_swin_attention_forward(const float* q, const float* k, const float* v, const float* bias_table, float* o, float* lse, int B, int Hp,
                                  int Wp, int ws, int shift_y, int shift_x, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head,
                                  float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(q && k && v && bias_table && o, "swin_attention_forward: null argument");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0 && (((uintptr_t)bias_table | (uintptr_t)lse) & 3) == 0,
            "swin_attention_forward: 16-byte aligned tensors (4-byte table and lse) required");
  SwinArgs a;
  if (int rc = swin_args(a, B, Hp, Wp, ws, shift_y, shift_x, H, Dh, q_tok, q_head, o_tok, o_head, scale, drop_p, seed, offset, "swin_attention_forward")) return rc;
  const size_t lds = (size_t)4 * (a.Tpad + a.L * 64) * sizeof(float);
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(swin_attn_fwd_kernel<32>), 4 * (232 + 64 * 64) * 4));   // ws = 8: above 64 KiB
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(swin_attn_fwd_kernel<64>), 4 * (232 + 64 * 64) * 4));
  const dim3 grid((a.nunits + 3) / 4);
  if (Dh == 32) hipLaunchKernelGGL(swin_attn_fwd_kernel<32>, grid, dim3(256), lds, ST(stream), q, k, v, bias_table, o, lse, a);
  else hipLaunchKernelGGL(swin_attn_fwd_kernel<64>, grid, dim3(256), lds, ST(stream), q, k, v, bias_table, o, lse, a);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

int mmskin_swin_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* bias_table, const float* o,
                                   const float* lse, float* dq, float* dk, float* dv, float* dbias_table, void* workspace, int B, int Hp,
                                   int Wp, int ws, int shift_y, int shift_x, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head,
                                   float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream) {
  ARG_CHECK(dO && q && k && v && bias_table && o && lse && dq && dk && dv, "swin_attention_backward: null argument");
  ARG_CHECK(!dbias_table || workspace, "swin_attention_backward: the table gradient needs the workspace");
  ARG_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) == 0 &&
                (((uintptr_t)bias_table | (uintptr_t)lse | (uintptr_t)dbias_table) & 3) == 0 && ((uintptr_t)workspace & 255) == 0,
            "swin_attention_backward: 16-byte aligned tensors (4-byte table and lse, 256-byte workspace) required");
  SwinArgs a;
  if (int rc = swin_args(a, B, Hp, Wp, ws, shift_y, shift_x, H, Dh, q_tok, q_head, o_tok, o_head, scale, drop_p, seed, offset, "swin_attention_backward")) return rc;
  const int nwin = B * a.nwy * a.nwx;
  const SwinWorkspace w(workspace, nwin, a.T, H);
  float* partial = dbias_table ? w.partial : nullptr;
  const size_t lds = (size_t)4 * (a.Tpad + 2 * a.L * (a.L + 1)) * sizeof(float);
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(swin_attn_bwd_kernel<32>), 4 * (232 + 2 * 64 * 65) * 4));
  HIP_CHECK_RET(opt_in_dynamic_lds(reinterpret_cast<const void*>(swin_attn_bwd_kernel<64>), 4 * (232 + 2 * 64 * 65) * 4));
  const dim3 grid((a.nunits + 3) / 4);
  if (Dh == 32) hipLaunchKernelGGL(swin_attn_bwd_kernel<32>, grid, dim3(256), lds, ST(stream), q, k, v, bias_table, o, dO, lse, dq, dk, dv, partial, a);
  else hipLaunchKernelGGL(swin_attn_bwd_kernel<64>, grid, dim3(256), lds, ST(stream), q, k, v, bias_table, o, dO, lse, dq, dk, dv, partial, a);
  HIP_CHECK_RET(hipGetLastError());
  if (dbias_table) return bias_grad_finalize(partial, nwin, a.T * H, a.T * H, dbias_table, w.red, ST(stream));
  return MMSKIN_OK;
}

}  // extern "C"
