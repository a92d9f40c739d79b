/* mmskin.h -- C ABI of libmmskin_hip.so: the MI355X (gfx950) implementation of the
 * MultimodalModel forward/backward hot path of life-ufes/multimodal-model-skin-lesion-classifier.
 *
 * The reference has no FFI / plugin boundary of its own: its boundary is the Python nn.Module
 * contract of src/scripts/benchmark/models/multimodalIntraInterModal.py:13-416 (ctor :14-28,
 * forward :162).  This header is the build-defined C replacement for the ATen operators that module
 * invokes; each entry point names the reference call site whose arithmetic it replaces.  The Python
 * shim in multimodal-model-skin-lesion-classifier_amd/models/ binds these with ctypes (see
 * INTEGRATION.md).
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (no torch types, no allocation
 * inside compute calls); `stream` is a hipStream_t passed as void*; all calls are asynchronous on that
 * stream and return 0 on success, otherwise a MMSKIN_ERR_* code with mmskin_last_error() describing
 * it.  Matrices are row-major.  dtype selects the backbone compute type: MMSKIN_F32 = exact fp32
 * MFMA (parity mode), MMSKIN_BF16 = bf16 MFMA with fp32 accumulation (throughput mode).
 */
#ifndef MMSKIN_H
#define MMSKIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMSKIN_F32 0
#define MMSKIN_BF16 1

const char* mmskin_last_error(void);
int mmskin_version(void);

/* ---------------------------------------------------------------------------------------------
 * Image encoder plan (resnet-18 / resnet-50).  Replaces `self.image_encoder(image)`
 * (multimodalIntraInterModal.py:167; factory loadImageModelClassifier.py:65-75) and its backward.
 * Parameters: ONE flat fp32 buffer in torchvision named_parameters() order (conv.weight OIHW,
 * bn.weight, bn.bias ...); buffers: ONE flat fp32 buffer (running_mean, running_var per BN).
 * tensor_info enumerates names/offsets/shapes so the host can expose them as state_dict entries.
 *
 * arch is a fixed name ("resnet-18", "resnet-50", "densenet169", "densenet169-features", "vgg16-features", "mobilenet-v2",
 * "efficientnet-b0", "efficientnet-b7") or the configured NAS trunk
 *     dynamic-cnn/<f0>-<f1>-...-<fn>/l<layers_per_block>/p<0|1>/k<kernel_size>        e.g. dynamic-cnn/64-128-256/l2/p1/k3
 * = [Conv2d(k, pad k/2, no bias) -> GroupNorm(8, f) -> ReLU] x layers per filter f, MaxPool2d(2, 2) after each block when p1, then
 * AdaptiveAvgPool2d(1): features [N, fn].  Parameters are named by their index in that Sequential ("0.weight", "1.weight", "1.bias",
 * "3.weight", ...); there are no buffers.  An optional fifth field "/t0" keeps the last layer's activation and runs the global average
 * as separate launches (for timing against the default fused tail, "/t1").  Any other spelling: MMSKIN_ERR_ARG.  Refused with
 * MMSKIN_ERR_UNSUPPORTED: k != 3, a filter that is not a multiple of 64 or above 1024, f0 != 64; with MMSKIN_ERR_ARG: no filter,
 * l < 1, height or width above 240, a map below 2x2 in front of a pool. */
typedef struct mmskin_backbone* mmskin_backbone_t;
int mmskin_backbone_create(const char* arch, int batch, int height, int width, int dtype, mmskin_backbone_t* out);
void mmskin_backbone_destroy(mmskin_backbone_t h);
int mmskin_backbone_num_tensors(mmskin_backbone_t h, int kind /*0 params, 1 buffers*/);
int mmskin_backbone_tensor_info(mmskin_backbone_t h, int kind, int index, char* name, int name_cap,
                                int64_t* offset, int64_t* numel, int* ndim, int64_t* shape4);
int64_t mmskin_backbone_param_numel(mmskin_backbone_t h);
int64_t mmskin_backbone_buffer_numel(mmskin_backbone_t h);
int64_t mmskin_backbone_workspace_bytes(mmskin_backbone_t h);
int mmskin_backbone_feature_dim(mmskin_backbone_t h);
/* spatial size of the plan's output: 1x1 for pooled features; arch "densenet169-features" returns the norm5
 * feature map [N][1664][H/32][W/32] (fp32 NCHW), the `densenet.features` the reference's MD-Net keeps
 * (multimodalMDNet.py:72-76) */
int mmskin_backbone_feature_hw(mmskin_backbone_t h, int* out_h, int* out_w);
/* Introspection for parity tests: where unit `index` (conv+BN, in parameter order) keeps its raw conv
 * output x, its post-activation output y and its BN coefficient vectors inside the workspace.
 * info12 = {x_off, y_off, coef_off (bytes), rows, Cout, OH, OW, Cin, H, W, pool_off, scratch0_off}.
 * MobileNet-V2 / EfficientNet plans report the same twelve fields with the real (unpadded) Cout / Cin, the unit's input
 * activation offset in place of pool_off and the first gradient buffer in place of scratch0_off; a depthwise unit is the one
 * whose named weight has shape [C][1][k][k]. */
int mmskin_backbone_num_units(mmskin_backbone_t h);
int mmskin_backbone_unit_info(mmskin_backbone_t h, int index, char* name, int name_cap, int64_t* info12);
/* What the ResNet plan decided for unit `index` when it was created (no GPU needed): an OR of
 *   MMSKIN_UNIT_ABN         algebraic BatchNorm backward: no dz and no BatchNorm-backward apply pass for this unit
 *   MMSKIN_UNIT_FWD2P       two-pass forward: the unit's raw convolution output is never stored
 *   MMSKIN_UNIT_GRAM        ... and its forward statistics come from the Gram matrix of its input, kept for backward
 *   MMSKIN_UNIT_DS          the unit is a block's downsample branch
 *   MMSKIN_UNIT_DS_COMPACT  ... whose data gradient is computed on the pixels the stride-2 convolution read only
 *   MMSKIN_UNIT_LAST_BLOCK  the unit belongs to the last block (its gradient arrives from the average pool)
 * Plans of the other architectures: MMSKIN_ERR_UNSUPPORTED. */
enum { MMSKIN_UNIT_ABN = 1, MMSKIN_UNIT_FWD2P = 2, MMSKIN_UNIT_GRAM = 4, MMSKIN_UNIT_DS = 8, MMSKIN_UNIT_DS_COMPACT = 16,
       MMSKIN_UNIT_LAST_BLOCK = 32 };
int mmskin_backbone_unit_flags(mmskin_backbone_t h, int index, int* flags);
/* Per-kernel-class timing with HIP events recorded on the launch stream (off by default).  Classes:
 * 0 conv fwd (implicit GEMM), 1 conv dgrad, 2 wgrad(+reduce), 3 BN fwd (finalize+apply), 4 BN bwd,
 * 5 weight staging, 6 stem pack/pool.  read() synchronises, returns the totals accumulated since
 * enable()/the last read(): milliseconds, algorithmic FLOPs, algorithmic bytes, launches; then resets. */
int mmskin_backbone_profile_enable(mmskin_backbone_t h, int on);
int mmskin_backbone_profile_read(mmskin_backbone_t h, double* ms7, double* flops7, double* bytes7, int64_t* launches7);
/* image_nchw: fp32 [batch,3,H,W]; features: fp32 [batch, feature_dim].  training!=0: batch-stat BN,
 * running stats updated in `buffers`, activations kept in `workspace` for the backward call. */
int mmskin_backbone_forward(mmskin_backbone_t h, const float* image_nchw, const float* params, float* buffers,
                            void* workspace, float* features, int training, void* stream);
/* param_grads: flat fp32, same layout as params; every element is written. */
/* Same forward from the uint8 NHWC batch the DataLoader decodes ([N][H][W][3]): Normalize + ToTensor of the
 * reference's transform (skinLesionDatasets.py:29,111-119: (u8/255 - mean)/std) run inside the stem packing
 * kernel, so the host->device copy is 1 byte per value instead of 4.  mean_std6: 6 HOST floats, mean rgb | std rgb. */
int mmskin_backbone_forward_u8(mmskin_backbone_t h, const uint8_t* image_nhwc, const float* mean_std6, const float* params,
                               float* buffers, void* workspace, float* features, int training, void* stream);
/* Grad-CAM / Grad-CAM++ consumers (src/services/XAI/models/cam.py:10-60, model_loader.py:36-41) hook the LAST nn.Conv2d
 * of image_encoder and differentiate the class score w.r.t. its output under model.eval().  With option
 * "keep_raw_eval" = 1 an eval forward keeps raw conv outputs (BatchNorm is then not folded into the convs);
 * last_conv_export returns that conv's output [N][C][OH][OW] (fp32) and last_conv_grad the gradient of the pooled
 * features w.r.t. it for a given d(score)/d(features) [N][C].  ResNet plans only. */
int mmskin_backbone_set_option(mmskin_backbone_t h, const char* key, int value);
/* option "reuse_staged" = 1 (serving): the caller vouches that parameters and BatchNorm buffers are unchanged since the
 * previous eval forward on this plan and workspace; the BN-folded staged weights and coefficient table already in the
 * workspace are then reused instead of rebuilt (ResNet plans; others restage).  Any training-mode or keep_raw_eval
 * forward invalidates the staged copy by itself. */
/* per-step device pointers: key "sd_mask" (EfficientNet plans) = fp32 [n_residual_blocks][batch] keep/scale factors of
 * torchvision's StochasticDepth(p, "row") for this training step (0 or 1/(1-p)); NULL disables stochastic depth */
int mmskin_backbone_set_pointer(mmskin_backbone_t h, const char* key, const void* device_ptr);
/* Gradient segments of the flat gradient arena, in the order backward completes them (ResNet: layer4, layer3,
 * layer2, layer1 + stem).  `wait_grad_segment` makes `stream` wait (hipStreamWaitEvent) until segment `index` of the
 * most recently enqueued backward is complete, so a data-parallel caller can all-reduce finished ranges under the rest
 * of backward.  Build-side addition (the reference is single-GPU, train_pad_20.py:509).  Plans that report
 * 0 segments are reduced as one range after backward. */
int mmskin_backbone_num_grad_segments(mmskin_backbone_t h, int* count);
int mmskin_backbone_grad_segment(mmskin_backbone_t h, int index, int64_t* offset, int64_t* numel);
int mmskin_backbone_wait_grad_segment(mmskin_backbone_t h, int index, void* stream);
int mmskin_backbone_last_conv_shape(mmskin_backbone_t h, int* C, int* OH, int* OW);
int mmskin_backbone_last_conv_export(mmskin_backbone_t h, const void* workspace, float* x_nchw, void* stream);
int mmskin_backbone_last_conv_grad(mmskin_backbone_t h, const float* dfeatures, const void* workspace, float* dx_nchw,
                                   void* stream);
int mmskin_backbone_backward(mmskin_backbone_t h, const float* dfeatures, const float* params, void* workspace,
                             float* param_grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Op-level convolution / batch-norm entry points (same kernels the plan uses; NCHW fp32 at the
 * boundary, converted to NHWC `dtype` inside `workspace`).  Used by the parity tests and by
 * consumers that need a single layer.  conv weight OIHW fp32, no bias (torchvision ResNet convs). */
int64_t mmskin_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int mmskin_conv2d_forward(const float* x, const float* w, float* y, int N, int Cin, int H, int W, int Cout, int kh,
                          int kw, int stride, int pad, int dtype, void* workspace, void* stream);
/* dx (may be null) and dw (may be null) from dy [N,Cout,OH,OW] */
int mmskin_conv2d_backward(const float* dy, const float* x, const float* w, float* dx, float* dw, int N, int Cin,
                           int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype, void* workspace,
                           void* stream);
/* bf16 data gradient with the consumer unit's BatchNorm-backward prologue fused into the epilogue (what the ResNet plan launches for every
 * conv -> BatchNorm -> ReLU unit, csrc/conv_gemm.hip profile 3 / csrc/conv3x3_c64.hip): dz = dgrad(dy) * (xc * scale + shift > 0) and
 * the per-row-block partial sums [rows][2][Cin] of dz and dz * xc.  Replaces conv_backward(input) + the ReLU / BatchNorm-backward
 * reductions autograd runs after it (train_pad_20.py:112).  Workspace: mmskin_conv2d_workspace_bytes. */
int mmskin_conv2d_dgrad_fused_rows(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int mmskin_conv2d_dgrad_fused(const float* dy, const float* w, const float* xc, const float* scale, const float* shift, float* dz,
                              float* partial, int* rows_written, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride,
                              int pad, void* workspace, void* stream);
/* The data gradient with any fused epilogue of csrc/conv_gemm.hip the ResNet plan attaches (DgradFuse), op level, fp32 or bf16:
 * v = dgrad(dy) + addend; v = 0 where the mask says so (mask_y > 0 | mask_bits | x * scale + shift > 0); dz = v; per row block the partial
 * sums [rows][2][Cin] of the stored dz and dz * x (partial), and of dz and dz * x2 (partial_b).  `flags` are the MMSKIN_CRD_* bits of
 * mmskin_conv_route below, so a caller can ask the route table which instantiation its launch runs; each names one operand, which must be
 * non-null exactly when its flag is set (SCALE_SHIFT: scale and shift, needs X; X2: x2 and partial_b, needs X and PARTIAL; PARTIAL:
 * partial and rows_written).  IN2, BIAS and EMPTY are refused.  addend, mask_y, x, x2: [N,Cin,H,W]; with ADDEND_S2 the addend is the
 * compact [N,Cin,ceil(H/2),ceil(W/2)] tensor added at the even pixels (1x1 / stride 1 layers).  ADDEND | ADDEND_IS_DIN: addend == dz, the
 * gradient is accumulated into what dz holds (pixels no tap reaches keep their value).  mask_bits is taken in the kernel's own layout, not
 * converted: one byte per 16-byte chunk of the NHWC `dtype` tensor [N*H*W][Cin], byte (row * Cin + c) * elem_bytes >> 4, bit e = element e
 * of the chunk passes (8 elements per byte in bf16, 4 in fp32).  partial / partial_b: mmskin_conv2d_dgrad_fused_rows(...) rows;
 * *rows_written = rows the launch produced.  A refused call has launched nothing. */
int64_t mmskin_conv2d_dgrad_epilogue_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int mmskin_conv2d_dgrad_epilogue(const float* dy, const float* w, const float* addend, const float* mask_y, const unsigned char* mask_bits,
                                 const float* x, const float* scale, const float* shift, const float* x2, float* dz, float* partial,
                                 float* partial_b, int* rows_written, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride,
                                 int pad, int flags, int dtype, void* workspace, void* stream);
/* The forward convolution with the light epilogue (FwdFuse) or the statistics slabs, op level, fp32 or bf16:
 * v = acc * mul + addend + bias; ReLU; y = v; mask_out bit = (stored value > 0), in the layout above over [N*OH*OW][Cout].  `flags` are
 * MMSKIN_CRF_* bits: MUL, BIAS ([Cout] fp32), ADDEND ([N,Cout,OH,OW]) and MASK_OUT name a pointer each, non-null exactly when set; RELU
 * names none; STATS: stat_sum, stat_sq [rows][Cout] (rows = mmskin_conv2d_forward_epilogue_stat_rows(...)) and stat_rows, which
 * receives the rows written (with ROWS_FREE the route may pick fewer); NO_OUT (needs STATS): nothing is stored, y is not written and may
 * be null.  GELU, OUT_F32 and RESIDUAL are refused (the Linear entry points own them).  A refused call has launched nothing. */
int64_t mmskin_conv2d_forward_epilogue_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int mmskin_conv2d_forward_epilogue_stat_rows(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int mmskin_conv2d_forward_epilogue(const float* x, const float* w, const float* mul, const float* bias, const float* addend, float* y,
                                   float* stat_sum, float* stat_sq, int* stat_rows, unsigned char* mask_out, int N, int Cin, int H, int W,
                                   int Cout, int kh, int kw, int stride, int pad, int flags, int dtype, void* workspace, void* stream);
/* launches of the layer-1 all-taps 3x3 kernel (csrc/conv3x3_c64.hip) since load */
int64_t mmskin_conv3x3_c64_launches(void);
int64_t mmskin_stem7x7_launches(void);   /* ... of the direct 7x7 stem convolution (stem7x7.hip) */
/* timing helper for kernel tuning: average microseconds of the forward conv kernel over `iters` launches
 * on NHWC buffers carved from `workspace` (>= conv2d_workspace_bytes; contents irrelevant) */
double mmskin_conv2d_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                          int iters, void* workspace, void* stream);
double mmskin_conv2d_dgrad_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                                int iters, void* workspace, void* stream);
double mmskin_conv2d_wgrad_time(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dtype,
                                int iters, void* workspace, void* stream);
/* number of conv / dgrad launches this process has sent to the 8-phase pipelined kernel (224 / 256-row tiles, csrc/conv_gemm.hip);
 * the parity tests assert through it that the kernel they mean to check is the one that ran */
int64_t mmskin_conv_pipe_launches(void);
/* launches of the ring weight-gradient kernel (wgrad_ring.hip) since load: tests assert the path they mean to cover ran */
int64_t mmskin_wgrad_ring_launches(void);
/* The weight-gradient plan of a convolution (the 7x7 / stride 2 stem and a 3-channel 3x3 first conv in the virtual form the plans run):
 * out = family, tile_o, tile_k, variant, nsplit, per_split, reduce, slab_floats.  variant: 1 = the 1x1 / stride 1 form of a staged or ring
 * kernel; MMSKIN_WG_RING3: window pieces per wave.  per_split counts pixel rows (STAGED, RING) or stages of whole image rows (TAPS3, RING3).
 * Pure host arithmetic, no device needed; MMSKIN_ERR_ARG when no kernel takes the shape.  Tests assert it so that a case keeps covering the
 * kernel it was written for.  mmskin_conv_wgrad_slab_check is the check every weight-gradient launcher makes before it launches: 0 when the
 * plan's slab_floats fit in capacity_floats, else MMSKIN_ERR_ARG. */
enum { MMSKIN_WG_STAGED = 0, MMSKIN_WG_TAPS3 = 1, MMSKIN_WG_RING = 2, MMSKIN_WG_RING3 = 3 };
enum { MMSKIN_WGR_DIRECT = 0, MMSKIN_WGR_LANES = 1 };
int mmskin_conv_wgrad_plan(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, int64_t out[8]);
int mmskin_conv_wgrad_slab_check(int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes,
                                 int64_t capacity_floats);
int64_t mmskin_wgrad3_ring_launches(void);   /* ... of the all-taps 3x3 ring kernel (wgrad3_ring.hip) */
/* The route of a convolution forward (op 0) or data gradient (op 1) launch with the fused operands `flags` names (csrc/conv_gemm.hip
 * conv_gemm_route; a Linear of M rows, K -> N is the convolution N = M, H = W = 1, Cin = K, Cout = N, 1x1): out = family, bm (tile rows
 * computed), step (valid rows per row block), bn (tile columns), nst (LDS stages; 8 = the pipelined loop), epi (epilogue instantiation),
 * group_m (grouped tile order, 0 = off), total_mblk (row blocks = statistics / partial rows written), nblk_n (column blocks).
 * MMSKIN_CG_C64 / MMSKIN_CG_STEM7 (conv3x3_c64.hip, stem7x7.hip): family and total_mblk only.  op 2: the 7x7 / stride 2 stem of an
 * N x 3 x H x W batch; op 3: the 3-channel 3x3 / pad 1 first conv at `stride`; both in the virtual form the plans run, other shape arguments
 * unused, flags: MMSKIN_CRF_STATS (op 3 also BIAS, ADDEND, RELU).  Pure host arithmetic, no device needed; MMSKIN_ERR_ARG when no kernel
 * takes the launch.  Tests assert it so that a case keeps covering the kernel it was written for. */
enum { MMSKIN_CG_TILE128 = 0, MMSKIN_CG_BIG256 = 1, MMSKIN_CG_PIPE = 2, MMSKIN_CG_C64 = 3, MMSKIN_CG_STEM7 = 4 };
enum {   /* op 0: statistics slabs | the caller takes the statistics row count | FwdFuse operands (a FwdFuse is passed when one is named) | no T output */
  MMSKIN_CRF_STATS = 1, MMSKIN_CRF_ROWS_FREE = 2, MMSKIN_CRF_BIAS = 4, MMSKIN_CRF_ADDEND = 8, MMSKIN_CRF_RELU = 16, MMSKIN_CRF_GELU = 32,
  MMSKIN_CRF_OUT_F32 = 64, MMSKIN_CRF_RESIDUAL = 128 /* gamma + fp32 residual (the transformer-residual epilogue) */, MMSKIN_CRF_MASK_OUT = 256,
  MMSKIN_CRF_MUL = 512, MMSKIN_CRF_NO_OUT = 1024
};
enum {   /* op 1: addend | the addend is din | DgradFuse operands (a DgradFuse is passed when one is named; EMPTY: one without operands); k2 = flags >> 16 */
  MMSKIN_CRD_ADDEND = 1, MMSKIN_CRD_ADDEND_IS_DIN = 2, MMSKIN_CRD_MASK_Y = 4, MMSKIN_CRD_MASK_BITS = 8, MMSKIN_CRD_X = 16, MMSKIN_CRD_SCALE_SHIFT = 32,
  MMSKIN_CRD_X2 = 64, MMSKIN_CRD_IN2 = 128, MMSKIN_CRD_BIAS = 256, MMSKIN_CRD_ADDEND_S2 = 512, MMSKIN_CRD_PARTIAL = 1024, MMSKIN_CRD_EMPTY = 2048
};
int mmskin_conv_route(int op, int N, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int elem_bytes, int flags, int64_t out[9]);
/* Algebraic BatchNorm backward of an expanding 1x1 convolution x = conv(y, w) (csrc/abn.hip; bf16 operands): with
 * dz = cA g + cB x + cC per channel, dy = dz w and dw = dz^T y are computed from g, y, w and the coefficients alone
 * (dy = [g | y][cA w ; w^T diag(cB) w] + cC w, dw = cA (g^T y) + cB (w (y^T y)) + cC (x) colsum(y)): neither dz nor x is read.
 * Replaces autograd's backward through nn.BatchNorm2d + nn.Conv2d of torchvision's Bottleneck.conv3 (train_pad_20.py:112). */
int64_t mmskin_abn_workspace_bytes(int N, int Cw, int C4, int H, int W);
int mmskin_abn_backward(const float* g, const float* y, const float* w, const float* cA, const float* cB, const float* cC, int N, int Cw,
                        int C4, int H, int W, float* dy, float* dw, void* workspace, void* stream);
/* ... with the Gram matrix y^T y and colsum(y) taken by their own launch first and g^T y alone afterwards: the order of the two-pass
 * forward, whose first pass computes them for the statistics below and keeps them for this backward */
int mmskin_abn_backward_kept_gram(const float* g, const float* y, const float* w, const float* cA, const float* cB, const float* cC, int N,
                                  int Cw, int C4, int H, int W, float* dy, float* dw, void* workspace, void* stream);
/* Batch statistics of x = conv1x1(y, w) without x: stat_sum[o] = sum x[.,o] = sum_k w[o][k] colsum(y)[k], stat_sq[o] = sum x[.,o]^2 =
 * w_o^T (y^T y) w_o (bf16 operands, fp32 Gram matrix from the ring weight-gradient kernel, double-precision contraction).  The first
 * pass of the two-pass BatchNorm forward of Bottleneck.conv3 + bn3 (train-mode nn.BatchNorm2d statistics, train_pad_20.py:102);
 * workspace: mmskin_abn_workspace_bytes. */
int mmskin_conv1x1_gram_stats(const float* y, const float* w, int N, int Cw, int C4, int H, int W, float* stat_sum, float* stat_sq,
                              void* workspace, void* stream);
/* training-mode BatchNorm2d + optional ReLU on NCHW fp32 tensors (batch statistics) */
int64_t mmskin_batchnorm_workspace_bytes(int N, int C, int H, int W);
int mmskin_batchnorm_forward(const float* x, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float* y, float* save_mean, float* save_invstd, int N, int C, int H,
                             int W, float eps, float momentum, int relu, int dtype, void* workspace, void* stream);
int mmskin_batchnorm_backward(const float* dy, const float* x, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta,
                              int N, int C, int H, int W, int relu, int dtype, void* workspace, void* stream);
/* ---- The MBConv family op by op (MobileNet-V2 / EfficientNet plans, torchvision MBConv / InvertedResidual): each entry launches what
 * the plan launches for one unit, on NCHW fp32 tensors, with NHWC `dtype` copies inside the workspace.
 *
 * Depthwise k x k convolution, k in {3, 5}, stride in {1, 2}, padding k / 2.  x [N][C][H][W] with C the PADDED channel count (a multiple
 * of 8; the plan uses multiples of 64), w and dw [c_valid][1][k][k]: channels >= c_valid get zero weights, as the plan stages them, so y
 * and dx are zero there whatever x / dy hold.  dx or dw may be NULL. */
int64_t mmskin_dwconv2d_workspace_bytes(int N, int C, int H, int W, int ksize, int stride);
int mmskin_dwconv2d_forward(const float* x, const float* w, float* y, int N, int C, int H, int W, int ksize, int stride, int c_valid,
                            int dtype, void* workspace, void* stream);
int mmskin_dwconv2d_backward(const float* dy, const float* x, const float* w, float* dx, float* dw, int N, int C, int H, int W, int ksize,
                             int stride, int c_valid, int dtype, void* workspace, void* stream);
/* training-mode BatchNorm2d + the plans' activations: y = act(bn(x) + res), act 0 none, 1 ReLU, 2 ReLU6, 3 SiLU; res may be NULL.
 * Backward takes the y the forward returned (ReLU / ReLU6 mask from it: 0 < y, y < 6 on the STORED value) and returns dx, dgamma, dbeta
 * and, with has_residual, dres = the masked dy (may be NULL).  SiLU behind a residual has no backward (MMSKIN_ERR_UNSUPPORTED): the
 * kernel recomputes the SiLU argument from x alone, and the plans' residual units carry no activation. */
int64_t mmskin_batchnorm_act_workspace_bytes(int N, int C, int H, int W);
int mmskin_batchnorm_act_forward(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float* y, float* save_mean, float* save_invstd, int N, int C, int H, int W, float eps,
                                 float momentum, int act, int dtype, void* workspace, void* stream);
int mmskin_batchnorm_act_backward(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                                  const float* save_mean, const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta,
                                  int N, int C, int H, int W, int act, int has_residual, int dtype, void* workspace, void* stream);
/* The two element-wise BatchNorm apply passes alone, on [rows][C] device tensors of element type `dtype` (fp32, or bf16 bit patterns) and
 * given coefficient vectors; C a multiple of 4 (fp32) / 8 (bf16).  For tests of the launch geometry at shapes the plans do not run.
 * Forward: y = act(x * scale + shift [+ res | + res * rscale + rshift]); relu != 0 with relu_cap 0: ReLU, > 0: capped ReLU, < 0: SiLU;
 * mask_bits (may be NULL): one byte per 16-byte chunk, bit e = (stored y of element e > 0).
 * Backward: dz = mask(dy) by mask_mode (0 none, 1 x * scale + shift > 0, 2 ymask > 0, 3 0 < ymask < 6, 4 times SiLU'(x * scale + shift)),
 * dx = cA * dz + cB * x + cC; dz (may be NULL) receives the masked dy. */
int mmskin_bn_apply_rows(const void* x, const void* res, const float* scale, const float* shift, const float* rscale, const float* rshift,
                         void* y, unsigned char* mask_bits, int64_t rows, int C, int relu, float relu_cap, int dtype, void* stream);
int mmskin_bn_bwd_apply_rows(const void* dy, const void* x, const void* ymask, const float* scale, const float* shift, int mask_mode,
                             const float* cA, const float* cB, const float* cC, void* dx, void* dz, int64_t rows, int C, int dtype,
                             void* stream);
/* Squeeze-excitation (torchvision SqueezeExcitation: y * sigmoid(fc2(silu(fc1(mean_hw y))))): y, y_se, dy_se, dy are [N][Cp][HW] with
 * Cp = C rounded up to 64 (the plan keeps the padding channels of y at zero); w1 [Csq][C], b1 [Csq], w2 [C][Csq], b2 [C] and their
 * gradients are unpadded.  The backward recomputes the forward's small activations. */
int64_t mmskin_se_workspace_bytes(int N, int Cp, int Csq, int HW);
int mmskin_se_forward(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* y_se, int N, int C, int Cp,
                      int Csq, int HW, int dtype, void* workspace, void* stream);
int mmskin_se_backward(const float* dy_se, const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* dy,
                       float* dw1, float* db1, float* dw2, float* db2, int N, int C, int Cp, int Csq, int HW, int dtype, void* workspace,
                       void* stream);
/* Row-mode stochastic depth on [N][per_sample] (per_sample a multiple of 8): y = branch * mask[n] + res;  out = dy * mask[n] */
int64_t mmskin_sd_workspace_bytes(int N, int64_t per_sample);
int mmskin_sd_forward(const float* branch, const float* res, const float* mask, float* y, int N, int64_t per_sample, int dtype,
                      void* workspace, void* stream);
int mmskin_sd_backward(const float* dy, const float* mask, float* out, int N, int64_t per_sample, int dtype, void* workspace, void* stream);
/* DenseNet / VGG plan kernels, op by op (csrc/densenet.hip, csrc/vgg.hip): the same conventions (NCHW fp32 at the boundary, NHWC `dtype`
 * inside the caller's workspace).  The dense-block and transition entries run the functions the plan runs; their backward entries run the
 * training forward first, so they take the forward's inputs.
 * Dense block of L layers (growth 32, bottleneck 128) on x [N,C0,H,W], C0 a multiple of 32.  params (mmskin_dense_block_param_numel floats),
 * per layer in torchvision order: norm1.weight | norm1.bias [Cin], conv1.weight [128,Cin], norm2.weight | norm2.bias [128],
 * conv2.weight [32,128,3,3], Cin = C0 + 32 i.  buffers per layer: norm1.running_mean | running_var [Cin], norm2.running_mean |
 * running_var [128] (training: updated; eval: read, norm2 folded into conv1).  cat [N,C0+32L,H,W]; table (training, may be null):
 * mean [C0+32L] | biased var [C0+32L] of every cat channel.  Backward: dcat [N,C0+32L,H,W] -> dx [N,C0,H,W], grads laid out as params. */
int64_t mmskin_dense_block_workspace_bytes(int N, int C0, int L, int H, int W);
int64_t mmskin_dense_block_param_numel(int C0, int L);
int mmskin_dense_block_forward(const float* x, const float* params, float* buffers, float* cat, float* table, int N, int C0, int L, int H, int W,
                               int training, int dtype, void* workspace, void* stream);
int mmskin_dense_block_backward(const float* dcat, const float* x, const float* params, float* dx, float* grads, int N, int C0, int L, int H,
                                int W, int dtype, void* workspace, void* stream);
/* Transition norm -> ReLU -> conv1x1 (C -> C/2) -> avgpool 2x2 of x [N,C,H,W] (C a multiple of 128, H, W >= 2) with the block's table
 * (mean [C] | var [C]) into the first C/2 channels of dst [N,Cdst,H/2,W/2] (Cdst >= C/2, a multiple of 8; the other channels are kept).
 * params: norm.weight | norm.bias [C], conv.weight [C/2,C]; buffers: running_mean | running_var [C]; conv_out (may be null) [N,C/2,H,W]:
 * the stored convolution output the pool read.  Backward: dnext [N,Cdst,H/2,W/2]
 * (the next block's gradient; channels >= C/2 are not read) -> dx [N,C,H,W], grads laid out as params; dconv_out (may be null)
 * [N,C/2,H,W]: the gradient of the convolution output as the un-pooling kernel stored it. */
int64_t mmskin_dense_transition_workspace_bytes(int N, int C, int H, int W, int Cdst);
int mmskin_dense_transition_forward(const float* x, const float* table, const float* params, float* buffers, float* dst, float* conv_out, int N,
                                    int C, int H, int W, int Cdst, int training, int dtype, void* workspace, void* stream);
int mmskin_dense_transition_backward(const float* dnext, const float* x, const float* table, const float* params, float* dx, float* grads,
                                     float* dconv_out, int N, int C, int H, int W, int Cdst, int dtype, void* workspace, void* stream);
/* mean and biased variance of channels [c0, c0+C) of x [rows][pitch] (slice_stats + bn_table_finalize); C, c0, pitch multiples of 8 */
int64_t mmskin_slice_stats_workspace_bytes(int64_t rows, int pitch, int c0, int C);
/* The fp64 reduction scratch of the BatchNorm / bias finalize kernels (host arithmetic, no launch; for tests).  Above
 * MMSKIN_BN_SINGLE_ROWS partial rows a finalize first reduces each slab to at most 64 rows of doubles: a slab whose rows are cols_total
 * floats apart needs mmskin_col_reduce_scratch_doubles(cols_total) = 64 * cols_total doubles.  mmskin_col_reduce_scratch_check is the
 * check every finalize makes before that stage writes: 0 when `slabs` slabs of nrows x cols_total fit in `doubles`, else MMSKIN_ERR_ARG. */
int64_t mmskin_col_reduce_scratch_doubles(int64_t cols_total);
int mmskin_col_reduce_scratch_check(int slabs, int nrows, int cols_total, int64_t doubles);
int mmskin_slice_stats(const float* x, int64_t rows, int pitch, int c0, int C, float* mean, float* var, int dtype, void* workspace, void* stream);
/* VGG: 2x2 / stride 2 max-pool (floor) of a post-ReLU map y [N,C,H,W] (C a multiple of 8, H, W >= 2): pooled [N,C,H/2,W/2] and idx, the
 * argmax tap 0..3 (first maximum, row-major in the window) as bytes in the kernel's layout [N,H/2,W/2,C].  Backward: dz [N,C,H,W] =
 * dpool at each window's argmax where y > 0, else 0. */
int64_t mmskin_maxpool2_relu_workspace_bytes(int N, int C, int H, int W);
int mmskin_maxpool2_relu_forward(const float* y, float* pooled, unsigned char* idx, int N, int C, int H, int W, int dtype, void* workspace,
                                 void* stream);
int mmskin_maxpool2_relu_backward(const float* dpool, const float* y, float* dz, int N, int C, int H, int W, int dtype, void* workspace,
                                  void* stream);
/* VGG: AdaptiveAvgPool2d(7) of x [N,C,H,W] -> out [N,C,7,7] (fp32), and dout [N,C,7,7] -> dx [N,C,H,W] */
int64_t mmskin_adaptive_avgpool_workspace_bytes(int N, int C, int H, int W);
int mmskin_adaptive_avgpool_forward(const float* x, float* out, int N, int C, int H, int W, int dtype, void* workspace, void* stream);
int mmskin_adaptive_avgpool_backward(const float* dout, float* dx, int N, int C, int H, int W, int dtype, void* workspace, void* stream);
/* DynamicCNN: GroupNorm(8 groups, C) + ReLU of a raw convolution output y [N,C,H,W], optionally followed by MaxPool2d(2, 2) in the same
 * kernel.  pool = 0: out = z [N,C,H,W], idx unused (may be NULL).  pool = 1: out = the pooled z [N,C,H/2,W/2] (floor; the un-pooled z is
 * never stored) and idx = the argmax tap 0..3 of every pooled element, bytes in the kernel's layout [N,H/2,W/2,C], format and tie-break of
 * mmskin_maxpool2_relu_forward.  mean / rstd (may be NULL): the statistics [N,8], from per-workgroup (count, mean, M2) partials combined by
 * Chan's formula in fp64 -- no atomics, bitwise repeatable.  Backward: gout = the gradient at `out` (same shape) -> dy [N,C,H,W], dgamma,
 * dbeta [C] (may be NULL); it recomputes the statistics, the argmax bytes and the ReLU mask from y, no mask is stored.
 * Errors, before any launch: groups != 8 or C not a multiple of 64 (or above 1024): MMSKIN_ERR_UNSUPPORTED (workspace_bytes: -1); a
 * non-positive extent, or a map smaller than 2x2 with pool: MMSKIN_ERR_ARG. */
int64_t mmskin_groupnorm8_relu_workspace_bytes(int N, int C, int H, int W, int groups, int pool);
int mmskin_groupnorm8_relu_forward(const float* y, const float* gamma, const float* beta, float* out, unsigned char* idx, float* mean, float* rstd,
                                   int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace, void* stream);
int mmskin_groupnorm8_relu_backward(const float* gout, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma,
                                    float* dbeta, int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace,
                                    void* stream);
/* The same operator where AdaptiveAvgPool2d(1) is its only consumer (the DynamicCNN trunk's last layer): feat [N,C] fp32 = the mean over the
 * (pooled, with pool) map of relu(GroupNorm(y)), reduced through per-workgroup partial rows combined in a fixed order (bitwise repeatable).
 * No activation, argmax or gradient tensor is stored: backward takes dfeat [N,C], forms dfeat / (OH * OW) in registers and, with pool,
 * recomputes each window's argmax from y (first maximum, row-major; a NaN wins).  mean, rstd, dgamma, dbeta may be NULL.  Same refusals
 * as mmskin_groupnorm8_relu_*. */
int64_t mmskin_groupnorm8_relu_gap_workspace_bytes(int N, int C, int H, int W, int groups, int pool);
int mmskin_groupnorm8_relu_gap_forward(const float* y, const float* gamma, const float* beta, float* feat, float* mean, float* rstd, int N, int C,
                                       int H, int W, int groups, int pool, float eps, int dtype, void* workspace, void* stream);
int mmskin_groupnorm8_relu_gap_backward(const float* dfeat, const float* y, const float* gamma, const float* beta, float* dy, float* dgamma,
                                        float* dbeta, int N, int C, int H, int W, int groups, int pool, float eps, int dtype, void* workspace,
                                        void* stream);
/* the ResNet stem: conv7x7/2 (OIHW [64,3,7,7]) -> BN(train) -> ReLU -> maxpool3x3/2; y [N,64,PH,PW] */
int64_t mmskin_stem_workspace_bytes(int N, int H, int W);
int mmskin_stem_forward(const float* x, const float* w, const float* gamma, const float* beta, float* y, int N, int H,
                        int W, float eps, int dtype, void* workspace, void* stream);
int mmskin_stem_backward(const float* dy, const float* x, const float* w, const float* gamma, const float* beta,
                         float* dw, float* dgamma, float* dbeta, int N, int H, int W, float eps, int dtype,
                         void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fusion-head operators (fp32).  Replace nn.Linear / nn.LayerNorm / nn.MultiheadAttention(L=1) /
 * torch.sigmoid gates / MetaBlock / GatedAlteredResidualBlock pointwise math of
 * multimodalIntraInterModal.py:172-412, metablock.py:27-32, gatedResidualBlock.py:12-17. */
/* y[M,N] = x[M,K] @ w[N,K]^T + b (b may be null) ; relu!=0 applies max(.,0) */
int mmskin_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int K, int N, int relu,
                          void* stream);
/* dy[M,N]; if y_relu is given dy is first masked by (y_relu > 0).  Any of dx[M,K], dw[N,K], db[N] may be
 * null.  dy_scratch[M,N] is required when y_relu is given (holds the masked dy). */
int mmskin_linear_backward(const float* dy, const float* x, const float* w, const float* y_relu, float* dy_scratch,
                           float* dx, float* dw, float* db, int M, int K, int N, void* stream);
/* Backward of h = gelu(x w^T + b) (nn.Linear -> nn.GELU, the first half of timm's Mlp) from dh and the saved pre-activation z [M][N]:
 * gelu'(z) is applied inside the pass that converts the gradient to bf16 for the dgrad / wgrad GEMMs and sums it for db, so the fp32
 * gradient of the pre-activation is never written.  dy_scratch [M][N] is used only off the bf16-operand large-GEMM path. */
int mmskin_linear_gelu_backward(const float* dh, const float* x, const float* w, const float* z, float* dy_scratch, float* dx, float* dw,
                                float* db, int M, int K, int N, void* stream);
/* The bf16-operand large-GEMM path converts x to bf16 for the forward GEMM and again for the backward's weight-gradient GEMM.
 * mmskin_linear_x16_pitch > 0 (the row pitch in elements; 0: this shape / mode makes no such copy) lets a caller keep the forward's
 * copy instead: _forward_keep writes it to x16_keep [M][pitch] (bf16), _backward_keep takes it in x's place (y_relu / z_gelu: the saved
 * output of a fused ReLU or pre-activation of a following GELU, at most one, as in mmskin_linear_backward / _gelu_backward).
 * Same arithmetic as mmskin_linear_forward / _backward: the kept copy is the tensor the scratch conversion would have produced. */
int mmskin_linear_x16_pitch(int M, int K, int N);
/* Which GEMM route a Linear of M rows, K inputs and N outputs takes in the current operand mode (mmskin_set_linear_dtype), forward and
 * backward alike; -1 for a non-positive dimension.  Tests assert it so that a case keeps covering the route it was written for:
 *   MMSKIN_LINEAR_SMALL        the strided exact-f32 MFMA GEMM of linear.hip (any shape; M < 2048 or a width off the classes below)
 *   MMSKIN_LINEAR_BIG_F32      fp32 mode, M >= 2048, K and N multiples of 64: the exact-f32 implicit-GEMM conv kernels as a 1x1 conv
 *   MMSKIN_LINEAR_BIG_BF16     bf16 mode, same shape class: bf16 operands, fp32 accumulation
 *   MMSKIN_LINEAR_PADDED_BF16  bf16 mode, M >= 2048, K and N multiples of 8 and >= 32, not both multiples of 64: bf16 operands
 *                              zero-padded to 64-multiple widths */
enum { MMSKIN_LINEAR_SMALL = 0, MMSKIN_LINEAR_BIG_F32 = 1, MMSKIN_LINEAR_BIG_BF16 = 2, MMSKIN_LINEAR_PADDED_BF16 = 3 };
int mmskin_linear_route(int M, int K, int N);
int mmskin_linear_forward_keep(const float* x, const float* w, const float* b, const float* res, float* y, void* x16_keep, int M, int K,
                               int N, int relu, void* stream);   /* res (optional, fp32 [M][N]): y = res + act(x w^T + b) */
int mmskin_linear_backward_keep(const float* dy, const void* x16, const float* w, const float* y_relu, const float* z_gelu, float* dy_scratch,
                                float* dx, float* dw, float* db, int M, int K, int N, void* stream);
/* A transformer MLP (timm Mlp: fc1 -> GELU -> fc2) with gradients, without gelu(z) in fp32: mmskin_gelu_forward_bf16 writes
 * h16 [rows][cols_pad] = bf16(gelu(z)) (zero pad columns; cols_pad = mmskin_linear_x16_pitch of the second Linear), and
 * mmskin_linear_forward_x16 runs the second Linear on it; the backward hands h16 to mmskin_linear_backward_keep. */
int mmskin_gelu_forward_bf16(const float* z, void* h16, int64_t rows, int cols, int cols_pad, void* stream);
int mmskin_linear_forward_x16(const void* x16, const float* w, const float* b, const float* res, float* y, int M, int K, int N, int relu,
                              void* stream);                     /* res as above: the block's skip connection in the same pass */
/* The same MLP with timm's StarReLU (metaformer.py: y = s * relu(z)^2 + b, s and b learnable scalars, device pointers to one float
 * each) in GELU's place: mmskin_star_relu_forward_bf16 writes h16 = bf16(s * relu(z)^2 + b); the backward of the first Linear applies
 * 2 s relu(z) inside the pass that converts dh for the bf16 GEMMs and writes dsb[0] = sum dh * relu(z)^2, dsb[1] = sum dh (fixed-order
 * reductions: bitwise repeatable).  Needs the kept operand of mmskin_linear_forward_keep and N % 4 == 0. */
int mmskin_star_relu_forward_bf16(const float* z, const float* s, const float* b, void* h16, int64_t rows, int cols, int cols_pad,
                                  void* stream);
int mmskin_linear_star_relu_backward_keep(const float* dh, const void* x16, const float* w, const float* z, const float* s, float* dsb,
                                          float* dx, float* dw, float* db, int M, int K, int N, void* stream);
/* Elementwise StarReLU for every other shape: y = s * relu(z)^2 + b; backward dz = dy * 2 s relu(z) (dz may be NULL) and dsb as above */
int mmskin_star_relu_forward(const float* z, const float* s, const float* b, float* y, int64_t n, void* stream);
int mmskin_star_relu_backward(const float* dy, const float* z, const float* s, float* dz, float* dsb, int64_t n, void* stream);
/* y = LN(x)*g + b over the last dim, optional fused ReLU; mean/rstd [M] saved for backward.  b may be NULL (a LayerNorm without
 * bias, timm metaformer's norms): the backward then writes no db.  The same holds for mmskin_layernorm_forward_mixed. */
int mmskin_layernorm_forward(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd,
                             int M, int N, float eps, int relu, void* stream);
int mmskin_layernorm_backward(const float* dy, const float* x, const float* g, const float* b, const float* mean,
                              const float* rstd, float* dx, float* dg, float* db, int M, int N, int relu, void* stream);
/* out = sigmoid(z) * v                                  (multimodalIntraInterModal.py:219-235) */
int mmskin_sigmoid_gate_forward(const float* z, const float* v, float* out, int64_t n, void* stream);
int mmskin_sigmoid_gate_backward(const float* dout, const float* z, const float* v, float* dz, float* dv, int64_t n,
                                 void* stream);
/* out = g*a + (1-g)*q, g = sigmoid(z)                   (gatedResidualBlock.py:15-16) */
int mmskin_gated_mix_forward(const float* z, const float* a, const float* q, float* out, int64_t n, void* stream);
int mmskin_gated_mix_backward(const float* dout, const float* z, const float* a, const float* q, float* dz, float* da,
                              float* dq, int64_t n, void* stream);
/* out = sigmoid(tanh(V*t1) + t2)                        (metablock.py:31) */
int mmskin_metablock_gate_forward(const float* V, const float* t1, const float* t2, float* out, int64_t n, void* stream);
int mmskin_metablock_gate_backward(const float* dout, const float* V, const float* t1, const float* t2, float* dV,
                                   float* dt1, float* dt2, int64_t n, void* stream);
/* One Adam step (torch.optim.Adam: g += weight_decay p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)) over one flat fp32 range of n elements: parameters, gradient,
 * both moments; step counts from 1; 16-byte aligned pointers.  The optimizer step of train_pad_20.py:54,113 for a parameter arena. */
int mmskin_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int64_t step, void* stream);
/* inverted dropout with a counter-based generator; mask[n] bytes (1 keep / 0 drop) */
int mmskin_dropout_forward(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed,
                           uint64_t offset, void* stream);
/* dropout on attention probabilities [rows][L] (attention_probs_dropout_prob / nn.MultiheadAttention(dropout=p)): the (row, key) generator
 * every attention kernel of the library applies or regenerates (fused forward / backward, one-wave-per-row kernels), so the unfused
 * chain softmax -> dropout -> bmm drops the same probabilities; mask as mmskin_dropout_forward (backward: mmskin_dropout_backward) */
int mmskin_attn_dropout_forward(const float* x, float* y, uint8_t* mask, int64_t n, int L, float p, uint64_t seed, uint64_t offset,
                                void* stream);
int mmskin_dropout_backward(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream);
/* out[M, Na+Nb] = [a | b]; backward splits */
int mmskin_concat2_forward(const float* a, const float* b, float* out, int M, int Na, int Nb, void* stream);
int mmskin_concat2_backward(const float* dout, float* da, float* db, int M, int Na, int Nb, void* stream);
/* softmax attention for the metadata TabTransformer / generic L>1 attention:
 * q,k,v [B,H,L,Dh] -> o [B,H,L,Dh], softmax probs p [B,H,L,L] saved for backward.  drop_p > 0 applies
 * training-mode dropout to the probabilities (nn.MultiheadAttention(dropout=...) inside
 * nn.TransformerEncoderLayer, tab_transformer.py:20-27) with the counter-based generator of
 * mmskin_dropout_forward: backward must be given the same (drop_p, seed, offset). */
int mmskin_attention_forward(const float* q, const float* k, const float* v, float* o, float* p, int B, int H, int L,
                             int Dh, float drop_p, uint64_t seed, uint64_t offset, void* stream);
int mmskin_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* p,
                              float* dq, float* dk, float* dv, int B, int H, int L, int Dh, float drop_p,
                              uint64_t seed, uint64_t offset, void* stream);
/* MD-Net fusion head (multimodalMDNet.py:21-29 MetaNet gate, :47-55 MetaBlock, :94-100 sum + GAP):
 * pooled[nc] = mean_hw(sigmoid(z[nc]) * feat[nc][hw] + sigmoid(tanh(feat[nc][hw] * t1[nc]) + t2[nc])), feat NCHW */
int mmskin_mdnet_fuse_forward(const float* feat, const float* z, const float* t1, const float* t2, float* pooled,
                              int64_t NC, int HW, void* stream);
int mmskin_mdnet_fuse_backward(const float* dpooled, const float* feat, const float* z, const float* t1, const float* t2,
                               float* dfeat /* may be NULL */, float* dz, float* dt1, float* dt2, int64_t NC, int HW,
                               void* stream);
/* Encoder-layer pieces for the HuggingFace text encoders (loadImageModelClassifier.py:170-181, bert-base-uncased):
 * strided batched GEMM  C[b](m,n) = sum_k A[b](m,k) * B[b](n,k)  with A[b](m,k) = a[b*sab + m*sam + k*sak] (likewise B),
 * C[b] = c + b*scb with row pitch ldc -- QK^T, PV and their gradients;
 * row softmax with scale and an additive per-batch key mask (mask_add [batch][L], may be NULL); exact (erf) GELU. */
int mmskin_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, int64_t sam, int64_t sak, int64_t sab,
               int64_t sbn, int64_t sbk, int64_t sbb, int64_t ldc, int64_t scb, void* stream);
int mmskin_softmax_forward(const float* x, const float* mask_add, const float* bias /* [rows_per_batch][L] or NULL */,
                           float* y, int64_t rows, int L, int64_t rows_per_batch, float scale,
                           int causal /* GPT-2: key j <= query i */, void* stream);
int mmskin_softmax_backward(const float* dy, const float* y, float* dx, int64_t rows, int L, float scale, void* stream);
/* pieces of the timm transformer blocks (BEiT: LayerScale residuals, mean pooling over patch tokens, bias gradients) */
int mmskin_colsum(const float* x, float* out, int M, int N, void* stream);
int mmskin_scale_add_forward(const float* x, const float* b, const float* gamma, float* y, int64_t n, int C, void* stream);
int mmskin_scale_mul(const float* dy, const float* v, float* out, int64_t n, int C, int per_channel, void* stream);
int mmskin_token_mean_forward(const float* x, float* out, int B, int L, int E, int start, void* stream);
int mmskin_token_mean_backward(const float* dout, float* dx, int B, int L, int E, int start, void* stream);
/* Fused attention, bf16 MFMA with fp32 accumulation / softmax / I/O:  o = dropout(softmax(q k^T * scale + bias + mask)) v  in one
 * kernel; the [B, H, L, L] scores never reach memory.  Replaces the QK^T GEMM -> softmax -> dropout -> PV GEMM chain of the
 * transformer encoders (timm ViT / BEiT blocks, transformers' BertSelfAttention / GPT2Attention; loadImageModelClassifier.py
 * :117-121, :170-181) in bf16-operand mode.  q, k, v, o: io_dtype (MMSKIN_F32 or MMSKIN_BF16), element (b, h, l, d) at index b*sb + h*sh + l*sl + d, the twelve
 * ELEMENT strides given as strides12 = {q_sb, q_sh, q_sl, k_*, v_*, o_*} (q / k / v: multiples of 16 bytes; pointers 16-byte aligned), so the output of a
 * fused qkv Linear is read in place.  mask_add [B][L] additive key mask or NULL; bias [H][L][L] additive score bias or NULL
 * (BEiT's relative-position bias); causal != 0: key j > query i masked; drop_p: dropout on the probabilities with the library's
 * counter-based generator on the element index of the [B, H, L, L] tensor (seed, offset as mmskin_dropout_forward);
 * lse (optional) [B][H][L] = log-sum-exp of the scaled, biased scores.  Dh in {32, 64}. */
int mmskin_flash_attention_forward(const void* q, const void* k, const void* v, const float* mask_add, const float* bias,
                                   void* o, float* lse, int B, int H, int L, int Dh, const int64_t* strides12, int io_dtype,
                                   float scale, int causal, float drop_p, uint64_t seed, uint64_t offset, void* stream);
/* Backward of the fused attention for TRAINABLE transformer blocks in bf16-operand mode (csrc/flash_attn_bwd.hip): dq, dk, dv from
 * q, k, v, o, d(o) and the forward's lse, the probabilities recomputed tile by tile (no [B, H, L, L] tensor is kept).  All tensors fp32;
 * strides15 = element strides (batch, head, token) of q, k, v, o (= dout) and of dq / dk / dv (shared), last dims contiguous; bias
 * [H][L][L] needs its transpose biasT [H][key][query] beside it; delta [B][H][L] is scratch; ds_out (optional) [B][H][L][L] receives
 * dS = d loss / d(scaled, biased score) so the caller can sum the bias gradient over the batch; dropout regenerated from (seed, offset)
 * exactly as the forward drew it.  Replaces autograd through timm / transformers attention (loadImageModelClassifier.py:117-131,170-181). */
int mmskin_flash_attention_backward(const float* q, const float* k, const float* v, const float* o, const float* dout, const float* lse,
                                    const float* mask_add, const float* bias, const float* biasT, float* delta, float* dq, float* dk,
                                    float* dv, float* ds_out, int B, int H, int L, int Dh, const int64_t* strides15, float scale,
                                    int causal, float drop_p, uint64_t seed, uint64_t offset, void* stream);
/* Inference lane of the transformer encoders in bf16-operand mode (no gradient flows: frozen encoders, evaluation): activations pass
 * between layers as bf16, so no fp32 <-> bf16 conversion passes run.  linear_forward_ex: x [M][K] and y [M][N] are fp32
 * (dtype MMSKIN_F32) or bf16 (MMSKIN_BF16) independently; w [N][K], b [N] fp32; act 0 none / 1 ReLU / 2 exact GELU, fused into the GEMM
 * epilogue; shapes off the large-GEMM path are computed through the fp32 entry point.  layernorm_forward_mixed: nn.LayerNorm with the
 * result written as fp32 (y_f32) and / or bf16 (y_bf16); N % 4 == 0, N <= 2048. */
int mmskin_linear_forward_ex(const void* x, int x_dtype, const float* w, const float* b, void* y, int y_dtype, int M, int K, int N,
                             int act, void* stream);
/* Small-sequence attention, one wave per (batch, head): L <= 64, Dh 32 or 64, fp32, softmax(q k^T * scale) v with optional dropout on the
 * probabilities (generator of mmskin_dropout_forward on element ((b*H + h)*L + i)*L + j).  q / k / v -- and dq / dk / dv -- are addressed by
 * the (batch, head, token) ELEMENT strides qkv_strides[3], o / dO by o_strides[3] (rows 16-byte aligned, Dh contiguous), so the packed
 * [B, L, 3, H, Dh] output of a fused qkv Linear is read in place and o is written token-major.  lse [B*H][L] (row log-sum-exp) is all the
 * backward needs besides q, k, v, o: no probability tensor is stored.  Replaces timm's window / global Attention.forward and
 * nn.MultiheadAttention's core for those shapes with gradients (DaViT WindowAttention: 49 tokens, Dh 32; hip_davit.py). */
int mmskin_attention_rows_forward(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int L, int Dh,
                                  const int64_t* qkv_strides, const int64_t* o_strides, float scale, float drop_p, uint64_t seed,
                                  uint64_t offset, void* stream);
int mmskin_attention_rows_backward(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                                   float* dq, float* dk, float* dv, int B, int H, int L, int Dh, const int64_t* qkv_strides,
                                   const int64_t* o_strides, float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream);
/* Window attention on an image-major token grid [B][nwy*ws][nwx*ws] (ws*ws <= 64, Dh 32 or 64): window (image, wy, wx) attends over its
 * ws*ws tokens WHERE THEY SIT -- the kernels of mmskin_attention_rows_* with the window -> token map in their addressing, so timm's
 * window_partition / window_reverse (davit.py SpatialBlock.forward; reached through loadImageModelClassifier.py:117-131) are index
 * arithmetic, not copies.  q_tok / q_head: element strides between tokens / heads of q, k, v (and dq, dk, dv); o_tok / o_head of o
 * (and dO).  lse [B*nwy*nwx][H][ws*ws].  Dropout as mmskin_attention_rows_forward with batch = window index. */
int mmskin_window_attention_forward(const float* q, const float* k, const float* v, float* o, float* lse, int B, int nwy, int nwx, int ws,
                                    int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head, float scale,
                                    float drop_p, uint64_t seed, uint64_t offset, void* stream);
int mmskin_window_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                                     float* dq, float* dk, float* dv, int B, int nwy, int nwx, int ws, int H, int Dh, int64_t q_tok,
                                     int64_t q_head, int64_t o_tok, int64_t o_head, float scale, float drop_p, uint64_t seed,
                                     uint64_t offset, void* stream);
/* Shifted-window attention of the Swin Transformer (timm swin_transformer.py SwinTransformerBlock._attn around WindowAttention; reached
 * through loadImageModelClassifier.py:117-131, train_pad_20.py:516 "swin-tiny"), fp32, one wave per (window, head), ws*ws <= 64, Dh 32 or 64,
 * on an image-major token grid [B][Hp][Wp]: window (wy, wx), row (r, c) of the image ROLLED by (-shift_y, -shift_x) is the token
 * ((wy ws + r + shift_y) mod Hp, (wx ws + c + shift_x) mod Wp) of the un-rolled activation -- q / k / v are read and o (dq, dk, dv) written
 * there, so neither roll nor window_partition / window_reverse is a copy.  logit_ij = scale q_i . k_j
 * + bias_table[(r_i - r_j + ws - 1)(2 ws - 1) + (c_i - c_j + ws - 1)][h] - 100 [region(i) != region(j)], the regions being timm's slices
 * [0, Hp - ws), [Hp - ws, Hp - shift), [Hp - shift, Hp) per axis of the rolled image (an axis with shift 0: no wrap, no mask; timm shifts
 * per axis, an axis no longer than the window stays unshifted).  bias_table
 * [(2 ws - 1)^2][H]; q_tok / q_head / o_tok / o_head and dropout as mmskin_window_attention_*; lse [B*(Hp/ws)*(Wp/ws)][H][ws*ws].
 * The backward also writes dbias_table (may be NULL: not computed), the sum of d(logit_ij) over images, windows and the pairs of each
 * relative position, through per-window partials in `workspace` (mmskin_swin_attention_workspace_bytes, -1 for a shape the kernels
 * refuse) and the fp64 column reducer: no atomics, bitwise repeatable.  Errors before any launch: ws*ws > 64, Dh not 32 / 64, Hp or Wp
 * not a multiple of ws, a shift outside [0, ws), dropout outside [0, 1), a null or misaligned pointer. */
int64_t mmskin_swin_attention_workspace_bytes(int B, int Hp, int Wp, int ws, int H);
int mmskin_swin_attention_forward(const float* q, const float* k, const float* v, const float* bias_table, float* o, float* lse, int B, int Hp,
                                  int Wp, int ws, int shift_y, int shift_x, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head,
                                  float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream);
int mmskin_swin_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* bias_table, const float* o,
                                   const float* lse, float* dq, float* dk, float* dv, float* dbias_table, void* workspace, int B, int Hp,
                                   int Wp, int ws, int shift_y, int shift_x, int H, int Dh, int64_t q_tok, int64_t q_head, int64_t o_tok, int64_t o_head,
                                   float scale, float drop_p, uint64_t seed, uint64_t offset, void* stream);
/* Channel attention of DaViT's ChannelBlock (timm davit.py ChannelAttention.forward; loadImageModelClassifier.py:117-131), fp32, on
 * token-major operands: per (batch, group of Dh = 32 channels)  A = softmax(scale * q^T k) [32 x 32] (the reduction runs over the N tokens),
 * x[n][i] = sum_j A[i][j] v[n][j].  q / k / v (and dq / dk / dv): element strides q_tok between tokens and q_b between batches, group g
 * at channel offset 32 g -- the packed [B, N, 3, G, 32] output of a fused qkv Linear is read in place; x / dO likewise with o_tok / o_b.
 * attn [B*G][32][32] is written by the forward and read by the backward (may be null when no backward follows).
 * scratch: mmskin_channel_attention_scratch_floats(B, G, N) floats (0 for N <= 256: may be null) -- per-chunk partial products. */
int64_t mmskin_channel_attention_scratch_floats(int B, int G, int N);
int mmskin_channel_attention_forward(const float* q, const float* k, const float* v, float* x, float* attn, float* scratch, int B, int G,
                                     int N, int Dh, int64_t q_tok, int64_t q_b, int64_t o_tok, int64_t o_b, float scale, void* stream);
int mmskin_channel_attention_backward(const float* dO, const float* q, const float* k, const float* v, const float* attn, float* dq,
                                      float* dk, float* dv, float* scratch, int B, int G, int N, int Dh, int64_t q_tok, int64_t q_b,
                                      int64_t o_tok, int64_t o_b, float scale, void* stream);
/* linear_lane: the lane Linear with a frozen transformer block's elementwise tail fused into the GEMM epilogue,
 *   y = residual + gamma * dropout(act(x w^T + b))     (residual fp32 [M][N], gamma fp32 [N], dropout: the generator of mmskin_dropout_forward
 *   on element row * N + column; each optional).  w is fp32 or an already-converted bf16 copy (w_dtype).  Replaces the nn.Linear ->
 *   nn.Dropout -> residual add chain of transformers' BertSelfOutput / BertOutput and timm's `x + gamma * proj(...)` (hip_bert.py, hip_beit.py).
 *   Only for shapes on the large bf16 GEMM path (rows >= 2048, 64-multiple widths, bf16-operand mode): MMSKIN_ERR_ARG otherwise. */
int mmskin_linear_lane(const void* x, int x_dtype, const void* w, int w_dtype, const float* b, const float* gamma,
                       const float* residual, float drop_p, uint64_t seed, uint64_t offset, void* y, int y_dtype, int M, int K,
                       int N, int act, void* stream);
int mmskin_layernorm_forward_mixed(const float* x, const float* g, const float* b, float* y_f32, void* y_bf16, int M, int N,
                                   float eps, void* stream);
/* Operand type of the large Linear GEMMs (rows >= 2048, 64-multiple widths: the transformer backbones' and BERT's
 * projections): MMSKIN_F32 = exact-f32 MFMA (default, parity mode), MMSKIN_BF16 = bf16 operands with fp32 accumulation
 * (BASELINE configs[3] is quoted in bf16); in that mode widths that are only multiples of 8 (DaViT's 96 / 288) run on the same kernels
 * through zero-padded bf16 operand copies (mmskin_linear_forward / _backward; exact zeros from the pad columns).  Process-wide; the
 * environment variable MMSKIN_LINEAR_DTYPE sets the initial value. */
int mmskin_set_linear_dtype(int dtype);
int mmskin_get_linear_dtype(void);
/* y = a + b, b broadcast over the leading dimension when nb < n (residual sums, position embeddings) */
int mmskin_add(const float* a, const float* b, float* y, int64_t n, int64_t nb, void* stream);
int mmskin_gelu_forward(const float* x, float* y, int64_t n, void* stream);
int mmskin_gelu_backward(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int mmskin_gelu_tanh_forward(const float* x, float* y, int64_t n, void* stream);      /* GPT-2 "gelu_new" */
int mmskin_gelu_tanh_backward(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* fp32 NHWC depthwise 3x3 convolution (stride 1, pad 1) with its gradients -- ConvPosEnc of timm's DaViT blocks */
int64_t mmskin_dwconv3_scratch_floats(int N, int H, int W, int C);
int mmskin_dwconv3_forward(const float* x, const float* w, float* w_stage, float* y, int N, int H, int W, int C, void* stream);
int mmskin_dwconv3_backward(const float* dy, const float* x, const float* w, float* w_stage, float* scratch, float* dx, float* dw,
                            int N, int H, int W, int C, void* stream);
/* DaViT's convolutional position encoding (timm davit.py ConvPosEnc.forward: x + proj(x), proj = depthwise 3x3 with bias) in one pass each
 * way: y = x + dwconv3(x, w) + b; backward dx = dy + dgrad(dy), dw, db = sum(dy) (from the weight-gradient pass: db needs dw).
 * Staging / scratch as mmskin_dwconv3_*. */
int mmskin_conv_pos_enc_forward(const float* x, const float* w, const float* b, float* w_stage, float* y, int N, int H, int W, int C,
                                void* stream);
int mmskin_conv_pos_enc_backward(const float* dy, const float* x, const float* w, float* w_stage, float* scratch, float* dx, float* dw,
                                 float* db, int N, int H, int W, int C, void* stream);
/* CAFormer SepConv core (timm metaformer.py SepConv: act1 -> dwconv) on fp32 NHWC z [N, H, W, C], C % 4 == 0:
 * y = dwconv7x7(s * relu(z)^2 + b, w), w [C, 1, 7, 7], stride 1, pad 3, no bias; s, b: device pointers to one float each.  The backward
 * reads dy and z once and writes dz (may be NULL), dw [C, 1, 7, 7] (may be NULL) and dsb[0..1] = the gradients of s and b (may be
 * NULL); its reductions run in a fixed order (bitwise repeatable).  scratch: mmskin_dw7_star_scratch_floats(N, H, W, C) floats. */
int64_t mmskin_dw7_star_scratch_floats(int N, int H, int W, int C);
int mmskin_dw7_star_forward(const float* z, const float* w, const float* s, const float* b, float* y, int N, int H, int W, int C,
                            void* stream);
int mmskin_dw7_star_backward(const float* dy, const float* z, const float* w, const float* s, const float* b, float* scratch, float* dz,
                             float* dw, float* dsb, int N, int H, int W, int C, void* stream);
/* CoaT factorized attention with convolutional relative position encoding (timm coat.py FactorAttnConvRelPosEnc.forward with its
 * ConvRelPosEnc) on the token-major packed output of a fused qkv Linear, fp32: qkv [B, N, 3, 8, Ch], N = 1 + H * W (token 0 = class token),
 * Ch in {8, 16, 32, 40, 64} -> att [B, N, 8 * Ch]:  att = Ch^-0.5 * q (softmax_N(k)^T v) + q_img . (dwconv(v_img) + bias), heads 0-1 through
 * w3 [2Ch, 1, 3, 3], heads 2-4 through w5 [3Ch, 1, 5, 5], heads 5-7 through w7 [3Ch, 1, 7, 7] ("same" padding); the class row gets no
 * convolution term.  The forward also writes F [B * 8, Ch, Ch] = softmax(k)^T v and stats [B * 8, 2, Ch] (column maximum and exp-sum of k)
 * for the backward, which writes d(qkv) in the packed layout and the six convolution gradients (every element written).  All reductions run
 * in a fixed order (bitwise repeatable).  scratch: mmskin_factor_attention_scratch_floats(B, H, W, Ch, backward) floats. */
int64_t mmskin_factor_attention_scratch_floats(int B, int H, int W, int Ch, int backward);
int mmskin_factor_attention_forward(const float* qkv, const float* w3, const float* b3, const float* w5, const float* b5, const float* w7,
                                    const float* b7, float* att, float* F, float* stats, float* scratch, int B, int H, int W, int Ch,
                                    void* stream);
int mmskin_factor_attention_backward(const float* dO, const float* qkv, const float* w3, const float* b3, const float* w5, const float* b5,
                                     const float* w7, const float* b7, const float* F, const float* stats, float* dqkv, float* dw3,
                                     float* db3, float* dw5, float* db5, float* dw7, float* db7, float* scratch, int B, int H, int W,
                                     int Ch, void* stream);
/* CoaT's convolutional position encoding (timm coat.py ConvPosEnc.forward) on a token tensor with a class token, fp32 x [B, 1 + H * W, C]:
 * the class row passes through, image rows y = x + dwconv3(x, w) + b on the H x W grid (w [C, 1, 3, 3]) -- no slice / concat copies.
 * backward: dx = dy + dgrad(dy) on the image rows, dy on the class row; dw, db (each may be NULL) through
 * mmskin_conv_pos_enc_tokens_scratch_floats(B, H, W, C) floats of scratch, summed in a fixed order. */
int64_t mmskin_conv_pos_enc_tokens_scratch_floats(int B, int H, int W, int C);
int mmskin_conv_pos_enc_tokens_forward(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int C, void* stream);
int mmskin_conv_pos_enc_tokens_backward(const float* dy, const float* x, const float* w, float* scratch, float* dx, float* dw, float* db, int B,
                                        int H, int W, int C, void* stream);
/* embedding gather for categorical metadata columns: table [ncols, card, E]; ids [B, ncols] int64 */
int mmskin_embedding_forward(const float* table, const int64_t* ids, float* out, int B, int ncols, int card, int E,
                             void* stream);
int mmskin_embedding_backward(const float* dout, const int64_t* ids, float* dtable, int B, int ncols, int card, int E,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Input side of the path: what the reference's Dataset does on the host before `model(image, metadata)`.
 * resize_u8: the val/test transform's A.Resize(h, w) (skinLesionDatasets.py:116-120 = cv2.resize INTER_LINEAR on the
 * decoded uint8 HWC image): [N][src_h][src_w][3] -> [N][dst_h][dst_w][3], uint8; Normalize + ToTensor then run inside
 * mmskin_backbone_forward_u8.
 * metadata_encode: OneHotEncoder(handle_unknown='ignore') + StandardScaler transform (skinLesionDatasets.py:133-183):
 * codes int32 [batch][n_cat] = index of the value among the column's fitted (sorted) categories, -1 = unseen;
 * col_offset int32 [n_cat + 1] = first one-hot slot of every column (col_offset[n_cat] = onehot_width); numeric fp32
 * [batch][n_num] (NaN = missing -> nan_fill, the reference's fillna(-1)); out fp32 [batch][onehot_width + n_num] =
 * one-hot blocks | (numeric - mean) / scale -- the tensor the reference hands to text_fc. */
/* Patch extraction for the patch-embedding GEMMs of the timm backbones (PatchEmbed 16x16/16 of ViT / BEiT, DaViT's 7x7/4
 * stem and 2x2/2 downsample convolutions; loadImageModelClassifier.py:117-121): cols [N*OH*OW][C*k*k], columns ordered
 * (c, ky, kx) like conv.weight.flatten(1), zeros for padding taps; x is fp32 NCHW (channels_last = 0) or NHWC (= 1).
 * backward: dx (same layout as x, every element written) = the transpose (sum over the windows containing a pixel). */
int mmskin_im2col_forward(const float* x, int N, int C, int H, int W, int k, int stride, int pad, int channels_last, float* cols,
                          void* stream);
int mmskin_im2col_backward(const float* dcols, int N, int C, int H, int W, int k, int stride, int pad, int channels_last, float* dx,
                           void* stream);
int mmskin_resize_u8(const uint8_t* src_nhwc, int N, int src_h, int src_w, uint8_t* dst_nhwc, int dst_h, int dst_w,
                     void* stream);
int mmskin_metadata_encode(const int32_t* codes, int n_cat, const int32_t* col_offset, int onehot_width, const float* numeric,
                           int n_num, const float* mean, const float* scale, float nan_fill, float* out, int batch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-time image augmentation (skinLesionDatasets.py:74-113, the A.Compose of the train transform) as ONE fused kernel
 * on the raw uint8 NHWC batch: Rotate(limit 45, BORDER_REFLECT) -> HorizontalFlip -> VerticalFlip -> GaussianBlur ->
 * CoarseDropout(fill 0) -> HueSaturationValue -> RandomBrightnessContrast(brightness_by_max), each stage skipped per sample
 * when its flag is off; Normalize + ToTensor then run inside mmskin_backbone_forward_u8.  The random draws happen on the host
 * (mmskin.preprocess.TrainAugment.sample); the kernel is a pure function of (src, table).  One record per sample, 160 bytes:
 *   minv[6]    float64  the INVERTED 2x3 matrix warpAffine uses, row major: src_x = minv[0]*x + minv[1]*y + minv[2],
 *                       src_y = minv[3]*x + minv[4]*y + minv[5] (getRotationMatrix2D about (W/2-0.5, H/2-0.5), inverted in
 *                       float64 on the host); read only when MMSKIN_AUG_ROTATE is set
 *   flags      uint32   MMSKIN_AUG_* bits, one per stage
 *   ksize      int32    GaussianBlur kernel size: 1 (no blur), 3, 5 or 7
 *   taps[4]    uint16   8-bit fixed-point Gaussian taps, taps[j] = weight at distance j from the centre (0 beyond ksize/2);
 *                       taps[0] + 2*(taps[1] + taps[2] + taps[3]) = 256
 *   hue, sat, val int32 floor() of the HueSaturationValue shifts: hue in [0, 180) (already reduced mod 180), sat / val in
 *                       [-255, 255]; H -> (H + hue) mod 180, S / V -> clip(x + shift, 0, 255)
 *   alpha, beta255 float32  RandomBrightnessContrast LUT: clip(float32(i) * alpha + beta255, 0, 255) truncated,
 *                       beta255 = float32(beta * 255); the multiply and the add each round to float32
 *   n_holes    int32    0..MMSKIN_AUG_MAX_HOLES CoarseDropout rectangles in use
 *   holes[8][4] int16   x1, y1, x2, y2 (half open, clipped to the image by the kernel), set to 0
 *   reserved[2] uint32  zero
 * Rotate is warpAffine's 8-bit INTER_LINEAR path (10-bit fixed-point row / column terms rounded to the 1/32 grid, 15-bit
 * weights summing to 32768, (sum + 2^14) >> 15); the flips evaluate that same formula at the flipped destination index;
 * GaussianBlur is separable with BORDER_REFLECT_101 and rounds half up once, after the vertical pass.
 * params_host is the table, N records in host memory: the call validates it (ksize, n_holes, taps, hue) and then uploads
 * exactly those bytes on `stream` into params_scratch, N records of device memory that the caller only provides (its
 * previous content is ignored; it must stay allocated until the kernel has run, in stream order).  The host table may be
 * reused as soon as the call returns.  Errors: H or W < 1 (or > 16384), N < 1 (or > 65535), ksize outside {1, 3, 5, 7}, n_holes outside
 * 0..MMSKIN_AUG_MAX_HOLES, taps that do not sum to 256, src == dst. */
#define MMSKIN_AUG_ROTATE 1u
#define MMSKIN_AUG_HFLIP 2u
#define MMSKIN_AUG_VFLIP 4u
#define MMSKIN_AUG_BLUR 8u
#define MMSKIN_AUG_DROPOUT 16u
#define MMSKIN_AUG_HSV 32u
#define MMSKIN_AUG_BC 64u
#define MMSKIN_AUG_MAX_HOLES 8
typedef struct mmskin_augment_params {
  double minv[6];
  uint32_t flags;
  int32_t ksize;
  uint16_t taps[4];
  int32_t hue, sat, val;
  float alpha, beta255;
  int32_t n_holes;
  int16_t holes[MMSKIN_AUG_MAX_HOLES][4];
  uint32_t reserved[2];
} mmskin_augment_params;
int mmskin_train_augment_u8(const uint8_t* src_nhwc, int N, int H, int W, const mmskin_augment_params* params_host,
                            mmskin_augment_params* params_scratch, uint8_t* dst_nhwc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Score-CAM (interpretability/ScoreCam.py:62-155), forward only.  fmap is the hooked feature map of ONE image, fp32
 * [C, fh, fw]; image is fp32 [3, H, W].  cam_c = min-max normalised torch.nn.Upsample(size=(H, W), mode='bilinear')
 * (align_corners=False) of channel c: src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = min(floor(src), in - 1),
 * i1 = min(i0 + 1, in - 1), value f0 + l * (f1 - f0) along x, then along y (weights 1 - l and l in the form that keeps a
 * constant channel exactly constant); a flat channel (max == min) gives an all-zero cam.  The normalised maps
 * are never stored: every kernel recomputes them from fmap, every multiply and add rounded to fp32 on its own.
 *   minmax   minmax[c] = (min, max) of the UPSAMPLED map of channel c, [C, 2]
 *   mask     out[j, ch, y, x] = image[ch, y, x] * cam_{c0 + j}[y, x] for j < n and 0 for n <= j < n_pad, fp32 NCHW
 *            [n_pad, 3, H, W]: the masked inputs of one chunk of channels, the ragged last chunk padded to the batch shape
 *   combine  heat[y, x] = sum_c scores[c] * cam_c[y, x] accumulated in fp32 in ascending channel order, ReLU, then
 *            (heat - min) / (max - min) over the [H, W] map.  The last division has no zero guard (ScoreCam.py:154): a flat
 *            combined map comes back as NaN.  channel_block: channels staged through LDS per round, 0 = as many as fit
 * minmax must come from mmskin_scorecam_minmax with the same fmap and sizes.  Errors (nothing is launched): an extent < 1,
 * H < fh or W < fw, n < 1, n > n_pad, c0 < 0 or c0 + n > C; MMSKIN_ERR_UNSUPPORTED for a feature map of more than 12272
 * samples per channel (the LDS tile). */
int mmskin_scorecam_minmax(const float* fmap, int C, int fh, int fw, int H, int W, float* minmax, void* stream);
int mmskin_scorecam_mask(const float* fmap, const float* minmax, const float* image, int C, int fh, int fw, int H, int W, int c0,
                         int n, int n_pad, float* out, void* stream);
int mmskin_scorecam_combine(const float* fmap, const float* minmax, const float* scores, int C, int fh, int fw, int H, int W,
                            int channel_block, float* heat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grad-CAM and Grad-CAM++ (interpretability/gradcam_atualizado.py:230-306), forward only, for R rows at once.  acts is the
 * hooked activation of N images, fp32 [N, C, fh, fw]; row_image is int32 [R] and maps a row to its image.  Its entries are
 * clamped to [0, N - 1] on the device: a bad entry reads the nearest image, never other memory.
 *   weights  weights[r, c], [R, C].  The gradient g at the activations is
 *              dfeat != NULL: g[r, c, i, j] = jac[row_image[r], c, i, j] * dfeat[r, c], jac [N, C, fh, fw], dfeat [R, C]
 *                             (a target whose tail to the pooled features is diagonal in the channel: jac is
 *                             d sum(features) / d acts, dfeat is d score / d features of the row)
 *              dfeat == NULL: g[r] = jac[r], jac [R, C, fh, fw] (any other target: the gradients autograd returned)
 *            mode 0, Grad-CAM:   w = mean_ij g
 *            mode 1, Grad-CAM++: alpha = g^2 / (2 g^2 + sum_ij(acts * g^3) + 1e-8), w = sum_ij alpha * relu(g)
 *            fp32 accumulation in a fixed order, no atomics
 *   map      raw[r, i, j] = sum_c weights[r, c] * acts[row_image[r], c, i, j], [R, fh, fw], fp32 accumulation in a fixed order
 *            (results repeat bit for bit); cam[r] = bilinear upsample (align_corners=False, the sampling of Score-CAM above)
 *            to [H, W] of (relu(raw[r]) - min) / (max - min + 1e-8), min and max over the row's fh x fw map, [R, H, W].
 *            Normalisation comes before the upsample (the reference's _normalize, then F.interpolate): the opposite order from
 *            Score-CAM.  A flat map gives zeros, not NaN.
 * Errors (nothing is launched): an extent < 1, R < 1, H < fh or W < fw, a mode other than 0 or 1; MMSKIN_ERR_UNSUPPORTED for a
 * feature map of more than 4096 samples per channel (the map kernel's LDS tile). */
int mmskin_gradcam_weights(const float* acts, const float* jac, const float* dfeat, const int32_t* row_image, int N, int R, int C,
                           int fh, int fw, int mode, float* weights, void* stream);
int mmskin_gradcam_map(const float* acts, const float* weights, const int32_t* row_image, int N, int R, int C, int fh, int fw, int H,
                       int W, float* raw, float* cam, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Faithfulness scores of a saliency map (mmskin.faithfulness.CamFaithfulness): deletion / insertion curves (Petsiuk et al.,
 * RISE) and average drop / increase in confidence (Chattopadhay et al., Grad-CAM++), forward only.  images and baseline are
 * fp32 [N, 3, H, W], saliency fp32 [N, H * W].
 *   rank     rank[n, p] = #{q : s[n,q] > s[n,p]} + #{q < p : s[n,q] == s[n,p]}, int32 [N, HW]: descending saliency, ties by
 *            ascending (row-major) pixel index; -0.0 == +0.0; a NaN ranks below every number and NaNs tie among themselves.
 *            Pair counting on integer keys: no atomics, a function of the input alone.
 *   blur     separable Gaussian of `planes` planes of H x W with reflect padding (no edge repeat): horizontal pass, then vertical,
 *            each acc = acc + taps[t] * x in ascending t from 0, every operation rounded to fp32 on its own.  taps is HOST memory,
 *            ksize floats (the caller computes them in fp64, normalises and rounds them); it is read before the call returns.
 *   mean     out[plane, :] = the plane's mean: fp64 partial sums of stride 256, a halving tree, one division, one rounding.
 *   perturb  out[j] for j < n is the image of row-table entry rows[j] = (image, k, mode), int32 [n, 3]; rows n .. n_pad are zeros;
 *            fp32 [n_pad, 3, H, W].  With count = (k * H * W) / S (integer):
 *              mode 0, deletion:     rank < count ? baseline : image
 *              mode 1, insertion:    rank < count ? image : baseline
 *              mode 2, explanation:  baseline + h * (image - baseline), h = min(max(saliency, 0), 1) (NaN -> 0), difference,
 *                                    product and sum each rounded to fp32
 *            per pixel, the same for the three colour planes.  Entries are clamped on the device (image to [0, N - 1], k to
 *            [0, S], mode to [0, 2]): a bad entry reads the nearest image, never other memory.
 *   curves   logits fp32 [>= N * P, C], P = 2 S + 3: row n * P + k is deletion step k of image n, n * P + S + 1 + k insertion
 *            step k, n * P + 2 S + 2 the explanation image.  target int32 [N] (clamped to [0, C - 1]) or NULL = the first largest
 *            logit of the image's deletion step 0, the clean image.  All in fp64 in a fixed order, no atomics:
 *              curves  [2, N, S + 1]  soft-max probability of the target class: deletion, insertion
 *              scalars [4, N]         deletion area, insertion area (trapezoids over x = k / S), average drop
 *                                     max(0, p - p_expl) / p, increase 1[p_expl > p], p = deletion step 0
 *              means   [4]            the means of the four over the N images;  target_out int32 [N] the class used
 * Errors (nothing is launched): an extent < 1, S < 1, S > 1024, S > H * W (perturb), n < 1, n > n_pad, ksize even or > 31,
 * ksize / 2 >= min(H, W); MMSKIN_ERR_UNSUPPORTED for H * W above mmskin_faith_max_pixels() = 65536 (rank, perturb). */
int mmskin_faith_max_pixels(void);
int mmskin_faith_rank(const float* saliency, int N, int HW, int32_t* rank, void* stream);
int mmskin_faith_blur(const float* x, int planes, int H, int W, const float* taps, int ksize, float* out, void* stream);
int mmskin_faith_mean(const float* x, int planes, int HW, float* out, void* stream);
int mmskin_faith_perturb(const float* images, const float* baseline, const int32_t* rank, const float* saliency, const int32_t* rows,
                         int N, int H, int W, int S, int n, int n_pad, float* out, void* stream);
int mmskin_faith_curves(const float* logits, const int32_t* target, int N, int S, int C, double* curves, double* scalars,
                        double* means, int32_t* target_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RISE saliency (Petsiuk et al., 2018; mmskin.rise.RISE), forward only: the image under many random smooth masks, the masks
 * averaged with the target-class probability of their forward as the weight.  A mask is a pure function of (seed, mask index j,
 * pixel); every kernel evaluates it in registers and no mask tensor exists in device memory.
 *
 * The mask.  grid = g (2 .. 16), p1 strictly inside (0, 1), image H x W, cell size ch = ceil(H / g), cw = ceil(W / g).  Mask j
 * has a binary cell grid G_j[g + 1][g + 1] and a shift (dy_j, dx_j), 0 <= dy < ch, 0 <= dx < cw, shared by all images of a call:
 *   key = mix64(seed), word(j, q) = mix64(key ^ (j * 1024 + q))      (mix64: the splitmix64 finaliser of every generator here)
 *   cell q = row * (g + 1) + col is on iff (word(j, q) >> 40) < floor(p1 * 2^24 + 0.5)
 *   dy = ((word(j, 1022) >> 32) * ch) >> 32,  dx = ((word(j, 1023) >> 32) * cw) >> 32        ((g + 1)^2 <= 289 < 1022)
 * Its value at pixel (y, x) is the bilinear upsample of G_j by (ch, cw) with half-pixel centres (align_corners = false) and edge
 * clamp, cropped at (dy, dx), stated in integers:
 *   ty = 2 (y + dy) + 1 - ch,  iy = floor(ty / (2 ch)),  ry = ty - iy * 2 ch;  tx, ix, rx likewise with x, dx, cw
 *   m = [ (2ch - ry)(2cw - rx) G[iy][ix] + (2ch - ry) rx G[iy][ix+1] + ry (2cw - rx) G[iy+1][ix] + ry rx G[iy+1][ix+1] ] / (4 ch cw)
 * with every index clamped to 0 .. g.  The numerator is an integer below 2^24; the kernels convert it and 4 ch cw to fp32 (both
 * exact) and divide once, so m is the correctly rounded fp32 of an exact rational.  Sums take that fp32 value widened to double.
 *
 *   masks       out fp32 [n, H, W] = masks j0 .. j0 + n - 1 (tests and drawing; not on the hot path)
 *   apply       one chunk of model inputs, fp32 [n_pad, 3, H, W]: row r0 + i of the image-major row space R = N * n_masks is
 *               (image r / n_masks, mask r % n_masks); out[i] = baseline + m * (image - baseline), difference, product and sum each
 *               rounded to fp32; the three colour planes of a pixel share m.  Rows n .. n_pad are zeros.  images and baseline
 *               are fp32 [N, 3, H, W].
 *   accumulate  launched once, after all chunks.  logits fp32 [>= N * n_masks, K] in that row order, clean_logits fp32 [N, K] of
 *               the unmasked images, target int32 [N] (clamped to [0, K - 1]) or NULL = the first largest clean logit, taken on
 *               the device.  w[n][j] = the fp64 soft-max probability of the target class of row (n, j).  Outputs, fp64, every sum
 *               in ascending j with one owner per element and no atomics (bitwise repeatable):
 *                 saliency_sum [N, H, W]  sum_j w[n][j] * m_j(p)          coverage [H, W]  sum_j m_j(p)
 *                 clean_prob   [N]        the probability of the target class on the clean image;  target_used int32 [N]
 *               workspace: mmskin_rise_workspace_bytes(N, n_masks) bytes (w, and 80 bytes of cell table per mask), 8-byte aligned.
 * Errors (nothing is launched): grid outside 2 .. 16, p1 outside (0, 1), an extent < 1, n_masks < 1, n < 1, n > n_pad,
 * r0 < 0 or r0 + n > N * n_masks, N, n or n_pad above 65535, K above 65536, a null argument; MMSKIN_ERR_UNSUPPORTED for n_masks
 * (masks: j0 + n) above 2^20 and for H * W above mmskin_faith_max_pixels().  workspace_bytes answers -1 for what it refuses. */
int mmskin_rise_masks(uint64_t seed, int j0, int n, int grid, double p1, int H, int W, float* out, void* stream);
int mmskin_rise_apply(const float* images, const float* baseline, int N, int H, int W, uint64_t seed, int grid, double p1, int n_masks,
                      int64_t r0, int n, int n_pad, float* out, void* stream);
int64_t mmskin_rise_workspace_bytes(int N, int n_masks);
int mmskin_rise_accumulate(const float* logits, const int32_t* target, const float* clean_logits, int N, int K, int H, int W,
                           uint64_t seed, int grid, double p1, int n_masks, double* saliency_sum, double* coverage, double* clean_prob,
                           int32_t* target_used, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Metadata-sensitivity sweeps (interpretability/flip_rate.py:164-256, inference_all_folds.py:116-140,
 * analyze_prediction_uncertainty.py:166-272): the image is encoded once, the fusion head runs on V metadata variants of the
 * batch (mmskin.sweep.MetadataSweep); these are the kernels before and after the head.
 *
 * metadata_variants: mutate + one-hot + standardise, fused.  codes, col_offset, onehot_width, numeric, mean, scale, nan_fill
 * are the inputs of mmskin_metadata_encode.  Columns are numbered categorical first: 0 .. n_cat - 1 are the columns of
 * `codes`, n_cat .. n_cat + n_num - 1 those of `numeric`.  The variant table holds V records of 32 bytes, one mutation of one
 * column each:
 *   op        int32    MMSKIN_META_*:
 *                        NONE        identity (the baseline is variant 0 by convention); column, a, b, value are ignored
 *                        CAT_SET     code = a
 *                        CAT_TOGGLE  code = (code == a) ? b : a    (the reference's `not bool(x)`, its gender swap and its
 *                                    FACE / FOREARM rule, flip_rate.py:167-181, each with the right (a, b))
 *                        NUM_ADD     raw value + `value`, before filling and scaling; NaN stays NaN and is then filled,
 *                                    as float('nan') + 5 followed by fillna(-1)
 *                        NUM_SET     raw value = `value`
 *   column    int32    the mutated column, numbered as above
 *   a, b      int32    category codes of that column, -1 .. count - 1 (-1 = a value unseen at fit time: an all-zero block)
 *   value     float32  operand of NUM_ADD / NUM_SET
 *   reserved[3] uint32 zero
 * mask (optional, device) uint8 [V][batch][n_cat + n_num], applied AFTER the record's op: non-zero blanks the cell -- a
 * numeric becomes missing (-> nan_fill), a categorical takes missing_code[column] (device int32 [n_cat]: the code of the
 * column's "EMPTY" category, or -1 when that value was not seen at fit time, which encodes as an all-zero block like
 * handle_unknown='ignore').  out fp32 [V][batch][out_width]: columns [0, onehot_width + n_num) as mmskin_metadata_encode
 * writes them (the same (x - mean) / scale: an unmutated, unmasked variant equals its output bit for bit), zeros beyond;
 * a smaller out_width truncates (the reference pads or cuts to the checkpoint's vocab_size, inference_all_folds.py:105-112).
 * A pure function of its inputs, no atomics, every output element written exactly once (no pre-zeroing).
 * variants_host is the table in host memory and col_offset_host a host copy of col_offset: the call validates the table
 * against them and then uploads exactly those bytes on `stream` into variants_scratch, V records of device memory that the
 * caller only provides (it must stay allocated until the kernel has run, in stream order).  Errors (nothing is launched):
 * V, batch or out_width < 1, no column at all, an unknown op, a column outside [0, n_cat + n_num), a CAT_* op on a numeric
 * column or a NUM_* op on a categorical one, a code outside -1 .. count - 1 of its column.
 *
 * sweep_reduce: logits in, answers out, nothing to the host.  logits [V][batch][C], fp32 (logits_dtype 0) or bf16 (1, what
 * the head delivers on the inference lane); base fp32 [batch][C], the baseline logits; labels int32 [batch] or NULL.
 * Per (v, b):
 *   probs   fp32 [V][batch][C]  soft-max of the logits, exp(x - max) / sum (NULL: not written)
 *   pred    int32 [V][batch]    FIRST index of the maximum LOGIT (the reference takes the argmax of the fp32 soft-max; the two
 *                               differ only where rounding in exp makes two probabilities equal although the logits differ)
 *   margin  fp32 [V][batch]     top-1 minus top-2 logit
 *   stats   fp32 [V][batch][4]  on p = clip(probs, 1e-12, 1) / sum (safe_probs) of the variant and q of the baseline:
 *                               entropy -sum p ln p (nats), KL(p || q), JS(p, q) = KL(p || m) / 2 + KL(q || m) / 2 with
 *                               m = (p + q) / 2, and p[base_pred] - q[base_pred]
 * Counters, ADDED TO so that several batches accumulate (the caller zeroes them once): flips int32 [V] (pred != base_pred),
 * transitions int32 [V][C][C] indexed [base_pred][pred], and with labels confusion int32 [V][C][C] indexed [label][pred].
 * Each workgroup counts into an LDS histogram and issues one integer atomic add per non-zero cell: the result does not
 * depend on launch order.  labels live on the device, so they are not inspected on the host: a row whose label is outside
 * [0, C) is skipped in `confusion` only.  2 <= C <= 64 (one class per lane), anything else is MMSKIN_ERR_UNSUPPORTED;
 * V or batch < 1 and null arguments are errors.  Nothing is launched on an error. */
#define MMSKIN_META_NONE 0
#define MMSKIN_META_CAT_SET 1
#define MMSKIN_META_CAT_TOGGLE 2
#define MMSKIN_META_NUM_ADD 3
#define MMSKIN_META_NUM_SET 4
typedef struct mmskin_meta_variant {
  int32_t op;
  int32_t column;
  int32_t a, b;
  float value;
  uint32_t reserved[3];
} mmskin_meta_variant;
int mmskin_metadata_variants(const int32_t* codes, int n_cat, const int32_t* col_offset, const int32_t* col_offset_host,
                             int onehot_width, const float* numeric, int n_num, const float* mean, const float* scale,
                             float nan_fill, const mmskin_meta_variant* variants_host, mmskin_meta_variant* variants_scratch, int V,
                             const uint8_t* mask, const int32_t* missing_code, float* out, int batch, int out_width, void* stream);
int mmskin_sweep_reduce(const void* logits, int logits_dtype, const float* base, const int32_t* labels, int V, int batch, int C,
                        float* probs, int32_t* pred, float* margin, float* stats, int32_t* flips, int32_t* transitions,
                        int32_t* confusion, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shapley values of the metadata columns on the model itself (csrc/shapley.hip, mmskin.shapley.MetadataShapley): the image is
 * encoded once, the fusion head runs on the rows of an antithetic permutation walk, these are the kernels before and after
 * the head.  Players are the encoder's M = n_cat + n_num COLUMNS (a categorical column is its whole one-hot block), numbered
 * categorical first as in metadata_variants.  With G background rows, P permutations and K = 2 P (M - 1):
 *     v(S) = (1/G) sum_g out(head(f, mix(x, b_g, S)))       mix takes column j from x if j is in S, else from b_g
 *     phi_j = (1/2P) sum_p [ v(S_{q+1}) - v(S_q) + v(T_{M-q}) - v(T_{M-q-1}) ]     q = position of j in permutation p
 * S_n / T_n = the first / last n entries of the permutation; S_0 = T_0 = empty and S_M = T_M = all are shared by all p.
 *
 * Row order of a batch's walk, mmskin_shapley_rows = batch (1 + G + K G) rows (-1 for extents out of range):
 *     rows [0, batch (K+1) G)      row ((b (K+1) + k) G + g): sample b, coalition k, background row g, where
 *                                  k = (p 2 + side) (M-1) + (n-1) is S_n (side 0) or T_n (side 1) of permutation p,
 *                                  n = 1 .. M-1, and k = K is the empty coalition (G rows)
 *     the last `batch` rows        row b of them is x_b unmixed (v(all), one row per sample)
 * Both entry points take a row range [row0, row1) of that order and the buffer of THAT RANGE (out / logits point at row0).
 *
 * shapley_coalitions: codes int32 [batch][n_cat], numeric fp32 [batch][n_num] (NaN = missing) of the explained rows, bg_codes
 * [G][n_cat] and bg_numeric [G][n_num] of the background; col_offset, onehot_width, mean, scale, nan_fill as
 * mmskin_metadata_encode takes them and col_offset_host a host copy; perm_host int32 [P][M] in HOST memory, validated (every
 * row a permutation of 0 .. M-1), inverted and uploaded on `stream` into pos_scratch, P x M int32 of device memory that the
 * caller only provides (allocated until the kernel has run).  out fp32 [row1 - row0][out_width]: each row is the encoding of
 * the mixed raw row exactly as mmskin_metadata_encode gives it (bit for bit; -1 = unseen code = all-zero block, NaN filled),
 * zeros beyond the encoder's width, cut when out_width is smaller.  Every element is written once, no atomics.
 *
 * shapley_reduce: logits [row1 - row0][C], fp32 (logits_dtype 0) or bf16 (1), of a range whose ends below batch (K+1) G are
 * multiples of G (whole coalitions).  output: MMSKIN_SHAPLEY_PROB (soft-max, exp(x - max) / sum in fp32) or _LOGIT.  It fills
 * v fp64 [batch][K + 2][C]: the mean over each coalition's G rows in fp64 in a fixed order, entry K = v(empty), K + 1 =
 * v(all).  The ranges of several calls fill v chunk by chunk.  finish != 0, on the call that completes v, then writes phi fp32
 * [batch][M][C] (the sum over p = 0 .. P-1 in fp64, in that order), base = v(empty) and full = v(all) fp32 [batch][C], and,
 * with abs_sum non-null, ADDS |phi| over b = 0 .. batch-1, in that order, into the caller-zeroed fp64 [M][C] abs_sum; it needs
 * perm_host / pos_scratch as above.  No atomics anywhere: two runs are bitwise equal.  An empty range with finish is allowed.
 * Errors (nothing is launched): an extent < 1, a table row that is not a permutation, a range outside the walk or one that
 * splits a coalition, null arguments; 2 <= C <= 64, anything else is MMSKIN_ERR_UNSUPPORTED. */
#define MMSKIN_SHAPLEY_PROB 0
#define MMSKIN_SHAPLEY_LOGIT 1
int64_t mmskin_shapley_rows(int batch, int G, int P, int M);
int mmskin_shapley_coalitions(const int32_t* codes, const float* numeric, int batch, const int32_t* bg_codes, const float* bg_numeric,
                              int G, int n_cat, const int32_t* col_offset, const int32_t* col_offset_host, int onehot_width, int n_num,
                              const float* mean, const float* scale, float nan_fill, const int32_t* perm_host, int32_t* pos_scratch,
                              int P, int64_t row0, int64_t row1, float* out, int out_width, void* stream);
int mmskin_shapley_reduce(const void* logits, int logits_dtype, int output, int batch, int G, int P, int M, int C, int64_t row0,
                          int64_t row1, double* v, int finish, const int32_t* perm_host, int32_t* pos_scratch, float* phi, float* base,
                          float* full, double* abs_sum, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LIME explanations of the encoded metadata columns on the model itself (csrc/lime.hip, mmskin.lime.MetadataLime): what lime's
 * LimeTabularExplainer(mode="regression", discretize_continuous=False).explain_instance(row, predict_fn, num_features=K) does,
 * with the network as predict_fn.  F <= 128 features (every encoded column, one-hot cells included, as a continuous feature),
 * N rows per explained sample, rows sample-major: row = b N + s.  mean / scale: fp64 [F] on the device, the StandardScaler of
 * the encoded training rows (scale has no zero: the caller replaces 0 by 1).
 *     row_0 = x bit for bit;  row_s[f] = n(s, f) * (float)scale[f] + (float)mean[f]   (around_instance: + x[f]), in fp32, unfused
 *     z = ((double)row - mean) / scale;  d_s = |z_s - z_0|_2;  w_s = sqrt(exp(-d_s^2 / (0.75 sqrt F)^2))
 * The generator: h = mix64(mix64(seed) ^ (sample << 40 | s << 8 | f)), mix64 = the splitmix64 finaliser (x += 0x9E3779B97F4A7C15;
 * x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), sample = sample0 + b;
 * u1 = ((h >> 41) + 0.5) 2^-23, u2 = (((h & 0xffffffff) >> 9) + 0.5) 2^-23, n = sqrtf(-2 logf(u1)) cosf(6.2831855f u2), fp32.
 * n depends on (seed, sample, s, f) only, so any row range gives the bytes of one full call.
 *
 * All three entry points take a row range [row0, row1) and the buffers OF THAT RANGE (out / rows / w / logits point at row0).
 *
 * lime_neighbourhood: x fp32 [batch][x_stride] -> out fp32 [row1 - row0][out_width] (columns >= F zero) and the weights
 * w [row1 - row0], fp32 (MMSKIN_LIME_W_F32) or fp64 (_F64), computed from the row just written.  Every element is written once.
 *
 * lime_reduce: the rows, their weights and the head's logits [row1 - row0][C] (fp32: logits_dtype 0, bf16: 1) are ADDED into the
 * caller-zeroed acc, mmskin_lime_accumulator_doubles(batch, N, F, C) doubles.  y = the logits (MMSKIN_LIME_LOGIT) or their
 * soft-max (_PROB: e = exp(x - max) taken in fp64 and rounded to fp32, summed over c = 0 .. C-1 in fp32, e / sum in fp32).  With
 * a = [z (F), 1, y (C)] it holds, per sample and per slab of 256 consecutive s, sum_s w a_i a_j for i <= F and all j, row-major
 * [F + 1][F + 1 + C], then sum_s w y_c^2 [C]: sum w, sum w z, sum w y, sum w z z^T, sum w z y^T, sum w y^2.  Every element is
 * summed over its slab's rows in ascending s, continuing from the value in memory, and the slabs are added in ascending order by
 * lime_solve: the result does not depend on where the rows were cut between calls.  Calls that share acc are ordered on one stream.
 *
 * lime_solve: per (sample, class), sklearn's Ridge(alpha, fit_intercept=True).fit(Z, y, sample_weight=w) in closed form from the
 * sums: zbar, ybar the weighted means, G = Zc^T W Zc, R = Zc^T W yc, Syy = sum w yc^2;  beta0 = (G + 0.01 I)^-1 R;  U = the K
 * features with the largest |beta0_j z_0j| (ties to the lower index; lime's `highest_weights`);  beta = (G_UU + I)^-1 R_U;
 * intercept = ybar - zbar_U beta;  score = 1 - (Syy - 2 beta R_U + beta^T G_UU beta) / Syy (Syy = 0: 1 if the numerator is 0,
 * else 0);  local_pred = intercept + z_0U beta.  Both systems by Cholesky in fp64.  Outputs, all fp64 but feature: coef and
 * feature (int32) [batch][C][K] in descending |beta| (ties to the lower index), intercept, score, local_pred [batch][C]; dense
 * [batch][C][F] (beta scattered, zeros elsewhere) when non-null; with abs_sum non-null, |beta| is ADDED over b = 0 .. batch-1, in
 * that order, into the caller-zeroed fp64 [F][C] abs_sum.  workspace: mmskin_lime_solve_workspace_bytes(batch, F, C) bytes.  The
 * call WAITS for the stream (it reads the factorisations' verdict back): a pivot that is not positive returns
 * MMSKIN_ERR_NUMERIC, that (sample, class) and abs_sum are left unwritten.  It cannot run under stream capture.
 * No atomics anywhere: two runs are bitwise equal.  Errors (nothing is launched): an extent < 1, F > 128, C > 64, K < 1 or K > F,
 * widths below F, a range outside the batch's rows or with row1 < row0, an unknown dtype or output, a null argument; the two
 * size queries return -1. */
#define MMSKIN_ERR_NUMERIC 4
#define MMSKIN_LIME_PROB 0
#define MMSKIN_LIME_LOGIT 1
#define MMSKIN_LIME_W_F32 0
#define MMSKIN_LIME_W_F64 1
int64_t mmskin_lime_accumulator_doubles(int batch, int N, int F, int C);
int64_t mmskin_lime_solve_workspace_bytes(int batch, int F, int C);
int mmskin_lime_neighbourhood(const float* x, int x_stride, int batch, const double* mean, const double* scale, int F, int N,
                              uint64_t seed, int64_t sample0, int around_instance, int64_t row0, int64_t row1, float* out,
                              int out_width, void* w, int w_dtype, void* stream);
int mmskin_lime_reduce(const float* rows, int width, const void* w, int w_dtype, const void* logits, int logits_dtype, int output,
                       const double* mean, const double* scale, int batch, int N, int F, int C, int64_t row0, int64_t row1,
                       double* acc, void* stream);
int mmskin_lime_solve(const double* acc, const float* x, int x_stride, const double* mean, const double* scale, int batch, int N,
                      int F, int C, int K, double* coef, int32_t* feature, double* intercept, double* score, double* local_pred,
                      double* dense, double* abs_sum, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Permutation importance of the metadata on a validation fold (csrc/permute.hip,
 * mmskin.permutation.MetadataPermutationImportance): sklearn.inspection.permutation_importance with the network as the estimator.
 * The fold's S <= MMSKIN_PERMUTATION_MAX_SAMPLES images are encoded once; for each of R repeats and G feature groups the fusion
 * head runs on the S rows whose columns of that group come from a shuffled sample, and the fold is scored again.  Groups are sets
 * of ENCODED columns: group int32 [width], group[j] = the group of column j in 0 .. G-1, or -1 for a column that is never shuffled
 * (a one-hot block is one group, so a shuffled row is bit for bit the encoding of the mixed raw row).
 * Row order of the study: row = (r G + g) S + s; a CELL (r, g) is S consecutive rows; R G S rows in all.
 *
 * permutation_indices: perm int32 [R][G][S], perm[r][g] = the positions i = 0 .. S-1 in ascending order of the 64-bit keys
 * (h_i >> 32) << 32 | i with h_i = mix64(mix64(seed) ^ (r << 40 | g << 20 | i)), mix64 as under LIME above.  A pure function of
 * (seed, r, g, S); S = 1 gives the identity.  One workgroup per cell sorts the keys in LDS.
 *
 * permuted_rows: x fp32 [S][x_stride] (x_stride >= width) -> out fp32 [row1 - row0][width], the rows [row0, row1) of the study
 * (out points at row0): column j of row (r, g, s) is x[perm[r][g][s]][j] where group[j] == g and x[s][j] elsewhere.  Every
 * element is written once, so any cut of the rows gives the bytes of one full call.  A table entry outside 0 .. S-1 is read as s.
 *
 * permutation_scores: logits fp32 [row1 - row0][K] of a range cut at multiples of S (whole cells; anything else is an error),
 * labels int64 [S] read in place (a label outside [0, K) counts nowhere).  For each cell of the range it WRITES
 *   confusion int32 [R G][K][K]      [true][predicted], predicted = the first arg-max of the logits
 *   counts    int64 [R G][3 K + 1]   pos[K], neg[K], wins2[K], nan: the block of mmskin_ovr_auc_counts below, on
 *                                    p = soft-max in fp32 (e_c = exp(x_c - max) taken in fp64 and rounded to fp32, summed over
 *                                    c = 0 .. K-1 in fp32, e_c / sum in fp32)
 * Integers only and no atomics: two runs are bitwise equal, and the ranges of several calls fill the cells chunk by chunk.
 *
 * permutation_finalize: per cell, in fp64: accuracy = trace / rows; balanced accuracy = the mean over the classes that occur of
 * their recall; auc = the mean over the classes with a positive and a negative row of wins2 / (2 pos neg), NaN when there is no
 * such class or nan > 0 (accuracy and balanced accuracy are NaN when no row counts).  metrics fp64 [3][G][R] in that order of
 * metrics, importances [3][G][R] = baseline[m] - metrics (baseline fp64 [3] on the device), mean and std [3][G] over r = 0 .. R-1
 * in that order, std with ddof = 0: sqrt(sum (v - mean)^2 / R).
 * Errors (nothing is launched, no GPU needed): an extent < 1 or out of range, S > MMSKIN_PERMUTATION_MAX_SAMPLES, a range
 * outside the study or one that splits a cell, width > x_stride, a null argument; 2 <= K <= 64, anything else is
 * MMSKIN_ERR_UNSUPPORTED. */
#define MMSKIN_PERMUTATION_MAX_SAMPLES 4096
int mmskin_permutation_indices(uint64_t seed, int R, int G, int S, int32_t* perm, void* stream);
int mmskin_permuted_rows(const float* x, int x_stride, const int32_t* group, const int32_t* perm, int R, int G, int S, int width,
                         int64_t row0, int64_t row1, float* out, void* stream);
int mmskin_permutation_scores(const float* logits, const int64_t* labels, int R, int G, int S, int K, int64_t row0, int64_t row1,
                              int32_t* confusion, int64_t* counts, void* stream);
int mmskin_permutation_finalize(const int32_t* confusion, const int64_t* counts, const double* baseline, int R, int G, int K,
                                double* metrics, double* importances, double* mean, double* std, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bootstrap confidence intervals of a fold's metrics (csrc/bootstrap.hip, mmskin.bootstrap.BootstrapMetrics): the non-parametric
 * bootstrap over the N rows of a validation fold, B replicates, each scored as exact integers.  scores fp32 [N][K] are the
 * soft-max rows of an evaluation pass; labels and preds int64 [N], read in place, both in [0, K) (the caller drops other rows; a
 * row whose label is outside counts nowhere, a prediction outside enters no confusion cell).
 * 1 <= N <= MMSKIN_BOOTSTRAP_MAX_ROWS, 2 <= K <= MMSKIN_BOOTSTRAP_MAX_CLASSES, 1 <= B <= MMSKIN_BOOTSTRAP_MAX_RESAMPLES.
 *
 * The generator keeps no state: key = mix64(seed) (mix64 as under LIME above); replicate b, draw t (0 <= t < N):
 * h = mix64(key ^ ((uint64) b << 32 | t)), u = h >> 32.  MMSKIN_BOOTSTRAP_PLAIN: draw t hits row (u N) >> 32 (64-bit arithmetic;
 * the bias of multiply-high is below N / 2^32).  MMSKIN_BOOTSTRAP_STRATIFIED: with c the label of row t and m_c the ascending list
 * of the n_c rows with label c, draw t hits m_c[(u n_c) >> 32], so every class keeps its count.  MMSKIN_BOOTSTRAP_POINT: no draws,
 * every weight is 1 (the fold itself).  w_b[i] = the number of draws of replicate b that hit row i; sum_i w_b[i] = N.  The
 * weights depend on (seed, b, N) only -- stratified: and on the labels -- never on the scores, on B or on the range of a call.
 *
 * The caller's tables, all int32 on the device (mmskin.ops.bootstrap_tables builds them with a device sort):
 *   order [K][N]        order[c][q] = the row at position q when the rows are sorted by scores[.][c], ascending
 *   lo, hi [K][N]       the tie group of position q in that order: scores[order[c][x]][c] == scores[order[c][q]][c] exactly for
 *                       lo[c][q] <= x < hi[c][q], 0 <= lo <= q < hi <= N
 *   members [N]         the rows in ascending order of (label, row); class_start [K + 1]: members[class_start[c] ..
 *                       class_start[c + 1]) are the rows with label c.  Read in stratified mode only (may be NULL otherwise).
 * An entry out of range is skipped, never followed.
 *
 * bootstrap_weights: w int32 [b1 - b0][N], the weights of replicates [b0, b1) (w points at b0).
 * bootstrap_replicates: for each replicate b of [b0, b1) it WRITES, once, and nothing outside those slices:
 *   confusion int32 [B][K][K]     confusion[b][y][p] = the sum of w_b[i] over the rows with label y and prediction p
 *   counts    int64 [B][3 K]      pos[K], neg[K] (weighted row counts), wins2[K]: wins2[c] = the sum over (i with label c, j with
 *                                 another label) of w_b[i] w_b[j] (2 [s[i][c] > s[j][c]] + [s[i][c] == s[j][c]]), the pair rule
 *                                 of mmskin_ovr_auc_counts below.  The scores must hold no NaN (the caller checks).
 * One workgroup per replicate; w_b lives in LDS only; integer LDS atomics and single-owner sums: bitwise repeatable.  In POINT
 * mode the integers equal mmskin_ovr_auc_counts and the criterion meter's confusion matrix on the same rows.
 *
 * bootstrap_finalize: metrics fp64 [M][B], M = mmskin_bootstrap_metric_columns(K) = 7 + 2 K, column m of replicate b at
 * metrics[m B + b]:  0 accuracy, 1 balanced_accuracy (mean recall over the classes that occur), 2 precision, 3 recall, 4 f1_score
 * (K = 2: of class 1; otherwise weighted by the true counts; a ratio with a zero denominator is 0), 5 auc (K = 2: of class 1;
 * otherwise the mean of the per-class AUCs weighted by pos over the classes with a positive and a negative row), 6 macro_auc
 * (their unweighted mean), 7 + c recall of class c, 7 + K + c AUC of class c = wins2 / (2 pos neg).  A metric that is undefined
 * in a replicate is NaN there.  summary fp64 [5][M]: n_valid (the replicates that are not NaN), mean, std (ddof = 1) over the
 * valid replicates summed in replicate order, and the q_lo and q_hi quantiles of the valid replicates by numpy's linear method
 * (0 <= q_lo <= q_hi <= 1); all NaN when n_valid = 0, std NaN when n_valid = 1.
 * bootstrap_compare: two metric tables fp64 [M][B] -> delta [M][B] = a - b (NaN if either is), its summary [5][M] as above, and
 * sign_counts int64 [M][2] = the number of replicates with delta <= 0 and with delta >= 0.
 * Errors (nothing is launched, no GPU needed): N, K or B outside the limits is MMSKIN_ERR_UNSUPPORTED with the limit's name in
 * the message; an unknown mode, a range outside [0, B], quantiles out of order, a null argument are MMSKIN_ERR_ARG. */
#define MMSKIN_BOOTSTRAP_MAX_ROWS 16384
#define MMSKIN_BOOTSTRAP_MAX_CLASSES 64
#define MMSKIN_BOOTSTRAP_MAX_RESAMPLES 8192
#define MMSKIN_BOOTSTRAP_PLAIN 0
#define MMSKIN_BOOTSTRAP_STRATIFIED 1
#define MMSKIN_BOOTSTRAP_POINT 2
int mmskin_bootstrap_metric_columns(int K);
int mmskin_bootstrap_weights(uint64_t seed, int mode, int N, int K, int B, const int64_t* labels, const int32_t* members,
                             const int32_t* class_start, int b0, int b1, int32_t* w, void* stream);
int mmskin_bootstrap_replicates(uint64_t seed, int mode, int N, int K, int B, const int64_t* labels, const int64_t* preds,
                                const int32_t* members, const int32_t* class_start, const int32_t* order, const int32_t* lo,
                                const int32_t* hi, int b0, int b1, int32_t* confusion, int64_t* counts, void* stream);
int mmskin_bootstrap_finalize(const int32_t* confusion, const int64_t* counts, int B, int K, double q_lo, double q_hi,
                              double* metrics, double* summary, void* stream);
int mmskin_bootstrap_compare(const double* metrics_a, const double* metrics_b, int B, int M, double q_lo, double q_hi, double* delta,
                             double* summary, int64_t* sign_counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Subgroup audit of a fold (csrc/subgroup.hip, mmskin.subgroup.SubgroupAudit): the bootstrap above scored per group of rows, so
 * that a group's replicate, another group's and the fold's are ONE resample and their differences are paired.  scores, labels,
 * preds, modes, the generator, members and class_start are those of the bootstrap section.  groups int32 [N], read in place: the
 * group of each row; an id outside [0, G) puts the row in no group -- it is still drawn and still carries weight, it is counted
 * nowhere.  1 <= N <= MMSKIN_SUBGROUP_MAX_ROWS, 2 <= K <= MMSKIN_BOOTSTRAP_MAX_CLASSES, 1 <= G <= MMSKIN_SUBGROUP_MAX_GROUPS,
 * G K K <= MMSKIN_SUBGROUP_MAX_CELLS, 1 <= B <= MMSKIN_BOOTSTRAP_MAX_RESAMPLES.  (N = 8192, G = 16, K = 8) and (N = 8192, G = 4,
 * K = 64) lie inside.
 *
 * The weights w_b are exactly those of mmskin_bootstrap_weights for the same (seed, mode, N, labels), in all three modes: they
 * depend neither on groups nor on G (one piece of code draws both).
 *
 * The caller's tables, all int32 on the device (mmskin.ops.subgroup_tables builds them with device sorts), with
 * key(i) = groups[i] if it lies in [0, G), else G:
 *   order [K][N]        order[c][q] = the row at position q when the rows are sorted by (key, scores[.][c]), ascending
 *   lo, hi [K][N]       the tie group of position q in that order: the positions lo[c][q] <= x < hi[c][q] hold the rows with the
 *                       key AND the score of position q, 0 <= lo <= q < hi <= N.  A tie group never crosses a group boundary.
 *   group_start [G + 1] group g owns the positions group_start[g] .. group_start[g + 1] of every class's order;
 *                       group_start[0] = 0, and the rows in no group lie from group_start[G] to N
 *   members, class_start as for the bootstrap (stratified mode only; may be NULL otherwise).
 * An entry out of range is skipped, never followed: a row index outside [0, N) counts nothing, a position <= 0 is read as "no
 * negative before it" and a position >= N as "every negative before it".
 *
 * subgroup_replicates: for each replicate b of [b0, b1) it WRITES, once, and nothing outside those slices:
 *   confusion int32 [B][G][K][K]  confusion[b][g][y][p] = the sum of w_b[i] over the rows of group g with label y and prediction p
 *   counts    int64 [B][G][3 K]   pos[K], neg[K] (weighted row counts within the group), wins2[K]: wins2[c] = the sum over (i with
 *                                 label c, j with another label, BOTH in group g) of w_b[i] w_b[j] (2 [s[i][c] > s[j][c]] +
 *                                 [s[i][c] == s[j][c]]), the pair rule of mmskin_ovr_auc_counts below
 * One workgroup per replicate; one prefix scan per class serves all G groups (a positive of group g at position q adds
 * w_q (P[lo_q] + P[hi_q] - 2 P[group_start[g]])); integer LDS atomics and single-owner sums: bitwise repeatable and independent
 * of how [0, B) is cut into calls.  With G = 1 and every row in group 0 the integers are those of mmskin_bootstrap_replicates.
 *
 * subgroup_finalize: metrics fp64 [G][M][B], M = mmskin_subgroup_metric_columns(K) = 7 + 4 K, column m of group g and replicate b
 * at metrics[(g M + m) B + b].  With n_g = sum_c pos[c] the group's weighted row count: columns 0 .. 7 + 2 K - 1 are the bootstrap
 * columns above on the group's integers (one device function computes both), 7 + 2 K + c the false-positive rate of class c =
 * (sum_y conf[y][c] - conf[c][c]) / (n_g - pos[c]), 7 + 3 K + c the predicted rate of class c = sum_y conf[y][c] / n_g; a zero
 * denominator gives NaN.  A group with n_g < min_rows (min_rows >= 1) in replicate b is NaN in every column of that replicate.
 * summary fp64 [G][5][M]: per group the summary of bootstrap_finalize.
 *
 * subgroup_gaps: metrics fp64 [G][M][B] (any M in 1 .. 7 + 4 MMSKIN_BOOTSTRAP_MAX_CLASSES) -> per column m and replicate b, over
 * the groups that are not NaN there: lowest, highest fp64 [M][B] (NaN when no group is defined), gap = highest - lowest (NaN when
 * fewer than two groups are defined); lowest_group int64 [M][G] = the number of replicates in which g is the lowest, ties going to
 * the smallest id; summary fp64 [3][5][M] for lowest, highest and gap.  Differences of two groups, of a group and the fold, or of
 * two models' gaps are two [M][B] tables through mmskin_bootstrap_compare.
 * Errors (nothing is launched, no GPU needed): an extent outside its limit is MMSKIN_ERR_UNSUPPORTED with the limit's name in the
 * message; an unknown mode, a range outside [0, B], quantiles out of order, min_rows < 1, a null argument are MMSKIN_ERR_ARG. */
#define MMSKIN_SUBGROUP_MAX_ROWS 8192
#define MMSKIN_SUBGROUP_MAX_GROUPS 64
#define MMSKIN_SUBGROUP_MAX_CELLS 16384
int mmskin_subgroup_metric_columns(int K);
int mmskin_subgroup_replicates(uint64_t seed, int mode, int N, int K, int G, int B, const int64_t* labels, const int64_t* preds,
                               const int32_t* groups, const int32_t* members, const int32_t* class_start, const int32_t* order,
                               const int32_t* lo, const int32_t* hi, const int32_t* group_start, int b0, int b1, int32_t* confusion,
                               int64_t* counts, void* stream);
int mmskin_subgroup_finalize(const int32_t* confusion, const int64_t* counts, int B, int G, int K, int64_t min_rows, double q_lo,
                             double q_hi, double* metrics, double* summary, void* stream);
int mmskin_subgroup_gaps(const double* metrics, int B, int G, int M, double q_lo, double q_hi, double* lowest, double* highest,
                         double* gap, int64_t* lowest_group, double* summary, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Calibration of a fold's probabilities (csrc/calibration.hip, mmskin.calibration.Calibration / TemperatureScaling): reliability
 * tables as exact integers, ECE / MCE / class-wise ECE, Brier score and NLL, their bootstrap, and post-hoc temperature scaling.
 * probs fp32 [N][K] are soft-max rows (0 <= p <= 1, no NaN: the caller checks); labels int64 [N], read in place, in [0, K) (the
 * caller drops other rows; a label outside is a hit nowhere and adds nothing to the sums).
 * 1 <= N <= MMSKIN_CALIBRATION_MAX_ROWS, 2 <= K <= MMSKIN_CALIBRATION_MAX_CLASSES, 1 <= n_bins <= MMSKIN_CALIBRATION_MAX_BINS,
 * 1 <= R <= MMSKIN_BOOTSTRAP_MAX_RESAMPLES.
 *
 * There are K + 1 tables.  Table 0 is the top-label table: the confidence of row i is p[i][pred_i] with pred_i the FIRST arg-max
 * of the row, its hit is [pred_i == label_i].  Table 1 + c is class c one-vs-rest: confidence p[i][c], hit [label_i == c].
 * Bins are right-closed.  edges fp32 [K + 1][n_bins + 1], per table, ascending, e_0 = 0 and e_{n_bins} = 1 (neither is read).  The
 * bin of a confidence p is the number of interior edges e_1 .. e_{n_bins - 1} that are < p, compared in fp32:
 * np.searchsorted(edges[1:-1], p, side="left").  So p = 0 lies in bin 0, a p exactly on an edge lies in the lower bin, and equal
 * edges leave empty bins between them.  The fixed-point confidence is q(p) = (int64) rint((double) p 2^30)
 * (MMSKIN_CALIBRATION_CONF_SCALE_LOG2 = 30, S = 2^30): exact for p >= 2^-7, otherwise off by at most 2^-31 per row.  Every table
 * entry is an integer, hence independent of the order of summation.
 *
 * calibration_codes: the per-fold pass, the same for every replicate: bin uint8 [K + 1][N], q int32 [K + 1][N], hit uint8
 * [K + 1][N] (table-major: the later passes read them coalesced along N).
 * calibration_bins: tables int64 [R][K + 1][n_bins][3] = per replicate, table and bin: count = sum w, hits = sum w hit,
 * conf = sum w q, over the rows of that bin; weights int32 [R][N].  Precondition of a weighted call: w >= 0 and, per replicate,
 * sum_i w[r][i] < 2^31 (bootstrap weights sum to N), so count and hits stay below 2^31 and conf below 2^61.  One workgroup owns a
 * (replicate, tile of tables) pair, accumulates it in LDS with integer atomics and WRITES its slice once, nothing outside the R
 * slices; the caller need not zero the buffer.  A code bin[t][i] >= n_bins is skipped, never followed.  weights == NULL: R is
 * taken as 1 and every weight as 1; the rows are spread over workgroups that finish with 64-bit integer global atomics into the
 * slice, which the entry zeroes on `stream` itself.  No floating-point atomics: bitwise repeatable.
 * calibration_sums: sums fp64 [R][2]: sums[r][0] = sum_i w_i sum_k (p_ik - [label_i == k])^2 (the multi-class Brier sum),
 * sums[r][1] = sum_i w_i (-log max(p[i][label_i], FLT_MIN)) (the NLL sum), in fp64.  The order is fixed: the rows are cut into
 * C = min(ceil(N / 4096), 256) chunks of ceil(N / C) rows, a workgroup of 256 threads sums one (chunk, replicate) -- thread t its
 * rows t, t + 256, ... in order, then a butterfly over the lanes and the waves in order -- and the chunk partials are added in
 * chunk order.  scratch: mmskin_calibration_sums_scratch_doubles(N, R) = 2 C R doubles (weights == NULL: R = 1), -1 out of range.
 * calibration_finalize: metrics fp64 [M][R], M = mmskin_calibration_metric_columns(K) = 6 + K, column m of replicate r at
 * metrics[m R + r].  With W = sum_b count_b of table 0 and d_b = |hits_b S - conf_b| (an exact integer):
 *   0 ece = sum_b d_b / (S W)              1 mce = max over the non-empty bins of d_b / (S count_b)     (both of table 0)
 *   2 classwise_ece = the mean over the classes of column 6 + c
 *   3 confidence_gap = (sum_b conf_b / S - sum_b hits_b) / W of table 0, formed as the exact integer sum_b conf_b - S sum_b hits_b
 *     over S W: signed, positive when the model is over-confident
 *   4 brier = sums[r][0] / W               5 nll = sums[r][1] / W               6 + c: the ece of table 1 + c
 * W = 0 gives NaN in that replicate.  summary fp64 [5][M] is that of bootstrap_finalize above: n_valid, mean, std (ddof = 1), and
 * the q_lo and q_hi quantiles by numpy's linear method.
 *
 * Temperature scaling.  src fp32 [N][K]: the logits z = src, or with from_probs != 0 saved probabilities, z = log(max(src,
 * FLT_MIN)) in fp64 (soft-max is shift invariant, so they serve as well).  betas: fp64 [G] ON THE HOST, read before the call
 * returns, 1 <= G <= MMSKIN_TEMPERATURE_MAX_CANDIDATES, each finite and > 0 (beta = 1 / T).  Per candidate, with pi = softmax(beta
 * z) formed stably in fp64 (shifted by the row's maximum, the variance about the row's mean), a row gives lse(beta z) - beta z_y,
 * E_pi[z] - z_y and Var_pi[z]; out fp64 [G][3] on the device are their sums over the rows whose label lies in [0, K): the NLL sum,
 * its first and its second derivative in beta.  One pass over the rows serves all G candidates (a workgroup reads a row once);
 * the order is fixed: workgroup j of W = min(ceil(N / 64), 1024) takes the 64-row tiles j, j + W, ..., sums a tile over its rows by
 * a butterfly and the tiles in order, and the W partials are added in order.  scratch: mmskin_temperature_scratch_doubles(N, G) =
 * 3 G W doubles, -1 out of range.  temperature_apply: out fp32 [N][K] = softmax(beta z), fp64 arithmetic, rounded once.
 * Errors (nothing is launched, no GPU needed): N, K, n_bins, R or G outside the limits is MMSKIN_ERR_UNSUPPORTED with the limit's
 * name in the message; quantiles out of order, a beta that is not finite and positive, a null argument are MMSKIN_ERR_ARG. */
#define MMSKIN_CALIBRATION_MAX_ROWS (1 << 24)
#define MMSKIN_CALIBRATION_MAX_CLASSES 64
#define MMSKIN_CALIBRATION_MAX_BINS 64
#define MMSKIN_CALIBRATION_CONF_SCALE_LOG2 30
#define MMSKIN_TEMPERATURE_MAX_CANDIDATES 64
int mmskin_calibration_metric_columns(int K);
int64_t mmskin_calibration_sums_scratch_doubles(int N, int R);
int64_t mmskin_temperature_scratch_doubles(int N, int G);
int mmskin_calibration_codes(const float* probs, const int64_t* labels, int N, int K, const float* edges, int n_bins, uint8_t* bin,
                             int32_t* q, uint8_t* hit, void* stream);
int mmskin_calibration_bins(int N, int K, int n_bins, const uint8_t* bin, const int32_t* q, const uint8_t* hit, const int32_t* weights,
                            int R, int64_t* tables, void* stream);
int mmskin_calibration_sums(const float* probs, const int64_t* labels, int N, int K, const int32_t* weights, int R, double* scratch,
                            double* sums, void* stream);
int mmskin_calibration_finalize(const int64_t* tables, const double* sums, int R, int K, int n_bins, double q_lo, double q_hi,
                                double* metrics, double* summary, void* stream);
int mmskin_temperature_stats(const float* src, int from_probs, const int64_t* labels, int N, int K, const double* betas, int G,
                             double* scratch, double* out, void* stream);
int mmskin_temperature_apply(const float* src, int from_probs, int N, int K, double beta, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The criterion (csrc/criterion.hip): one forward and one backward launch for three kinds of loss on logits [B][C], row-major,
 * fp32 (logits_dtype 0) or bf16 (1); all arithmetic fp32.  1 <= B <= 2^20, 2 <= C <= 1024.  With m = max z_i,
 * ls = ln sum exp(z_i - m), ce = ls - (z_i[y] - m), p = softmax(z_i):
 *   CE     torch nn.CrossEntropyLoss(weight=w)     row value w[y] ce;  `mean` = sum w[y] ce / sum w[y] over the valid rows
 *   FOCAL  the reference's models/focalLoss.py     row value (1 - pt)^gamma (alpha[y] ce), pt = exp(-ce), 1 - pt formed as
 *                                                  -expm1(-ce);  `mean` = the plain mean over B.  gamma is 0 (then the factor is
 *                                                  skipped: the result IS CE, bit for bit) or >= 1
 *   SOFT   models/softtargetsCrossEntropy.py       row value -sum_c t[c] (z[c] - m - ls) w[c], targets fp32 [B][C]; `mean` over
 *                                                  B only, as the reference
 * targets: int64 [B] labels (CE, FOCAL), read in place and never inspected on the host: a label outside [0, C) -- torch's
 * ignore_index -100 included -- gives no loss, no gradient and does not count in CE's `mean` (all rows ignored: nan, as torch).
 * weight: fp32 [C] (w / alpha) or NULL for all ones.  loss: fp32, one value, or [B] for MMSKIN_REDUCE_NONE.  loss is fp32 also
 * for bf16 logits.
 * scratch: mmskin_criterion_scratch_floats(B, C, kind) floats (-1 for a shape out of range), not initialised by the caller.
 * The forward leaves the rows' (m, ls), the per-workgroup partial sums and the divisor of `mean` there; the backward reads
 * them, so the buffer lives until the backward has run.  ticket: one int32 that is ZERO before the first call and that the
 * kernel leaves zero; calls that share it must be ordered on one stream.  The batch reduction has a fixed order (64-row
 * partials, then a tree in the workgroup that arrives last): forward and backward are bitwise repeatable.
 * meter (optional): a caller-zeroed block { double loss_sum; int64 rows; int32 confusion[C][C]; }.  The forward adds, from one
 * thread after the reduction, rows = the valid rows of the batch (SOFT: B) and loss_sum = rows x the batch's `mean` loss --
 * the sum of the row values, except for CE under class weights -- whatever `reduction` is; and with labels it adds 1 to
 * confusion[y][first arg-max of the logits] per valid row (integer atomics).  probs_out (optional) fp32 [B][C]: the soft-max.
 * backward: dloss is one device float, or [B] for MMSKIN_REDUCE_NONE; dlogits [B][C] in the logits' dtype, every element
 * written:  CE g w[y] (p_j - [j = y]) with g = dloss / sum w[y] for `mean`;  FOCAL g alpha[y] (gamma (1 - pt)^(gamma - 1) pt ce
 * + (1 - pt)^gamma) (p_j - [j = y]), g = dloss / B for `mean`;  SOFT (dloss / B) (p_j sum_c t[c] w[c] - t[j] w[j]).  targets
 * and weight get no gradient.  Errors (MMSKIN_ERR_ARG, nothing launched, no GPU needed): B or C out of range, an unknown dtype,
 * kind or reduction, SOFT with a reduction other than `mean`, FOCAL with 0 < gamma < 1 or gamma < 0, a null argument. */
#define MMSKIN_CRITERION_CE 0
#define MMSKIN_CRITERION_FOCAL 1
#define MMSKIN_CRITERION_SOFT 2
#define MMSKIN_REDUCE_NONE 0
#define MMSKIN_REDUCE_SUM 1
#define MMSKIN_REDUCE_MEAN 2
int64_t mmskin_criterion_scratch_floats(int B, int C, int kind);
int mmskin_criterion_forward(const void* logits, int logits_dtype, const void* targets, const float* weight, int kind, int reduction,
                             float gamma, int B, int C, float* loss, float* scratch, int32_t* ticket, void* meter, float* probs_out,
                             void* stream);
int mmskin_criterion_backward(const void* logits, int logits_dtype, const void* targets, const float* weight, int kind, int reduction,
                              float gamma, int B, int C, const float* dloss, const float* scratch, void* dlogits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-vs-rest AUC of an evaluation pass as exact integer counts (csrc/auc.hip).  probs: fp32 [N][C], row-major, contiguous
 * (the rows the criterion's probs_out collected); labels: int64 [N], read in place.  counts: int64 [3 C + 1] on the device,
 *   counts[c]          pos[c]    rows with label c
 *   counts[C + c]      neg[c]    rows with a label in [0, C) other than c
 *   counts[2 C + c]    wins2[c]  sum over the pairs (i with label c, j with another label in [0, C)) of
 *                                2 [probs[i][c] > probs[j][c]] + [probs[i][c] == probs[j][c]]
 *   counts[3 C]        nan       NaN entries of probs in the rows that count
 * Rows whose label lies outside [0, C) count nowhere, as in the criterion's meter; a NaN compares as neither greater nor equal.
 * auc[c] = wins2[c] / (2 pos[c] neg[c]) is the Mann-Whitney statistic: the area under the ROC curve by trapezoids, ties at half
 * weight.  All sums are integers (64-bit integer atomics), so the block is bitwise repeatable and independent of the launch
 * geometry.  N^2 compares: a row is compared in the column of its own label only.  The entry zeroes `counts` on `stream` itself
 * and allocates nothing.  2 <= C <= 1024, 1 <= N < 2^31; anything else, or a null argument, is MMSKIN_ERR_ARG with nothing
 * launched (no GPU needed). */
int mmskin_ovr_auc_counts(const float* probs, const int64_t* labels, int64_t N, int C, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-vs-rest ROC and precision-recall curves of an evaluation pass as exact integers (csrc/curves.hip, mmskin.curves.FoldCurves).
 * probs: fp32 [N][C], row-major, contiguous; labels: int64 [N], read in place.  Rows whose label lies outside [0, C) count
 * nowhere, as in mmskin_ovr_auc_counts.  Per class c, with s_i = probs[i][c] over the valid rows:
 *   pos[c], neg[c]   the valid rows with label c, and the valid rows minus pos[c]
 *   thr[c][k]        the distinct values of the column under float ==, descending: thr[c][0] > ... > thr[c][n_points[c] - 1]; the
 *                    stored value is that of the tie group's row with the lowest index (-0 == +0 is one group)
 *   tp[c][k]         #{i : y_i == c, s_i >= thr[c][k]}          fp[c][k]  #{i : y_i != c, s_i >= thr[c][k]}
 * A NaN score is neither greater nor equal: it is no threshold and counts in no tp or fp, but its row counts in pos / neg, and
 * counts[2 C] reports the NaN entries of the valid rows.
 * mmskin_ovr_curves writes thr fp32 [C][N], tp and fp int32 [C][N] (every slot: those at and past n_points[c] are zero),
 * n_points int32 [C] and counts int64 [2 C + 1] = { pos[C], neg[C], nan }; it zeroes what it must on `stream` itself.  The ROC
 * start (0, 0) at threshold +inf and the precision-recall end (precision 1, recall 0) are NOT stored.  With them,
 * sklearn's roc_curve(y == c, s, drop_intermediate=False) is fpr = [0, fp / neg], tpr = [0, tp / pos], thresholds = [inf, thr];
 * precision_recall_curve is the reversed tp / (tp + fp) and tp / pos with (1, 0) appended, thresholds the reversed thr.
 * Everything is an integer or a copy of an input: bitwise repeatable, independent of the launch geometry.  N^2 C compares.
 * scratch: mmskin_ovr_curves_scratch_ints(N, C) int32 values, not initialised by the caller; -1 out of range.
 *
 * mmskin_ovr_curves_summary: summary fp64 [C][S], S = mmskin_ovr_curves_summary_columns(n_spec, n_sens) = 5 + 3 (n_spec + n_sens)
 * (-1 when a count is outside 0 .. MMSKIN_CURVES_MAX_OPERATING_POINTS), from the arrays above; specificities fp64 [n_spec] and
 * sensitivities fp64 [n_sens] on the DEVICE.  With tp_{-1} = fp_{-1} = 0:
 *   0 auc                = W / (2 pos neg), W = sum_k (fp_k - fp_{k-1}) (tp_k + tp_{k-1}), an integer that equals wins2[c] of
 *                          mmskin_ovr_auc_counts: the trapezoid area IS the Mann-Whitney statistic
 *   1 average_precision  = sum_k ((tp_k - tp_{k-1}) / pos) (tp_k / (tp_k + fp_k)); fixed order: thread t of 512 adds its points
 *                          t, t + 512, ... in order, then a butterfly over the lanes, then the waves in order
 *   2 youden_j, 3 youden_threshold, 4 youden_index: the stored point that maximises tp_k / pos - fp_k / neg, compared as the exact
 *                          integer tp_k neg - fp_k pos; on ties the first point.  J = that integer / (pos neg)
 *   5 + 3 a ..           sensitivity at specificity q_a, its threshold and index: among the points with
 *                          (double) (neg - fp_k) >= q_a * (double) neg (one fp64 multiply, no division) the largest tp_k / pos and
 *                          the first point that reaches it; no such point: 0, +inf, -1 (the (0, 0) start)
 *   5 + 3 n_spec + 3 b.. specificity at sensitivity t_b, its threshold and index: among the points with
 *                          (double) tp_k >= t_b * (double) pos the largest (neg - fp_k) / neg and the first that reaches it, which
 *                          is the first admissible point; no such point (t_b > 1, or NaN scores): NaN, NaN, -1
 * A class with pos == 0 or neg == 0 keeps its integer arrays but every summary value is NaN; a class without a stored point
 * (every score NaN) has NaN for Youden's three.  Indices are stored as fp64 (exact below 2^53).
 * 2 <= C <= 1024, 1 <= N < 2^31; anything else, or a null argument, is MMSKIN_ERR_ARG with nothing launched (no GPU needed). */
#define MMSKIN_CURVES_MAX_OPERATING_POINTS 8
int64_t mmskin_ovr_curves_scratch_ints(int64_t N, int C);
int mmskin_ovr_curves_summary_columns(int n_spec, int n_sens);
int mmskin_ovr_curves(const float* probs, const int64_t* labels, int64_t N, int C, int32_t* scratch, float* thr, int32_t* tp,
                      int32_t* fp, int32_t* n_points, int64_t* counts, void* stream);
int mmskin_ovr_curves_summary(const float* thr, const int32_t* tp, const int32_t* fp, const int32_t* n_points, const int64_t* counts,
                              int64_t N, int C, const double* specificities, int n_spec, const double* sensitivities, int n_sens,
                              double* summary, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-sample predictive uncertainty (csrc/uncertainty.hip, mmskin.uncertainty.PredictiveUncertainty): the views of test-time
 * augmentation, the reduction of T stochastic passes to per-row statistics, and the risk-coverage ranking of a fold.
 *
 * mmskin_dihedral_views: src [B][C][H][W] of elements of elem_bytes = 1, 2 or 4 bytes (copied, never interpreted); dst
 * [V][B][C][H][W], one slab per set bit of the 8-bit view_mask, in ascending view id.  View v is y = rot90(x, k = v & 3) over the
 * last two axes (counter-clockwise, torch.rot90 / np.rot90) followed by a flip along W when v & 4 (torch.flip(y, (3,))):
 *   0 x[i][j]              1 x[j][W-1-i]          2 x[H-1-i][W-1-j]      3 x[H-1-j][i]
 *   4 x[i][W-1-j]          5 x[H-1-j][W-1-i]      6 x[H-1-i][j]          7 x[j][i]          (the source of y[i][j])
 * The odd views (bits 1, 3, 5, 7: mask & 0xaa) turn the plane by a quarter and need H == W; views 0, 2, 4, 6 take any shape.  A
 * pure permutation, bit-exact; the source is read once and every element of the V slabs is written exactly once, nothing else.
 * Errors (MMSKIN_ERR_ARG, nothing launched, no GPU needed): an extent below 1, elem_bytes other than 1, 2, 4, view_mask outside
 * 1 .. 255, a quarter-turn view with H != W, a null argument, src == dst.
 *
 * mmskin_uncertainty_reduce: logits fp32, element (t, n, c) at logits[t pass_stride + n row_stride + c] (strides in elements:
 * row_stride >= C, pass_stride >= 0; a contiguous [T][N][C] block has pass_stride = N C, row_stride = C).
 * 1 <= T <= MMSKIN_UNCERTAINTY_MAX_PASSES, 2 <= C <= MMSKIN_UNCERTAINTY_MAX_CLASSES, 1 <= N <= 2^24.  Per row n, in fp64, over
 * t = 0 .. T - 1 in that order, with p_t = softmax of pass t (exp(x - max) / sum, the sum over the classes a butterfly):
 *   mean_prob fp64 [N][C]   (sum_t p_t) / T
 *   prob_std  fp64 [N][C]   sqrt((sum_t (p_t - mean)^2) / T): the population standard deviation, from a second walk over the passes
 *   votes     int32 [N][C]  the passes whose arg-max LOGIT is class c, the first index among equal logits
 *   pred      int32 [N]     the first index of the largest mean probability
 *   stats     fp64 [N][7]   0 confidence = mean_prob[pred]          1 margin = confidence - the largest other mean probability
 *                           2 predictive entropy H[mean_prob], nats   3 expected entropy (sum_t H[p_t]) / T
 *                           4 mutual information max(col 2 - col 3, 0) 5 variation ratio 1 - max_c votes[c] / T
 *                           6 prob_std[pred]
 * H[p] = -sum_c p_c log p_c with 0 log 0 = 0.  A row with a non-finite logit in any pass gets NaN in mean_prob, prob_std and
 * stats, zero votes and pred = -1.  One wave per row and no atomics: a row's output depends on neither the other rows of the call
 * nor the launch geometry, and a call is bitwise repeatable.  T or C outside the limits is MMSKIN_ERR_UNSUPPORTED with the limit's
 * name in the message; N or a stride out of range, a null argument are MMSKIN_ERR_ARG; nothing is launched (no GPU needed).
 *
 * mmskin_risk_coverage: score fp64 [N] (larger = less sure; no NaN: the caller checks), wrong uint8 [N] (non-zero = the prediction
 * is an error), 1 <= N <= MMSKIN_BOOTSTRAP_MAX_ROWS.  counts int32 [N][4]: row i holds, over all j, n_lt = #{score_j < score_i},
 * n_eq = #{score_j == score_i} (i itself included), e_lt and e_eq = the wrong rows among each.  N^2 compares from LDS tiles,
 * integer atomics into the block, which the entry zeroes on `stream` itself: exact and independent of the launch geometry.
 * mmskin_risk_coverage_summary: out fp64 [8] from counts and wrong.  The rows are ranked by ascending score; e(k) is the number of
 * errors among the k surest rows, and inside a tie group (ranks n_lt + 1 .. n_lt + n_eq) it is the expectation over the order of
 * the ties, e(k) = e_lt + (k - n_lt) e_eq / n_eq:
 *   0 aurc = (1 / N) sum_{k = 1 .. N} e(k) / k, the area under the risk-coverage curve
 *   1 the optimal aurc for the same number of errors E, all of them ranked last: (1 / N) sum_{k > N - E} (k - (N - E)) / k
 *   2 e-aurc = col 0 - col 1
 *   3 the error-detection AUROC of the score: wins2 / (2 E (N - E)) with wins2 = sum over the wrong rows of 2 (n_lt - e_lt) +
 *     (n_eq - e_eq), the Mann-Whitney count of auc_pairs.h (ties at half weight); NaN when E = 0 or E = N
 *   4 the error rate E / N      5 N      6 E      7 the number of distinct scores
 * The two sums have a fixed order (one workgroup: thread t of 1024 adds its ranks t + 1, t + 1025, ..., a butterfly over the
 * lanes, the waves in order); the rest is integer.  Counts that are no ranking (a rank that no tie group covers) give NaN in
 * columns 0 and 2.  N outside the limit is MMSKIN_ERR_UNSUPPORTED with the limit's name in the message, a null argument is
 * MMSKIN_ERR_ARG; nothing is launched (no GPU needed). */
#define MMSKIN_UNCERTAINTY_MAX_PASSES 4096
#define MMSKIN_UNCERTAINTY_MAX_CLASSES 64
int mmskin_dihedral_views(const void* src, void* dst, int B, int C, int H, int W, int elem_bytes, int view_mask, void* stream);
int mmskin_uncertainty_reduce(const float* logits, int64_t pass_stride, int64_t row_stride, int T, int N, int C, double* mean_prob,
                              double* prob_std, int32_t* votes, int32_t* pred, double* stats, void* stream);
int mmskin_risk_coverage(const double* score, const uint8_t* wrong, int N, int32_t* counts, void* stream);
int mmskin_risk_coverage_summary(const int32_t* counts, const uint8_t* wrong, int N, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Split-conformal prediction sets of a fold (csrc/conformal.hip, mmskin.conformal.ConformalPredictor).  probs [N][C] are soft-max
 * rows, fp32 or fp64 (probs_fp64 != 0), no NaN (the caller checks); labels int64 [N] in [0, C) (the caller drops other rows; one
 * outside is never followed as an index and counts nowhere).  2 <= C <= MMSKIN_CONFORMAL_MAX_CLASSES; a study and a fit hold
 * 1 <= N <= MMSKIN_CONFORMAL_MAX_ROWS rows, score and apply 1 .. 2^24; 1 <= R <= MMSKIN_BOOTSTRAP_MAX_RESAMPLES.
 *
 * The order of a row (csrc/conformal_order.h): class a stands above class b iff p_a > p_b, or p_a == p_b and a < b; rank(c) = 1 +
 * the number of classes above c.  The scores, all fp64 from (double) p, with P(c) = the sum of p over the classes above c added one
 * by one in rank order, and u the row's number in [0, 1] (below):
 *   MMSKIN_CONFORMAL_LAC    s(c) = 1 - p_c
 *   MMSKIN_CONFORMAL_APS    s(c) = P(c) + u p_c
 *   MMSKIN_CONFORMAL_RAPS   s(c) = (P(c) + u p_c) + lam max(0, rank(c) - k_reg), lam >= 0, k_reg >= 0
 * randomized == 0: u = 1.  Otherwise, with key = mix64(seed) (mix64 as under LIME above), row i of the call has
 * u = (mix64(key ^ (0xFFFFFFFF << 32 | (uint32) (row0 + i))) >> 11) 2^-53.  No product or sum is fused.  Class c is in the set
 * of a row iff s(c) <= qhat[c]; qhat[c] = +inf admits class c always.
 * conformal_score: score fp64 [N][C], rank uint8 [N][C] (either may be NULL), and, with a workspace, the scores class-major inside
 * it for conformal_study / conformal_fit (then N <= MMSKIN_CONFORMAL_MAX_ROWS).
 * conformal_apply: mask uint64 [M] (bit c = class c is in the set) and size int32 [M] = its population, from qhat fp64 [C] on the
 * device.
 *
 * conformal_study, replicates [r0, r1) of R, one workgroup each.  The split of replicate r has exactly n_cal calibration rows,
 * 1 <= n_cal <= N - 1.  Replicate 0 is the identity order: the rows 0 .. n_cal - 1.  Replicate r >= 1: u_i = mix64(key ^
 * ((uint64) r << 32 | i)) >> 32, and the calibration rows are the n_cal rows with the smallest (u_i, i) (the 48-bit key u_i << 16 |
 * i; keys are distinct).  MMSKIN_CONFORMAL_STRATIFIED: the same per class, over the rows of class c (members [N] int32 = the rows
 * in ascending (label, row) order, class_start [C + 1] int32), taking cal_count[c] of them (int32 [C], the caller's; replicate 0:
 * the first cal_count[c] members of the class).  mmskin.conformal.cal_counts states the rule: floor(n_cal n_c / N) each, and
 * one more for the n_cal - sum classes with the largest remainder n_cal n_c mod N, a tie going to the lower class.
 * The threshold: qhat = the k-th smallest true-label score s_i(y_i) over the n calibration rows, k = ceil((n + 1)(1 - alpha))
 * evaluated in fp64 as written, 0 < alpha < 1; k > n gives +inf.  An order statistic, never interpolated.  order [N] int32 lists
 * the rows by ascending (s_i(y_i), i).  MMSKIN_CONFORMAL_MONDRIAN: one qhat[c] per class from the calibration rows of class c
 * (n = their number; none: +inf); order then lists the rows by ascending (y_i, s_i(y_i), i) and class_start is read.
 * It WRITES, once per replicate, qhat fp64 [R][C] (the same value C times unless Mondrian) and counts int64 [R][8 + 5 C] over
 * the test rows: 0 n_test, 1 covered (y in the set), 2 the total set size, 3 empty sets, 4 singleton sets, 5 singleton sets that
 * are {y}, then hist[C + 1] (sets per size), size_covered[C + 1] (covered rows per set size), class_rows[C] (test rows per true
 * class), class_covered[C], class_in[C] (the sets that hold class c).  All integer LDS atomics and ballots: bitwise repeatable, and
 * a function of (inputs, seed, options, r) alone -- not of R, of the range of a call, or of the launch shape.
 * conformal_fit: qhat fp64 [C] with every row calibrating (n = N; flags: MMSKIN_CONFORMAL_MONDRIAN or 0).
 * conformal_finalize: metrics fp64 [M][R], M = mmskin_conformal_metric_columns(C) = 6 + 2 C, inside the workspace: 0 coverage =
 * covered / n_test, 1 mean set size, 2 singleton rate, 3 singleton accuracy (NaN without a singleton), 4 empty rate, 5 the worst
 * class coverage over the classes with a test row, 6 + c the coverage of class c (NaN without a test row), 6 + C + c qhat[c];
 * summary fp64 [5][M] is that of bootstrap_finalize above (an infinite qhat gives an infinite mean and a NaN std).
 * workspace: mmskin_conformal_workspace_bytes(N, C, R) bytes (-1 out of range), one buffer for score, study / fit and finalize.
 * Errors (nothing is launched, no GPU needed), all MMSKIN_ERR_ARG with the field's name in the message: num_classes, n_rows,
 * n_resamples, alpha, n_cal, score, k_reg, lam, row0, flags, a range outside [0, R], quantiles out of order, a null argument. */
#define MMSKIN_CONFORMAL_MAX_ROWS 32768
#define MMSKIN_CONFORMAL_MAX_CLASSES 64
#define MMSKIN_CONFORMAL_LAC 0
#define MMSKIN_CONFORMAL_APS 1
#define MMSKIN_CONFORMAL_RAPS 2
#define MMSKIN_CONFORMAL_STRATIFIED 1
#define MMSKIN_CONFORMAL_MONDRIAN 2
int mmskin_conformal_count_columns(int C);
int mmskin_conformal_metric_columns(int C);
int64_t mmskin_conformal_workspace_bytes(int N, int C, int R);
int mmskin_conformal_score(const void* probs, int probs_fp64, int64_t N, int C, int kind, int randomized, double lam, int k_reg,
                           uint64_t seed, int64_t row0, double* score, uint8_t* rank, void* workspace, void* stream);
int mmskin_conformal_apply(const void* probs, int probs_fp64, int64_t M, int C, int kind, int randomized, double lam, int k_reg,
                           uint64_t seed, int64_t row0, const double* qhat, uint64_t* mask, int32_t* size, void* stream);
int mmskin_conformal_study(uint64_t seed, int N, int C, int R, int n_cal, double alpha, int flags, const int64_t* labels,
                           const int32_t* order, const int32_t* members, const int32_t* class_start, const int32_t* cal_count,
                           int r0, int r1, const void* workspace, double* qhat, int64_t* counts, void* stream);
int mmskin_conformal_fit(int N, int C, double alpha, int flags, const int64_t* labels, const int32_t* order,
                         const int32_t* class_start, const void* workspace, double* qhat, void* stream);
int mmskin_conformal_finalize(const int64_t* counts, const double* qhat, int N, int C, int R, double q_lo, double q_hi, void* workspace,
                              double* summary, void* stream);

/* ---------------------------------------------------------------------------------------------
 * `custom-cnn` image encoder pieces (loadImageModelClassifier.py:50-60): small direct kernels for
 * shapes the MFMA implicit GEMM does not cover (Cin=3, Cout=16).  NCHW fp32. */
int mmskin_direct_conv2d_forward(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H, int W,
                                 int Cout, int kh, int kw, int stride, int pad, int relu, void* stream);
int mmskin_direct_conv2d_backward(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int N,
                                  int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, void* stream);
/* maxpool(k, stride=k) followed by global average pool: y[N,C]; idx for backward */
int mmskin_pool_gap_forward(const float* x, float* y, int32_t* idx, int N, int C, int H, int W, int k, void* stream);
int mmskin_pool_gap_backward(const float* dy, const int32_t* idx, float* dx, int N, int C, int H, int W, int k,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMSKIN_H */
