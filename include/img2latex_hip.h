/*
 * img2latex_hip.h -- C ABI of libimg2latex_hip.so (MI355X / gfx950, HIP).
 *
 * The reference (Jeremy-Cleland/hmer-img2latex) has no FFI: its hot path is
 * the Python class surface of img2latex.model calling ATen through torch.nn.
 * Each entry point below replaces the ATen work of the cited reference lines;
 * hmer-img2latex_amd/img2latex_amd/model/ binds them with ctypes and
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes; every pointer is a DEVICE pointer
 *     into a caller-owned, contiguous, 16-byte-aligned fp32/int32 buffer unless
 *     the parameter is documented as a HOST array of device pointers.
 *   - explicit stream (a hipStream_t passed as void*; NULL = default stream);
 *     every call only ENQUEUES work, it never synchronises or allocates.
 *   - workspace is caller-provided; its size comes from *_workspace_bytes().
 *   - return value: I2L_OK (0) or a negative I2L_ERR_* code; never throws,
 *     never aborts; no global state (thread-compatible): the library reads no
 *     environment variable and keeps nothing between calls -- where an entry
 *     point has more than one kernel behind it, the choice is the explicit
 *     `flags` argument (I2L_FLAG_*, 0 = automatic); streams and events used
 *     beside `stream` live in caller-owned objects (i2l_lanes).  The only
 *     file-scope data are function-local "attribute already set on device d"
 *     bit masks (an idempotent cache of hipFuncSetAttribute).
 *   - tensors are row-major with the reference's (PyTorch) shapes.
 */
#ifndef IMG2LATEX_HIP_H
#define IMG2LATEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2L_OK 0
#define I2L_ERR_ARG (-1)          /* null pointer / non-positive dimension           */
#define I2L_ERR_UNSUPPORTED (-2)  /* dimension outside what the kernels are built for */
#define I2L_ERR_WORKSPACE (-3)    /* workspace missing or too small                   */
#define I2L_ERR_LAUNCH (-4)       /* HIP reported a launch error                      */

#define I2L_MAX_LSTM_LAYERS 4
#define I2L_MAX_BEAM 8
#define I2L_MAX_NBEST 16   /* rows per image of i2l_beam_decode_nbest */

typedef void* i2l_stream_t;

/* Kernel-selection flags (bit-or; 0 = automatic = the fastest kernel built for the shape).  Every variant computes
 * the same function; tests run the variants against each other and callers use them to fall back. */
#define I2L_FLAG_EXACT_FP32 0x1        /* conv / linear / training GEMMs: exact fp32 products (fp32 MFMA / VALU fmaf
                                          chains) instead of the 3 x bf16 split on the bf16 matrix cores             */
#define I2L_FLAG_NO_GROUP 0x2          /* beam search, training recurrences: one workgroup per image / row instead of
                                          the grouped kernels (4 co-resident workgroups exchanging through L2)       */
#define I2L_FLAG_RESNET_NO_RING 0x4    /* i2l_conv_bn_act_bf16_fwd: single-buffered GEMM instead of the LDS ring      */
#define I2L_FLAG_RESNET_IM2COL_STEM 0x8 /* i2l_conv_bn_act_bf16_fwd: im2col image + GEMM instead of the fused stem    */
#define I2L_FLAG_WEIGHTS_PACKED 0x10    /* i2l_conv3x3_relu_pool2_fwd without argmax_out: the workspace still holds the packed
                                          (3 x bf16) filter image an EARLIER call wrote for the SAME weights -- the caller
                                          kept the buffer and the weights have not changed -- so the weight-only packing
                                          launch is skipped; ignored by the kernels that do not pack                 */
#define I2L_FLAG_AGENT_SCOPE_EXCHANGE 0x20 /* grouped kernels (greedy, beam, training recurrences): every exchange store at
                                          agent scope (sc1, write-through) -- the HSA-memory-model-conformant flavour --
                                          even when the group's members share an XCD and the faster L2-local
                                          (workgroup-scope) stores would be used; same results, ~0.8 us per step slower */
#define I2L_FLAG_TEST_SHORT_TIMEOUT 0x40 /* grouped kernels, TEST hook: every poll limit 2 ms instead of (10 ms + 50 us per
                                          step) for a workgroup's first poll and 3 s for the later ones               */
#define I2L_FLAG_TEST_DROP_MEMBER 0x80 /* grouped kernels, TEST hook: member 3 of every group exits at once, so its peers
                                          time out: exercises the failure path (ids -3 / len -3 / NaN, host fallback)  */
#define I2L_FLAG_DECODE_GROUP8 0x1000  /* i2l_greedy_decode_ex (ids only: no logits_out, no forced tokens): the grouped kernel
                                          with EIGHT members x EIGHT rows per group -- one wave per SIMD and ~80 KB of LDS
                                          per CU instead of two waves and 140 KB, so that a conv workgroup of the NEXT
                                          batch's encoder fits beside it; same ids                                   */
#define I2L_FLAG_DECODE_BATCHED 0x2000  /* the Python layer's switch for i2l_greedy_decode_batched (LSTMDecoder.run_steps takes that entry
                                          instead of i2l_greedy_decode_ex) and i2l_sample_decode_batched (LSTMDecoder.sample_steps
                                          takes that entry instead of i2l_sample_decode); the C entries ignore it */
#define I2L_FLAG_BEAM_BATCHED 0x80000   /* the Python layer's switch for i2l_beam_decode_batched, as I2L_FLAG_DECODE_BATCHED is for the greedy entry
                                          (Seq2SeqModel.beam_search_batch takes that entry instead of i2l_beam_decode); the C entries ignore it */
#define I2L_FLAG_TRAIN_BATCHED 0x100000 /* i2l_decoder_train_fwd / _bwd: the step-batched recurrences on the matrix cores -- one plain launch per
                                          (step, layer) over the whole batch, split-bf16 products, state in global memory -- where
                                          i2l_decoder_train_batched_ok says 1 and I2L_FLAG_EXACT_FP32 is clear (also at layers 1 / hidden 256,
                                          instead of the grouped recurrences: A/B); a request, ignored elsewhere; default off.  Every other
                                          entry that takes decoder flags ignores it.  (Bits 20-23 are also I2L_FLAG_RESNET_PATCH_SHAPE's field:
                                          that one is read by i2l_conv_bn_act_bf16_fwd alone, which never sees decoder flags.) */
#define I2L_FLAG_DECODE_GROUP16 0x8000 /* i2l_greedy_decode_ex (ids only): the grouped kernel with SIXTEEN members x SIXTEEN rows per
                                          group and the per-step products (LSTM gates, logits) on the matrix cores as split-bf16
                                          v_mfma_f32_16x16x32_bf16 bursts (fp32-grade: 3 bf16 pieces per operand, 6 partial
                                          products) -- ~250 registers and 49 KB of LDS per CU, and a burst that conv waves on
                                          the same CU barely stretch; same ids up to fp32 near-ties.  Wins over _GROUP8 if both set */
#define I2L_FLAG_CONV_COL_READY 0x10000 /* i2l_conv_f32_bwd: the workspace is the one the matching i2l_conv_f32_fwd call used and
                                          nothing has written to it since, so its head still holds the column image of x: skip
                                          the im2col launch (the caller keeps one workspace per unit on its tape)               */
#define I2L_FLAG_RESNET_WIDE_TILES 0x40000 /* i2l_conv_bn_act_bf16_fwd: 128-column tiles even where 64-column tiles balance the CUs better (A/B) */
#define I2L_FLAG_RESNET_NO_PATCH 0x20000 /* i2l_conv_bn_act_bf16_fwd, 3x3 / stride 1 / pad 1: the implicit-GEMM ring kernel instead of
                                          the kernel that stages the input patch in LDS (A/B switch) */
#define I2L_FLAG_DECODE_REGION_CLEARED 0x2000000 /* i2l_greedy_decode_ex, grouped kernels: the caller has zeroed the workspace's group region
                                             (i2l_decoder_group_status_offset / _region_bytes) since its last use, ordered before this call: the
                                             launch skips its own memset (GreedyPipeline clears it on the encoder stream, off the decode queue) */
#define I2L_FLAG_CONV_NO_SPARSE_WGRAD 0x4000 /* i2l_conv3x3_relu_pool2_bwd with dx == NULL, Cin <= 3, Cout % 32 == 0: the
                                          implicit-im2col GEMM instead of the sparse first-block kernel (A/B, tests)   */
#define I2L_FLAG_RESNET_RING_DEPTH(n) (((n) & 0xF) << 8)   /* force the ring depth (2..4; 5 = four stages of 32-deep K tiles); 0 = automatic */
#define I2L_FLAG_RESNET_PATCH_SHAPE(n) (((n) & 0xF) << 20) /* 3x3 / stride 1 layers: force tile shape n (1..5: 160x128, 96x128,
                                                              128x128, 320x64, 256x64 pixels x channels); 0 = by balance */

int i2l_version(void);
const char* i2l_error_string(int code);
/* Side lanes of the training backward pass (caller-owned; the library itself keeps no state, see the header comment).
 * i2l_decoder_train_bwd, i2l_linear_bias_act_bwd and i2l_conv3x3_relu_pool2_bwd take an `i2l_lanes* lanes` argument.
 * NULL: everything is enqueued on `stream`.  Otherwise the WEIGHT gradients (and bias sums) -- which nothing in the
 * backward chain consumes -- are enqueued on the caller's side streams (lane 0: decoder + Linear, lane 1: conv blocks;
 * with one lane both share it), forked from `stream` by an event at the point where their inputs are complete, beside
 * the data-gradient chain that stays on `stream`.  The caller must call i2l_lanes_join(lanes, stream) before anything
 * reads those gradients and keep every buffer passed to the calls (workspace, activations, dy) alive until then.  Same
 * kernels, same sums: results identical to lanes == NULL.  The reference has no counterpart: its autograd engine orders
 * `loss.backward()` (trainer.py:337) before `optimizer.step()` (trainer.py:343) by itself.
 *   create:  `streams` = n (1..I2L_MAX_LANES) non-default streams of the CURRENT device, owned by the caller and alive as
 *            long as the object; the object adds the events it records on them
 *   destroy: releases the events (not the streams); NULL is accepted
 * One object serves one host thread at a time (like a stream's enqueue order, its fork / join events are not re-entrant);
 * two threads training on one device create one each. */
#define I2L_MAX_LANES 4
typedef struct i2l_lanes i2l_lanes;
int i2l_lanes_create(const i2l_stream_t* streams, int n, i2l_lanes** out);
int i2l_lanes_destroy(i2l_lanes* lanes);
int i2l_lanes_join(i2l_lanes* lanes, i2l_stream_t stream);
/* Enqueues a one-wave kernel on `stream` that returns once (int32)(*flag - value) >= 0 -- `flag` a caller-owned device word
 * -- or after timeout_us (<= 100000) microseconds, whichever comes first.  GreedyPipeline's dependency between decode(i)
 * and encoder(i + 1): i2l_greedy_decode_ex publishes `resident_value` to `resident_flag` once the grouped decode kernel's
 * workgroups are all resident, and the encoder stream waits for it here, so that the conv workgroups never get onto the
 * compute units before the decode's (no counterpart in the reference, which runs one batch at a time,
 * predictor.py:205-381).  The wait is bounded, so a signal that never comes costs time, never a hang. */
int i2l_stream_wait_value32(const uint32_t* flag, uint32_t value, float timeout_us, i2l_stream_t stream);

/* ------------------------------------------------------------------------
 * Encoder (reference img2latex/model/encoder.py)
 * ---------------------------------------------------------------------- */

/* One CNN block: y = maxpool2x2(relu(conv3x3_pad1(x, w) + bias)), floor pooling.
 * Replaces nn.Conv2d + nn.ReLU + nn.MaxPool2d, encoder.py:78-95 executed at :122.
 * x (B,Cin,H,W)  w (Cout,Cin,3,3)  bias (Cout)  y (B,Cout,H/2,W/2), NCHW fp32.
 * Arithmetic: with Cin <= 3 or Cin % 16 == 0, Cout % 32/64 == 0 the products
 * run on the bf16 matrix cores with every fp32 operand split exactly into three bf16 pieces (six partial
 * products, fp32 accumulation): fp32-grade results (~2^-24 relative per product), not bit-identical to an fmaf
 * chain.  flags & I2L_FLAG_EXACT_FP32 and other shapes use the exact fp32 kernels.  With argmax_out (training forward)
 * the split kernels also list every pooling window whose arg max or ReLU gate is decided by less than 2^-13 of its
 * magnitude, and a fix-up kernel re-evaluates those windows with fp32 FMAs, so the discrete decisions the backward
 * pass branches on are an fp32 computation's.  The same split applies to i2l_linear_bias_act_fwd for K >= 2048.
 * Limits of the split arithmetic (tests/test_hip_parity.py::test_bf16x3_*): the error class is that of an fp32 fmaf
 * chain, |err| <= ~2^-22 (sum |x||w| + |b|), for operands of magnitude 0 or >= 2^-110 (below that the low split
 * pieces fall into bf16's subnormal range and the class degrades towards bf16); inputs must be finite -- a
 * non-finite input affects only the outputs whose receptive field holds it, but their value is unspecified (NaN
 * where the fp32 product would be +-Inf; ReLU's max may drop a NaN). */
size_t i2l_conv_workspace_bytes(int Cin, int Cout);   /* packed-weight scratch; 0 when none is needed */
/* argmax_out: NULL, or (B,Cout,H/2,W/2) uint8 receiving the position 2*dy+dx of each pooling
 * window's maximum (first maximum wins, as ATen) -- what the backward pass needs. */
int i2l_conv3x3_relu_pool2_fwd(const float* x, const float* w, const float* bias, float* y,
                               uint8_t* argmax_out, int B, int Cin, int H, int W, int Cout, void* workspace,
                               size_t workspace_bytes, int flags, i2l_stream_t stream);

/* Backward of one CNN block (autograd of encoder.py:78-95 under loss.backward(), trainer.py:337):
 * given dy (B,Cout,H/2,W/2), the block's input x, output y and pooling argmax, computes
 * dw (Cout,Cin,3,3), db (Cout) and, unless dx is NULL, dx (B,Cin,H,W).  Gradients are overwritten. */
size_t i2l_conv_bwd_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int i2l_conv3x3_relu_pool2_bwd(const float* x, const float* w, const float* y, const uint8_t* argmax,
                               const float* dy, float* dx, float* dw, float* db, int B, int Cin, int H,
                               int W, int Cout, void* workspace, size_t workspace_bytes, int flags,
                               i2l_lanes* lanes, i2l_stream_t stream);

/* y = act(x @ w^T + bias): nn.Flatten + nn.Linear + nn.ReLU, encoder.py:105-107,125-127
 * (also nn.Linear(Hd->V), decoder.py:90).  x (M,K)  w (N,K)  bias (N) or NULL  y (M,N).
 * relu != 0 applies ReLU.  Split-K partials live in the workspace. */
size_t i2l_linear_workspace_bytes(int M, int K, int N);
int i2l_linear_bias_act_fwd(const float* x, const float* w, const float* bias, float* y,
                            int M, int K, int N, int relu, void* workspace, size_t workspace_bytes,
                            int flags, i2l_stream_t stream);
/* Backward of the above: dy (M,N) -> dx (M,K) (or NULL), dw (N,K), db (N) (or NULL: a layer without bias, e.g. the
 * ResNet convolutions that reach this entry through an im2col image); with relu != 0 the gradient is first masked by
 * y > 0.  Gradients are overwritten. */
size_t i2l_linear_bwd_workspace_bytes(int M, int K, int N);
int i2l_linear_bias_act_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx,
                            float* dw, float* db, int M, int K, int N, int relu, void* workspace,
                            size_t workspace_bytes, int flags, i2l_lanes* lanes, i2l_stream_t stream);

/* ResNet encoder building blocks (reference encoder.py:132-249: torchvision ResNet trunk at :242),
 * inference, bf16 on the matrix cores with fp32 accumulation.  Activations are NHWC bf16 (void*).
 *   y = act( BatchNorm_eval(conv(x, w)) + residual )    w (Cout,Cin,kh,kw) fp32, bn_* (Cout) fp32
 * i2l_conv_bn_bf16_pack is the weight-only preparation (bf16 filter image, BatchNorm folded into
 * scale/bias); its result stays valid until a weight or BatchNorm statistic changes.
 * x is NHWC bf16 (B,H,W,Cin), or the NCHW fp32 image batch when x_is_nchw_f32 != 0 (the stem);
 * residual is NHWC bf16 (B,Ho,Wo,Cout) or NULL; y NHWC bf16 (B,Ho,Wo,Cout).
 * Kernel choice: K = kh*kw*Cin a multiple of 64 with NHWC bf16 input runs the ring-buffered direct-to-LDS GEMM
 * (I2L_FLAG_RESNET_NO_RING: the single-buffered kernel); the 7x7 / stride 2 / pad 3 / 3 -> 64 stem on fp32 images runs
 * the fused stem kernel and needs no workspace (I2L_FLAG_RESNET_IM2COL_STEM: im2col image + GEMM); every other
 * shape goes through an im2col image in the workspace.  All paths compute the same bf16 x bf16 -> fp32 sums.
 * The size query is made for NHWC bf16 input and for the stem: fp32 images always go through the column image
 * (B*Ho*Wo rows of kh*kw*Cin bf16, padded to 8, rounded up to 256 bytes) unless the fused stem takes them, and the
 * call returns I2L_ERR_WORKSPACE when the workspace is smaller than that (Cin % 64 == 0, or a 1x1 / stride 1 conv
 * with Cin % 8 == 0, where the query answers 256 bytes). */
size_t i2l_conv_bf16_packed_bytes(int Cout, int Cin, int kh, int kw);
int i2l_conv_bn_bf16_pack(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                          const float* bn_var, float bn_eps, void* packed, size_t packed_bytes, int Cout,
                          int Cin, int kh, int kw, i2l_stream_t stream);
size_t i2l_conv_bf16_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                     int flags);
int i2l_conv_bn_act_bf16_fwd(const void* x, int x_is_nchw_f32, const void* packed, const void* residual,
                             void* y, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                             int pad, int relu, void* workspace, size_t workspace_bytes, int flags,
                             i2l_stream_t stream);
/* nn.MaxPool2d(3, stride 2, padding 1) on NHWC bf16: (B,H,W,C) -> (B,(H-1)/2+1,(W-1)/2+1,C), C % 8 == 0 (else
 * I2L_ERR_UNSUPPORTED).  i2l_global_avgpool_bf16_fwd below accepts any C (8 channels per thread when C % 8 == 0). */
/* Bottleneck tail + the next block's head in ONE launch (r04; encoder.py:185-249, torchvision Bottleneck.forward's
 * `out = relu(bn3(conv3(out)) + identity)` followed by the next block's `relu(bn1(conv1(x)))`):
 *   y[p][256] = relu(bn3(conv3(o2[p][64])) + identity[p][256]),  z[p][n2] = relu(bn1'(conv1'(y[p])))      NHWC bf16
 * The 128-position tile of y is completed in LDS, written out once (the next block's identity) and multiplied by conv1'
 * from LDS, so y is not read back: layer1 of the bottleneck ResNets is bound by exactly those bytes.  `packed3` /
 * `packed1_next` = i2l_conv_bn_bf16_pack of the two 1x1 convs.  Same roundings as the two launches it replaces (bit-identical
 * y and z).  Shapes: c_mid 64, c_out 256, n2 64 or 128; otherwise I2L_ERR_UNSUPPORTED (the caller makes two launches). */
int i2l_bottleneck_join_bf16_fwd(const void* o2, const void* packed3, const void* identity, void* y, const void* packed1_next,
                                 void* z, long positions, int c_mid, int c_out, int n2, i2l_stream_t stream);
int i2l_maxpool3x3s2_bf16_fwd(const void* x, void* y, int B, int H, int W, int C, i2l_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) + Flatten: NHWC bf16 (B,H,W,C) -> fp32 (B,C). */
int i2l_global_avgpool_bf16_fwd(const void* x, float* y, int B, int H, int W, int C, i2l_stream_t stream);

/* ResNet encoder in TRAINING mode (encoder.py:185-249 under model.train(): every BatchNorm2d of the torchvision trunk
 * normalises with batch statistics and updates its running statistics -- the frozen ones too, freeze_backbone only
 * clears requires_grad, :201-210 -- and layer4 + the Linear, or with freeze_backbone=False every layer, get gradients).
 * fp32 GRADE throughout, as the reference's fp32 branch (trainer.py:334-343): activations, raw conv outputs z and
 * gradients are NHWC fp32 = row-major (M = B*H*W, C) matrices; the convolutions are GEMMs on the split-bf16
 * matrix-core kernel (3 bf16 pieces per operand, fp32 accumulation; I2L_FLAG_EXACT_FP32: fp32 MFMA).
 *
 * Convolution without bias (torchvision's convs have none): x_kind 1 = NHWC fp32 (B,H,W,Cin), 2 = NCHW fp32 (the image
 * batch of the stem); w (Cout,Cin,kh,kw) fp32 as stored by nn.Conv2d; z / dz (B,Ho,Wo,Cout) NHWC fp32.
 *   fwd: z = conv(x, w)
 *   bwd: dw (Cout,Cin,kh,kw) = d/dw, dx (B,H,W,Cin) NHWC fp32 = d/dx; either may be NULL (dx needs x_kind 1).
 * The workspace holds the fp32 column image (none for 1x1 / stride 1) at its head, for dx its gradient, and the GEMM slabs;
 * backward_dx != 0 sizes it for a call with dx (a workspace of that size also serves the forward call, and handing the
 * SAME one to the backward call with I2L_FLAG_CONV_COL_READY saves the second im2col). */
size_t i2l_conv_f32_workspace_bytes(int x_kind, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                                    int pad, int backward_dx);
int i2l_conv_f32_fwd(const float* x, int x_kind, const float* w, float* z, int B, int H, int W, int Cin, int Cout,
                     int kh, int kw, int stride, int pad, void* workspace, size_t workspace_bytes, int flags,
                     i2l_stream_t stream);
int i2l_conv_f32_bwd(const float* x, int x_kind, const float* w, const float* dz, float* dx, float* dw, int B, int H,
                     int W, int Cin, int Cout, int kh, int kw, int stride, int pad, void* workspace,
                     size_t workspace_bytes, int flags, i2l_stream_t stream);
/* nn.BatchNorm2d in training mode on a row-major (M, C) fp32 matrix z, C % 8 == 0 (+ residual add, + ReLU):
 *   fwd: mean and biased variance from ONE pass over z - c (c = row 0 of z: a shift of the order of the mean, so that no
 *        digits cancel; slab sums combined in double); running_* (may both be NULL) <- (1 - momentum) * running +
 *        momentum * (mean, UNBIASED variance);
 *        y = act(gamma * (z - mean) * invstd + beta + residual); save_mean / save_invstd (C)
 *   bwd: g = dy masked by y_relu > 0 (y_relu NULL: no ReLU);  dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat));
 *        dgamma = sum g * xhat, dbeta = sum g (either may be NULL); dres (may be NULL) = g (or += g): the gradient of
 *        the residual branch. */
size_t i2l_bn_train_workspace_bytes(int64_t M, int C);
int i2l_bn_train_fwd_f32(const float* z, const float* residual, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, int relu, float* y,
                         float* save_mean, float* save_invstd, int64_t M, int C, void* workspace,
                         size_t workspace_bytes, i2l_stream_t stream);
int i2l_bn_train_bwd_f32(const float* dy, const float* y_relu, const float* z, const float* gamma, const float* save_mean,
                         const float* save_invstd, float* dz, float* dgamma, float* dbeta, float* dres,
                         int dres_accumulate, int64_t M, int C, void* workspace, size_t workspace_bytes,
                         i2l_stream_t stream);
/* The same trunk under model.eval() at fp32 grade (encoder.py:185-199 builds it, :242 runs it; the reference's fp32
 * branch, trainer.py:334-343): every unit of torchvision's BasicBlock / Bottleneck -- conv, BatchNorm2d on its RUNNING
 * statistics, the shortcut add of the block's last unit, ReLU -- is ONE GEMM launch whose epilogue finalises an element as
 *   v = fmaf(sum_k, scale[n], shift[n]);  v += residual[m][n];  v = relu ? max(v, 0) : v
 * on the complete K sum (after the deterministic slab reduction where K is split: the result does not depend on the split).
 *
 * i2l_bn_eval_fold_f32 (encoder.py:185-199: the nn.BatchNorm2d layers of the torchvision trunk, in eval mode):
 *   scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, evaluated in double and rounded once
 *   to fp32 each (the shift against the rounded scale), so the fold adds no error of its own; all arrays (C) fp32.
 * i2l_conv_bn_act_f32_fwd (encoder.py:185-199,242: conv1/bn1/relu, the blocks' convN/bnN and downsample.0/.1):
 *   y = act(scale * conv(x, w) + shift + residual), y and residual (may be NULL) (B,Ho,Wo,Cout) NHWC fp32; x, x_kind
 *   (1 = NHWC fp32, 2 = NCHW fp32), w, flags (I2L_FLAG_EXACT_FP32: fp32 MFMA GEMM) and the workspace
 *   (i2l_conv_f32_workspace_bytes(..., backward_dx = 0)) as i2l_conv_f32_fwd.  Refused before any launch: a NULL x, w,
 *   scale, shift or y and a non-positive dimension (I2L_ERR_ARG), x_kind outside {1, 2} (I2L_ERR_UNSUPPORTED), a
 *   missing or too small workspace (I2L_ERR_WORKSPACE). */
int i2l_bn_eval_fold_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, float* scale_out, float* shift_out, int C, i2l_stream_t stream);
int i2l_conv_bn_act_f32_fwd(const float* x, int x_kind, const float* w, const float* scale, const float* shift,
                            const float* residual, float* y, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                            int stride, int pad, int relu, void* workspace, size_t workspace_bytes, int flags,
                            i2l_stream_t stream);
/* The two halves of the convolution entry points above, on their own: col (B*Ho*Wo, Cin*kh*kw) fp32 with the column
 * order (ci, ky, kx) of the weight tensor, and the deterministic gather of a column-image gradient back to
 * dx (B,H,W,Cin) NHWC fp32.  x_kind: 0 = NHWC bf16, 1 = NHWC fp32, 2 = NCHW fp32. */
int i2l_im2col_f32(const void* x, int x_kind, int B, int H, int W, int C, int kh, int kw, int stride, int pad,
                   float* col, i2l_stream_t stream);
int i2l_col2im_f32(const float* dcol, int B, int H, int W, int C, int kh, int kw, int stride, int pad, float* dx,
                   int accumulate, i2l_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC fp32 and its backward (x = the forward input; the first maximum of a window takes its
 * gradient, as ATen); nn.AdaptiveAvgPool2d(1) + Flatten (B,H,W,C) -> (B,C) and its backward.  The two forward passes
 * need C % 4 == 0 (else I2L_ERR_UNSUPPORTED); the two backward passes accept any C. */
int i2l_maxpool3x3s2_f32_fwd(const float* x, float* y, int B, int H, int W, int C, i2l_stream_t stream);
int i2l_maxpool3x3s2_f32_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, i2l_stream_t stream);
int i2l_global_avgpool_f32_fwd(const float* x, float* y, int B, int H, int W, int C, i2l_stream_t stream);
int i2l_global_avgpool_bwd_f32(const float* dfeat, float* dx, int B, int H, int W, int C, i2l_stream_t stream);

/* ------------------------------------------------------------------------
 * Decoder (reference img2latex/model/decoder.py, seq2seq.py, predictor.py)
 * ---------------------------------------------------------------------- */

/* Weights of LSTMDecoder as the reference's state_dict holds them (decoder.py:69-90).
 * w_ih/w_hh/b_ih/b_hh are HOST arrays of `layers` device pointers:
 *   w_ih[0] (4H, 2E), w_ih[l>0] (4H, H), w_hh[l] (4H, H), b_ih[l], b_hh[l] (4H); gate order i,f,g,o. */
typedef struct i2l_decoder_weights {
    const float* embedding;      /* (V, E)  decoder.embedding.weight     */
    const float* const* w_ih;    /* decoder.lstm.weight_ih_l{l}          */
    const float* const* w_hh;    /* decoder.lstm.weight_hh_l{l}          */
    const float* const* b_ih;    /* decoder.lstm.bias_ih_l{l}            */
    const float* const* b_hh;    /* decoder.lstm.bias_hh_l{l}            */
    const float* w_out;          /* (V, H)  decoder.output_layer.weight  */
    const float* b_out;          /* (V)     decoder.output_layer.bias    */
    int vocab, embed, hidden, layers;
} i2l_decoder_weights;

/* Bytes of workspace i2l_decoder_prepare() fills for a batch of `rows` encoder rows. */
size_t i2l_decoder_workspace_bytes(int rows, int vocab, int embed, int hidden, int layers);

/* Re-lay the decoder weights for the step kernels (gate-interleaved transposes),
 * fold the token-side half of W_ih_l0 into a (V,4H) table, and compute the per-row
 * constant  enc @ W_ih_l0[:, E:]^T + b_ih_l0 + b_hh_l0  (the half of the layer-0 gate
 * GEMM that does not change over the decode loop; cat([emb, enc]) at decoder.py:228,274).
 * With the reference's Attention over a length-1 source the context equals enc
 * bit-for-bit (decoder.py:338-341, softmax over one element), so `enc` serves both the
 * attention and the no-attention decoder.  enc (rows, E).  `what` selects the part to
 * (re)build: the weight images must be rebuilt whenever a weight changes, the row part
 * whenever enc changes; everything it writes is in `workspace`. */
#define I2L_PREP_WEIGHTS 1   /* transposes + token table: depends on the weights only          */
#define I2L_PREP_ROWS 2      /* per-row constant: depends on enc (and W_ih_l0, biases)        */
#define I2L_PREP_ALL 3
int i2l_decoder_prepare(const i2l_decoder_weights* w, const float* enc, int rows, int what,
                        void* workspace, size_t workspace_bytes, i2l_stream_t stream);

/* Stop rules of the two greedy loops of the reference. */
#define I2L_STOP_NONE 0    /* run all `steps`; Seq2SeqModel._greedy_search stops only when ALL
                              rows emit END in one step (seq2seq.py:220) -- the host finds that
                              step in the returned ids                                          */
#define I2L_STOP_STICKY 1  /* Predictor.predict_batch: a row is finished after its first END
                              (predictor.py:343); a row's ids after its END are -1              */

/* Token selection. */
#define I2L_SELECT_LOGITS 0   /* argmax(logits / temperature)           seq2seq.py:213-215      */
#define I2L_SELECT_SOFTMAX 1  /* argmax(softmax(logits / temperature))  predictor.py:295-297,333: the row-per-workgroup
                                 kernel evaluates the fp32 probabilities literally; the grouped kernel takes the arg max of
                                 the scaled logits, which is the same token unless the two largest are adjacent floats
                                 AND smaller than 2 in magnitude (only then can rounding make their probabilities equal
                                 and hand the tie to the lower index) */
#define I2L_SELECT_SAMPLE 2   /* multinomial over the top-k / top-p masked softmax  predictor.py:299-331 (i2l_sample_decode) */

/* The decode loop: `steps` iterations of [embedding lookup, LSTM step (all layers),
 * output projection, token selection], one persistent launch, no host sync inside.
 * Replaces the loops at seq2seq.py:210-221 and predictor.py:283-347 and, with
 * steps == 1, LSTMDecoder.decode_step (decoder.py:197-284).
 *   workspace   filled by i2l_decoder_prepare() for these `rows`; its trailing scratch region (exchange
 *               granules of the grouped kernel) is WRITTEN by the call: one decode at a time per workspace
 *   tok0        (rows) int32 first input token of every row
 *   forced      (rows, steps) int32 or NULL; if given, the input token of step t is
 *               forced[r][t] (teacher forcing) instead of the previous selection
 *   h0, c0      (L, rows, H) or NULL (zeros, decoder.py:231-244)
 *   ids_out     (rows, steps) int32 or NULL   selected token per step
 *   logits_out  (rows, steps, V) or NULL      raw logits (before temperature)
 *   h_out,c_out (L, rows, H) or NULL          state after the last executed step
 * First index wins ties, as torch.argmax.
 * Kernel choice: L == 1, H == 256, V <= 512, select != I2L_SELECT_SAMPLE, no state in/out, steps >= 8 run the
 * grouped kernel (4 workgroups share 4 rows and keep the weights on chip, in-launch exchanges bounded by a 3 s
 * wall-clock limit); everything else the row-per-workgroup kernel.  If a bounded wait expires (GPU heavily
 * oversubscribed) every id of the affected rows is -3, every requested logit of those rows is NaN and no other
 * output is defined; i2l_greedy_decode_ex with rows_per_workgroup != 0 selects the row-per-workgroup kernel,
 * which needs no co-resident partner. */
int i2l_greedy_decode(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                      const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                      float temperature, int select, int stop, int end_id,
                      int32_t* ids_out, float* logits_out, float* h_out, float* c_out,
                      i2l_stream_t stream);

/* Same as i2l_greedy_decode with an explicit number of batch rows per workgroup (0 = automatic, else 1, 2
 * or 4; a non-zero value also selects the row-per-workgroup kernel), flags (I2L_FLAG_AGENT_SCOPE_EXCHANGE,
 * I2L_FLAG_DECODE_GROUP8) and a RESIDENCY SIGNAL: with resident_flag != NULL (a caller-owned device word) the launch
 * stores resident_value there as soon as its workgroups own their compute units -- a grouped kernel when its last group
 * has completed the placement exchange, any other kernel at once -- for i2l_stream_wait_value32 on another stream
 * (GreedyPipeline: the encoder of batch i + 1 starts beside the decode of batch i, never before it).  If a group times
 * out the word is not written; the waiter's own bound then ends the wait.  Results do not depend on these parameters. */
int i2l_greedy_decode_ex(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                         const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                         float temperature, int select, int stop, int end_id, int rows_per_workgroup,
                         int32_t* ids_out, float* logits_out, float* h_out, float* c_out, int flags,
                         uint32_t* resident_flag, uint32_t resident_value, i2l_stream_t stream);

/* The same loop (seq2seq.py:210-221, predictor.py:283-347; steps == 1: LSTMDecoder.decode_step, decoder.py:197-284) for
 * decoders the grouped kernels do not take -- the shipped hidden 512 / 2 layers (configs/config.yaml:38-50) first of all --
 * STEP-BATCHED on the matrix cores: per step one split-bf16 GEMM + LSTM cell launch per layer (decoder.py:247, 277), one
 * for the logits (decoder.py:250, 280) and one for the selection, all rows of the batch together, so a weight slab is read
 * once per row tile instead of once per row.  The launch boundary is the only barrier: nothing polls, nothing can time
 * out (no -3 ids).  Arguments as i2l_greedy_decode_ex (select: I2L_SELECT_LOGITS / _SOFTMAX, else I2L_ERR_ARG); results
 * agree with it to fp32 rounding (split-bf16 products: the error class of an fp32 fmaf chain), not bit for bit.
 *   scratch     i2l_decode_batched_scratch_bytes(rows, vocab, hidden, layers) bytes of device memory, written by the call:
 *               h (2, L, rows, H), c (L, rows, H), one row of logits per batch row, token / finished / live-row words.
 *               The size query returns 0 for dimensions the kernels refuse (rows <= 0, hidden % 64 != 0 or > 2048,
 *               layers > I2L_MAX_LSTM_LAYERS); the call returns I2L_ERR_WORKSPACE when scratch_bytes is smaller.
 *   stop        I2L_STOP_STICKY: ids are -1 after a row's first END; once every row has ended the remaining launches
 *               return at once (they are still enqueued: no host read happens inside the call).  h_out / c_out of rows
 *               that ended are unspecified.
 *   resident_flag  published at once.  flags: none used.
 * Every refusal is decided on the host before the first HIP call. */
size_t i2l_decode_batched_scratch_bytes(int rows, int vocab, int hidden, int layers);
int i2l_greedy_decode_batched(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                              const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                              float temperature, int select, int stop, int end_id, int32_t* ids_out,
                              float* logits_out, float* h_out, float* c_out, void* scratch, size_t scratch_bytes,
                              int flags, uint32_t* resident_flag, uint32_t resident_value, i2l_stream_t stream);

/* The sampling branch of Predictor.predict_batch (predictor.py:295-331, taken when temperature > 0 and
 * (top_k > 0 or top_p > 0)): probs = softmax(logits/T); top-k keeps p >= k-th largest; top-p drops a
 * token once the probability mass sorted ahead of it exceeds top_p; renormalise; ONE multinomial draw per
 * row and step by inverse CDF with a counter-based uniform of (seed, row, step) -- deterministic for a
 * seed, not bit-comparable with torch.multinomial.  probs_out (rows, steps, V) or NULL receives the final
 * sampling distribution of every step.  vocab <= 2048. */
int i2l_sample_decode(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                      const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                      float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                      float* h_out, float* c_out, i2l_stream_t stream);

/* i2l_sample_decode for decoders the grouped kernels do not take, STEP-BATCHED on the matrix cores: the loop, the scratch
 * (i2l_decode_batched_scratch_bytes), the dimension rules and the sticky stop of i2l_greedy_decode_batched, with a sampling
 * launch in the place of its selection launch -- one workgroup per row: softmax(logits / T) in fp32; the top-k threshold by
 * a radix selection on the probabilities' bit patterns; the top-p cut by a sort of (bit pattern, index) keys, descending
 * with the lower index first among equal values, and a scan of the sorted masses; one draw by inverse CDF over index order
 * at uniform01(seed, row, step) * total, the first column with a non-zero probability whose cdf exceeds it (the arg max if
 * rounding leaves none).  No column walks the vocabulary: O(V log V) per row and step where i2l_sample_decode is O(V^2).
 * A seed draws the same uniforms as in i2l_sample_decode; the logits agree with its logits to fp32 rounding, so the ids
 * agree wherever no mask and no draw sits on a near-tie.  Bitwise reproducible from call to call.
 *   temperature > 0, top_k >= 0, top_p >= 0, not both 0, rows > 0, steps > 0, else I2L_ERR_ARG; vocab > 2048 and the
 *   dimensions i2l_greedy_decode_batched refuses: I2L_ERR_UNSUPPORTED; scratch_bytes too small: I2L_ERR_WORKSPACE.
 *   probs_out (rows, steps, V) or NULL; h_out / c_out (L, rows, H) or NULL.  flags: none used.
 * Every refusal is decided on the host before the first HIP call. */
int i2l_sample_decode_batched(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                              const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                              float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                              float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                              i2l_stream_t stream);

/* One application of the same device code to the caller's logits: (rows, ld) fp32, ld >= vocab, columns >= vocab are not
 * read.  Row r draws at uniform01(seed, r, step).  ids_out (rows) int32; probs_out (rows, vocab) or NULL receives the
 * masked, renormalised distribution.  Needs no decoder and no workspace.  Argument rules as above (step >= 0, ld >= vocab
 * else I2L_ERR_ARG; vocab > 2048: I2L_ERR_UNSUPPORTED), decided on the host before the first HIP call. */
int i2l_sample_logits(const float* logits, int ld, int rows, int vocab, float temperature, int top_k, float top_p,
                      uint64_t seed, int step, int32_t* ids_out, float* probs_out, i2l_stream_t stream);

/* BRACKET-CONSTRAINED step-batched decode: a greedy or sampled row whose groups nest and which ends on END within
 * `steps` (csrc/bracket_rules.inc.h holds the rules, once, for device and host).
 *   cls    (device, vocab bytes) one class byte per column: 0 neutral, 1..4 opens a group of kind 0..3, 5..8 closes a
 *          group of kind 0..3, 255 -- and every other value -- is never emitted.  END is end_id, whatever its byte says.
 *   state  (device, >= i2l_bracket_state_bytes(rows) = 16 bytes per row) uint64 stack (2 bits per open group, the
 *          outermost in the low bits), int32 depth (0..32), int32 ended.  All-zero bytes are the initial state.
 * With rem = steps - t - 1 and d = depth, a row that has not ended may emit at step t: END iff d == 0; a neutral column
 * iff d + 1 <= rem; an open iff d < 32 and d + 2 <= rem; a closer iff d > 0 and the innermost open group is of its kind.
 * d + 1 <= steps - t holds throughout, so a column is always allowed and every row emits END at depth 0 within `steps`
 * steps, each group closed by a closer of its own kind.  Only a table that lacks the closer of a kind it opens can leave
 * no column allowed: the pick is then end_id.  A row that has emitted END is not constrained any more, under either
 * stop rule.  What is guaranteed is nesting and the END; arity (\frac's two groups) and meaning are not.
 * Greedy: the first-index arg max of i2l_greedy_decode_batched's rule over the allowed columns.  Sampling: i2l_sample_
 * decode_batched's rule on the row with -INFINITY in every disallowed column -- probability exactly 0 there, the others
 * renormalise; top-k, top-p and the draw are unchanged.  If no allowed column has a logit above -inf the pick is the
 * first allowed column.  logits_out receives the raw, unmasked logits.
 *
 * i2l_greedy_decode_constrained: the arguments, dimension rules and scratch of i2l_greedy_decode_batched without
 * `forced`, plus cls, state, state_bytes; the call zeroes the state.  end_id outside [0, vocab), cls or state NULL:
 * I2L_ERR_ARG; state_bytes too small: I2L_ERR_WORKSPACE.  i2l_sample_decode_constrained: i2l_sample_decode_batched plus
 * the same three.  Every refusal is decided on the host before the first HIP call; the library keeps no state. */
size_t i2l_bracket_state_bytes(int rows);   /* 16 per row, 0 for rows <= 0 */
int i2l_greedy_decode_constrained(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                  const int32_t* tok0, const float* h0, const float* c0, float temperature, int select,
                                  int stop, int end_id, int32_t* ids_out, float* logits_out, float* h_out, float* c_out,
                                  void* scratch, size_t scratch_bytes, int flags, uint32_t* resident_flag,
                                  uint32_t resident_value, const uint8_t* cls, void* state, size_t state_bytes,
                                  i2l_stream_t stream);
int i2l_sample_decode_constrained(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                  const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                                  float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                                  float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                                  const uint8_t* cls, void* state, size_t state_bytes, i2l_stream_t stream);

/* One application of the same device code to the caller's logits, as i2l_sample_logits: step `step` of `steps` for
 * (rows, ld) fp32 logits, columns >= vocab not read.  top_k == 0 && top_p == 0: the arg max under `select`
 * (I2L_SELECT_LOGITS / _SOFTMAX); otherwise a draw at uniform01(seed, row, step) and probs_out (rows, vocab) or NULL.
 * Reads and ADVANCES the caller's state (rows x 16 bytes; the caller zeroes it before step 0).  allowed_out (rows, vocab)
 * uint8 or NULL receives the mask (all ones for a row that has ended).  temperature <= 0, top_k < 0, top_p < 0, an
 * unknown select, rows / vocab / steps <= 0, ld < vocab, step outside [0, steps), end_id outside [0, vocab), a NULL
 * logits / cls / state / ids_out: I2L_ERR_ARG; sampling with vocab > 2048: I2L_ERR_UNSUPPORTED. */
int i2l_constrained_pick_logits(const float* logits, int ld, int rows, int vocab, float temperature, int select, int top_k,
                                float top_p, uint64_t seed, int step, int steps, const uint8_t* cls, int end_id, void* state,
                                int32_t* ids_out, float* probs_out, uint8_t* allowed_out, i2l_stream_t stream);

/* ARGUMENT-COMPLETE step-batched decode: the bracket-constrained decode above under a stronger rule set
 * (csrc/argument_rules.inc.h holds the rules, once, for device and host): groups nest, END arrives within `steps`, and
 * every column that demands arguments gets them.
 *   cls    (device, vocab bytes) bits 0..3 the class of the bracket table (0 neutral, 1..4 open, 5..8 close), bits 4..5
 *          the number of arguments the column demands (0..3), bit 6 "loose": each argument is a brace group or ONE plain
 *          token (class 0, no demand, not END); without it each is a brace group (opened by a class 1 column that
 *          demands nothing).  Valid iff the low nibble is <= 8, bit 7 is clear, loose comes with a count > 0 and a
 *          closer demands nothing; every other byte is never emitted.  A byte without argument bits means what it means
 *          to i2l_greedy_decode_constrained, and a table of such bytes gives that entry's picks.
 *   state  (device, >= i2l_argument_state_bytes(rows) = 32 bytes per row) uint64 stack, uint64 pending (2 bits per level
 *          0..31: arguments owed there), uint32 loose (1 bit per level), int32 depth, int32 owed (the fewest tokens that
 *          discharge every owed argument), int32 ended.  All-zero bytes are the initial state.
 * Where an argument is owed only an argument opener -- or a plain token, if it is loose -- may be emitted; elsewhere the
 * bracket rules hold, and a column is refused when owed + depth + 1 after it would exceed the emissions left, or when
 * its demand would land on level 32.  Guaranteed beyond nesting and the END: every demanded argument is present.  Not
 * guaranteed: double scripts, a sensible single-token argument, delimiters after \left, matching environment names,
 * meaning.  The three entries take the argument lists of i2l_greedy_decode_constrained, i2l_sample_decode_constrained
 * and i2l_constrained_pick_logits and refuse what they refuse, state_bytes < 32 * rows included. */
size_t i2l_argument_state_bytes(int rows);   /* 32 per row, 0 for rows <= 0 */
int i2l_greedy_decode_arguments(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                const int32_t* tok0, const float* h0, const float* c0, float temperature, int select,
                                int stop, int end_id, int32_t* ids_out, float* logits_out, float* h_out, float* c_out,
                                void* scratch, size_t scratch_bytes, int flags, uint32_t* resident_flag,
                                uint32_t resident_value, const uint8_t* cls, void* state, size_t state_bytes,
                                i2l_stream_t stream);
int i2l_sample_decode_arguments(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                                float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                                float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                                const uint8_t* cls, void* state, size_t state_bytes, i2l_stream_t stream);
int i2l_arguments_pick_logits(const float* logits, int ld, int rows, int vocab, float temperature, int select, int top_k,
                              float top_p, uint64_t seed, int step, int steps, const uint8_t* cls, int end_id, void* state,
                              int32_t* ids_out, float* probs_out, uint8_t* allowed_out, i2l_stream_t stream);

/* ENSEMBLE decode (this package: the reference decodes with one model): n decoders of ONE vocabulary choose every token
 * together, on the step-batched loop.  Each member runs its own LSTM and logits launches on its own state along the
 * SHARED tokens; one launch per step combines the members' rows (csrc/ensemble_rules.inc.h holds the rule, once, for
 * device and host) and the selection kernels of the entries above pick from the combined row.  With weights w_m
 * normalised to sum 1 and lp_m = log_softmax of member m's raw logits over [0, vocab) (no temperature):
 *   I2L_ENSEMBLE_LOGPROB  y[v] = sum_m w_m lp_m[v]            (geometric mean, left unnormalised)
 *   I2L_ENSEMBLE_PROB     y[v] = log(sum_m w_m exp(lp_m[v]))  (arithmetic mean)
 * y is "the ensemble's logits": the division by the temperature, select, the top-k / top-p sampling, the constraint masks
 * and dist_out treat it as they treat one model's logits.  A column that is -inf in one member is -inf under LOGPROB;
 * under PROB the other members decide.  n == 1: no combination, the call is i2l_greedy_decode_batched /
 * i2l_sample_decode_batched (or their constrained forms) bit for bit.  A step is sum(layers) + n + 2 launches on `stream`.
 *   members     n records (this package): weights, the workspace i2l_decoder_prepare built for them and these rows,
 *               optional h0 / c0 (both or neither) and h_out / c_out, each (layers, rows, hidden) of THAT member, and
 *               weight (finite, > 0; normalised by the call).  Members may differ in embed, hidden and layers.
 *   select      I2L_SELECT_LOGITS / _SOFTMAX: the arg max, top_k / top_p / seed ignored, dist_out (rows, steps, vocab) or
 *               NULL receives the combined rows y.  I2L_SELECT_SAMPLE: i2l_sample_decode_batched's draw, dist_out receives
 *               the sampling distributions.
 *   cls_kind    I2L_CONSTRAIN_NONE (cls, state ignored), _BRACKETS (i2l_greedy_decode_constrained's table and 16-byte
 *               states) or _ARGUMENTS (i2l_greedy_decode_arguments' table and 32-byte states); the call zeroes the state.
 *   scratch     i2l_ensemble_scratch_bytes(members, n, rows) bytes of device memory (0 for members the call refuses).
 * Refused on the host before the first HIP call: n < 1, a NULL member / weights / workspace / tok0, vocabularies that
 * differ, a weight that is not finite and > 0, an unknown combine, select, stop or cls_kind, rows or steps <= 0, the
 * sampling arguments i2l_sample_decode_batched refuses, `forced` together with sampling or a constraint, end_id outside
 * [0, vocab) or a NULL cls / state under a constraint (all I2L_ERR_ARG); n > I2L_MAX_ENSEMBLE, dimensions
 * i2l_greedy_decode_batched refuses, sampling with vocab > 2048 (I2L_ERR_UNSUPPORTED); scratch_bytes or state_bytes too
 * small (I2L_ERR_WORKSPACE).  flags: none used.  The library keeps no state. */
#define I2L_MAX_ENSEMBLE 8
#define I2L_ENSEMBLE_LOGPROB 0
#define I2L_ENSEMBLE_PROB 1
#define I2L_CONSTRAIN_NONE 0
#define I2L_CONSTRAIN_BRACKETS 1
#define I2L_CONSTRAIN_ARGUMENTS 2
typedef struct i2l_ensemble_member {
    const i2l_decoder_weights* w;
    const void* workspace;
    const float* h0;
    const float* c0;
    float* h_out;
    float* c_out;
    float weight;
} i2l_ensemble_member;
size_t i2l_ensemble_scratch_bytes(const i2l_ensemble_member* members, int n, int rows);
int i2l_ensemble_decode(const i2l_ensemble_member* members, int n, int combine, int rows, int steps, const int32_t* tok0,
                        const int32_t* forced, float temperature, int select, int top_k, float top_p, uint64_t seed,
                        int stop, int end_id, const uint8_t* cls, int cls_kind, void* state, size_t state_bytes,
                        int32_t* ids_out, float* dist_out, void* scratch, size_t scratch_bytes, int flags,
                        i2l_stream_t stream);

/* CONSENSUS decode (this package: the reference draws one sample per image): `samples` draws of each of `images` images
 * in ONE step-batched loop, scored, and ranked on the device (csrc/sample_rank_rules.inc.h holds the rules, once, for
 * device and host).  Row i * samples + s of the loop is sample s of image i: the rows of an image share its encoder row
 * of the workspace -- prepared for `images` rows, not images * samples -- and tok0[i]; the uniform of a row stays
 * uniform01(seed, row, step), so the samples of an image differ.  The stop rule is sticky and the start state zero.
 *   score     per sample, fp64: the sum over its steps up to and including END of the log-probability of the committed
 *             token under the softmax of the RAW logits over the columns the row's constraint allows (no temperature,
 *             no top-k / top-p truncation; a forbidden column enters as -inf; a constraint's fallback pick adds 0):
 *             (x[pick] - max) - logf(sum expf(x - max)) in fp32, the beam search's formula, so a sample and a beam
 *             hypothesis of the same tokens carry comparable scores.
 *   cut       a sample's sequence is its tokens before the first end_id (all `steps` without one); len = tokens after
 *             START, END included (sequence length + 1 if it ended, else steps); finished = 1 iff it holds END.
 *   risk      risk[s] = sum over the image's samples s' of the Levenshtein distance of the two cut sequences (int32).
 *   rank      I2L_RANK_CONSENSUS: ascending risk, then descending score, then ascending sample index; key = (double)risk
 *             (the minimum-Bayes-risk candidate first).  I2L_RANK_LOGPROB: descending key = score / length_norm[len]
 *             (length_norm: i2l_beam_decode_nbest's DEVICE table of steps + 1 fp64 values, or NULL = all ones), then
 *             ascending sample index.  Duplicates are kept: every image reports `samples` entries.
 *   constrain_kind  I2L_CONSTRAIN_NONE (cls ignored), _BRACKETS or _ARGUMENTS with the [vocab] class table of
 *             i2l_sample_decode_constrained / _arguments; the rows' states live in the scratch and are zeroed by the call.
 *   scratch   i2l_sample_multi_scratch_bytes(...) bytes of device memory (0 for dimensions the call refuses).
 *   outputs   DEVICE arrays in SAMPLE order: ids_out (images, samples, steps) int32, -1 behind END; len_out, finished_out,
 *             risk_out int32, score_out, key_out fp64, all (images, samples); order_out (images, samples) int32: the
 *             sample indices of an image, best first.
 * A step is layers + 2 launches, the ranking two more at the end; no poll, no cooperative launch.
 * Refused on the host before the first HIP call: NULL weights / workspace / tok0 or any NULL output,
 * images, samples or steps <= 0, an unknown rank or constrain_kind, the sampling arguments i2l_sample_decode_batched
 * refuses, a NULL cls or an end_id outside [0, vocab) under a constraint (I2L_ERR_ARG); samples > I2L_MAX_NBEST, steps >
 * I2L_MAX_RANK_STEPS, dimensions i2l_sample_decode_batched refuses (I2L_ERR_UNSUPPORTED); scratch NULL or too small
 * (I2L_ERR_WORKSPACE).  flags: none used.  The library keeps no state.
 *
 * i2l_sample_rank is the ranking alone on a caller's DEVICE ids (images, samples, steps) and scores (images, samples):
 * the same cut, risk, key and order; dist_out (images, samples, samples) int32 or NULL receives the distances.  Same
 * limits and refusals (NULL ids / score / outputs, images, samples or steps <= 0, unknown rank: I2L_ERR_ARG). */
#define I2L_RANK_CONSENSUS 0
#define I2L_RANK_LOGPROB 1
#define I2L_MAX_RANK_STEPS 1024
size_t i2l_sample_multi_scratch_bytes(int images, int samples, int vocab, int hidden, int layers, int steps,
                                      int constrain_kind);
int i2l_sample_decode_multi(const i2l_decoder_weights* w, const void* workspace, int images, int samples, int steps,
                            const int32_t* tok0, float temperature, int top_k, float top_p, uint64_t seed, int end_id,
                            int constrain_kind, const uint8_t* cls, int rank, const double* length_norm, void* scratch,
                            size_t scratch_bytes, int32_t* ids_out, int32_t* len_out, int32_t* finished_out,
                            double* score_out, int32_t* risk_out, double* key_out, int32_t* order_out, int flags,
                            i2l_stream_t stream);
int i2l_sample_rank(const int32_t* ids, int images, int samples, int steps, int end_id, const double* score, int rank,
                    const double* length_norm, int32_t* len_out, int32_t* finished_out, int32_t* risk_out,
                    double* key_out, int32_t* order_out, int32_t* dist_out, i2l_stream_t stream);

/* Beam search for `images` independent images, `beam` beams each (<= I2L_MAX_BEAM):
 * per image exactly Seq2SeqModel._beam_search at batch 1 (seq2seq.py:234-298) --
 * log_softmax in fp32, top-k sorted descending with lower index first on ties, scores
 * accumulated in fp64, stable descending selection, ended beams retire one iteration
 * later, no length normalisation.  workspace prepared for rows == images.
 *   seq_out  (images, steps+1) int32: best sequence, START stripped, cut at END, -1 padded
 *   len_out  (images) int32;  score_out (images) fp64 or NULL.
 * Kernel choice: hidden == 256, one layer, vocab <= 512, 2 <= beam <= 6 run the grouped kernel (four workgroups
 * share 12 beam slots = 12/beam images and keep the weights on chip; per step they exchange h and, per slot, each
 * member's local top-k and (max, sum exp), from which log_softmax is assembled); other shapes, and
 * flags & I2L_FLAG_NO_GROUP, run one workgroup per image.  Both give the same sequences; scores agree to fp32
 * log_softmax rounding.  If a poll of the grouped kernel times out (GPU shared or oversubscribed) the affected
 * images get len_out = -3 and no other output: call again with I2L_FLAG_NO_GROUP. */
size_t i2l_beam_workspace_bytes(int images, int beam, int hidden, int layers, int steps);
int i2l_beam_decode(const i2l_decoder_weights* w, const void* workspace, int images, int beam,
                    int steps, int start_id, int end_id, void* beam_workspace,
                    size_t beam_workspace_bytes, int32_t* seq_out, int32_t* len_out,
                    double* score_out, int flags, i2l_stream_t stream);

/* The same search (seq2seq.py:234-298 per image: log_softmax in fp32 and top-k :266-267, fp64 scores and the stable
 * descending selection :268-280, ended beams retire one iteration later :258-260, `completed.extend(beams); break`
 * :282-284, max(completed) else beams[0] :286-297) for decoders the grouped beam kernel does not take -- the shipped
 * hidden 512 / 2 layers at the reference's default beam_size 2 (configs/config.yaml:45-50,76) first of all -- STEP-BATCHED
 * on the matrix cores: the images x beam slots are the rows of one step, row r = slot r % beam of image r / beam.  Per
 * step: the split-bf16 GEMM + LSTM cell launch of i2l_greedy_decode_batched per layer, its logits launch, and one launch
 * (a workgroup per image) that ranks the image's candidates, writes the histories, gathers h and c of the new slots from
 * their parents and retires ended slots.  One device word counts the images still searching; once it is 0 the remaining
 * launches return at once (they are still enqueued: no host read happens inside the call).  Nothing polls, nothing can
 * time out: len_out is never -3.  Outputs and semantics as i2l_beam_decode (workspace prepared for rows == images);
 * sequences agree with it wherever the ranking has no fp32 near-tie, scores to fp32 rounding.
 *   scratch  i2l_beam_batched_scratch_bytes(images, beam, vocab, hidden, layers, steps) bytes of device memory, written
 *            by the call: the token / parent histories (images, steps, beam), h and c as (2, L, images * beam, H) each,
 *            one padded row of logits per slot, per slot the fp64 score, last token and live flag, per image the beam
 *            count, the best completed beam and the done flag, and the live-image word.
 * Accepted: hidden % 64 == 0 and <= 2048, layers <= I2L_MAX_LSTM_LAYERS, 1 <= beam <= I2L_MAX_BEAM, beam <= vocab,
 * vocab <= 2048 (the top-k scan marks taken columns in 32 bits per lane).  For other dimensions, images <= 0 or steps <= 0
 * the size query returns 0; the call returns I2L_ERR_ARG for NULL or non-positive arguments, I2L_ERR_UNSUPPORTED for
 * refused dimensions, I2L_ERR_WORKSPACE when scratch_bytes is smaller.  flags: none used.  Every refusal is decided on
 * the host before the first HIP call. */
size_t i2l_beam_batched_scratch_bytes(int images, int beam, int vocab, int hidden, int layers, int steps);
int i2l_beam_decode_batched(const i2l_decoder_weights* w, const void* workspace, int images, int beam, int steps,
                            int start_id, int end_id, void* scratch, size_t scratch_bytes, int32_t* seq_out,
                            int32_t* len_out, double* score_out, int flags, i2l_stream_t stream);

/* N-best beam search with length-normalised ranking: the search of i2l_beam_decode_batched (the same launches per step,
 * the same candidates, fp64 scores, stable selection, retirement one iteration later and both `break`s), with another
 * ending.  Every completed beam b is kept with key(b) = score(b) / length_norm[n(b)], n = its tokens after START, END
 * included; the result rows of an image are `completed` sorted by key, descending and stable (earlier-retired first, slot
 * order within a step), cut to nbest.  If the search ran out of steps (neither `break` fired) and rows are left, the
 * final beams follow, by key, stable in slot order; such a row has finished = 1 iff its last token is END (the
 * reference never retires a beam that ends at the very last step).  Rows from `completed` have finished = 1.  With
 * nbest = 1 and length_norm NULL, seq / len / score are those of i2l_beam_decode_batched, bit for bit.
 *   length_norm  DEVICE array of steps + 1 fp64 values, finite and > 0 (the caller validates them), or NULL = all ones;
 *                the kernel only divides (correctly rounded: a host restatement gets the same keys).  [0] is used only
 *                when start_id == end_id.
 *   seq_out      (images, nbest, steps + 1) int32: START stripped, cut at END, -1 padded
 *   len_out      (images, nbest) int32;  score_out (images, nbest) fp64 raw sums;  key_out (images, nbest) fp64 or NULL
 *   finished_out (images, nbest) int32 or NULL;  count_out (images) int32 rows filled.
 *   Rows >= count: len = -1, ids = -1, score = key = -inf, finished = 0.  Every element of every output is written.
 *   scratch      i2l_beam_nbest_scratch_bytes(...) bytes: that of i2l_beam_decode_batched plus per image nbest entries
 *                (key, score, history row, slot).
 * Accepted: as i2l_beam_decode_batched, and 1 <= nbest <= I2L_MAX_NBEST whatever the beam width (nbest > beam is legal:
 * `completed` grows by up to `beam` entries per step).  Refusals as there (a NULL score_out or count_out is I2L_ERR_ARG
 * too; nbest <= 0: I2L_ERR_ARG, nbest > I2L_MAX_NBEST: I2L_ERR_UNSUPPORTED), decided on the host before the first HIP
 * call; the size query returns 0 for refused dimensions.  flags: none used.  The library keeps no state. */
size_t i2l_beam_nbest_scratch_bytes(int images, int beam, int nbest, int vocab, int hidden, int layers, int steps);
int i2l_beam_decode_nbest(const i2l_decoder_weights* w, const void* workspace, int images, int beam, int nbest, int steps,
                          int start_id, int end_id, const double* length_norm, void* scratch, size_t scratch_bytes,
                          int32_t* seq_out, int32_t* len_out, double* score_out, double* key_out, int32_t* finished_out,
                          int32_t* count_out, int flags, i2l_stream_t stream);

/* Well-formed N-best beam search: i2l_beam_decode_nbest in which every hypothesis ever ranked is a prefix the bracket rules
 * of i2l_greedy_decode_constrained allow, so every returned row nests its groups and ends on END.  A live slot at step t
 * extends only by the columns its bracket state allows at rem = steps - t - 1; its candidates are the top
 * min(beam, #allowed) of them, and their log-probs are the log-softmax over the allowed columns only (a forbidden column
 * enters the softmax as -inf, as in i2l_sample_decode_constrained), so scores are log-probabilities under the constrained
 * model and a forced closer or END costs 0.  A new beam inherits its parent's state advanced by its token.  At step
 * steps - 1 the only candidate of every live slot is END: the search never runs out of steps, every filled row has
 * finished = 1.  If a slot has no allowed column with a logit above -inf (a table in which an open kind has no closer, or
 * non-finite logits) its single candidate is (end_id, 0.0): defined, but that row is not well formed.
 *   cls          DEVICE array of `vocab` class bytes, as for i2l_greedy_decode_constrained; end_id's entry is ignored
 *   scratch      i2l_beam_nbest_constrained_scratch_bytes(...) bytes: that of i2l_beam_decode_nbest plus 16 bytes of
 *                bracket state per slot, zeroed by the call
 * Everything else -- outputs, length_norm, ranking, accepted dimensions, refusals -- as i2l_beam_decode_nbest; a NULL cls or
 * an end_id outside [0, vocab) is I2L_ERR_ARG.  nbest = 1 with a NULL length_norm is the constrained single-best search.
 * The same launches per step as i2l_beam_decode_nbest; every refusal is decided on the host before the first HIP call.
 * flags: none used.  The library keeps no state. */
size_t i2l_beam_nbest_constrained_scratch_bytes(int images, int beam, int nbest, int vocab, int hidden, int layers,
                                                int steps);
int i2l_beam_decode_nbest_constrained(const i2l_decoder_weights* w, const void* workspace, int images, int beam, int nbest,
                                      int steps, int start_id, int end_id, const double* length_norm, void* scratch,
                                      size_t scratch_bytes, int32_t* seq_out, int32_t* len_out, double* score_out,
                                      double* key_out, int32_t* finished_out, int32_t* count_out, int flags,
                                      const uint8_t* cls, i2l_stream_t stream);

/* Additive attention, general source length S (Attention.forward, decoder.py:312-343):
 * context[b] = softmax_s(v . tanh(W [hidden[b] ; enc[b,s]] + b_a)) @ enc[b].
 * hidden (B,H)  enc (B,S,E)  w_attn (H, H+E)  b_attn (H)  v (H)  context (B,E). */
int i2l_attention_context_fwd(const float* hidden, const float* enc, const float* w_attn,
                              const float* b_attn, const float* v, float* context,
                              int B, int S, int H, int E, i2l_stream_t stream);

/* ------------------------------------------------------------------------
 * Training step (reference img2latex/training/trainer.py:303-343, fp32 branch)
 * ---------------------------------------------------------------------- */

/* Gradient buffers, same shapes / key names as i2l_decoder_weights (HOST arrays of device pointers). */
typedef struct i2l_decoder_grads {
    float* embedding;
    float* const* w_ih;
    float* const* w_hh;
    float* const* b_ih;
    float* const* b_hh;
    float* w_out;
    float* b_out;
} i2l_decoder_grads;

/* Teacher-forced LSTMDecoder.forward in training mode (decoder.py:100-195) for input tokens
 * (B,T) int32 [= formulas[:, :-1], seq2seq.py:115-120]; keeps what BPTT needs in `workspace`.
 * dropout_p: nn.Dropout p in [0, 1) (anything else, NaN included, is I2L_ERR_ARG in both calls; 0 disables).  The masks
 * are a counter-based hash of (seed, stream, element index), never stored: the hash, the streams, the element indices and
 * which half of X is masked on which path are stated once in DESIGN.md, section 4, "The dropout mask rule";
 * attention_path: 0 = decoder.py:121-143 (dropout on cat[emb,enc]), 1 = :144-193 (dropout on emb).
 * logits_out (B,T,V).  flags: I2L_FLAG_NO_GROUP (row-per-workgroup recurrences), I2L_FLAG_EXACT_FP32 (GEMMs),
 * I2L_FLAG_TRAIN_BATCHED (step-batched recurrences); the caller MUST pass the same flags to the backward call: forward
 * and backward of one step have to agree on the path (the step-batched backward keeps its scratch where the forward kept
 * GX, and accepts dimensions the row kernels refuse).  If a bounded wait of the grouped recurrence expires its outputs are
 * NaN (the loss and every gradient become NaN; i2l_grad_clip_adam_step then skips the update).
 * Accepted: embed % 4 == 0, hidden % 64 == 0, layers <= I2L_MAX_LSTM_LAYERS, hidden <= 1024 -- with
 * I2L_FLAG_TRAIN_BATCHED honoured, hidden <= 2048.  i2l_decoder_train_batched_ok (pure host code) returns 1 for the
 * dimensions at which the flag is honoured (I2L_FLAG_EXACT_FP32 clear) and 0 otherwise.  The workspace size does not
 * depend on the flag. */
size_t i2l_decoder_train_workspace_bytes(int B, int T, int vocab, int embed, int hidden, int layers);
int i2l_decoder_train_batched_ok(int vocab, int embed, int hidden, int layers);
int i2l_decoder_train_fwd(const i2l_decoder_weights* w, const float* enc, const int32_t* tokens, int B, int T,
                          float dropout_p, uint64_t seed, int attention_path, void* workspace,
                          size_t workspace_bytes, float* logits_out, int flags, i2l_stream_t stream);
/* Backward of the above for a given dlogits (B,T,V): fills every gradient of `grads` (overwrite)
 * and denc_out (B,E).  `workspace` must be the one the forward call filled. */
int i2l_decoder_train_bwd(const i2l_decoder_weights* w, const int32_t* tokens, int B, int T, float dropout_p,
                          uint64_t seed, int attention_path, void* workspace, size_t workspace_bytes,
                          const float* dlogits, const i2l_decoder_grads* grads, float* denc_out,
                          int flags, i2l_lanes* lanes, i2l_stream_t stream);

/* nn.CrossEntropyLoss(ignore_index=pad, label_smoothing=eps) over `rows` = B*T rows of logits (rows,V)
 * (trainer.py:111-115,335-336).  loss_sum_and_count_out[0] = SUM over non-pad rows of the per-row loss,
 * [1] = number of non-pad rows (loss = [0]/[1]); dlogits_out (rows,V) or NULL = gradient of the SUM
 * (divide by the GLOBAL count after the data-parallel all-reduce). */
size_t i2l_ce_workspace_bytes(int rows);
int i2l_ce_label_smooth_fwd_bwd(const float* logits, const int32_t* targets, int rows, int vocab, int pad_id,
                                float label_smoothing, void* workspace, size_t workspace_bytes,
                                float* dlogits_out, float* loss_sum_and_count_out, i2l_stream_t stream);

/* Word-level distillation (this package; the reference trains on the data set's tokens alone): the loss above plus the
 * divergence of the student's token distribution from that of n teachers, at every kept row, in one fused launch and an
 * ordered sum -- no (rows, vocab) intermediate.  csrc/distill_rules.inc.h states the rule; per row with target t != pad_id,
 * student logits x, teacher rows z_m, weights w_m (normalised to sum 1 as in i2l_ensemble_decode):
 *   hard = (1-eps)(lse(x) - x[t]) + eps(lse(x) - mean_v x[v])      exactly i2l_ce_label_smooth_fwd_bwd's row loss
 *   y    = the ensemble's row under `combine` (I2L_ENSEMBLE_LOGPROB / _PROB, csrc/ensemble_rules.inc.h); n == 1: y = z_0
 *   q = softmax(y / temperature), p = softmax(x / temperature)     the temperature is applied to y, not to the members
 *   soft = temperature^2 sum_v q[v](log q[v] - log p[v])           a term with q[v] == 0 is 0
 *   row loss = alpha hard + (1 - alpha) soft
 *   dlogits[v] = alpha (softmax(x)[v] - (1-eps)[v == t] - eps/vocab) + (1 - alpha) temperature (p[v] - q[v])
 * loss_sum_and_count_out[0] = SUM of the row losses (alpha parts[0] + (1 - alpha) parts[1] up to rounding), [1] = the
 * number of non-pad rows, an exact integer; parts_out (2 floats or NULL) = SUM of hard, SUM of soft, unweighted;
 * dlogits_out (rows, vocab) or NULL = gradient of the SUM, as above.  The three sums are fixed-order double sums:
 * deterministic, and the same with and without dlogits_out / parts_out.
 * A pad row adds exactly 0 to every sum and has exactly zero dlogits; it is selected, not multiplied: neither the
 * student's nor the teachers' values at pad rows are read, so a NaN there reaches no output.  Teacher logits at kept rows
 * must be finite (-inf or NaN there is outside the rule); a NaN in the student's row gives NaN sums, after which
 * i2l_grad_clip_adam_step skips the update.  Teacher m's logits are (rows, ld) with ld >= vocab.
 * Accepted: 1 <= n <= I2L_MAX_ENSEMBLE, combine one of the two rules, weights finite and > 0, temperature finite and > 0,
 * 0 <= alpha <= 1, rows >= 1, every vocab >= 1 (a row longer than 512 columns is re-read, not refused).  Anything else is
 * I2L_ERR_ARG, a short workspace I2L_ERR_WORKSPACE; both are answered by host code before the first HIP call and leave
 * every output untouched. */
typedef struct i2l_distill_teacher {
    const float* logits;   /* (rows, ld) */
    int ld;                /* >= vocab */
    float weight;
} i2l_distill_teacher;
size_t i2l_ce_distill_workspace_bytes(int rows);
int i2l_ce_distill_fwd_bwd(const float* logits, const int32_t* targets, int rows, int vocab, int pad_id,
                           float label_smoothing, const i2l_distill_teacher* teachers, int n, int combine,
                           float temperature, float alpha, void* workspace, size_t workspace_bytes,
                           float* dlogits_out, float* loss_sum_and_count_out, float* parts_out, i2l_stream_t stream);

/* Minimum-risk fine-tuning (this package; the reference trains on the gold prefix alone): train on the model's own draws,
 * each weighted by how its Levenshtein similarity to the gold formula compares with the image's other draws.
 * csrc/risk_rules.inc.h states the rules; the four entries below are the launches a training step adds.
 *
 * i2l_risk_rows: formulas (images, steps + 1) int32 = [START, tokens, END, PAD ...]; draws (images, samples, steps) int32
 * as i2l_sample_decode_multi leaves them (-1 behind END).  Per image and draw n:
 *   cut        draw: its ids before the first end_id (all `steps` without one); gold: formulas[1:] before the first
 *              end_id or pad_id
 *   dist_out   the exact Levenshtein distance d of the two;  len_out  the draw's number of tokens
 *   reward_out r = 1 - d / max(len_draw, len_gold), 1 when both are empty, in double, rounded to fp32 once
 *   advantage_out  A[n] = r[n] - (sum over m != n of r[m], in index order) / (samples - 1), in double from the double
 *              rewards, rounded once
 * and the batch of images (samples + 1) sequences, image-major, each steps + 1 tokens (rows_out), one value per sequence in
 * coef_out / smooth_out / part_out:
 *   sequence b (samples + 1)           the gold row as it stands; coef alpha, smooth label_smoothing, part 0
 *   sequence b (samples + 1) + 1 + n   [START, draw n through its END, pad_id ...]; coef (float)((1 - (double)alpha) A[n])
 *                                      from the double advantage, smooth 0, part 1
 * A pad_id the model sampled before its END stays in the row (where the loss masks it like a gold PAD) and counts in the
 * distance and the length.  One workgroup per image, one wave per draw; no atomics, no polls; every element of the eight
 * outputs is written.
 * Accepted: images, steps >= 1, steps <= I2L_MAX_RANK_STEPS, 2 <= samples <= I2L_MAX_NBEST, 0 <= alpha <= 1,
 * 0 <= label_smoothing < 1.  A NULL pointer, a non-positive dimension, alpha or label_smoothing outside its range:
 * I2L_ERR_ARG; samples < 2 or > I2L_MAX_NBEST, steps > I2L_MAX_RANK_STEPS: I2L_ERR_UNSUPPORTED.
 *
 * i2l_ce_weighted_fwd_bwd: i2l_ce_label_smooth_fwd_bwd whose token row i belongs to sequence i / steps (logits
 * (seqs * steps, vocab), targets (seqs * steps)), each sequence with its own coefficient, smoothing and part:
 *   dlogits[i][v] = keep coef (softmax(x)[v] - (1 - eps)[v == t] - eps / vocab),   eps = seq_smooth[seq]
 *   loss_sum_and_count_out[0] = SUM_i coef row_loss_i (row_loss as in i2l_ce_label_smooth_fwd_bwd with the sequence's eps),
 *   [1] = the UNWEIGHTED number of non-pad rows; parts_out (4 floats or NULL) = [loss sum, non-pad rows] of the sequences
 *   with seq_part == 0, then of all the others, unweighted.  Fixed-order double sums.  With every coefficient 1 and one
 *   smoothing value every output equals i2l_ce_label_smooth_fwd_bwd's bit for bit.  workspace:
 *   i2l_ce_weighted_workspace_bytes(seqs * steps).  NULL pointers (dlogits_out and parts_out may be NULL), non-positive
 *   dimensions: I2L_ERR_ARG; seqs * steps >= 2^31: I2L_ERR_UNSUPPORTED; a short workspace: I2L_ERR_WORKSPACE.
 *
 * i2l_rows_repeat: out[r * times + j][:] = in[r][:], in (rows, width), out (rows * times, width) fp32.
 * i2l_rows_fold:   out[r][:] = sum_j in[r * times + j][:], an fp32 sum in the order j = 0 .. times - 1; in (rows * times,
 * width), out (rows, width).  The gradient of i2l_rows_repeat.  NULL pointers, non-positive dimensions or more than 2^38
 * elements: I2L_ERR_ARG.
 *
 * Every refusal of the four is host code before the first HIP call and leaves every output untouched. */
int i2l_risk_rows(const int32_t* formulas, const int32_t* draws, int images, int samples, int steps, int start_id,
                  int end_id, int pad_id, float alpha, float label_smoothing, int32_t* rows_out, float* coef_out,
                  float* smooth_out, int32_t* part_out, int32_t* dist_out, int32_t* len_out, float* reward_out,
                  float* advantage_out, i2l_stream_t stream);
size_t i2l_ce_weighted_workspace_bytes(int rows);
int i2l_ce_weighted_fwd_bwd(const float* logits, const int32_t* targets, int seqs, int steps, int vocab, int pad_id,
                            const float* seq_coef, const float* seq_smooth, const int32_t* seq_part, void* workspace,
                            size_t workspace_bytes, float* dlogits_out, float* loss_sum_and_count_out, float* parts_out,
                            i2l_stream_t stream);
int i2l_rows_repeat(const float* in, int rows, int width, int times, float* out, i2l_stream_t stream);
int i2l_rows_fold(const float* in, int rows, int width, int times, float* out, i2l_stream_t stream);

/* clip_grad_norm_(max_norm) + Adam(lr, betas, eps, coupled L2 weight_decay) over flat fp32 buffers of
 * n elements (trainer.py:91-93,338-342).  grads hold the gradient of the SUM loss; count_ptr (device,
 * may be NULL = 1) is the number of non-pad target tokens the sum runs over (the GLOBAL count after the
 * data-parallel all-reduce).  step >= 1 is the optimizer step number (bias correction).
 * stats_out (device, 4 floats): total gradient norm, clip coefficient, 1/count, skipped (1.0 when the total norm
 * was not finite -- Inf/NaN gradients, e.g. after a grouped kernel's timeout -- and the call therefore left
 * params, exp_avg and exp_avg_sq untouched, exactly what GradScaler's skipped step does; else 0.0).
 * max_norm <= 0: no clipping.  lr, the betas, eps, weight_decay and max_norm are taken at their fp32 values; the bias
 * corrections are evaluated in double from those and rounded once, so a step is within fp32 rounding (tested: 2^-23 |p|
 * + 2^-21 |update|) of torch.optim.Adam + clip_grad_norm_ in float64 on the same fp32-valued hyperparameters.  Against
 * torch.optim.Adam called with the Python doubles 0.9 / 0.999 the update differs by 7e-6 of itself (measured: the
 * largest over steps 1..5), because 0.999f != 0.999; a float ABI cannot remove that.  The workspace also carries the
 * number of skipped calls so far (zero it once before the first call; the bias correction uses step minus that
 * number, so `step` may simply count calls). */
size_t i2l_optimizer_workspace_bytes(void);
int i2l_grad_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                            const float* count_ptr, float max_norm, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int step, void* workspace, size_t workspace_bytes,
                            float* stats_out, i2l_stream_t stream);

/* ------------------------------------------------------------------------
 * Evaluation metrics (reference img2latex/training/metrics.py), SURVEY section 8(f)-4
 * ---------------------------------------------------------------------- */

/* Integer statistics of `pairs` (prediction, target) id sequences, one workgroup per pair:
 *   lev_out[p]       the corner dist_tab[rows][cols] of levenshtein_distance's table, metrics.py:63-83
 *                    (equal tokens copy the diagonal neighbour, otherwise 1 + min(up, left, diagonal))
 *   match_out[p][g]  g = 0..3: sum over the DISTINCT (g+1)-grams of the prediction of
 *                    min(count in prediction, count in target) -- bleu_n_score's matching_grams_sum,
 *                    metrics.py:136-160; 0 for g >= max_n or when either sequence is shorter than g+1
 *   tla_out[p][0..1] token_list_accuracy's (correct, non-pad) counts over the first min(len) positions,
 *                    metrics.py:259-274; may be NULL
 * pred (pairs, pred_stride) / target (pairs, target_stride) int32 rows, lengths clamped to [0, max_len].
 * The float formulas on top (1 - d / max_len; precisions, geometric mean, brevity penalty) are host
 * arithmetic in float64, exactly as the reference writes them (img2latex_amd/training/metrics.py). */
int i2l_sequence_metrics(const int32_t* pred, const int32_t* pred_len, int pred_stride, const int32_t* target,
                         const int32_t* target_len, int target_stride, int pairs, int max_len, int max_n,
                         int pad_id, int32_t* lev_out, int32_t* match_out, int32_t* tla_out, i2l_stream_t stream);

/* Host helper (no GPU work): mean BLEU-n and mean Levenshtein similarity (calculate_metrics, metrics.py:184-223) from the
 * integer statistics of i2l_sequence_metrics, `pairs` rows of `stride` >= 9 int32 = [lev, match 1..4, 2 unused, gen_len,
 * true_len].  The reference's float64 formulas operation by operation (libm log / exp = CPython's math.log / math.exp):
 * bit-identical scores without 256 x 2 interpreter calls per batch. */
int i2l_scores_from_statistics(const int32_t* stats, int pairs, int stride, int n, double* bleu_mean_out,
                               double* lev_mean_out);

/* Error analysis: the edit script of every (target, prediction) pair and the token confusion matrix of a split.  The
 * rules are csrc/edit_align_rules.inc.h's.  For a target r[0, m) and a prediction p[0, n), D[i][j] is the Levenshtein table
 * of r[0, i) against p[0, j) (the recurrence of i2l_sequence_metrics' lev_out, so D[m][n] is that integer).  THE script is
 * the backtrace from (m, n) to (0, 0) that takes at (i, j) the first of: a match (i, j > 0, r[i-1] == p[j-1], D[i][j] ==
 * D[i-1][j-1]); a substitution of r[i-1] by p[j-1] (i, j > 0, D[i][j] == D[i-1][j-1] + 1); a deletion of r[i-1] (i > 0,
 * D[i][j] == D[i-1][j] + 1); an insertion of p[j-1].  It is reported in forward order, one byte per operation: 0 match,
 * 1 substitution, 2 deletion, 3 insertion.
 *   pred (pairs, pred_stride) / target (pairs, target_stride) int32 rows; lengths clamped to [0, stride] on the device
 *   ops_out         [pairs][4] int32: matches, substitutions, deletions, insertions (the last three sum to lev_out); may be NULL
 *   script_out      [pairs][pred_stride + target_stride] uint8, the first script_len_out[pair] bytes written; NULL together
 *   confusion       (vocab + 1) x (vocab + 1) uint32, ACCUMULATED into by integer atomics (the caller zeroes it once): row =
 *                   target id or `vocab` for "nothing", column = predicted id or `vocab`.  A match or substitution of a by
 *                   b adds 1 to [a][b], a deletion of a to [a][vocab], an insertion of b to [vocab][b]; an operation with
 *                   an id outside [0, vocab) is in the script and in ops_out and adds nothing.  May be NULL.
 * One launch, one wave per pair: Myers' bit-vector column pass with two vectors kept per column, in LDS while they fit
 * (pairs of up to 256 x 256 tokens), else in `scratch` (i2l_edit_alignment_scratch_bytes, 0 when none is needed; the call
 * returns I2L_ERR_WORKSPACE when scratch_bytes is smaller).  I2L_ERR_ARG: a NULL input, non-positive pairs / strides /
 * vocab, all three outputs NULL, one of script_out / script_len_out NULL.  I2L_ERR_UNSUPPORTED: a stride above 1024 (the
 * decode's step limit) or vocab > 2048.  Every refusal is decided before the first HIP call.  The library keeps no state. */
size_t i2l_edit_alignment_scratch_bytes(int pairs, int pred_stride, int target_stride);
int i2l_edit_alignment(const int32_t* pred, const int32_t* pred_len, int pred_stride, const int32_t* target,
                       const int32_t* target_len, int target_stride, int pairs, int vocab, void* scratch,
                       size_t scratch_bytes, int32_t* ops_out, uint8_t* script_out, int32_t* script_len_out,
                       uint32_t* confusion, i2l_stream_t stream);

/* Margins of a confusion matrix: row_total[vocab + 1] (occurrences of each target token, its deletions included; [vocab]:
 * all insertions), col_total[vocab + 1] (occurrences of each predicted token, its insertions included; [vocab]: all
 * deletions), diag[vocab] (matches of each token).  Each may be NULL, not all.  Deterministic: no atomics. */
int i2l_confusion_margins(const uint32_t* confusion, int vocab, uint32_t* row_total, uint32_t* col_total, uint32_t* diag,
                          i2l_stream_t stream);

/* The n <= 1024 largest non-zero cells of a confusion matrix among the kinds selected by `kinds` (an OR of the bits
 * below), in the order count descending, then row ascending, then column ascending: row_out / col_out / count_out [n],
 * *listed_out = the number listed (fewer than n when fewer cells qualify; the entries behind it are -1, -1, 0).  Two
 * launches; scratch (i2l_confusion_top_scratch_bytes) is the caller's.  I2L_ERR_ARG: NULL pointers, n <= 0, kinds without a
 * known bit or with an unknown one; I2L_ERR_UNSUPPORTED: n > 1024, vocab > 2048; I2L_ERR_WORKSPACE. */
#define I2L_CONFUSION_SUBSTITUTIONS 1   /* off the diagonal, both indices < vocab */
#define I2L_CONFUSION_DELETIONS 2       /* column `vocab`                         */
#define I2L_CONFUSION_INSERTIONS 4      /* row `vocab`                            */
#define I2L_CONFUSION_MATCHES 8         /* the diagonal                           */
#define I2L_CONFUSION_ALL 15
size_t i2l_confusion_top_scratch_bytes(int vocab);
int i2l_confusion_top(const uint32_t* confusion, int vocab, int kinds, int n, void* scratch, size_t scratch_bytes,
                      int32_t* row_out, int32_t* col_out, uint32_t* count_out, int32_t* listed_out, i2l_stream_t stream);

/* The id post-processing between the decode loop and the metrics, on the device (cli.py:466-481 with
 * predictor.py:350-358,384-391 and tokenizer.py:166-192): per row keep, in order, the ids BEFORE the first stop
 * position -- id == end_id, or id < 0 (the sticky stop rule's filler) -- that are not one of drop_ids[0..n_drop)
 * (DEVICE array of <= 8 ids: the special tokens LaTeXTokenizer.decode(skip_special_tokens=True) removes;
 * for target rows: the PAD id, with end_id = -1 so that nothing stops a row).  ids (rows, stride) int32, `width`
 * columns used; out_ids (rows, out_stride >= width); out_len (rows).  Bit-exact integer work. */
int i2l_compact_ids(const int32_t* ids, int rows, int width, int stride, int end_id, const int32_t* drop_ids,
                    int n_drop, int32_t* out_ids, int out_stride, int32_t* out_len, i2l_stream_t stream);

/* Token ids -> text on the device: LaTeXTokenizer.decode(skip_special_tokens=True) (tokenizer.py:166-192) on top of the
 * predictor's END handling (predictor.py:350-358,384-391), i.e. what Predictor.predict_batch returns per row.
 * Row rule = i2l_compact_ids': keep, in order, the ids before the first stop position (id == end_id, or id < 0; with
 * end_id = -1 only a negative id stops a row) that are not one of drop_ids[0..n_drop) (DEVICE array, <= 8); a kept id
 * outside [0, vocab) reads as unk_id.  Text rule = " ".join: token v is tok_bytes[tok_off[v] .. tok_off[v + 1]) (DEVICE
 * arrays, tok_off of vocab + 1 ascending int32; the bytes are opaque -- UTF-8 in practice), one 0x20 between consecutive
 * kept tokens, none in front of the first or behind the last; a zero-length token still takes its separators; a row with
 * nothing kept is the empty string.  Row r is out_bytes[out_off[r] .. out_off[r + 1]), packed without gaps; out_off has
 * rows + 1 int32 (the exclusive scan of the row sizes, [rows] = the total).
 * *status (device word) = 0, or 1 when the total exceeds out_capacity: out_off is complete all the same (the caller
 * learns the size needed) and no byte at or beyond out_capacity is written.
 * I2L_ERR_UNSUPPORTED before any launch: n_drop > 8; vocab <= 0; rows * width * (longest token + 1) beyond int32 (the
 * byte counts are int32).  For that bound, and to refuse offsets that do not ascend (I2L_ERR_ARG), the call READS
 * tok_off from the host with one blocking copy of vocab + 1 words: the table must be complete when it is called.
 * Three launches on `stream` (size per row, scan over the rows -- any number of them --, write); the writing pass maps
 * lanes to OUTPUT bytes, so neighbouring lanes store neighbouring bytes.  workspace: rows int32. */
size_t i2l_detokenize_workspace_bytes(int rows);
int i2l_detokenize(const int32_t* ids, int rows, int width, int stride, int end_id, const int32_t* drop_ids, int n_drop,
                   const uint8_t* tok_bytes, const int32_t* tok_off, int vocab, int unk_id, uint8_t* out_bytes,
                   int64_t out_capacity, int32_t* out_off, int32_t* status, void* workspace, size_t workspace_bytes,
                   i2l_stream_t stream);

/* Text -> token ids on the device: LaTeXTokenizer.encode / encode_batch (tokenizer.py:143-164,196-232) and the data
 * set's "START formula END" rule (dataset.py:333-335, collator :59-66).  Row r is text[row_off[r] .. row_off[r + 1])
 * (DEVICE arrays: uint8 text of text_bytes, int32 row_off of rows + 1; read on the device only -- no host
 * synchronisation, the offsets change with every batch).
 * Token rule = str.split() without an argument: tokens are the maximal runs of bytes outside every whitespace character;
 * leading / trailing whitespace, an empty row and an all-whitespace row give no token.  Whitespace is exactly the 29 code
 * points of str.isspace() -- U+0009-000D, 001C-0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000 -- matched
 * by their UTF-8 byte patterns (09-0D, 1C-20; C2 85, C2 A0; E1 9A 80; E2 80 80..8A, E2 80 A8, E2 80 A9, E2 80 AF; E2 81
 * 9F; E3 80 80) at any byte position: exact for well-formed UTF-8, which the caller promises.  Every other byte is opaque
 * token content.
 * Id rule (tokenizer.py:162) = the id of the table key whose bytes EQUAL the token's bytes, else unk_id; a hash match
 * never decides alone, and a token of any length works (one longer than the longest key is UNK without a probe).
 * Row rule (tokenizer.py:155-156,219-227): with add_special = 1, start_id first and end_id behind the last token (the
 * literal text "<START>" inside a row is an ordinary token for the table); the row is then cut to `width` (an over-long
 * row loses its END) and padded with pad_id.  out_ids (rows, out_stride >= width) int32: all `width` columns of every
 * row are written, nothing behind them; out_len (rows) = ids before the padding (<= width); out_count (rows, or NULL) =
 * the count before the cut, START and END included.
 * *status (device word, cleared by the call) = 0, or bit 0: some row was cut; bit 1: some row's offsets were unusable
 * (end < start, or outside [0, text_bytes]) -- such a row is an empty row and no byte outside `text` is ever read; bit 2:
 * the table image does not describe itself (wrong magic or sizes) -- every token is then unk_id.
 * The table is the self-contained image i2l_tokenize_table_build writes on the HOST (HOST pointers: n keys, key i =
 * tok_bytes[tok_off[i] .. tok_off[i + 1]) with id tok_id[i]; image of i2l_tokenize_table_bytes(n, tok_off[n] -
 * tok_off[0]) bytes, 0 when that is beyond int32), uploaded once per tokenizer: open addressing with linear probing over
 * a power of two of 16-byte slots (FNV-1a hash, key start, key length, id), load factor <= 1/2, the key bytes behind
 * them.  A zero-length key is accepted and can never be hit (a token has a byte); the same key twice is I2L_ERR_ARG, a
 * too-small image I2L_ERR_WORKSPACE.
 * I2L_ERR_UNSUPPORTED before any launch: width <= 0; out_stride < width; text_bytes beyond int32.  rows == 0 is I2L_OK
 * with no launch.  Otherwise one memset of *status and ONE kernel on `stream`: a wave per row, lane = byte (neighbouring
 * lanes read neighbouring bytes), 64 bytes at a time with the whitespace state, the last two pattern lengths and the
 * token count carried from chunk to chunk (rows of any length); the lane of a token's first byte hashes, probes and
 * compares.  No workspace. */
size_t i2l_tokenize_table_bytes(int n, int64_t key_bytes);
int i2l_tokenize_table_build(const uint8_t* tok_bytes, const int32_t* tok_off, const int32_t* tok_id, int n, void* image,
                             size_t image_bytes);
int i2l_tokenize(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows, const void* table,
                 size_t table_bytes, int unk_id, int pad_id, int start_id, int end_id, int add_special, int width,
                 int32_t* out_ids, int out_stride, int32_t* out_len, int32_t* out_count, int32_t* status,
                 i2l_stream_t stream);

/* Text -> ragged token ids (CSR) on the device: a whole corpus tokenized once, e.g. a data set's formulas file.  Inputs,
 * token rule, id rule and add_special are i2l_tokenize's (DEVICE text / row_off, the table image, the special ids); the
 * difference is the row rule: a row is never cut and never padded.  Row r is out_ids[out_off[r] .. out_off[r + 1]),
 * packed without gaps; with add_special = 1 it is start_id, the row's tokens, end_id (an empty row: those two).
 * out_off has rows + 1 **int64** entries (the exclusive scan of the row counts, [rows] = the total): the rows of a text
 * of up to 2^31 - 1 bytes hold up to 2^30 tokens plus two per row, so the total needs no int32 refusal.
 * *status (device word, cleared by the call) = 0, or I2L_TOKENIZE_PACKED_OVERFLOW (bit 0): the total exceeds
 * out_capacity (ids) -- out_off is complete all the same (the caller learns the size needed) and no id at or beyond
 * out_capacity is written; bits 1 and 2 are i2l_tokenize's: some row's offsets were unusable (it reads as an empty row),
 * the table image does not describe itself (every token is unk_id).
 * I2L_ERR_UNSUPPORTED before any launch: text_bytes beyond int32; rows > 2^31 - 1025.  rows == 0: only the scan runs
 * (out_off[0] = 0).  Otherwise three launches on `stream`, no host wait: count per row (a wave per row, lane = byte,
 * i2l_tokenize's chunk scan without a look-up), scan (one workgroup, chunks of 1024 rows with a running carry: any
 * number of rows), write (i2l_tokenize's row body: chunk scan, walk, probe, compare).  workspace: rows int32. */
#define I2L_TOKENIZE_PACKED_OVERFLOW 1
size_t i2l_tokenize_packed_workspace_bytes(int rows);
int i2l_tokenize_packed(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows, const void* table,
                        size_t table_bytes, int unk_id, int start_id, int end_id, int add_special, int32_t* out_ids,
                        int64_t out_capacity, int64_t* out_off, int32_t* status, void* workspace, size_t workspace_bytes,
                        i2l_stream_t stream);

/* Im2LatexCollator (dataset.py:59-66) from the CSR store i2l_tokenize_packed wrote: ids (n_ids int32) and off
 * (rows + 1 int64), DEVICE arrays.  index: B int64 store rows (DEVICE; repeats allowed).  Row b of out (B, out_stride >=
 * width) int32 is store row index[b] followed by pad_id up to `width`; columns behind `width` are not written.
 * *status (device word, cleared by the call) = 0, or I2L_COLLATE_ROW_TOO_LONG (bit 0): a store row is longer than
 * `width`; I2L_COLLATE_BAD_INDEX (bit 1): an index outside [0, rows), or offsets that do not lie inside [0, n_ids].
 * Such a row is written as pad_id only and no store word outside a row is read.
 * I2L_ERR_UNSUPPORTED: width <= 0, out_stride < width.  B == 0 is I2L_OK with no launch.  Otherwise one memset and ONE
 * launch on `stream`: a wave per row, lane = column (neighbouring lanes write neighbouring columns). */
#define I2L_COLLATE_ROW_TOO_LONG 1
#define I2L_COLLATE_BAD_INDEX 2
int i2l_collate_ids(const int32_t* ids, int64_t n_ids, const int64_t* off, int64_t rows, const int64_t* index, int B, int width,
                    int pad_id, int32_t* out, int out_stride, int32_t* status, i2l_stream_t stream);

/* n byte ranges of a resident buffer -> a compact batch buffer: range i is src[src_off[i] .. src_off[i] + size[i]) and
 * goes to dst[dst_off[i] ..) (int64 DEVICE arrays; the destinations must not overlap each other or src).  A size of 0 is
 * legal; any source and any destination alignment works.  src_bytes / dst_bytes are the buffers' sizes: a range that
 * leaves either (or a negative size / offset) is not copied and sets *status (device word, cleared by the call) to 1.
 * max_size = the largest size[i] (it sizes the grid: 16 KB tiles, several workgroups per large range; a range beyond it
 * is still copied whole).  Lanes map to consecutive groups of 16 destination bytes, stored with aligned 16-byte stores;
 * the source is one 16-byte load when its alignment agrees, else aligned words shifted together; the < 16 bytes at
 * either end, and the groups at a range's ends whose words would reach outside it, go byte by byte -- no byte outside a
 * source range is read, none outside a destination range written.
 * I2L_ERR_UNSUPPORTED: n > 65535.  n == 0 is I2L_OK with no launch.  Otherwise one memset and ONE launch on `stream`. */
int i2l_gather_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* size, int n,
                         int64_t max_size, uint8_t* dst, int64_t dst_bytes, const int64_t* dst_off, int32_t* status,
                         i2l_stream_t stream);

/* PNG pages decoded on the device: inflate (RFC 1950 / 1951), unfilter (PNG 9.2, types 0 .. 4) and conversion to the page
 * PIL hands the data set (data/dataset.py decode_page), n images in ONE launch, a wave per image.  The container is
 * parsed on the host (data/png.py): `z` (DEVICE, z_bytes) holds the images' concatenated IDAT payloads -- their zlib
 * streams, undecompressed -- and the PLTE bytes of palette images.  8-bit, non-interlaced images only.
 * NOTE, unlike the other batch entry points (i2l_gather_ragged_u8 takes DEVICE lists): `images` is a HOST array of n
 * descriptors.  The streams are untrusted, so every descriptor is checked against the buffers BEFORE anything is
 * launched, and that needs them on the host; the call then copies them into the workspace itself.  The copy is from
 * pageable memory and therefore SYNCHRONOUS: the call blocks the host until `stream` has reached and performed it
 * (it waits on the stream before it launches), after which the caller's array may be freed or reused.  Not for use
 * inside a stream capture.
 *   colour_type 0 (gray):        channels must be 1, the page is (h, w, 1)
 *   colour_type 2 (RGB):         channels must be 3, the page is (h, w, 3)
 *   colour_type 4 (gray+alpha):  channels 1: gray; 3: gray three times; alpha dropped
 *   colour_type 6 (RGBA):        channels 1: L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 (Pillow); 3: RGB; alpha dropped
 *   colour_type 3 (palette):     PLTE look-up (pal_n entries of 3 bytes at z + pal_off), then as RGBA without alpha
 * The page of image i is written interleaved at pixels + out_off; the pages must not overlap.  status[i] (DEVICE, n
 * int32) = 0 or an I2L_PNG_E_* code: the stream must have a valid zlib header (CM 8, window <= 32 K, no dictionary),
 * consist of stored / fixed / dynamic blocks up to a final one, inflate to exactly height * (1 + width * bpp) bytes with
 * every match inside the output so far, carry the right Adler-32 and end with it; every filter byte must be <= 4 and
 * every palette index below pal_n.  An image with a non-zero status leaves an undefined page of ITS OWN; no byte outside
 * the n pages is written, no byte outside an image's own stream (and palette) is read, whatever the streams hold.
 * I2L_ERR_ARG before any launch: a descriptor that does not fit (unknown colour type, channels, a stream, palette or page
 * outside its buffer, overlapping pages, width or height < 1), a missing pointer, a workspace not 16-byte aligned;
 * I2L_ERR_UNSUPPORTED: an image of more than 2^27 filtered bytes, n > 2^20; I2L_ERR_WORKSPACE.  n == 0 is I2L_OK with
 * no launch.  Otherwise two small synchronous copies (above) and ONE launch on `stream`; no state is kept.
 * workspace: i2l_png_decode_workspace_bytes(n, the sum over the images of height * (1 + width * bpp)). */
typedef struct i2l_png_image {
    int64_t z_off, z_len;     /* the zlib stream within z */
    int64_t pal_off;          /* PLTE bytes within z, -1: none */
    int64_t out_off;          /* the page within pixels */
    int32_t width, height, colour_type;
    int32_t pal_n;            /* palette entries (colour type 3: 1 .. 256) */
    int32_t channels;         /* of the page: 1 or 3 */
    int32_t reserved;
} i2l_png_image;
#define I2L_PNG_E_HEADER 1
#define I2L_PNG_E_TRUNCATED 2
#define I2L_PNG_E_BLOCK_TYPE 3
#define I2L_PNG_E_STORED_LEN 4
#define I2L_PNG_E_CODE_LENGTHS 5
#define I2L_PNG_E_SYMBOL 6
#define I2L_PNG_E_DISTANCE 7
#define I2L_PNG_E_TOO_MANY 8
#define I2L_PNG_E_TOO_FEW 9
#define I2L_PNG_E_TRAILING 10
#define I2L_PNG_E_ADLER 11
#define I2L_PNG_E_FILTER 12
#define I2L_PNG_E_PALETTE 13
size_t i2l_png_decode_workspace_bytes(int n, int64_t filtered_bytes_total);
int i2l_png_decode(const uint8_t* z, int64_t z_bytes, const i2l_png_image* images, int n, uint8_t* pixels,
                   int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes, i2l_stream_t stream);

/* Text -> the fitted vocabulary on the device: LaTeXTokenizer.fit (tokenizer.py:80-117).  text / row_off / rows and the
 * token rule are i2l_tokenize's (DEVICE arrays, str.split() per row; a row boundary separates tokens).  Every distinct
 * token is counted; the tokens are ordered by count descending, ties by first occurrence in the corpus (the smallest
 * byte offset into `text` of any occurrence: Counter's insertion order under a stable sort), so the order is unique and
 * does not depend on scheduling.  A token whose bytes equal one of the n_skip skip strings (HOST pointers: string i =
 * skip_bytes[skip_off[i] .. skip_off[i + 1]), at most 8 strings and 256 bytes together -- the special tokens, which
 * keep their ids) is counted and not emitted.
 * Outputs (DEVICE), in rank order r = 0 .. emitted - 1: token r = out_bytes[out_off[r] .. out_off[r + 1]) packed without
 * gaps (out_off: out_capacity + 1 int32), out_count[r], out_first[r] (its first byte offset in `text`); out_capacity
 * tokens and out_byte_capacity bytes at most, nothing is written beyond either.
 * meta (DEVICE, I2L_VOCAB_FIT_META_WORDS int32, all written by the call): [0] distinct tokens to emit, [1] distinct
 * tokens skipped, [2] tokens in total, [3] the largest token count of a row, [4] bytes the emitted tokens need,
 * [5] status, [6..7] 0, [8 + i] the count of skip string i (0 when it does not occur).
 * status bits: I2L_VOCAB_FIT_FULL -- more than slots / 2 distinct tokens, or a probe found no slot: the results are not to
 * be used, call again with more slots; I2L_VOCAB_FIT_BAD_OFFSETS -- i2l_tokenize's rule, the row reads as empty;
 * I2L_VOCAB_FIT_OUT_TOO_SMALL -- [0] > out_capacity or [4] > out_byte_capacity (both still say what is needed).
 * slots: a power of two in [2, 2^28], the open-addressing table in the workspace (24 bytes per slot;
 * i2l_vocab_fit_workspace_bytes is pure host code and returns 0 for rows < 0 or unusable slots).  The workspace
 * (8-byte aligned) is cleared on `stream` by the call itself; the library keeps no state between calls.
 * flags: 0, or I2L_VOCAB_FIT_NO_AGGREGATE -- count with one global atomic per token instead of gathering per workgroup
 * in LDS first (same results; kept for the ablation in profiles/vocab_fit_cost.py).
 * I2L_ERR_UNSUPPORTED before any launch: text_bytes beyond int32, n_skip > 8, more than 256 skip bytes; I2L_ERR_ARG: a
 * negative size, slots no power of two, unknown flags, a missing pointer, descending skip offsets; I2L_ERR_WORKSPACE.
 * Launches on `stream`, no host synchronisation: count (a wave per row, lane = byte; find-or-claim by ONE 64-bit
 * compare-and-swap of (offset << 32 | length) of a representative occurrence, nothing waits), compact, bitonic sort by
 * (~count << 32 | first offset), offsets + meta, emit. */
#define I2L_VOCAB_FIT_META_WORDS 16
#define I2L_VOCAB_FIT_FULL 1
#define I2L_VOCAB_FIT_BAD_OFFSETS 2
#define I2L_VOCAB_FIT_OUT_TOO_SMALL 4
#define I2L_VOCAB_FIT_NO_AGGREGATE 1
size_t i2l_vocab_fit_workspace_bytes(int rows, int64_t slots);
int i2l_vocab_fit(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows, const uint8_t* skip_bytes,
                  const int32_t* skip_off, int n_skip, int64_t slots, int flags, uint8_t* out_bytes,
                  int64_t out_byte_capacity, int32_t* out_off, int32_t* out_count, int32_t* out_first, int out_capacity,
                  int32_t* meta, void* workspace, size_t workspace_bytes, i2l_stream_t stream);

/* masked_accuracy, metrics.py:226-238 (trainer.py:391,526): over rows = B*T logits rows of `vocab` floats,
 * correct_total_out[0] = #(argmax == target and target != pad), [1] = #(target != pad); first index wins
 * ties.  The (B,T,V) logits never leave the device (the reference copies them to the host every step). */
int i2l_masked_accuracy(const float* logits, const int64_t* targets, int64_t rows, int vocab, int64_t pad_id,
                        uint64_t* correct_total_out, i2l_stream_t stream);

/* The per-batch statistics of Trainer.validate (trainer.py:510-559) from the teacher-forced logits in ONE read of them:
 * logits (batch, steps, vocab) fp32 contiguous, targets (batch, steps) int32 = formulas[:, 1:].  Per (b,t) row the
 * label-smoothed CE term of nn.CrossEntropyLoss(ignore_index=pad, label_smoothing) (:111-115,521-523; the formula of
 * i2l_ce_label_smooth_fwd_bwd, 0 where target == pad) and torch.argmax's first-index arg max (:541; NaN counts as the
 * largest value); a non-pad target outside [0, vocab) is clamped into it for the loss, as i2l_ce_label_smooth_fwd_bwd
 * does.  Written, not accumulated (so a caller can aim them at slot i of a per-epoch record):
 *   loss_sum_count_out[2]   fp32 [SUM over non-pad rows of the row loss, number of non-pad rows] -- the convention of
 *                           i2l_ce_label_smooth_fwd_bwd: the batch's loss.item() is [0] / [1]; fixed-order double sum
 *   correct_total_out[2]    int64 [#(argmax == target != pad), #(target != pad)]: masked_accuracy, :524-526
 *   argmax_out (batch, steps) int32 or NULL
 *   pred_len_out (batch)    first t with argmax == pad, else steps (:547-553); NULL = not wanted
 *   target_len_out (batch)  first t with target == pad, else steps (:555-559); NULL = not wanted
 * Two launches (a wave per row; one finishing workgroup), no atomics: bit-identical results run to run.  Rows of
 * vocab <= 2048 are held in registers (exact two-pass max / sum exp / sum x); 16-byte loads when vocab % 4 == 0 and
 * logits is 16-byte aligned.  The workspace (i2l_teacher_forced_eval_workspace_bytes) is the caller's.  I2L_ERR_ARG for
 * batch or steps < 0, vocab < 1, label_smoothing outside [0, 1) or a missing pointer; I2L_ERR_WORKSPACE when it is too
 * small.  batch * steps == 0 writes zero counts. */
size_t i2l_teacher_forced_eval_workspace_bytes(int batch, int steps);
int i2l_teacher_forced_eval(const float* logits, const int32_t* targets, int batch, int steps, int vocab, int pad_id,
                            float label_smoothing, void* workspace, size_t workspace_bytes, int32_t* argmax_out,
                            int32_t* pred_len_out, int32_t* target_len_out, float* loss_sum_count_out,
                            int64_t* correct_total_out, i2l_stream_t stream);

/* Where the grouped greedy kernel's status words live inside the decoder workspace (0: these dimensions have no
 * grouped path): uint32 [0] != 0 -> a poll timed out (the ids are -3), [1] groups that completed the placement
 * exchange in the last launch, [2] of those, the groups whose four workgroups measured themselves on ONE XCD and
 * therefore exchanged through that XCD's L2 (the fast flavour).  Diagnostics: read after synchronising the stream. */
size_t i2l_decoder_group_status_offset(int rows, int vocab, int embed, int hidden, int layers);
size_t i2l_decoder_group_region_bytes(int rows, int vocab, int embed, int hidden, int layers);   /* bytes of that region (status + exchange granules) */

/* TWO batches in one 16-member grouped launch, a range of the steps of each (GreedyPipeline's split decode): the rows of
 * both are row tiles of the same matrix-core operands and share the launch's per-step exchanges, so a launch of n steps
 * advances two batches by n steps for much less than two launches would take.  A batch is decoded by two such calls on
 * one stream: steps [0, n) -- which leaves the LSTM state, the last token and the stop mask of every row in a state block
 * inside the batch's workspace (i2l_decoder_group_state_offset / _bytes) -- then steps [n, steps), which resumes from it;
 * the ids of a batch are bit-equal to i2l_greedy_decode_ex with I2L_FLAG_DECODE_GROUP16 however its steps are cut and
 * whatever batch sits in the other tile.
 *   workspace    of i2l_decoder_prepare() for this batch's `rows` (Genc, state block); alive and unchanged until the
 *                call that runs the batch's last steps has completed
 *   rows, steps  of the whole batch; ids_out is (rows, steps) int32, the call writes columns first_step .. + n_steps - 1
 *   first_step, n_steps   the range run by this call; n_steps == 0: as if the half were absent
 *   tok0         (rows) int32 first input tokens (read when first_step == 0)
 * `older` / `newer`: either may be NULL (a launch with one tile: the first or the last of a sequence).  The weights, the
 * status words and the exchange region are those of `newer`'s workspace (of `older`'s when newer is absent): both batches
 * must belong to the SAME weights, which the caller guarantees, and that region must be large enough for the groups of
 * both (I2L_ERR_UNSUPPORTED otherwise: equal row counts always are).  temperature, select (I2L_SELECT_LOGITS / _SOFTMAX),
 * end_id, flags (I2L_FLAG_AGENT_SCOPE_EXCHANGE, I2L_FLAG_DECODE_REGION_CLEARED, the test hooks) and the residency signal:
 * as i2l_greedy_decode_ex.  Supported where that entry runs the 16-member kernel (layers 1, hidden 256, vocab <= 512)
 * and only with stop == I2L_STOP_NONE -- under a sticky stop a range of steps has no fixed length --; everything else
 * returns I2L_ERR_UNSUPPORTED before anything is enqueued and callers keep i2l_greedy_decode_ex.  If a bounded wait
 * expires, every id of the affected rows of BOTH batches is -3; a batch whose first range failed gets -3 from the call
 * that was to resume it, which then runs the other batch alone. */
typedef struct {
    const void* workspace;
    int rows, steps;
    int first_step, n_steps;
    const int32_t* tok0;
    int32_t* ids_out;
} i2l_decode_half;
int i2l_greedy_decode_halves(const i2l_decoder_weights* w, const i2l_decode_half* older, const i2l_decode_half* newer,
                             float temperature, int select, int stop, int end_id, int flags,
                             uint32_t* resident_flag, uint32_t resident_value, i2l_stream_t stream);
/* The state block of i2l_greedy_decode_halves inside the decoder workspace (bytes 0: these dimensions have no such launch). */
size_t i2l_decoder_group_state_offset(int rows, int vocab, int embed, int hidden, int layers);
size_t i2l_decoder_group_state_bytes(int rows, int vocab, int embed, int hidden, int layers);

/* ------------------------------------------------------------------------
 * Image preprocessing (reference img2latex/data/utils.py:18-90, data/transforms.py:26-56), SURVEY section 8(f)-3
 * ---------------------------------------------------------------------- */

/* Host helpers (no GPU work): Pillow's LANCZOS coefficient tables for resampling `in_size` source samples to
 * `out_size` (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc over the full source range, double
 * precision, libm sin): bounds_out (out_size, 2) = first source sample and count, kk_out (out_size, ksize) = 22-bit
 * fixed-point weights, ksize = i2l_lanczos_ksize(in_size, out_size). */
int i2l_lanczos_ksize(int in_size, int out_size);
int i2l_lanczos_coeffs(int in_size, int out_size, int32_t* bounds_out, int32_t* kk_out);
/* The same tables for a named Pillow filter (values of PIL.Image.Resampling): LANCZOS is what load_image asks for
 * (transforms.py:20-24), BICUBIC what Image.resize() defaults to -- the PIL.Image branch of Predictor._prepare_image
 * (predictor.py:432-439) resizes straight to (800, 64) with it, aspect ratio NOT kept. */
#define I2L_FILTER_LANCZOS 1
#define I2L_FILTER_BICUBIC 3
int i2l_resample_ksize(int filter, int in_size, int out_size);
int i2l_resample_coeffs(int filter, int in_size, int out_size, int32_t* bounds_out, int32_t* kk_out);
/* n tables at once on up to `threads` host threads: entry i (in_sizes[i] -> out_sizes[i]) is written at out +
 * offsets[i] as bounds (out, 2) followed by weights (out, ksize).  No global state: the threads live for the call. */
int i2l_resample_coeffs_batch(int filter, int n, const int32_t* in_sizes, const int32_t* out_sizes,
                              const int64_t* offsets, int32_t* out, int threads);

/* The same tables built ON THE DEVICE for n resamplings at once (in_sizes / out_sizes / offsets are DEVICE arrays; entry i
 * is written at tables + offsets[i] as i2l_resample_coeffs_batch lays it out; max_out_size = the largest out_sizes[i]):
 * the host function's double-precision arithmetic repeated operation by operation, with the device's sin() in place of
 * libm's -- both faithfully rounded, so a 22-bit weight can differ by one unit where the normalised value sits within
 * ~1e-16 of a rounding boundary (about once in 1e9 weights).  i2l_resample_coeffs stays the Pillow-identical reference.
 * A batch of ragged pages then uploads nothing but its pixels, sizes and plans (the host-side tables cost
 * more than the device chain). */
int i2l_resample_coeffs_device(int filter, int n, const int32_t* in_sizes, const int32_t* out_sizes, const int64_t* offsets,
                               int32_t* tables, int max_out_size, i2l_stream_t stream);
/* Host helper (no GPU work): copies n host buffers srcs[i] (sizes[i] bytes) to dst + offsets[i] on up to `threads` host
 * threads that live for the call -- the separate page arrays PIL hands the reference's load_image, gathered into the
 * one pinned block that is uploaded. */
int i2l_pack_host(const void* const* srcs, const int64_t* sizes, const int64_t* offsets, int n, void* dst, int threads);

/* One image of a ragged batch.  Offsets index `pixels` (bytes), `tables` (int32 elements) and the workspace
 * (bytes).  Bounds are ABSOLUTE source indices as i2l_resample_coeffs writes them; when need_h the kernel itself
 * subtracts ybox_first from the vertical ones (Resample.c: "Shift bounds for vertical pass"), so one table serves
 * every image of the same (source size, target size). */
typedef struct i2l_resize_plan {
    int64_t src_offset;            /* first byte of the uint8 image: (src_h, src_w) or (src_h, src_w, 3) interleaved */
    int64_t tmp_offset;            /* intermediate image (tmp_rows, new_w, out_c) uint8 in the workspace             */
    int64_t bh_offset, kh_offset;  /* horizontal bounds / weights                                                    */
    int64_t bv_offset, kv_offset;  /* vertical bounds / weights                                                      */
    int32_t src_h, src_w, src_c;
    int32_t new_w;                 /* int(round(out_h * src_w / src_h)), transforms.py:33-36; = out_w for a plain resize */
    int32_t ybox_first, tmp_rows;  /* source rows the vertical pass needs                                            */
    int32_t need_h, need_v;        /* new_w != src_w, out_h != src_h                                                 */
    int32_t kh_ksize, kv_ksize;
} i2l_resize_plan;

/* load_image for n decoded images: convert("L"/"RGB") -> LANCZOS resize to (new_w, out_h) -> right-pad (white for
 * 1 channel; Pillow's integer colour 255 = (255,0,0) for 3 channels, as the reference executes) or centre-crop to
 * out_w -> /255 -> [-1,1] (1 channel) or ImageNet mean/std (3 channels) when `normalize`.  out (n, out_c, out_h,
 * out_w) fp32, bit-identical to the reference's tensor.  plans / tables live in device memory; max_tmp_px = the
 * largest tmp_rows*new_w over the batch (0 when no image needs a horizontal pass).  normalize: 0 = /255 only,
 * 1 = load_image's rule above, 2 = x * 2 - 1 on every channel (the PIL.Image branch of Predictor._prepare_image,
 * predictor.py:447-451).  The filter is whatever the plan's tables were built with. */
int i2l_preprocess_images(const uint8_t* pixels, const i2l_resize_plan* plans, const int32_t* tables, int n,
                          int max_tmp_px, int out_c, int out_h, int out_w, int normalize, void* workspace,
                          float* out, i2l_stream_t stream);

/* The tensor branch of Predictor._prepare_image (predictor.py:483-491): torch.nn.functional.interpolate(mode=
 * "bilinear", align_corners=False) of `planes` fp32 images (in_h, in_w) -> (out_h, out_w), contiguous.  The source
 * coordinate max(0, (float)in / out * (dst + 0.5) - 0.5) is one fused multiply-add in fp32, as ATen compiles it; results
 * within 1e-6 x max |in| of ATen's fp32 CPU result (tested; measured 1.2e-7 over up- and down-scaling shapes) and within
 * 8 x 2^-24 x max |the four neighbours| of the float64 blend at those coordinates. */
int i2l_resize_bilinear_f32(const float* in, float* out, int64_t planes, int in_h, int in_w, int out_h, int out_w,
                            i2l_stream_t stream);

/* ------------------------------------------------------------------------
 * Train-time augmentation (reference img2latex/data/dataset.py:486-492: RandomRotation(degrees=5, fill=(255,)) then
 * RandomAffine(degrees=0, translate=(0.02, 0.02), fill=(255,)) on the decoded page, before load_image's chain)
 * ---------------------------------------------------------------------- */

/* One image's warp.  On PIL images both transforms resample NEAREST and end in two Pillow calls,
 *     rot = page.rotate(angle, NEAREST, expand=False, center=None, fillcolor=white)
 *     out = rot.transform(rot.size, AFFINE, (1, 0, -tx, 0, 1, -ty), NEAREST, fillcolor=white)
 * with white = 255 on every band, angle uniform in [-degrees, degrees], tx = int(round(u)) for u uniform in
 * [-translate[0]*W, translate[0]*W] and ty likewise from translate[1]*H.  Pillow's nearest affine is 16.16 fixed point
 * (libImaging/Geometry.c): with FIX(v) = floor(v*65536 + 0.5) and Image.rotate's matrix m (PIL/Image.py; doubles:
 * a = -radians(angle % 360), m = [round(cos a, 15), round(sin a, 15), 0, round(-sin a, 15), round(cos a, 15), 0],
 * (m2, m5) = m applied to (-W/2, -H/2), m2 += W/2, m5 += H/2),
 *     a0, a1, a3, a4 = FIX(m0), FIX(m1), FIX(m3), FIX(m4);  a2 = FIX(m2 + m0*0.5 + m1*0.5);  a5 = FIX(m5 + m3*0.5 + m4*0.5)
 * and output pixel (x, y) is source pixel (yin, xin), xin = (a2 + a0*x + a1*y) >> 16, yin = (a5 + a3*x + a4*y) >> 16
 * (arithmetic shift), when 0 <= xin < W and 0 <= yin < H, else the fill.  The shift pass reduces to (x - tx, y - ty)
 * exactly, so both passes are ONE gather per output pixel: x' = x - tx, y' = y - ty; the fill if (x', y') is off the
 * page; otherwise the rotation look-up at (x', y'), which may itself give the fill.  angle 0 is the identity
 * (a = {65536, 0, 32768, 0, 65536, 32768}); Pillow's transpose shortcuts for 90 / 180 / 270 are not reproduced.  The
 * coefficients come from the host (Python doubles, data/augment.py); the device sums the indices in 64 bits. */
typedef struct i2l_affine_params {
    int32_t a0, a1, a2, a3, a4, a5;    /* 16.16 fixed point, as above */
    int32_t tx, ty;                    /* shift in whole pixels       */
} i2l_affine_params;

/* The warp of a ragged batch of interleaved uint8 pages in ONE launch: page i is the (src_h, src_w, src_c) image at
 * pixels + plans[i].src_offset (src_c 1 or 3; the layout i2l_preprocess_images reads, and only those four fields of the
 * plan are read), warped by params[i] with fill 255 into out + plans[i].src_offset.  Bytes of `out` outside the pages are
 * not written, so the same plans and tables then run unchanged on `out`.  plans and params are DEVICE arrays; out must
 * not alias pixels.  max_side = the largest src_h / src_w of the batch, max_page_bytes = the largest src_h*src_w*src_c
 * (it sizes the grid).  I2L_ERR_UNSUPPORTED before any launch for max_side > 16384; a page of the batch beyond that
 * (a wrong max_side) is left unwritten. */
int i2l_affine_nearest_u8(const uint8_t* pixels, uint8_t* out, const i2l_resize_plan* plans,
                          const i2l_affine_params* params, int n, int max_side, int64_t max_page_bytes,
                          i2l_stream_t stream);

/* The same gather on a dense (n, c, h, w) fp32 batch (what the reference's data loaders yield: pages already through
 * load_image): image i warped by params[i] (DEVICE array), every channel alike, fill[ch] (HOST array of c values, read
 * during the call) where the look-up leaves the page.  A gather: the values are copied, no arithmetic touches them.
 * I2L_ERR_UNSUPPORTED before any launch for c > 4 or a side above 16384. */
int i2l_affine_nearest_f32(const float* x, float* out, const i2l_affine_params* params, const float* fill, int n,
                           int c, int h, int w, i2l_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IMG2LATEX_HIP_H */
