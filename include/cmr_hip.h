/* libcmr_hip.so -- C ABI of the MI355X (gfx950) kernels behind CMR-Agent's hot path.
 *
 * The reference (y2w-oc/CMR-Agent) has NO FFI: its hot path is PyTorch op sequences inside
 * models/*.py and environment/environment.py plus the third-party torch_scatter extension.  Each
 * entry point below therefore cites the reference op sequence (file:line) it replaces; the
 * Python host layer (cmr_agent_amd/models, cmr_agent_amd/environment) keeps the reference's
 * nn.Module / function API on top of these calls (see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - every function returns 0 (CMR_OK), -1 (bad argument) or -2 (launch failure); none throws,
 *     allocates or synchronises; all work is enqueued on `stream` (graph-capturable);
 *   - the caller owns every buffer, including workspaces (sizes from the *_workspace_bytes helpers);
 *   - tensors are fp32, row-major "channels-last": images [B,H,W,C], point/token sets [B*L, C];
 *     `ld*` arguments are row strides in floats; float4-accessed buffers must be 16-byte aligned;
 *   - index tensors handed over by the reference API are int64; internal row ids are int32 GLOBAL
 *     row numbers (batch offset already added, cmr_index_to_global_i32).
 */
#ifndef CMR_HIP_H
#define CMR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define CMR_OK 0
#define CMR_EINVAL -1
#define CMR_ELAUNCH -2
#define CMR_EUNSUPPORTED -3

enum { CMR_ACT_NONE = 0, CMR_ACT_RELU = 1, CMR_ACT_LRELU = 2, CMR_ACT_GELU = 3, CMR_ACT_ELU1 = 4 };

/* ---- dense contractions (fp32 MFMA) -------------------------------------------------------- */

/* Y[r,:n_out] = act([X1[r,:k1] | X2[map(r),:k2]] W^T + bias + RES[r % res_mod]),  W = [n_out][k1+k2].
 * map(r) = idx2[r] if idx2 else r / div2.  Replaces nn.Linear / Conv1d(k=1) / Conv2d(k=1) (+ folded
 * BatchNorm, + activation, + residual) and the cat/gather feeding them: PointNN.py:96-123,149-156,
 * 209-226,260-282; PointViT.py:66-73; ImageViT.py:81-133; IMGPCEncoder.py:36-102;
 * LinearAttention.py:46-48,63,68; IMGPCEnDecoder.py:77-81; MultiHeadModel.py:34-39,61-67,126-131,
 * 227-233; CMRAgent.py:57-59,70-86,92-101. */
int cmr_linear_f32(const float* x1, int64_t ld1, int k1, const float* x2, int64_t ld2, int k2, const int32_t* idx2,
                   int64_t div2, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres,
                   int64_t res_mod, float* y, int64_t ldy, int64_t rows, int n_out, int act, float act_param,
                   hipStream_t stream);
/* Whole ConvBNReLURes1D block in one kernel (PointNN.py:260-282 with BN folded):
 *   hid = lrelu(W1 x + b1);  y = lrelu(W2 hid + b2 + (Wsc x | x)),  x = [x1[:, :k1] | x2[map][:, :kx-k1]].
 * The hidden activations stay in MFMA accumulator registers (transposed GEMM: accumulators of layer 1 are the
 * B-operand fragments of layer 2).  b1 / b2 may be per-batch rows (stride > 0: the broadcast global max-pool
 * concatenation of CMRAgent.py:95-99 folded into the bias); colmax_part receives per-32-row-tile channel maxima
 * of y (CMRAgent.py:95) and is reduced by cmr_colmax_partials_f32.  (kx, ch, co, shortcut) must be one of the
 * instantiated shapes, otherwise CMR_EUNSUPPORTED is returned and the caller composes cmr_linear_f32 calls. */
int cmr_cbr_block_f32(const float* x1, int64_t ld1, int k1, const float* x2, int64_t ld2, const int32_t* idx2,
                      int64_t div2, int kx, int ch, int co, const float* w1, const float* b1, int64_t b1_stride,
                      const float* w2, const float* b2, int64_t b2_stride, const float* wsc, float* y, int64_t ldy,
                      float* colmax_part, int64_t rows, int64_t rows_per_batch, float slope, hipStream_t stream);
/* bf16 matrix-core variant of the same block (same arguments, fp32 rows / weights / biases; operands rounded to bf16 on their
 * way into v_mfma_f32_32x32x16_bf16, fp32 accumulation; the hidden activations go from the accumulator registers of the first
 * GEMM straight into the second as its bf16 operand).  Enabled by cmr_agent_amd.ops.CONV_BF16 (BASELINE configs[2] / [3]). */
int cmr_cbr_block_bf16_f32(const float* x1, int64_t ld1, int k1, const float* x2, int64_t ld2, const int32_t* idx2,
                           int64_t div2, int kx, int ch, int co, const float* w1, const float* b1, int64_t b1_stride,
                           const float* w2, const float* b2, int64_t b2_stride, const float* wsc, float* y, int64_t ldy,
                           float* colmax_part, int64_t rows, int64_t rows_per_batch, float slope, hipStream_t stream);
int cmr_colmax_partials_f32(const float* part, float* out, int B, int tiles_per_batch, int C, hipStream_t stream);
/* The glue between two ConvBNReLURes1D blocks of the agent's 3-D branch in one launch (CMRAgent.py:92-101: cat([feat, max over the points])
 * in front of every block after the first): g [B][64] = column maxima of the block kernel's per-tile maxima (as cmr_colmax_partials_f32; g
 * optional), y1 [B][n1] = g w1^T + b1 and y2 [B][n2] = g w2^T + b2 -- the broadcast half of the next block's input folded into its per-sample
 * biases (w1 [n1][64], w2 [n2][64] contiguous; 64-term fp32 sums in the lane order of the skinny cmr_linear_f32 path: the same maxima, products
 * within a unit or two in the last place of the three launches it replaces).  C = 64, n1 % 4 == 0, n2 % 4 == 0; CMR_EUNSUPPORTED (-3) otherwise. */
int cmr_colmax_bias2_f32(const float* part, int B, int tiles_per_batch, int C, const float* w1, const float* b1, int n1, const float* w2,
                         const float* b2, int n2, float* g, float* y1, float* y2, hipStream_t stream);

/* y = LayerNorm_64(x) * gamma + beta (+ res).  ImageViT.py:139-140, IMGPCEncoder.py:86-87 (eps 1e-6),
 * LinearAttention.py:33-34,64,69,71 (eps 1e-5, residual x + norm2(.)). */
int cmr_layernorm64_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, const float* res,
                        int64_t ldres, float* y, int64_t ldy, int64_t rows, hipStream_t stream);

/* 3x3 convolution, pad 1, stride 1|2, NHWC, w = [9][Cout][Cin] (BN folded), y = lrelu(conv + bias + res) + post.
 * ImageResNet.py:9-14,24-36 (ResidualBlock convs + strided shortcut), IMGPCEnDecoder.py:90-94 (post = 2-D
 * sine table, utils/positional_embedding_2d.py:35-40), MultiHeadModel.py:70-72,236-238, CMRAgent.py:34-56.
 * pool = 2 fuses the following AvgPool2d(2,2) (CMRAgent.py:39,45,51; y is then [B,Ho/2,Wo/2,Cout]); returns
 * CMR_EUNSUPPORTED (-3) for maps too small for the tiled kernel: the caller then pools with cmr_avgpool_nhwc_f32. */
int cmr_conv3x3_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias,
                         const float* res, const float* post, float* y, int Cout, int stride, float slope, int pool,
                         hipStream_t stream);

/* Same convolution (stride 1) by Winograd F(2x2,3x3): u = G g G^T of the folded weights, transformed host-side and
 * stored as MFMA A fragments [16 positions][Cout/32][Cin/8][64 lanes][4] with lane 32h+l holding
 * U[pos][32 tile + l][8 kgroup + 4h .. +3] (16*Cout*Cin floats; cmr_agent_amd/models/_pack.py:winograd_u); input / output transforms, the 16 position GEMMs and the epilogue of cmr_conv3x3_nhwc_f32
 * (bias, residual, LeakyReLU, table, optional 2x2 average pool) are fused in one kernel.
 * Launch policy of the PERSISTENT kernel (maps of >= 200 tiles), per call -- the library keeps no state:
 *   cu_budget  CUs it may occupy (0 = all; rounded down to a multiple of 8).  It fills a CU completely, so a branch forked onto another
 *              stream only progresses between its launches unless it is left some CUs (the image tower beside the point tower);
 *   slices     workgroups per CU of that budget, each walking 1 / slices of the tiles (never fewer than 8 tiles per workgroup), so CUs
 *              return to the dispatcher during the launch; <= 1 = one workgroup per CU.  Results do not depend on either. */
int cmr_conv3x3_wino_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* u, const float* bias,
                              const float* res, const float* post, float* y, int Cout, float slope, int pool,
                              int cu_budget, int slices, hipStream_t stream);
/* The same convolution (no table operand) where the input is sparsely occupied and the other operands stay the same from call to call
 * (CMRAgent._embed_2d: the projected half of the observation on top of the image half of one registration).  Only the virtual tiles
 * order[0 .. *nlive) (8x16 output pixels x 64 couts; id = ((b tiles_y + ty) tiles_x + tx) Cout / 64 + cout group) are multiplied; the tiles
 * order[*nlive .. ntiles) of y are copied from y0 [B][H / pool][W / pool][Cout], or, with y0 null (pool 1 only), receive the epilogue of a
 * zero product, act(bias + res).  order (a permutation of all tiles) and nlive are read on the DEVICE.  F(2x2,3x3) output pixels are a
 * function of their own 3x3 input support alone, bit for bit, so with every tile live whose 1-pixel surrounding holds a non-zero input and
 * y0 = the dense result on an all-zero input the result equals the dense call's (finite weights assumed: 0 x Inf is not 0).  Served where
 * the dense call runs the persistent kernel (Cin >= 64, >= 200 tiles, 0 <= slope <= 1), CMR_EUNSUPPORTED (-3) otherwise. */
int cmr_conv3x3_wino_list_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* u, const float* bias, const float* res,
                                   float* y, int Cout, float slope, int pool, const int* order, const int* nlive, const float* y0,
                                   int cu_budget, int slices, hipStream_t stream);
/* The lists of two chained convolutions (H x W maps, Cout1 then Cout2 channels) from the byte maps cmr_observation_proj_reach_f32 marks:
 * order_m = the tiles with reach_m set in ascending order, then the others in ascending order, each expanded to its Cout_m / 64 virtual
 * tiles; *nlive_m = live virtual tiles.  Both maps are cleared for the next observation.  One launch. */
int cmr_wino_tile_lists(uint8_t* reach1, uint8_t* reach2, int B, int H, int W, int Cout1, int Cout2, int* order1, int* nlive1,
                        int* order2, int* nlive2, hipStream_t stream);
/* cmr_conv3x3_wino_list_nhwc_f32 that copies only the tiles order[*nlive .. *nend) (nend on the device; null: every tile) and leaves the
 * tiles order[*nend .. ntiles) of y UNWRITTEN: for a map whose only reader is a list launch that reads none of their pixels. */
int cmr_conv3x3_wino_list_nend_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* u, const float* bias, const float* res,
                                        float* y, int Cout, float slope, int pool, const int* order, const int* nlive, const int* nend,
                                        const float* y0, int cu_budget, int slices, hipStream_t stream);
/* The lists of two STAGES of two chained convolutions each -- stage 0 on H x W maps with Cout0 channels, stage 1 on its 2 x 2 pooled output
 * (H / 2 x W / 2, Cout1 channels; H, W even) -- from the four byte maps cmr_observation_proj_reach_staged_f32 marks (reach1 / reach2: stage
 * 0's first / second convolution, reach3 / reach4: stage 1's).  The second convolution's list of a stage (order2, order4) is
 * cmr_wino_tile_lists's: marked tiles ascending, then the others.  The first one's (order1, order3) has three parts, each ascending: the
 * marked tiles ("live"), the unmarked ones with a tile marked for the SECOND convolution in their 3 x 3 tile neighbourhood of the same
 * sample ("copy": the second convolution reads a one-pixel halo around its live tiles), the rest (read by nobody).  counts [6] = live,
 * live + copy of order1 and live of order2, then the same of order3 / order4, in virtual tiles.  The four maps are cleared.  One launch. */
int cmr_wino_tile_lists_staged(uint8_t* reach1, uint8_t* reach2, uint8_t* reach3, uint8_t* reach4, int B, int H, int W, int Cout0, int Cout1,
                               int* order1, int* order2, int* order3, int* order4, int* counts, hipStream_t stream);
/* Training forward of a 3x3 convolution that feeds a batch-statistics BatchNorm (models/ImageResNet.py:5-40 under Train_Geo.py:166-174):
 * y = conv(x) + bias as the call above with slope 1, no residual / table / pool, AND the sums the BatchNorm needs, accumulated by the helper
 * waves of the wave-specialised kernel while they finish the output tiles (they wait 25 - 50 % of a launch): part [parts][2][64] = per helper
 * wave the sums of (y - bias) and (y - bias)^2 over its pixels -- the separate cmr_bn_stats_f32 pass over y goes away.
 * parts = cmr_conv3x3_wino_stats_parts(...): 0 when this form is not served (Cout = 64, Cin >= 64, maps of >= 200 8x16-pixel tiles are): the
 * caller runs the plain entry point and cmr_bn_stats_f32.  cmr_bn_stats_from_sums_f32(part, parts, B H W, 64, bias, ...) finishes the
 * statistics. */
int64_t cmr_conv3x3_wino_stats_parts(int B, int H, int W, int Cin, int Cout, int cu_budget, int slices);
int cmr_conv3x3_wino_stats_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* u, const float* bias, float* y, int Cout,
                                    int cu_budget, int slices, float* part, int64_t parts, hipStream_t stream);
/* Data gradient of a stride-1 3x3 convolution whose INPUT was lrelu_{bn_slope}(BatchNorm(bn_x)) with no other consumer (ImageResNet.py:9-14
 * conv -> BatchNorm -> LeakyReLU -> conv under Train_Geo.py:166-174): dx [B][H][W][Cout] = conv(dy; u) (u from the transposed / flipped
 * weights, no bias) AND, from the same helper waves, the two sums of that BatchNorm's backward reduction over the pixels they finish --
 * part [parts][2][64] = sum d, sum d xhat with d = dx * act'(bn_x * stat[2] + stat[3]), xhat = (bn_x - stat[0]) stat[1]: what
 * cmr_bn_bwd_f32's first pass over (dx, bn_x) computes.  bn_x [B][H][W][Cout], bn_stat [4][Cout]; shapes and parts as the statistics
 * launch above (0 <= bn_slope <= 1).  cmr_bn_bwd_from_sums_f32 finishes the BatchNorm backward.  COMPILED OUT by default (answers -3;
 * csrc/conv_wino.hip CMR_WS_BNBWD: its registers cost every launch of the kernel more than the update gains). */
int cmr_conv3x3_wino_bnbwd_nhwc_f32(const float* dy, int B, int H, int W, int Cin, const float* u, float* dx, int Cout, const float* bn_x,
                                    const float* bn_stat, float bn_slope, int cu_budget, int slices, float* part, int64_t parts,
                                    hipStream_t stream);
/* Stride-2 3x3 convolution (the two strided convolutions of a down-sampling ResidualBlock, ImageResNet.py:9-14, :24-27) with the weights
 * as MFMA A fragments [9 taps][Cout/32][Cin/8][64 lanes][4] read straight from L2 (cmr_agent_amd/models/_pack.py:conv_s2_frags): same
 * arithmetic and epilogue as cmr_conv3x3_nhwc_f32 at stride 2 (bias, residual, LeakyReLU), two barriers per 16-channel halo chunk instead
 * of one per tap.  Served: Cin = 64, Cout % 64 == 0, no table operand; otherwise CMR_EUNSUPPORTED (-3) and the caller uses
 * cmr_conv3x3_nhwc_f32. */
int cmr_conv3x3_s2_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* wfrag, const float* bias, const float* res,
                            const float* post, float* y, int Cout, float slope, hipStream_t stream);
/* MiniResNet block 0 (3 -> 64 channels, 1x1 shortcut), NCHW image in, NHWC features out (fp32, or bf16 when out_bf16 != 0: the
 * bf16-stored image tower of the bf16 mode).  tmp_nchw is scratch of [B][6][H][W] floats (conv-a output | a copy of the image);
 * 0 <= slope <= 1.  ImageResNet.py:50 with :9-23. */
int cmr_stem_block_f32(const float* x_nchw, const float* w_a, const float* b_a, const float* w3, const float* w1,
                       const float* b_b, float* tmp_nchw, void* y_nhwc, int out_bf16, int B, int H, int W, float slope,
                       hipStream_t stream);

/* AvgPool2d((kh,kw), stride=(kh,kw)) on NHWC; (kh,kw)=(H,W) is the global pool.  CMRAgent.py:39,45,51,56. */
int cmr_avgpool_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, int kh, int kw, hipStream_t stream);

/* out = cat([f, nearest_upsample(proxy, scale)], channel).  IMGPCEnDecoder.py:85-89. */
int cmr_upsample_concat_f32(const float* f, const float* proxy, float* out, int B, int H, int W, int C1, int C2,
                            int scale, hipStream_t stream);

/* non-overlapping PxP patches as rows [(ky,kx,c)] for the stride-P patch conv.  ImageViT.py:19-22,51. */
int cmr_patchify_nhwc_f32(const float* x, float* out, int B, int H, int W, int C, int P, hipStream_t stream);
/* The patch embedding itself (ImageViT.py:37-56: Conv2d(C, n_out, kernel = stride = P) + position rows) as ONE GEMM that reads the P x P
 * patches of x [B][H][W][C] in place: y[(b, Y, X)][:] = sum_{py,px,c} w[:][(py P + px) C + c] x[b][P Y + py][P X + px][c] + bias (+ res
 * rows, row % res_mod when res_mod > 0).  = cmr_patchify_nhwc_f32 + cmr_linear_f32 without the patchified copy.  P P C % 64 == 0,
 * (P C) % 8 == 0, at most 65 536 patches. */
int cmr_patch_embed_f32(const float* x_nhwc, int B, int H, int W, int C, int P, const float* w, int64_t ldw, const float* bias,
                        const float* res, int64_t ldres, int64_t res_mod, float* y, int64_t ldy, int n_out, hipStream_t stream);
/* bf16 mode: y = act(x W^T + bias (+ res)) for the big contiguous row maps on the bf16 matrix cores (rows and weights rounded to bf16,
 * fp32 accumulate, fp32 tensors): K in {32, 64, 128}, n_out <= 128 (K = 128: <= 64); other shapes return CMR_EUNSUPPORTED (-3) and the
 * caller uses cmr_linear_f32.  Same argument meaning as cmr_linear_f32 without the second source. */
int cmr_linear_rows_bf16_f32(const float* x, int64_t ldx, int k, const float* w, int64_t ldw, const float* bias, const float* res,
                             int64_t ldres, int64_t res_mod, float* y, int64_t ldy, int64_t rows, int n_out, int act, float act_param,
                             hipStream_t stream);

/* [batch][R][C] -> [batch][C][R]: layout changes at the nn.Module boundary (NCHW <-> NHWC). */
int cmr_transpose_f32(const float* x, float* y, int batch, int R, int Cn, hipStream_t stream);

/* ---- attention ----------------------------------------------------------------------------- */

/* softmax(Q K^T / sqrt(8)) V, 8 heads x 8 dims.  ImageViT.py:93-104, IMGPCEncoder.py:45-53. */
int cmr_mha_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* o,
                int64_t ldo, int B, int Tq, int Tk, hipStream_t stream);
/* The same attention with the exponentials through libm's expf instead of v_exp_f32(x log2 e) (about 25 % slower): the no-dropout forward
 * of the training tape, whose backward kernels (cmr_mha_bwd_f32) recompute the probabilities with expf. */
int cmr_mha_expf_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* o, int64_t ldo, int B,
                     int Tq, int Tk, hipStream_t stream);
/* LayerNorm(64) + the block's query / key / value projections + the attention above in ONE launch (inference; ImageViT.py:81-108,
 * IMGPCEncoder.py:36-58, :93-94 -- x and y pass through the SAME norm): o = softmax(Q K^T / sqrt 8) V with Q = LN(x) Wq^T + bq,
 * K | V = LN(y) Wk|v^T + bk|v (y == x: self-attention).  Every workgroup (64 queries of one (batch, head)) normalises and projects the
 * source rows onto its head's dims while staging them, so q / k / v never exist in memory.  wq_frag / wkv_frag: [8 heads][16][64] floats
 * (cmr_agent_amd/models/_pack.py:mha_ln_frags).  Same value as cmr_ln64_linear_f32 + cmr_mha_f32 up to fp32 summation order. */
int cmr_mha_ln_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gamma, const float* beta, float eps,
                   const float* wq_frag, const float* wkv_frag, const float* bq, const float* bk, const float* bv, float* o, int64_t ldo,
                   int B, int Tq, int Tk, hipStream_t stream);
/* kvsum[b] = { KV[h][d][v] = sum_s K~ V / S (512), Ksum[h][d] (64) }.  LinearAttention.py:55-58. */
int64_t cmr_la_reduce_workspace_bytes(int B, int S);
int cmr_la_reduce_f32(const float* kf, int64_t ldk, const float* v, int64_t ldv, float* kvsum, void* workspace,
                      int64_t workspace_bytes, int B, int S, hipStream_t stream);
/* msg = (Q~ KV) * S / (Q~ Ksum + eps).  LinearAttention.py:59-60. */
int cmr_la_apply_f32(const float* qf, int64_t ldq, const float* kvsum, float* msg, int64_t ldm, int B, int L, int S,
                     float eps, hipStream_t stream);

/* Tail of CMRAgent.forward (CMRAgent.py:52-56 global pool + two 1x1 convs, :101-116 the three MLP heads on
 * cat([embed_2d, embed_3d])) in one launch, one workgroup per sample.  x [B][npix][128] is the activated output of the
 * last 3x3 conv; weights are the PyTorch [out][in] matrices; head i: 256 -> n0 -> n1 -> n2 with LeakyReLU(slope)
 * between, logits written to out[b * ldo + 0..n2).  r_act / t_act (optional, int64 [B][degree]): the deterministic actions of
 * CMRAgent.action_from_logits (CMRAgent.py:118-123), argmax over each group of num_steps logits with the first maximum on ties
 * (= cmr_argmax_rows_f32 on the same rows), emitted by the same launch. */
int cmr_agent_heads_f32(const float* x, int B, int npix, const float* w24, const float* b24, const float* w26,
                        const float* b26, const float* e3d,
                        const float* r_w0, const float* r_b0, const float* r_w1, const float* r_b1, const float* r_w2, const float* r_b2,
                        int r_n0, int r_n1, int r_n2, float* r_out, int r_ldo,
                        const float* t_w0, const float* t_b0, const float* t_w1, const float* t_b1, const float* t_w2, const float* t_b2,
                        int t_n0, int t_n1, int t_n2, float* t_out, int t_ldo,
                        const float* v_w0, const float* v_b0, const float* v_w1, const float* v_b1, const float* v_w2, const float* v_b2,
                        int v_n0, int v_n1, int v_n2, float* v_out, int v_ldo,
                        int num_steps, int degree_r, int degree_t, int64_t* r_act, int64_t* t_act,
                        float slope, hipStream_t stream);
/* Training forward of the same tail (Train_Agent.py:263-305 through CMRAgent.py:52-56, 101-116): the logits and, in `saves`, every
 * intermediate the backward needs -- pooled [B][128] | t1 = lrelu(conv 24) [B][128] | e2d = conv 26 [B][128] | per head (r, t, v):
 * h0 [B][n0], h1 [B][n1] (post-activation) -- from ONE launch instead of 13 (column mean, two 1x1 convs, nine head layers).
 * saves_floats >= B (384 + sum of n0 + n1 over the heads).  Weights [out4][in4] as stored in the flat bucket. */
int cmr_agent_heads_train_f32(const float* x, int B, int npix, const float* w24, const float* b24, const float* w26,
                              const float* b26, const float* e3d,
                              const float* r_w0, const float* r_b0, const float* r_w1, const float* r_b1, const float* r_w2, const float* r_b2,
                              int r_n0, int r_n1, int r_n2, float* r_out, int r_ldo,
                              const float* t_w0, const float* t_b0, const float* t_w1, const float* t_b1, const float* t_w2, const float* t_b2,
                              int t_n0, int t_n1, int t_n2, float* t_out, int t_ldo,
                              const float* v_w0, const float* v_b0, const float* v_w1, const float* v_b1, const float* v_w2, const float* v_b2,
                              int v_n0, int v_n1, int v_n2, float* v_out, int v_ldo,
                              float* saves, int64_t saves_floats, float slope, hipStream_t stream);
/* The same tail with every weight matrix stored TRANSPOSED: W^T [in][out4] (out4 = the output width padded to a multiple of 4 with zero
 * columns; hidden widths n0, n1 multiples of 16): a lane owns four outputs and a wave a slice of the inputs, so that a layer is one memory
 * round trip and no cross-lane reduction (35 -> ~15 us per agent step on the serial chain of a registration).  Same arguments otherwise;
 * results agree with cmr_agent_heads_f32 to fp32 rounding of the sums (other summation order). */
int cmr_agent_heads_t_f32(const float* x, int B, int npix, const float* w24t, const float* b24, const float* w26t, const float* b26,
                          const float* e3d,
                          const float* r_w0t, const float* r_b0, const float* r_w1t, const float* r_b1, const float* r_w2t, const float* r_b2,
                          int r_n0, int r_n1, int r_n2, float* r_out, int r_ldo,
                          const float* t_w0t, const float* t_b0, const float* t_w1t, const float* t_b1, const float* t_w2t, const float* t_b2,
                          int t_n0, int t_n1, int t_n2, float* t_out, int t_ldo,
                          const float* v_w0t, const float* v_b0, const float* v_w1t, const float* v_b1, const float* v_w2t, const float* v_b2,
                          int v_n0, int v_n1, int v_n2, float* v_out, int v_ldo,
                          int num_steps, int degree_r, int degree_t, int64_t* r_act, int64_t* t_act, float slope, hipStream_t stream);

/* Pre-LN transformer block (ImageViT.py:61-158 = PointViT.py:96-183 = IMGPCEncoder.py:14-102) in three launches.
 * Weights marked _f are MFMA A fragments: W [n_out][k] stored as [n_out/32][k/8][64 lanes][4] with lane 32h+l holding
 * W[32 tile + l][8 kgroup + 4h .. +3] (cmr_agent_amd/models/_pack.py:frag_pack).
 *   cmr_ln64_linear_f32: out_x = LN(x) Wx^T + bx and (y != NULL) out_y = LN(y) Wy^T + by with the SAME LayerNorm
 *                        (attention_norm feeds query and key/value, IMGPCEncoder.py:93-94); n_out multiples of 64.
 *   cmr_vit_out_ffn_f32: x1 = ctx Wo^T + bo + x (attn.out + residual); out = x1 + fc2(gelu(fc1(LN(x1))))
 *                        (ffn_norm, Mlp 64 -> 1024 -> 64, exact erf GELU). */
int cmr_ln64_linear_f32(const float* x, int64_t ldx, int64_t rows_x, const float* wf_x, const float* bias_x, int n_out_x,
                        float* out_x, int64_t ldo_x, const float* y, int64_t ldy, int64_t rows_y, const float* wf_y,
                        const float* bias_y, int n_out_y, float* out_y, int64_t ldo_y, const float* gamma, const float* beta,
                        float eps, hipStream_t stream);
int cmr_vit_out_ffn_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const float* wo_f, const float* bo,
                        const float* ln_g, const float* ln_b, float eps, const float* w1_f, const float* b1, const float* w2_f,
                        const float* b2, float* out, int64_t ldo, int64_t rows, hipStream_t stream);
/* The same block tail on 16-row tiles (v_mfma_f32_16x16x4_f32): twice the workgroups for the small proxy sets of this path
 * (3 344 / 2 048 rows -> 209 / 128 workgroups).  Weights as 16x16x4 A fragments [n_out/16][k/16][64 lanes][4], lane = 16 g + m
 * holding W[16 To + m][16 T + 4 g + r], r = 0..3 (cmr_agent_amd/models/_pack.py:frag_pack16); same arguments otherwise. */
int cmr_vit_out_ffn16_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const float* wo_f16, const float* bo,
                          const float* ln_g, const float* ln_b, float eps, const float* w1_f16, const float* b1,
                          const float* w2_f16, const float* b2, float* out, int64_t ldo, int64_t rows, hipStream_t stream);
/* bf16 matrix-core variants of the two kernels above (same arguments; the _f weights are bf16 A fragments
 * [n_out/32][k/16][64 lanes][8], cmr_agent_amd/models/_pack.py:frag_pack_bf16 -- natural k order for wf_x / wf_y / wo_f, accumulator
 * order for w1_f / w2_f; products on v_mfma_f32_32x32x16_bf16, fp32 accumulation; LayerNorm, GELU, biases, residuals fp32). */
int cmr_ln64_linear_bf16_f32(const float* x, int64_t ldx, int64_t rows_x, const void* wf_x, const float* bias_x, int n_out_x,
                             float* out_x, int64_t ldo_x, const float* y, int64_t ldy, int64_t rows_y, const void* wf_y,
                             const float* bias_y, int n_out_y, float* out_y, int64_t ldo_y, const float* gamma, const float* beta,
                             float eps, hipStream_t stream);
int cmr_vit_out_ffn_bf16_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const void* wo_f, const float* bo,
                             const float* ln_g, const float* ln_b, float eps, const void* w1_f, const float* b1, const void* w2_f,
                             const float* b2, float* out, int64_t ldo, int64_t rows, hipStream_t stream);

/* Fused linear-attention layer (LinearAttention.py:38-73) in two kernels; the unfused entry points above stay for
 * callers that need the intermediates.
 *   cmr_la_kv_state_f32:    y [B*S, 64] -> K = elu(Wk y)+1 (:45-46,52), V = (Wv y)/S (:47,57) -> kvsum [B][576] in the
 *                           layout of cmr_la_reduce_f32 (KV[h][d][v] at h*64 + d*8 + v, Ksum[h][d] at 512 + h*8 + d).
 *                           Deterministic (per-wave partials in `workspace`, summed in a fixed order).
 *   cmr_la_query_layer_f32: x [B*L, 64] -> Q = elu(Wq x)+1 -> message (:58-60) -> merge -> LayerNorm (:63-64)
 *                           -> mlp(cat[x, message]): 128 -> 128 ReLU -> 64 (:67) -> LayerNorm (:68) -> x + . (:70).
 *                           Weights are the PyTorch [out][in] matrices (no bias, as in the reference).
 *                           CMR_EUNSUPPORTED when the B states do not fit in LDS beside the weights (B > 11). */
int64_t cmr_la_kv_state_workspace_bytes(int B, int S);
int cmr_la_kv_state_f32(const float* y, int64_t ldy, const float* wk, const float* wv, float* kvsum, void* workspace,
                        int64_t workspace_bytes, int B, int S, hipStream_t stream);
/* The same state with the two projections on the bf16 matrix cores (rows and weights rounded to bf16, fp32 accumulate; elu + 1, 1 / S and
 * the row contraction K^T V stay fp32): the bf16 mode's source side of the layer, next to cmr_la_query_layer_bf16_f32.  Same arguments and
 * workspace. */
int cmr_la_kv_state_bf16_f32(const float* y, int64_t ldy, const float* wk, const float* wv, float* kvsum, void* workspace,
                             int64_t workspace_bytes, int B, int S, hipStream_t stream);
int cmr_la_query_layer_f32(const float* x, int64_t ldx, const float* kvsum, const float* wq, const float* wmerge,
                           const float* ln1_g, const float* ln1_b, const float* w_mlp0, const float* w_mlp3,
                           const float* ln2_g, const float* ln2_b, float* out, int64_t ldo, int B, int L, int S, float eps,
                           float ln_eps, hipStream_t stream);
/* bf16 matrix-core variant of the same layer (same arguments; the four GEMMs on v_mfma_f32_32x32x16_bf16 with fp32 accumulation,
 * operands rounded to bf16; the per-head state product, both LayerNorms and the residual stay fp32).  Enabled by
 * cmr_agent_amd.ops.CONV_BF16. */
int cmr_la_query_layer_bf16_f32(const float* x, int64_t ldx, const float* kvsum, const float* wq, const float* wmerge,
                                const float* ln1_g, const float* ln1_b, const float* w_mlp0, const float* w_mlp3,
                                const float* ln2_g, const float* ln2_b, float* out, int64_t ldo, int B, int L, int S,
                                float eps, float ln_eps, hipStream_t stream);

/* Front half of the vector attention of GroupPointTransformer / KnnPointTransformer (PointNN.py:151-170, 219-226) in one
 * launch, per row r (a (point, owning node) or (node, neighbour) pair):
 *   k, v = [Wk | Wv] (W10 feat[r] + b10)           when feat != NULL   (group transformer)
 *        = kv[ik ? ik[r] : r][0:64], [64:128]      when feat == NULL   (kNN transformer: precomputed table)
 *   pos = Wd2 relu(Wd0 (pa4[ia ? ia[r] : r / diva] - pb4[ib[r]]) + bd0) + bd2        (Wd0: [64][4], 3 columns used)
 *   a_out[r] = Wg2 relu(Wg0 (q[iq ? iq[r] : r / divq] - k + pos) + bg0) + bg2 ;  vp_out[r] = v + pos
 * a_out / vp_out are [rows][64] and feed cmr_segment_softmax_f32.  Replaces cmr_rel_pos_f32 + cmr_vecattn_prep_f32 +
 * six cmr_linear_f32 launches. */
int cmr_vecattn_front_f32(const float* feat, int64_t ldf, const float* w10, const float* b10, const float* wkv, const float* kv,
                          int64_t ldkv, const int32_t* ik, const float* q, int64_t ldq, const int32_t* iq, int64_t divq,
                          const float* pa4, const int32_t* ia, int64_t diva, const float* pb4, const int32_t* ib,
                          const float* wd0, const float* bd0, const float* wd2, const float* bd2, const float* wg0,
                          const float* bg0, const float* wg2, const float* bg2, float* a_out, float* vp_out, int64_t rows,
                          hipStream_t stream);
/* The same front under model.train() (Train_Geo.py:166-174): k and v from their own [*][64] maps (row ikv ? ikv[r] : r of both), q gathered
 * as above, and beside
 * a_out / vp_out the three activations a layer-by-layer backward reads, all [rows][64]: hd = relu(fc_delta[0]), t = q - k + pos,
 * g1 = relu(fc_gamma[0]).  Replaces four cmr_linear_f32 launches, the gather of q and cmr_vecattn_mix_f32 of a training step.  rows a
 * multiple of 32, else CMR_EUNSUPPORTED. */
int cmr_vecattn_front_train_f32(const float* k, int64_t ldk, const float* v, int64_t ldv, const int32_t* ikv, const float* q, int64_t ldq,
                                const int32_t* iq,
                                int64_t divq, const float* pa4, const int32_t* ia, int64_t diva, const float* pb4, const int32_t* ib,
                                const float* wd0, const float* bd0, const float* wd2, const float* bd2, const float* wg0, const float* bg0,
                                const float* wg2, const float* bg2, float* a_out, float* vp_out, float* hd_out, float* t_out, float* g1_out,
                                int64_t rows, hipStream_t stream);
/* ... and with k, v computed inside as well (group transformer: x = W10 feat + b10, k = Wk x, v = Wv x): x_out [rows][64] is stored for the
 * projections' backward, k and v never leave the registers. */
int cmr_vecattn_front_kv_train_f32(const float* feat, int64_t ldf, const float* w10, const float* b10, const float* wk, const float* wv,
                                   const float* q, int64_t ldq, const int32_t* iq, int64_t divq, const float* pa4, const int32_t* ia,
                                   int64_t diva, const float* pb4, const int32_t* ib, const float* wd0, const float* bd0, const float* wd2,
                                   const float* bd2, const float* wg0, const float* bg0, const float* wg2, const float* bg2, float* a_out,
                                   float* vp_out, float* hd_out, float* t_out, float* g1_out, float* x_out, int64_t rows,
                                   hipStream_t stream);

/* ---- loss / metric values of the heads (forward only) ---------------------------------------- */

/* MultiHeadModel.py:68-97 on 2-class logits rows [rows][ld >= 2] with int64 labels: out4 = {focal loss (focal_loss.py:55-110,
 * gamma 2, mean), precision, recall, accuracy}; rows = B * n (accuracy is (correct / B) / n as in the reference).  A non-zero
 * label is class 1, here and in cmr_focal_bwd_f32. */
int64_t cmr_focal_metrics_workspace_bytes(int64_t rows);
int cmr_focal_metrics_f32(const float* logits, int64_t ld, const int64_t* label, float alpha, int64_t rows, int B, float* out4,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* MultiHeadModel.py:141-178, 240-268: circle loss over the n sampled (point, pixel) pairs of every sample.  pc_feat rows
 * [B*N][64], img_feat NHWC [B][h][w][64], pc_idx int64 [B][n], xy_int int64 [B][2][n] (x, y), xy_float [B][2][n];
 * out[0] = lambda * mean. */
int64_t cmr_circle_loss_workspace_bytes(int B, int n);
int cmr_circle_loss_f32(const float* pc_feat, const float* img_feat, const int64_t* pc_idx, const int64_t* xy_int,
                        const float* xy_float, int B, int N, int h, int w, int n, float dist_thres, float pos_margin,
                        float neg_margin, float log_scale, float lambda, float* out, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream);

/* Match evaluation of the geometric features (MultiHeadModel.py:180-216 cal_match_accuracy, :285-315 cal_matcning_ground_truth,
 * Test_Geo.py:91-122): for every selected point the nearest pixel feature in L2, argmin over the sample's h*w pixels, ties to the lower
 * pixel index (torch.argmin).  pc_feat rows [B*N][C], img_feat [B][h*w][C] (NHWC), C must be 64; mask [B*N] with mask_bytes 1 (u8 /
 * bool) or 8 (int64), non-zero = selected.  idx int32 [B*N] = pixel p (x = p % w, y = p / w) or -1 on unselected rows; dist (optional)
 * f32 [B*N] = the minimum distance (NaN on unselected rows).  counts int32 [B][4] = {selected, selected with |xy(p) - gt_xy| <= thr,
 * selected whose pixel has img_overlap != 0, both}; gt_xy (optional) f32 [B][2][N] (x row, y row; non-finite is never an inlier),
 * img_overlap (optional) u8 [B*h*w].  Workspace: cmr_feat_match_workspace_bytes(B, N). */
int64_t cmr_feat_match_workspace_bytes(int B, int N);
int cmr_feat_match_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask, int mask_bytes,
                       const float* gt_xy, float thr, const uint8_t* img_overlap, int32_t* idx, float* dist, int32_t* counts,
                       void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Match filtering ahead of PnP-RANSAC (port extension; ops.feat_match_filter, MultiHeadModel.pose_from_matches,
 * Test_Geo.py --mutual / --ratio).  Inputs as cmr_feat_match_f32: pc_feat rows [B*N][C], img_feat [B][h*w][C], C must be 64, mask [B*N]
 * with mask_bytes 1 or 8.  Per sample, S = the selected rows, d(n, p) = the L2 distance of point n and pixel p:
 *   idx int32 [B*N]    argmin_p d(n, p), ties to the lowest p: cmr_feat_match_f32's idx bit for bit (same arithmetic); -1 outside S;
 *   d1 (optional) f32 [B*N]  that minimum; d2 (optional) f32 [B*N]  min of d(n, p) over the pixels OUTSIDE the window of the best pixel,
 *                      max(|x_p - x_best|, |y_p - y_best|) > excl_radius (>= 0; 0 = the plain second nearest), +inf when there is none;
 *                      both NaN outside S;
 *   rev (optional) int32 [B*h*w]  argmin over n in S of d(n, p) as a row number, ties to the lowest n; -1 when S is empty;
 *   keep u8 [B*N]      n in S and (!mutual or rev[idx[n]] == n) and (ratio <= 0 or d1 <= ratio * d2) and (max_dist <= 0 or
 *                      d1 <= max_dist), on distances (not squares), in fp32; an infinite d2 passes;
 *   counts int32 [B][4] = {|S|, kept, kept and inlier, selected and inlier}; inlier as cmr_feat_match_f32: gt_xy (optional, f32
 *                      [B][2][N]) finite and within thr of the best pixel.
 * The reverse sweep runs only with mutual or rev, the windowed one only with ratio > 0 or d2.  Everything is enqueued on the stream (no
 * host round trip); every output is a plain store of the workgroup that owns the row / pixel and the counts are integer atomics, so
 * two calls agree bit for bit and a sample depends on its own rows only.  Workspace: cmr_feat_match_filter_workspace_bytes(B, N, h, w),
 * 16-byte aligned. */
int64_t cmr_feat_match_filter_workspace_bytes(int B, int N, int h, int w);
int cmr_feat_match_filter_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                              int mask_bytes, int mutual, float ratio, int excl_radius, float max_dist, const float* gt_xy, float thr,
                              int32_t* idx, uint8_t* keep, int32_t* counts, float* d1, float* d2, int32_t* rev, void* workspace,
                              int64_t workspace_bytes, hipStream_t stream);

/* Dual-softmax match confidence ahead of PnP-RANSAC (port extension; ops.match_conf, MultiHeadModel.match_features_conf,
 * MultiHeadModel.pose_from_matches(min_conf=), Test_Geo.py --min-conf).  Inputs as cmr_feat_match_filter_f32: pc_feat rows [B*N][C],
 * img_feat [B][h*w][C], C must be 64 (else CMR_EUNSUPPORTED), mask [B*N] with mask_bytes 1 or 8, gt_xy (optional) f32 [B][2][N],
 * h*w <= 2^24, temperature T > 0 and finite, 0 <= min_conf <= 1 (0 = no threshold).  Per sample, S = the selected rows, d2(n, p) = the
 * squared L2 distance of point n and pixel p, s(n, p) = -d2(n, p) / T:
 *   idx int32 [B*N]    argmin_p d(n, p), ties to the lowest p: cmr_feat_match_f32's idx bit for bit (same arithmetic); -1 outside S;
 *   d1 (optional) f32 [B*N]  that minimum distance, cmr_feat_match_filter_f32's d1 bit for bit; NaN outside S;
 *   row_lse (optional) f32 [B*N]  log of the sum over ALL h*w pixels p of exp s(n, p); NaN outside S;
 *   col_lse (optional) f32 [B*h*w]  log of the sum over n in S of exp s(n, p); -inf when S is empty;
 *   conf f32 [B*N]     min(1, exp(2 s(n, idx[n]) - row_lse[n] - col_lse[idx[n]])): the match's probability under the softmax over its
 *                      row times that under the softmax over its column; NaN outside S; in (0, 1], a value under the smallest normal
 *                      fp32 may come out as 0;
 *   keep u8 [B*N]      n in S and (min_conf <= 0 or conf[n] >= min_conf);
 *   counts int32 [B][4] = {|S|, kept, kept and inlier, selected and inlier}; inlier as cmr_feat_match_f32: sqrtf(dx^2 + dy^2) <= thr
 *                      against gt_xy, a non-finite gt_xy is never an inlier.
 * Two distance sweeps (points x pixels, pixels x points), each carrying an online log-sum-exp in base 2 whose running maximum is the
 * running minimum of the distance.  Everything is enqueued on the stream (no host round trip); every output is a plain store of the
 * workgroup / thread that owns it, the sums are folded in a fixed order that depends only on the sample's own selected count and the map
 * size, and the counts are integer atomics (at most one per word and workgroup): two calls agree bit for bit and a sample's outputs are
 * the same bits alone and inside any batch.  Workspace: cmr_match_conf_workspace_bytes(B, N, h, w), 16-byte aligned. */
int64_t cmr_match_conf_workspace_bytes(int B, int N, int h, int w);
int cmr_match_conf_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask, int mask_bytes,
                       float temperature, float min_conf, const float* gt_xy, float thr, int32_t* idx, float* conf, uint8_t* keep,
                       int32_t* counts, float* d1, float* row_lse, float* col_lse, void* workspace, int64_t workspace_bytes,
                       hipStream_t stream);

/* Camera pose from 2-D/3-D correspondences, PnP inside RANSAC (port extension; MultiHeadModel.pose_from_matches,
 * Test_Geo.py --pnp).  pts f32 [B][3][N] (planar, data['pc']), uv f32 [B][2][N] pixel coordinates on the map K refers to, mask [B*N]
 * with mask_bytes 1 (u8 / bool) or 8 (int64), non-zero = use; K f32 [B][3][3].  Per sample: the selected rows in row order; n_hyp
 * hypotheses, each from 4 distinct list positions drawn by a 32-bit hash of (seed, sample, hypothesis, counter), Lambda Twist P3P in
 * float64 on three, the fourth choosing among the solutions; a correspondence is an inlier of K[R|t] when z > 0 and its reprojection
 * error is <= thr (fp32); the hypothesis with most inliers (ties to the lowest index) is refined by up to refine_iters Gauss-Newton
 * steps on its inlier set and kept refined if the inliers do not drop.  pose f32 [B][4][4] maps pts into the camera frame (data['P']);
 * inliers int32 [B]; status int32 [B] = 0 ok, 1 fewer than 4 correspondences, 2 no valid hypothesis (both: identity pose, 0 inliers);
 * hyp_inliers (optional) int32 [B][n_hyp] = inliers per hypothesis, -1 for an invalid one.  Deterministic: a sample's outputs depend
 * only on its own inputs, its index b and seed.  Workspace: cmr_pnp_ransac_workspace_bytes(B, N, n_hyp), 8-byte aligned. */
int64_t cmr_pnp_ransac_workspace_bytes(int B, int N, int n_hyp);
int cmr_pnp_ransac_f32(const float* pts, const float* uv, const void* mask, int mask_bytes, const float* K, int B, int N, int n_hyp,
                       float thr, uint32_t seed, int refine_iters, float* pose, int32_t* inliers, int32_t* status, int32_t* hyp_inliers,
                       void* ws, int64_t ws_bytes, hipStream_t stream);

/* Pose-guided matching (port extension; ops.guided_match, MultiHeadModel.refine_pose_from_matches, Test_Geo.py --guided,
 * Test_Agent.py --refine): the nearest pixel feature of every selected point inside a window round its projection under a given pose.
 * pts f32 [B][3][N] (data['pc']), pc_feat rows [B*N][C], img_feat [B][h*w][C], C must be 64, mask [B*N] with mask_bytes 1 or 8, pose f32
 * [B][4][4] mapping pts into the camera frame (data['P'], pnp_pose), K f32 [B][3][3] for the h x w map (h*w <= 2^24), 0 <= radius <= 16,
 * max_dist >= 0 (0 = off).  Per sample and selected row n, all in fp32: X_c = R x + t, p = K X_c, u = p0 / p2, v = p1 / p2, centre
 * (cx, cy) = (rint u, rint v), half to even.  The row is IN VIEW iff p2 > 0, u and v are finite and [cx - r, cx + r] x [cy - r, cy + r]
 * meets the map (decided on the floats); the window is clipped to the map.
 *   idx int32 [B*N]    the pixel p = y * w + x of the clipped window with the least L2 feature distance, lowest p on a tie; -1 for an
 *                      unselected or out-of-view row;
 *   dist (optional) f32 [B*N]  that distance, the direct sum of (a - b)^2 in fp32 (order: DESIGN.md 4n), NaN where idx = -1;
 *   proj (optional) f32 [B][2][N]  (u, v) as computed, NaN for unselected rows and rows with p2 <= 0;
 *   keep u8 [B*N]      in view and (max_dist <= 0 or dist <= max_dist).  A window without one finite score (NaN features) gives
 *                      idx = the window's first pixel and dist = +inf, so it is kept only when max_dist is off: feed finite features;
 *   counts int32 [B][4] = {selected, in view, kept, kept and inlier}; inlier as cmr_feat_match_f32: gt_xy (optional, f32 [B][2][N])
 *                      finite and within thr of the matched pixel.
 * Everything is enqueued on the stream (no host round trip); every output element is a plain store by the one thread / 16-lane group
 * that owns the row and the counts are integer atomics, so two calls agree bit for bit and a sample depends on its own rows only.
 * Workspace: cmr_guided_match_workspace_bytes(B, N), 16-byte aligned. */
int64_t cmr_guided_match_workspace_bytes(int B, int N);
int cmr_guided_match_f32(const float* pts, const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                         int mask_bytes, const float* pose, const float* K, int radius, float max_dist, const float* gt_xy, float thr,
                         int32_t* idx, uint8_t* keep, int32_t* counts, float* dist, float* proj, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream);

/* Gauss-Newton pose refinement from a given pose (port extension; ops.pnp_refine): cmr_pnp_ransac_f32's refinement step,
 * startable from any pose, the accumulation split over the correspondences.  pts f32 [B][3][N], uv f32 [B][2][N], mask [B*N] with
 * mask_bytes 1 or 8, K f32 [B][3][3], pose_in f32 [B][4][4] (finite), thr > 0, 0 <= iters <= 1000.  Per sample: the WORKING SET is fixed
 * once -- the selected rows that are inliers of K[R|t] of pose_in under cmr_pnp_ransac_f32's fp32 predicate; up to iters Gauss-Newton
 * steps on it (left increment, J^T J, J^T r and cost in float64 summed in a fixed order, 6x6 Cholesky; a step is kept only if the next
 * evaluation's cost is lower, else undone and the loop stops); the result is recounted over ALL selected rows and kept if that count is
 * >= the working set's size.  pose f32 [B][4][4]; inliers int32 [B]; status int32 [B]: 0 = pose is the refined pose (iters = 0: pose_in
 * and its count), 1 = fewer than 4 rows in the working set (pose = pose_in, inliers = that number), 2 = refinement not kept: non-finite
 * sums or a failed first factorisation, or the recount dropped (pose = pose_in, inliers = the working set's size).  A factorisation
 * counts as failed when a pivot is <= 1e-13 of its diagonal entry (cmr_pnp_ransac_f32 asks only for > 0); the same test ends the loop
 * at a later step too, and then the pose accepted so far goes to the recount (status 0).  3 + 2 (iters + 1) launches whatever the data, no atomics, no host round trip; two calls
 * agree bit for bit and a sample depends on its own rows only.  Workspace: cmr_pnp_refine_workspace_bytes(B, N), 16-byte aligned. */
int64_t cmr_pnp_refine_workspace_bytes(int B, int N);
int cmr_pnp_refine_f32(const float* pts, const float* uv, const void* mask, int mask_bytes, const float* K, const float* pose_in, int B,
                       int N, float thr, int iters, float* pose, int32_t* inliers, int32_t* status, void* ws, int64_t ws_bytes,
                       hipStream_t stream);

/* Sub-pixel match positions by a parabola fit on feature distances (port extension; ops.match_subpixel,
 * MultiHeadModel.pose_from_matches / refine_pose_from_matches with subpixel=True, Test_Geo.py / Test_Agent.py --subpixel): turns the idx
 * of cmr_feat_match_f32, cmr_feat_match_filter_f32 or cmr_guided_match_f32 into float pixel coordinates for cmr_pnp_ransac_f32 /
 * cmr_pnp_refine_f32.  pc_feat rows [B*N][C], img_feat [B][h*w][C], C must be 64 (else CMR_EUNSUPPORTED), h*w <= 2^24, idx int32 [B*N],
 * mask (optional) [B*N] with mask_bytes 1 or 8, gt_xy (optional) f32 [B][2][N], thr in pixels.
 * A row is MATCHED iff (mask is null or non-zero) and 0 <= idx < h*w; any other index is treated as unmatched and never dereferenced.
 * For a matched row p = idx, x = p % w, y = p / w and s(q) = the squared L2 distance of the point feature and pixel q, the direct sum of
 * (a - b)^2 in fp32 (order: DESIGN.md 4o), not the |q|^2 - 2 p.q expansion.  Along x, with s0 = s(p), sm = s(p - 1), sp = s(p + 1),
 * num = sm - sp, den = (sm - s0) + (sp - s0): the axis is FITTED iff 1 <= x <= w - 2, num and den are finite and den > 0; then
 * dx = clamp(0.5 * num / den, -0.5, +0.5), else dx = 0.  Along y the same with p -+ w and 1 <= y <= h - 2.  (The clamp matters for
 * guided matches: a window minimum on the window's edge need not be a local minimum of the map.)
 *   uv f32 [B][2][N]     (x + dx, y + dy), pixel centres at the integers as (p % w, p / w); NaN in both planes for an unmatched row;
 *   counts int32 [B][4] = {matched, fitted on both axes, matched with the INTEGER pixel within thr of gt_xy, matched with the SUB-PIXEL
 *                        position within thr}; the predicate is cmr_feat_match_f32's: sqrtf(dx^2 + dy^2) <= thr in fp32, a non-finite
 *                        gt_xy is never an inlier; both inlier counts are 0 when gt_xy is null.  The call zeroes counts itself.
 * No workspace, no host round trip, no floating-point atomics: one memset and one launch on the stream; every uv element is a plain
 * store by the 16-lane group that owns the row and the counts are integer atomics (one per workgroup and word), so two calls agree bit
 * for bit and a sample depends on its own rows only. */
int cmr_match_subpixel_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const int32_t* idx,
                           const void* mask, int mask_bytes, const float* gt_xy, float thr, float* uv, int32_t* counts,
                           hipStream_t stream);

/* Pose scoring (port extension; ops.pose_score, MultiHeadModel.score_poses / search_pose, Test_Agent.py --verify /
 * --search, Test_Geo.py --verify): the truncated feature-metric cost of P candidate poses per sample in one sweep, with no ground truth.
 * pts f32 [B][3][N] (data['pc']), pc_feat rows [B*N][C], img_feat [B][h*w][C], C must be 64, mask [B*N] with mask_bytes 1 or 8, poses f32
 * [B][P][4][4] each mapping pts into the camera frame, 1 <= P <= 4096, K f32 [B][3][3] for the h x w map (h*w <= 2^24), 0 <= radius <= 16,
 * tau finite and > 0.  Per sample b, pose p and selected row n the quantities are cmr_guided_match_f32's, all in fp32 with the same
 * operations in the same order: X_c = R x + t, p = K X_c, u = p0 / p2, v = p1 / p2, centre (cx, cy) = (rint u, rint v), half to even; the
 * row is IN VIEW iff p2 > 0, u and v are finite and [cx - r, cx + r] x [cy - r, cy + r] meets the map (decided on the floats); dist =
 * sqrtf of the least direct sum of (a - b)^2 over the window clipped to the map (order: DESIGN.md 4n), +inf for a window without one
 * finite score.  Row cost: d = min(dist, tau) in fp32 if the row is in view, else d = tau; c = (double)d * (double)d.  So a row that is
 * out of view, behind the camera or under a NaN pose costs tau^2, the most a row can cost.
 *   score f64 [B][P]       the sum of c over the selected rows;
 *   counts int32 [B][P][2] = {in view, close = in view and dist <= tau};
 *   selected int32 [B]     the selected rows.  A sample without one gives score 0, counts 0, selected 0.
 * Two launches on the stream whatever P is, no memset, no atomics, no host round trip.  The float64 sum has a fixed order that depends
 * only on the sample's own rows and mask (256-row slices; inside a slice the selected rows in increasing n dealt to 16 groups, each
 * summing its rows in order, the groups added in order; then the slices in order): two calls agree bit for bit, a pose scored in a batch
 * of P equals the same pose scored alone bit for bit, and a sample depends on its own rows only.
 * Workspace: cmr_pose_score_workspace_bytes(B, N, P), 16-byte aligned. */
int64_t cmr_pose_score_workspace_bytes(int B, int N, int P);
int cmr_pose_score_f32(const float* pts, const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                       int mask_bytes, const float* poses, int P, const float* K, int radius, float tau, double* score, int32_t* counts,
                       int32_t* selected, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Point visibility and depth rendering under a pose (port extension; ops.visibility, MultiHeadModel.visible_points /
 * render_depth, refine_pose_from_matches / search_pose with visible=, Test_Geo.py / Test_Agent.py --visible): a one-cell z-buffer of the
 * cloud on the h x w map and, per queried row, the test of its depth against the nearest depth round its projection.  No features are
 * read, so h x w may be the 1/4-scale feature map or the full image (h*w <= 2^24).  pts f32 [B][3][N] (data['pc']), pose f32 [B][4][4]
 * mapping pts into the camera frame, K f32 [B][3][3] for the h x w map; mask [B*N] selects the rows that are QUERIED, occ_mask [B*N] the
 * rows that OCCLUDE (null: every row of the sample occludes); mask_bytes and occ_mask_bytes are 1 or 8 each (occ_mask_bytes is checked
 * even when occ_mask is null); 0 <= radius <= 16; rel_tol >= 0, abs_tol >= 0, both finite.  All of this is refused up front with
 * CMR_EINVAL; nothing depends on the data.
 * Per sample b and row n, all in fp32 with cmr_guided_match_f32's operations in the same order: X_c = R x + t, p = K X_c, u = p0 / p2,
 * v = p1 / p2, centre (cx, cy) = (rint u, rint v), half to even; the row is IN VIEW iff p2 > 0, u and v are finite, 0 <= cx <= w - 1 and
 * 0 <= cy <= h - 1 (decided on the floats: cmr_guided_match_f32's predicate at radius 0); its depth is z = p2.
 * Z[b][y][x] = the least z over the occluder rows in view whose centre is (x, y), +inf where there is none (an unsigned integer atomic
 * min on the bits of the positive floats: order independent).  A queried row that is not an occluder does not enter Z.
 * zmin = the least Z over the (2 radius + 1)^2 window round the row's own centre, clipped to the map; bound = zmin * opr + abs_tol with
 * opr = (float)(1.0 + (double)rel_tol), the product and the sum each rounded to fp32 (no fma); visible = selected and in view and
 * z <= bound.  An empty window has zmin = +inf and the row is visible.
 *   visible u8 [B*N]          0 for unselected rows;
 *   counts int32 [B][4]     = {selected, selected and in view, visible, occluder rows in view}; the call zeroes it;
 *   depth_map (optional) f32 [B][h*w] = Z; 4-byte aligned;
 *   cell (optional) int32 [B*N]  cy * w + cx for every row of mask | occ_mask that is in view, else -1;
 *   depth (optional) f32 [B*N]   z for the rows of mask | occ_mask with p2 > 0, else NaN.
 * A NaN pose gives nothing in view, Z all +inf and nothing visible; a sample without a selected row gives visible 0 and counts[0..2] 0.
 * Three launches on the stream whatever the data (fill of Z and counts, splat, test), no host round trip; every visible / cell / depth
 * element is a plain store by the thread that owns the row, Z is an integer atomic min, counts are integer atomics, one per workgroup
 * and word: two calls agree bit for bit and a sample depends on its own rows only.
 * Workspace: cmr_visibility_workspace_bytes(B, N, h, w), 16-byte aligned (holds Z, cell and depth where the caller passes none). */
int64_t cmr_visibility_workspace_bytes(int B, int N, int h, int w);
int cmr_visibility_f32(const float* pts, const void* mask, int mask_bytes, const void* occ_mask, int occ_mask_bytes, const float* pose,
                       const float* K, int B, int N, int h, int w, int radius, float rel_tol, float abs_tol, uint8_t* visible,
                       int32_t* counts, float* depth_map, int32_t* cell, float* depth, void* workspace, int64_t workspace_bytes,
                       hipStream_t stream);

/* Point painting and z-buffered attribute rendering under a pose (port extension; ops.paint_points / ops.render_points,
 * MultiHeadModel.paint_points / render_points, Test_Geo.py / Test_Agent.py --paint): the image laid over the cloud and the cloud laid
 * over the image.  Common to both: pts f32 [B][3][N] (data['pc']), pose f32 [B][4][4] mapping pts into the camera frame, K f32 [B][3][3]
 * for the H x W image / h x w map (1 <= H*W <= 2^24), mask [B*N] with mask_bytes 1 or 8 selecting the rows (null: every row; mask_bytes
 * is checked all the same); 1 <= B <= 65535, 1 <= N <= 65535 * 256.  Per selected row, in fp32 with cmr_guided_match_f32's operations
 * in the same order: X_c = R x + t, p = K X_c, u = p0 / p2, v = p1 / p2; the row is IN VIEW iff p2 > 0, u and v are finite,
 * 0 <= rint u <= W - 1 and 0 <= rint v <= H - 1 (half to even, decided on the floats: cmr_visibility_f32's predicate and cell).
 * Anything outside the contract is refused up front with CMR_EINVAL; nothing depends on the data.
 *
 * cmr_paint_points_f32: image f32 planar [B][C][H][W], 1 <= C <= 64, values expected finite; PAINTED = selected and in view.
 *   mode 0 (nearest): the value is the pixel (rint u, rint v).
 *   mode 1 (bilinear): pixel centres on the integers; x0 = floorf u, fx = u - x0 (likewise y); the four taps (x0, y0) .. (x0 + 1, y0 + 1)
 *     with every index clamped to the image (border replicate: a row up to half a pixel outside the outermost centres is in view and reads
 *     the edge); lerp(a, b, t) = a + t * (b - a) with the difference, the product and the sum each rounded to fp32 (no fma);
 *     value = lerp(lerp(I00, I01, fx), lerp(I10, I11, fx), fy).
 *   colors f32 [B][C][N]    0 on the rows that are not painted;
 *   painted u8 [B*N];
 *   counts int32 [B][2]   = {selected, painted}; the call zeroes it;
 *   uv (optional) f32 [B][2][N] = (u, v) as computed; NaN for unselected rows and where p2 <= 0 (cmr_guided_match_f32's proj).
 * A NaN pose paints nothing.  Two launches on the stream (zero of counts, paint), no workspace, no host round trip; every colors /
 * painted / uv element is a plain store by the thread that owns the row and counts are integer atomics, one per workgroup and word.
 *
 * cmr_render_points_f32: every selected row in view goes to the cell (rint u, rint v) with the 64-bit key (bits of z = p2) << 32 | n; a
 * cell keeps the least key (one unsigned 64-bit atomic min per row: positive floats order like their bits, so the nearest row wins and
 * equal depths go to the lowest n, whatever the order of arrival).  0 <= splat <= 4 is a square footprint: a pixel's key is the least key
 * of the cells within splat of it in both axes, clipped to the map (taken as a window minimum when the maps are written).
 *   index_map int32 [B][h*w]  the owning row n, -1 where there is none;
 *   depth_map f32 [B][h*w]    the owner's z, +inf where there is none;
 *   attr_map (optional, with attr f32 [B][C][N], 1 <= C <= 64; both or neither, C = 0 without) f32 [B][C][h*w] = attr[b][c][owner],
 *     `fill` (any float, NaN included) where there is none;
 *   counts int32 [B][3]     = {selected, selected and in view, pixels with an owner}; the call zeroes it.
 * Three launches on the stream whatever the data (fill of the key map and counts, splat, resolve), no memset, no host round trip, no
 * floating-point atomic: two calls agree bit for bit and a sample depends on its own rows only.
 * Workspace: cmr_render_points_workspace_bytes(B, h, w), 16-byte aligned (the key map). */
int cmr_paint_points_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* image, int B,
                         int N, int C, int H, int W, int mode, float* colors, uint8_t* painted, int32_t* counts, float* uv,
                         hipStream_t stream);
int64_t cmr_render_points_workspace_bytes(int B, int h, int w);
int cmr_render_points_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* attr, int C,
                          int B, int N, int h, int w, int splat, float fill, int32_t* index_map, float* depth_map, float* attr_map,
                          int32_t* counts, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Oriented-disc (surfel) rendering of the cloud from its normals, and the depth test against a map the caller brings (port extension,
 * DESIGN.md 4z; ops.render_surfels / ops.depth_test, MultiHeadModel.render_surfels, dense_depth(surfels=), visible=dict(surfels=...)).
 * Every selected point is drawn as a disc in space: centred on the point, perpendicular to its normal, r metres wide; every pixel of
 * its window intersects its own ray with the disc's plane.  pts f32 [B][3][N] (data['pc']); normals f32 [B][3][N] in the cloud's frame,
 * any length (the zero vector = no normal); mask [B*N] with mask_bytes 1 or 8 (null: every row; mask_bytes is checked all the same);
 * pose f32 [B][4][4] mapping pts into the camera frame; K f32 [B][3][3] for the h x w map, 1 <= h*w <= 2^24; radius >= 0 and
 * range_slope >= 0, both finite; 0 <= max_px <= 16; 0 <= min_cos <= 1; attr f32 [B][C][N] with attr_map, 1 <= C <= 64 (both or
 * neither, C = 0 without); fill any float; 1 <= B <= 65535, 1 <= N <= 65535 * 256.  Anything else is refused up front with CMR_EINVAL;
 * nothing depends on the data, and K is never read on the host.
 * Camera model: fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5].  A sample whose K does not have K[3] = 0, K[6] = K[7] = 0,
 * K[8] = 1 and fx, fy finite and > 0 draws nothing and reports status 1.
 * Per selected row n, in fp32:
 *   X_c = (x_c, y_c, z_c) = R x + t and p = K X_c, u = p0 / p2, v = p1 / p2 by cmr_guided_match_f32's fmaf chains (so z_c = p2 under
 *     the camera model, and the centre's cell agrees bit for bit with the other pose operations);
 *   n_c = R n by the same pattern without the translation: n_cx = fmaf(R00, nx, fmaf(R01, ny, R02 * nz)), likewise y and z;
 *   r = range_slope * z_c + radius, the product and the sum each rounded (no fma).
 * The row is DRAWN iff it is selected, p2 > 0, u and v are finite, the (2 max_px + 1)^2 window round (rint u, rint v) touches the map
 * (cmr_guided_match_f32's predicate at radius max_px: the centre itself may lie outside), the three floats of its normal are finite, r is
 * finite and > 0, and z_c > r (no part of the disc reaches the camera plane).
 * Per pixel (x, y) of a drawn row's window that lies inside the map, pixel centres on the integers, every operation below a plain fp32
 * operator rounded on its own (no fma), n = n_c:
 *   dy = (y - cy) / fy;   dx = ((x - cx) - s * dy) / fx;   n2 = (nx * nx + ny * ny) + nz * nz;
 *   if n2 == 0 (no normal: fronto-parallel):  tau = z_c;  o = (tau * dx - x_c, tau * dy - y_c, 0);
 *   else:  nd = (nx * dx + ny * dy) + nz;  nX = (nx * x_c + ny * y_c) + nz * z_c;  tau = nX / nd;
 *          rejected unless nd != 0, tau finite and tau > 0;
 *          rejected unless nd * nd >= ((min_cos * min_cos) * n2) * ((dx * dx + dy * dy) + 1)   (the grazing cap: the cosine between the
 *          ray and the normal is at least min_cos; no square root, no unit normal);
 *          o = (tau * dx - x_c, tau * dy - y_c, tau - z_c);
 *   COVERED iff (ox * ox + oy * oy) + oz * oz <= r * r (the rim is inclusive).  The pixel's depth under this row is tau.
 * A pixel keeps the least 64-bit key (bits of tau) << 32 | n over the rows that cover it (one unsigned 64-bit atomic min; positive
 * floats order like their bits): the nearest surfel wins, equal depths go to the lowest n, the order of arrival is irrelevant.
 * The window walked is smaller than (2 max_px + 1)^2 where it provably holds every covered pixel.  A covered pixel's ray meets the disc
 * at Q = X_c + o with |o| <= r, so Q_z >= z_c - r > 0, and Q_y / Q_z - y_c / z_c = (o_y - (y_c / z_c) o_z) / Q_z, at most
 * r sqrt(1 + (y_c / z_c)^2) / (z_c - r) <= r (1 + |y_c / z_c|) / (z_c - r) in size; likewise in x.  With x = cx + fx Q_x / Q_z + s Q_y / Q_z
 * the pixel lies within hx = (fx (1 + |x_c / z_c|) + |s| (1 + |y_c / z_c|)) r / (z_c - r) of u and within hy = fy (1 + |y_c / z_c|) r /
 * (z_c - r) of v (f r / z_c alone is too small off the axis and for a disc that is near).  fp32 rounding moves the rim by a small
 * fraction of a pixel, so both are widened by 2^-12 of themselves and by one pixel: the walk covers floor(u - hx) .. ceil(u + hx)
 * by floor(v - hy) .. ceil(v + hy), cut to the (2 max_px + 1)^2 window and to the map.
 *   index_map int32 [B][h*w]   the owning row, -1 where there is none;
 *   depth_map f32 [B][h*w]     the owner's tau at that pixel, +inf where there is none;
 *   normal_map (optional) f32 [B][3][h*w]: the owner's n_c / sqrtf(n2) (correctly rounded square root and divisions), negated when
 *     nX > 0 so that it faces the camera; (0, 0, -1) for a zero normal; 0 where there is no owner;
 *   attr_map f32 [B][C][h*w] = attr[b][c][owner], `fill` where there is none;
 *   counts int32 [B][4]      = {selected, drawn, pixels with an owner, status}; the call writes all four;
 *   surfel (optional) f32 [B][8][N] = (x_c, y_c, z_c, n_cx, n_cy, n_cz, r, drawn as 0 / 1) as computed, NaN in the first seven planes of
 *     the rows that are not drawn: a float32 restatement of the per-pixel part started from it gives index_map and depth_map bit for bit.
 * Accuracy of tau against exact arithmetic on the same inputs, u = 2^-24, for r <= z_c / 2: a term of nd carries at most 7 roundings
 * (the four of dx, its product, two sums), the terms sum to at most sqrt(3) |n| |d| in size (d = (dx, dy, 1)), and the grazing cap gives
 * |nd| >= min_cos |n| |d|: at most 7 sqrt(3) u / min_cos < 12.2 u / min_cos relative.  A term of nX carries 3 (its product, two sums) and
 * the terms sum to at most sqrt(3) |n| |X_c|, with
 * |X_c| <= tau |d| + r <= 2 tau |d| and |nX| = tau |nd|: at most 6 sqrt(3) u / min_cos < 10.4 u / min_cos.  The division adds u.  In all
 * |tau - exact| <= 24 u tau / min_cos = 12 2^-23 tau / min_cos to first order; the tests allow c = 16: 16 2^-23 tau / min_cos.  The error
 * X_c itself carries (three fmas per component: 3 u S_j, S_j = sum_k |R_jk| |x_k| + |t_j|) moves tau by at most |n| |dX| / |nd| <=
 * 3 sqrt(3) u max_j S_j / min_cos; the tests allow 8 2^-23 max_j S_j / min_cos for it, cmr_visibility_f32's projection term.
 * Three launches on the stream whatever the data (fill of the key map and counts, splat, resolve), no memset, no host round trip, no
 * floating-point atomic; every output element is a plain store by the thread that owns it, the key map is an integer atomic min, counts
 * are integer atomics, one per workgroup and word: two calls agree bit for bit and a sample depends on its own rows only.
 * Workspace: cmr_render_surfels_workspace_bytes(B, h, w), 16-byte aligned (the key map).
 *
 * cmr_depth_test_f32: cmr_visibility_f32's test against a z-buffer the caller brings -- Z f32 [B][h*w], 4-byte aligned, +inf = empty, a
 * NaN cell is ignored -- e.g. the depth_map above.  pts, mask (not null here: the rows that are queried), mask_bytes, pose, K, radius
 * 0 .. 16, rel_tol and abs_tol are cmr_visibility_f32's; the projection, the in-view predicate (radius 0), the window minimum zmin over
 * the (2 radius + 1)^2 cells clipped to the map and bound = zmin * opr + abs_tol, opr = (float)(1.0 + (double)rel_tol), the product and
 * the sum rounded separately, are its operations: handed cmr_visibility_f32's own depth_map it returns that call's `visible` bit for
 * bit.  K is used as cmr_visibility_f32 uses it (all nine entries; no camera-model check).
 *   visible u8 [B*N]          0 for unselected rows;
 *   counts int32 [B][3]     = {selected, selected and in view, visible}; the call zeroes it.
 * Two launches on the stream (zero of counts, test), no workspace, no host round trip. */
int64_t cmr_render_surfels_workspace_bytes(int B, int h, int w);
int cmr_render_surfels_f32(const float* pts, const float* normals, const void* mask, int mask_bytes, const float* pose, const float* K,
                           const float* attr, int C, int B, int N, int h, int w, float radius, float range_slope, int max_px, float min_cos,
                           float fill, int32_t* index_map, float* depth_map, float* normal_map, float* attr_map, int32_t* counts,
                           float* surfel, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cmr_depth_test_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* Z, int B, int N,
                       int h, int w, int radius, float rel_tol, float abs_tol, uint8_t* visible, int32_t* counts, hipStream_t stream);

/* Pose scoring by mutual information (port extension; ops.pose_mi, MultiHeadModel.score_poses_mi, Test_Geo.py /
 * Test_Agent.py --verify-mi): per candidate pose the joint histogram of a per-point attribute (the LiDAR reflectance) and the grey value
 * of the pixel the point lands on, its entropies and the mutual information (Pandey et al., targetless camera-LiDAR calibration) -- a
 * score that reads the sensors alone, not the geometric model's features.  pts f32 [B][3][N] (data['pc']), attr f32 [B][N], mask [B*N]
 * with mask_bytes 1 or 8 (null: every row; mask_bytes is checked all the same), poses f32 [B][P][4][4] each mapping pts into the camera
 * frame, 1 <= P <= 4096, K f32 [B][3][3] for the H x W image, grey f32 [B][H][W] (one plane, 1 <= H*W <= 2^24), mode 0 (nearest) or 1
 * (bilinear) with cmr_paint_points_f32's meaning, 2 <= bins = nb <= 64, a_lo < a_hi and g_lo < g_hi all finite and such that
 * nb / (hi - lo) is finite in fp32; hist 16-byte aligned; 1 <= B <= 65535, 1 <= N <= 65535 * 256.  Anything else is refused up front
 * with CMR_EINVAL; nothing depends on the data.
 * Per sample b, pose p and selected row n: IN VIEW is cmr_paint_points_f32's predicate under that pose (cmr_visibility_f32's cell), and
 * the row's grey value g is, bit for bit, what cmr_paint_points_f32 returns for it at C = 1 in the same mode.  The row is COUNTED iff it
 * is in view and attr[b][n] and g are both finite.  bin(x, lo, scale) = min(nb - 1, max(0, (int)floorf((x - lo) * scale))), the
 * difference and the product two separately rounded fp32 operations (no fma), scale = nb / (hi - lo) computed in double and rounded
 * once to fp32; values outside [lo, hi] go to the end bins.
 *   hist int32 [B][P][nb][nb]  hist[ba][bg] = the counted rows with attribute bin ba and grey bin bg; always produced (it is the
 *                              workspace);
 *   counts int32 [B][P][2]   = {in view, counted};
 *   selected int32 [B]         the selected rows;
 *   entropy f64 [B][P][3]    = {H_a, H_g, H_ag} in nats, each H = ln n - (sum of c ln c) / n over the non-zero marginal / joint counts,
 *                              n = the counted rows; the marginals are exact integer sums;
 *   mi f64 [B][P]            = (H_a + H_g) - H_ag.  n = 0 gives zeros everywhere; a NaN pose counts nothing.
 * Three launches on the stream whatever the data (fill of hist / counts / selected, histogram, entropies), no host round trip, no
 * floating-point atomic: every sum that crosses threads is an integer (LDS and global integer atomics), so hist and counts do not
 * depend on B, P, the chunking of the poses, the slicing of the rows or the order of the atomics -- two calls agree bit for bit, a pose
 * scored alone equals the same pose in a batch of P, and a sample depends on its own rows only.  Order of the float64 sums of c ln c (it
 * depends on nb alone): joint -- thread t of 256 adds the cells t, t + 256, ... of the flat index ba * nb + bg in increasing order from
 * 0.0, then the 256 partial sums fold as a binary tree, v[t] += v[t + s] for s = 128, 64, ..., 1; each marginal -- its nb terms in
 * increasing bin order from 0.0. */
int cmr_pose_mi_f32(const float* pts, const float* attr, const void* mask, int mask_bytes, const float* poses, int P, const float* K,
                    const float* grey, int B, int N, int H, int W, int mode, int bins, float a_lo, float a_hi, float g_lo, float g_hi,
                    int32_t* hist, int32_t* counts, int32_t* selected, double* entropy, double* mi, hipStream_t stream);

/* Image-guided densification of a sparse depth / attribute map (port extension; ops.densify, MultiHeadModel.dense_depth,
 * Test_Geo.py / Test_Agent.py --dense-depth): the joint bilateral filter as a normalised convolution.  All maps contiguous.
 *   depth f32 [B][h][w]: a pixel is a SAMPLE iff its depth is finite and > 0 (+inf, as cmr_render_points_f32 and cmr_visibility_f32 write
 *     it, 0, negatives and NaN are empty); attr f32 [B][C][h][w], 1 <= C <= 4, or null with C = 0, read at samples only; guide f32
 *     [B][Cg][h][w], 1 <= Cg <= 4, or null with Cg = 0, expected finite (not checked); 0 <= radius <= 16; sigma_s > 0; sigma_r > 0
 *     (ignored without a guide); min_weight finite and >= 1e-24; keep 0 or 1; fill any float; 1 <= h*w <= 2^24; 1 <= B <= 65535.
 * For pixel p and every sample q of the map with |qx - px| <= radius and |qy - py| <= radius:
 *   w(p, q) = exp(-(|p - q|^2 / (2 sigma_s^2) + sum_c (G_c(p) - G_c(q))^2 / (2 sigma_r^2)))   (the second term only with a guide),
 *   S0 = sum w, S1 = sum w z(q), A_c = sum w a_c(q), n = the number of such samples; the sums run line by line, left to right, in fp32,
 *   one hardware exponential per sample (weights below 2^-126 count as 0).
 * The pixel is FILLED iff S0 >= min_weight.  keep = 1: a pixel that is a sample returns its own depth and attributes bit for bit.
 *   dense_depth f32 [B][h][w]      = S1 / S0 where filled, +inf elsewhere
 *   dense_attr f32 [B][C][h][w]    = A_c / S0 where filled, `fill` elsewhere; null iff attr is null
 *   conf f32 [B][h][w]             = S0 as computed, 0 where n = 0
 *   count int32 [B][h][w] or null  = n
 *   counts int32 [B][3]            = {samples in the map, pixels with n > 0, filled pixels}; the call zeroes it (integer atomics)
 * Two launches on the stream whatever the data (zero of counts, the tiled gather), no workspace, no host round trip, no floating-point
 * atomic: two calls agree bit for bit and a sample's result depends on its own maps only.  Anything outside the contract is refused up
 * front with CMR_EINVAL. */
int cmr_densify_f32(const float* depth, const float* attr, int C, const float* guide, int Cg, int B, int h, int w, int radius,
                    float sigma_s, float sigma_r, float min_weight, int keep, float fill, float* dense_depth, float* dense_attr,
                    float* conf, int32_t* count, int32_t* counts, hipStream_t stream);

/* ---- rollout ops of the training loop ---------------------------------------- */

/* environment.py:143-176 (expert): residual pose target * source^-1 -> extrinsic-xyz Euler angles (folded back when the
 * x angle exceeds 3 rad) and translation -> nearest entries of the float64 step tables.  act_r int64 [B,1] / act_t [B,2]
 * (six_dof = 0: y rotation, x / z translation) or [B,3] each. */
int cmr_expert_action_f32(const float* pose_source, const float* pose_target, const double* r_steps, const double* t_steps,
                          int num_steps, int six_dof, int64_t* act_r, int64_t* act_t, int B, hipStream_t stream);
/* environment.py:263-302 (reward): distance[b] = mean over mask[b] != 0 of |pc_in_cam - (pc - centroid(pc))|^2 on planar
 * [B,3,N] clouds; reward[b] = +0.5 / -0.5 / 0 against prev_distance[b] (0 when prev_distance is NULL). */
int cmr_reward_f32(const float* pc, const float* pc_in_cam, const int64_t* mask, const float* prev_distance, float* distance,
                   float* reward, int B, int N, hipStream_t stream);
/* buffer.py:24-33 (discounted): out[r][i] = vals[r][i] + gamma * out[r][i+1] over rows of length T. */
int cmr_discounted_f32(const float* vals, float* out, float gamma, int64_t rows, int T, hipStream_t stream);

/* ---- point-cloud ops ----------------------------------------------------------------------- */

/* planar [B,C,N] (the reference's point layout) -> rows [B*N, Cpad], Cpad in {4, 8}, zero padded. */
int cmr_planar_to_rows_f32(const float* x, float* y, int B, int C, int N, int Cpad, hipStream_t stream);
/* out[r] = [x1[r] | x2[map(r)]]: a materialised torch.cat for the one consumer that needs it as a
 * residual (CMRAgent.py:97-99 feeding the identity shortcut of state_3d_embed[3]). */
int cmr_concat_rows_f32(const float* x1, int64_t ld1, int C1, const float* x2, int64_t ld2, int C2, const int32_t* idx2,
                        int64_t div2, float* out, int64_t rows, hipStream_t stream);
int cmr_index_to_global_i32(const int64_t* idx, int32_t* out, int B, int N, int M, hipStream_t stream);

/* CSR of the points owned by each node (replaces the expanded-index torch_scatter calls,
 * PointNN.py:171,175,182; third-party torch_scatter, version unpinned in the reference). */
int cmr_csr_build_i32(const int32_t* key, int32_t* count, int32_t* offsets, int32_t* order, int B, int n_per_batch,
                      int seg_per_batch, hipStream_t stream);

/* 16 nearest nodes of every node, ascending distance.  PointNN.py:215-216 (square_distance + argsort). */
int cmr_knn16_f32(const float* xyz4, int32_t* out, int B, int M, hipStream_t stream);

/* K nearest candidates (rows c4 [B*N,4]) of every query (rows q4 [B*S,4]), 1 <= K <= 64: out int64 [B,S,K] = LOCAL candidate indices in
 * ascending distance, equal distances in ascending index -- square_distance(new_xyz, xyz).argsort()[:, :, :K] of pointnet_util.py:114-116
 * (sample_and_group, knn=True) and :232-234 (PointNetSetAbstractionMsg).  N < K: the missing entries are -1. */
int cmr_knn_f32(const float* q4, const float* c4, int64_t* out, int B, int S, int N, int K, hipStream_t stream);

/* nearest candidate per query.  PointViT.py:85-87 (node -> proxy), dataset/KittiDataset.py:366-367 (point -> node). */
int cmr_nearest_f32(const float* q4, const float* c4, int32_t* out_global, int64_t* out_local, int B, int Nq, int Nc,
                    hipStream_t stream);

/* out[r] = a[map_a(r)] - b[map_b(r)] (xyz rows).  PointNN.py:164-166, :223. */
int cmr_rel_pos_f32(const float* a, const int32_t* ia, int64_t diva, const float* b, const int32_t* ib, int64_t divb,
                    float* out, int64_t rows, hipStream_t stream);

/* t = q[map_q] - k[map_k] + pos ; vp = v[map_k] + pos.  PointNN.py:162,168,179 and :220,225,228. */
int cmr_vecattn_prep_f32(const float* q, int64_t ldq, const int32_t* iq, int64_t divq, const float* k, int64_t ldk,
                         const float* v, int64_t ldv, const int32_t* ik, const float* pos, float* t, float* vp,
                         int64_t rows, hipStream_t stream);

/* per-segment, per-channel softmax(attn*scale) weighted sum of vp.  PointNN.py:170-182 and :226-228. */
int cmr_segment_softmax_f32(const float* attn, const float* vp, const int32_t* order, const int32_t* offsets,
                            int fixed_len, float scale, float* out, int64_t nseg, hipStream_t stream);

/* torch_scatter.scatter_{sum,max,mean} over CSR segments (mode 0 / 1 / 2; empty segments -> 0): the op API of the
 * third-party extension the reference calls at PointNN.py:171-182 and environment.py:79. */
int cmr_segment_reduce_f32(const float* src, int64_t lds, const int32_t* order, const int32_t* offsets, float* out,
                           int64_t ldo, int64_t nseg, int C, int mode, hipStream_t stream);

/* out[r,:C] = src[idx[r],:C].  pointnet_util.py:36-47 (index_points), torch.gather of feature rows. */
int cmr_gather_rows_f32(const float* src, int64_t lds, const int32_t* idx, float* out, int64_t ldo, int64_t rows, int C,
                        hipStream_t stream);

/* pointnet_util.py:50-70 (start index explicit), :73-93, :19-33.  start[b] outside [0, N) is forced into the cloud (the
 * reference raises IndexError at xyz[batch_indices, farthest]; a kernel cannot, and must not read outside the cloud). */
int cmr_fps_f32(const float* xyz4, const int64_t* start, int64_t* out, int B, int N, int npoint, hipStream_t stream);
/* The same sampling with several workgroups per cloud (slices in registers, one 64-bit atomic max + an arrival counter per
 * round; bit-identical indices): for clouds above 16 384 points (BASELINE configs[4]: 65 536), B * groups <= 256.  ws = scratch of
 * cmr_fps_workspace_bytes.  The waits between the workgroups of a cloud are bounded; a cloud whose workgroups could not all
 * become resident in time (CU-filling kernels of another stream) is recomputed by ONE workgroup in the same call (repair
 * launch behind the cooperative one; no host round trip, capturable), so `out` always holds the reference's indices.  After
 * the call the int32 word at ws + B*npoint*8 + 4*(B + b) is 0 (cloud b sampled cooperatively) or 2 (repaired). */
int64_t cmr_fps_workspace_bytes(int B, int N, int npoint);
int cmr_fps_ws_f32(const float* xyz4, const int64_t* start, int64_t* out, int B, int N, int npoint, void* ws, int64_t ws_bytes,
                   hipStream_t stream);
/* The same call with the spin bound as an argument (polls per round before a workgroup gives its cloud up; 0 = give up at once):
 * lets a caller trade waiting for the repair pass, and lets the tests drive the repair path on purpose. */
int cmr_fps_ws_spin_f32(const float* xyz4, const int64_t* start, int64_t* out, int B, int N, int npoint, void* ws, int64_t ws_bytes,
                        int spin_limit, hipStream_t stream);
int cmr_ball_query_f32(const float* xyz4, const float* new4, int64_t* out, int B, int N, int S, int nsample,
                       float radius2, hipStream_t stream);
int cmr_square_distance_f32(const float* a4, const float* b4, float* out, int B, int N, int M, hipStream_t stream);

/* pointnet_util.py:287-296 (PointNetFeaturePropagation): 3 nearest of xyz2 + inverse-distance weights, then
 * the weighted sum of their feature rows. */
int cmr_three_nn_f32(const float* q4, const float* c4, int32_t* idx, float* wgt, int B, int Nq, int Nc,
                     hipStream_t stream);
int cmr_weighted_gather3_f32(const float* src, int64_t lds, const int32_t* idx, const float* wgt, float* out, int64_t ldo,
                             int64_t rows, int C, hipStream_t stream);
/* its backward w.r.t. src (train-mode PointNetFeaturePropagation): out[t] = sum of wgt[e] * dy[e / 3] over the entries e of idx that name
 * row t, in ascending e through the CSR (offsets, order) of idx over the nseg source rows (cmr_csr_build_i32): deterministic, no atomics. */
int cmr_weighted_scatter3_f32(const float* dy, int64_t ldd, const float* wgt, const int32_t* order, const int32_t* offsets, float* out,
                              int64_t ldo, int64_t nseg, int C, hipStream_t stream);

/* per-batch max / mean over rows.  CMRAgent.py:95 (torch.max over points), environment.py:46,88 (pc.mean). */
int64_t cmr_colreduce_workspace_bytes(int B, int N, int C);
int cmr_colmax_f32(const float* x, int64_t ldx, float* out, void* ws, int64_t ws_bytes, int B, int N, int C,
                   hipStream_t stream);
int cmr_colmean_f32(const float* x, int64_t ldx, float* out, void* ws, int64_t ws_bytes, int B, int N, int C,
                    hipStream_t stream);

/* ---- agent iteration ------------------------------------------------------------------------ */

/* environment.py:24-126: projection, in-frustum test, scatter-mean numerator/denominator, state_3d.  acc [B*h*w][64] and
 * cnt [B*h*w] must be zero on entry: zero_first = 1 clears them here (two memsets), zero_first = 0 relies on the caller
 * (cmr_observation_finalize_f32 with clear = 1 re-zeroes exactly the cells that were hit). */
int cmr_project_scatter_f32(const float* pc4, const float* feat, const uint8_t* overlap, const float* pose,
                            const float* Kmat, const float* mean4, float* acc, float* cnt, float* state3d, int B, int N,
                            int h, int w, int zero_first, hipStream_t stream);
/* state2d = [img_feat | acc / max(cnt,1)]; proj (optional) receives the second half alone as [B,h,w,64].  state2d may be null
 * when proj is given (a caller that consumes the two halves separately, as CMRAgent's first convolution does: the 128-channel
 * map is then neither written nor is img_feat read).  clear = 1: cells with cnt > 0 are reset to zero after they have been read. */
int cmr_observation_finalize_f32(const float* img_feat, float* acc, float* cnt, float* state2d, float* proj,
                                 int B, int h, int w, int write_img, int clear, hipStream_t stream);
/* The projected half of the observation alone, maintained in place across the steps of a registration (inference loops that hand the two
 * halves of state_2d to CMRAgent separately; environment.observation_from_a_pose(materialize_state_2d = False)): proj [B,h,w,64], cnt
 * [B*h*w] and cell [B*N] (int32, the cell of every point in the previous call, -1 = none) are STATE owned by the caller -- zero / zero / -1
 * before the first call, untouched between calls.  Each call zeroes the cells of the previous call per point, projects with `pose`, writes
 * state3d [B*N,8] like cmr_project_scatter_f32 and adds feat / count into the cells hit now: proj = scatter_mean (environment.py:39-80) with
 * the mean formed as a sum of pre-divided terms, cells without points 0.  Three launches over the points; the full map is never swept. */
int cmr_observation_proj_f32(const float* pc4, const float* feat, const uint8_t* overlap, const float* pose, const float* Kmat,
                             const float* mean4, float* proj, float* cnt, int32_t* cell, float* state3d, int B, int N, int h, int w,
                             hipStream_t stream);
/* ... and, in the same launches, the reach of the cells hit now on the 8x16 tile grid of the stride-1 convolutions that read proj: byte maps
 * reach1 / reach2 [B][ceil(h / 8)][ceil(w / 16)] (both or neither) receive a 1 for every tile whose area dilated by 1 / 2 pixels holds such a
 * cell.  Zero before the first call; cmr_wino_tile_lists consumes and clears them. */
int cmr_observation_proj_reach_f32(const float* pc4, const float* feat, const uint8_t* overlap, const float* pose, const float* Kmat,
                                   const float* mean4, float* proj, float* cnt, int32_t* cell, float* state3d, int B, int N, int h, int w,
                                   uint8_t* reach1, uint8_t* reach2, hipStream_t stream);
/* ... and the reach on the tile grid of the half-resolution stage behind them (two more 3x3 convolutions on the 2 x 2 pooled map; its 8x16
 * tiles cover 16 x 32 cells): reach3 / reach4 [B][ceil(h / 16)][ceil(w / 32)] (both or neither, with reach1 / reach2; h, w, h / 2, w / 2
 * even) receive a 1 for every tile whose 16 x 32 footprint dilated by 4 / 6 cells holds a cell hit now.  cmr_wino_tile_lists_staged
 * consumes and clears all four. */
int cmr_observation_proj_reach_staged_f32(const float* pc4, const float* feat, const uint8_t* overlap, const float* pose, const float* Kmat,
                                          const float* mean4, float* proj, float* cnt, int32_t* cell, float* state3d, int B, int N, int h,
                                          int w, uint8_t* reach1, uint8_t* reach2, uint8_t* reach3, uint8_t* reach4, hipStream_t stream);
/* environment.py:179-260 (step + euler_angles_to_matrix 'XYZ'), :14-21 (to_disentangled). */
int cmr_pose_step_f32(float* pose, const int64_t* act_r, const int64_t* act_t, const double* r_steps,
                      const double* t_steps, int B, int six_dof, hipStream_t stream);
int cmr_to_disentangled_f32(float* pose, const float* mean4, int B, hipStream_t stream);
/* CMRAgent.py:118-127 (deterministic action = argmax). */
int cmr_argmax_rows_f32(const float* x, int64_t* out, int outer, int inner, int n, int64_t stride_outer,
                        int64_t stride_inner, hipStream_t stream);
/* MultiHeadModel.py:330-341 (softmax over 2 classes, thresholds .5/.8). */
int cmr_softmax2_f32(const float* logits, int64_t ld, float* prob, uint8_t* pred_lo, uint8_t* pred_hi, float thr_lo,
                     float thr_hi, int64_t rows, hipStream_t stream);
/* MultiHeadModel.py:233,241 (F.normalize over channels). */
int cmr_l2norm64_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, hipStream_t stream);

/* ---- agent update: training-mode forward, backward, optimizer ------------------ */
/* The reference trains CMRAgent with `agent.train(); loss.backward(); optimizer.step()` on minibatches of 10 buffered
 * samples (Train_Agent.py:256-305).  There is no FFI to mirror; these entry points are what the Python host layer
 * (cmr_agent_amd/train/agent_update.py) calls in place of torch autograd.  Data-gradient contractions reuse the forward
 * entry points (cmr_conv3x3_wino_nhwc_f32 / cmr_conv3x3_nhwc_f32 / cmr_linear_f32) with transposed weights. */

/* nn.BatchNorm2d / nn.BatchNorm1d in train() mode (CMRAgent.py:35,41,47,53; PointNN.py:265,268,277 via CMRAgent.py:25-29)
 * over a row map x [rows, C]: batch mean / biased variance per channel; stat [4][C] = (mean, rstd, gamma*rstd,
 * beta - mean*gamma*rstd); running_mean / running_var (optional) are updated with `momentum` and the unbiased variance. */
int64_t cmr_bn_workspace_bytes(int64_t rows, int C);
int cmr_bn_stats_f32(const float* x, int64_t ldx, int64_t rows, int C, float eps, float momentum, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float* stat, void* ws, int64_t ws_bytes,
                     hipStream_t stream);
/* BatchNorm statistics from partial sums a producer left (cmr_conv3x3_wino_stats_nhwc_f32): part [parts][2][C] = sums of (x - pivot[c]) and
 * (x - pivot[c])^2 over disjoint row sets covering all `rows` rows (pivot null = 0); stat [4][C] and the running statistics exactly as
 * cmr_bn_stats_f32 leaves them. */
/* cmr_bn_bwd_f32 (z null: mask from the sign of x * stat[2] + stat[3]; no add / masked output) with the reduction's partial sums given:
 * part [parts][2][C] as cmr_conv3x3_wino_bnbwd_nhwc_f32 leaves them.  ws: 2 C floats. */
int cmr_bn_bwd_from_sums_f32(const float* dz, int64_t lddz, float slope, const float* x, int64_t ldx, const float* stat, const float* part,
                             int64_t parts, float* dx, int64_t lddx, float* dgamma, float* dbeta, int64_t rows, int C, void* ws, int64_t ws_bytes,
                             hipStream_t stream);
int cmr_bn_stats_from_sums_f32(const float* part, int64_t parts, int64_t rows, int C, const float* pivot, float eps, float momentum,
                               const float* gamma, const float* beta, float* running_mean, float* running_var, float* stat, hipStream_t stream);
/* y = LeakyReLU_slope(x * scale + shift + (res * rscale + rshift | res)): BatchNorm application + activation, and the
 * `final_relu(net(x) + shortcut(x))` of ConvBNReLURes1D (PointNN.py:282).  Null scale / rscale = identity; slope 1 = none. */
int cmr_affine_act_f32(const float* x, int64_t ldx, const float* scale, const float* shift, const float* res, int64_t ldres,
                       const float* rscale, const float* rshift, float* y, int64_t ldy, int64_t rows, int C, float slope,
                       hipStream_t stream);
/* Backward of [BatchNorm(train) -> LeakyReLU]: dz = gradient w.r.t. the activation output z, x = the BatchNorm input, stat from
 * cmr_bn_stats_f32.  z null: slope 1 = no activation; slope != 1 = the activation sat directly on the BatchNorm output (no residual in
 * between) and its mask is taken from the sign of x * scale + shift, recomputed with cmr_affine_act_f32's own fused multiply-add (the
 * stored output is then not read: one map pass less in each of the two sweeps; CMR_EINVAL unless 0 <= slope <= 1, the range in which that
 * sign is the forward's mask -- a caller with a residual in front of the activation MUST pass z).  dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) (+ add),
 * dgamma = sum dy xhat, dbeta = sum dy (written when non-null).  dzm (optional): receives dy = dz * act'(z), the gradient at the
 * activation's input -- what a residual branch added in front of the activation gets (`lrelu(BN(x) + res)`, ImageResNet.py:36-40,
 * PointNN.py:282), from the same pass instead of a separate activation-backward sweep. */
int64_t cmr_bn_bwd_workspace_bytes(int64_t rows, int C);
int cmr_bn_bwd_f32(const float* dz, int64_t lddz, const float* z, int64_t ldz, float slope, const float* x, int64_t ldx,
                   const float* stat, const float* add, int64_t ldadd, float* dx, int64_t lddx, float* dzm, int64_t lddzm,
                   float* dgamma, float* dbeta, int64_t rows, int C, void* ws, int64_t ws_bytes, hipStream_t stream);
/* The reduction half of cmr_bn_bwd_f32 alone (same workspace): coef [2][C] = (mean(dy), mean(dy xhat)), dgamma, dbeta. */
int cmr_bn_bwd_coef_f32(const float* dz, int64_t lddz, const float* z, int64_t ldz, float slope, const float* x, int64_t ldx,
                        const float* stat, float* coef, float* dgamma, float* dbeta, int64_t rows, int C, void* ws, int64_t ws_bytes,
                        hipStream_t stream);
/* Backward of a train-mode [1x1 conv -> BatchNorm -> LeakyReLU (+ residual)] layer on a big row map in one pass over the maps
 * (Train_Geo.py:166-174 through PointNN.py:96-123 MiniPointNet / :260-282 ConvBNReLURes1D; Train_Agent.py:296-305 through
 * CMRAgent.py:25-33): with h = x W^T + b the BatchNorm input, z the layer output and (stat, coef) from cmr_bn_stats_f32 /
 * cmr_bn_bwd_coef_f32:  d = dz * act'(z) (-> dzm when non-null),  dh = scale (d - c1 - xhat c2),  dw (+)= dh^T x,  dx = dh W (+ res;
 * dx may alias res; dx null: weight gradient only).  stat = coef = null: no BatchNorm (dh = d).  z null: no activation.  db non-null:
 * (+)= column sums of dh (the bias gradient of a layer without BatchNorm).  seg_db non-null: seg_db [rows / seg_rows][n] = the column sums
 * of dh per seg_rows-row segment (per sample: the gradient of a per-sample vector broadcast to its points, CMRAgent.py:95-99).
 * mask_from_h: z was never stored (the next layer consumed it through cmr_linear_bn_fwd_f32's prologue): act' from the sign of
 * h * stat[2] + stat[3].  xstat non-null: x is the PREVIOUS layer's BatchNorm input, the operand is lrelu_{xslope}(x * xstat[2] +
 * xstat[3]), dx is the gradient at that never-stored activation and the previous layer's BatchNorm-backward reduction comes out of the
 * same pass: xcoef [2][k] (= cmr_bn_bwd_coef_f32's result for it), xdgamma / xdbeta [k] (written when non-null).
 * Serves n, k in {64, 128} (xstat: n = 64) and rows a multiple of 32; anything else -> CMR_EUNSUPPORTED (compose cmr_bn_bwd_f32,
 * cmr_linear_wgrad_f32 and cmr_linear_f32 on the transposed weights). */
int64_t cmr_bn_linear_bwd_workspace_bytes(int64_t rows, int n, int k);
int cmr_bn_linear_bwd_f32(const float* dz, int64_t lddz, const float* z, int64_t ldz, float slope, const float* h, int64_t ldh,
                          const float* stat, const float* coef, int mask_from_h, float* dzm, int64_t lddzm, const float* x, int64_t ldx,
                          const float* xstat, float xslope, float* xcoef, float* xdgamma, float* xdbeta, const float* w, int64_t ldw,
                          const float* res, int64_t ldres, float* dx, int64_t lddx, int64_t rows, int n, int k, float* dw, int64_t lddw,
                          int accumulate, float* db, int accumulate_db, int64_t seg_rows, float* seg_db, void* ws, int64_t ws_bytes,
                          hipStream_t stream);
/* The same layer backward with its two products (dw = dh^T x', dx = dh W) on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32
 * accumulate; operands rounded to bf16, round-to-nearest-even, on the way into LDS) for the bf16 mode of the agent update (BASELINE
 * configs[2]; Train_Agent.py:296-305 through CMRAgent.py:25-33, 92-101).  Maps stay fp32 in HBM; masks, the BatchNorm-backward arithmetic,
 * db / seg_db (sums of the UNROUNDED dh), the lazy operand's sums, partial sums and their reduction exactly as cmr_bn_linear_bwd_f32.
 * Same arguments, shapes served and return codes; its own workspace size. */
int64_t cmr_bn_linear_bwd_bf16_workspace_bytes(int64_t rows, int n, int k);
int cmr_bn_linear_bwd_bf16_f32(const float* dz, int64_t lddz, const float* z, int64_t ldz, float slope, const float* h, int64_t ldh,
                          const float* stat, const float* coef, int mask_from_h, float* dzm, int64_t lddzm, const float* x, int64_t ldx,
                          const float* xstat, float xslope, float* xcoef, float* xdgamma, float* xdbeta, const float* w, int64_t ldw,
                          const float* res, int64_t ldres, float* dx, int64_t lddx, int64_t rows, int n, int k, float* dw, int64_t lddw,
                          int accumulate, float* db, int accumulate_db, int64_t seg_rows, float* seg_db, void* ws, int64_t ws_bytes,
                          hipStream_t stream);
/* Forward of the same layer with its statistics from the same pass: h [rows][n] = x' W^T + bias and stat [4][n] = the batch statistics
 * of h exactly as cmr_bn_stats_f32 defines them (mean, rstd, scale, shift; running statistics updated when given).  pro_stat non-null:
 * x' = lrelu_{pro_slope}(x * pro_stat[2 k ..] + pro_stat[3 k ..]) -- x is then the PREVIOUS layer's BatchNorm input and that layer's
 * activated output is never written (PointNN.py:96-123 layer_1 -> layer_2 -> layer_3, :260-282 net[0] -> net[3]).  bias_seg_rows > 0:
 * bias is [rows / bias_seg_rows][n] with row stride bias_stride, one row per segment (sample) of bias_seg_rows rows: the broadcast half of
 * cat([feat, max]) times its weights (CMRAgent.py:95-99).  n, k in {64, 128}, rows a multiple of 32; else CMR_EUNSUPPORTED (compose
 * cmr_linear_f32 + cmr_bn_stats_f32). */
int64_t cmr_linear_bn_fwd_workspace_bytes(int64_t rows, int n, int k);
int cmr_linear_bn_fwd_f32(const float* x, int64_t ldx, int k, const float* pro_stat, float pro_slope, const float* w, int64_t ldw,
                          const float* bias, int64_t bias_seg_rows, int64_t bias_stride, float* h, int64_t ldh, int64_t rows, int n, float eps,
                          float momentum, const float* gamma, const float* beta, float* running_mean, float* running_var, float* stat,
                          void* ws, int64_t ws_bytes, hipStream_t stream);
/* The same layer forward with its product on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulate; x' and W rounded to bf16,
 * round-to-nearest-even) for the bf16 mode of the agent update (BASELINE configs[2]; CMRAgent.py:25-33, 92-101 under Train_Agent.py:296-305):
 * h stays fp32 in HBM, stat = the batch statistics of THAT h (per-wave pivoted sums merged in double), running statistics as
 * cmr_linear_bn_fwd_f32 leaves them.  Same arguments and shapes served (+ w 16-byte aligned, ldw % 4 == 0); its own workspace size. */
int64_t cmr_linear_bn_fwd_bf16_workspace_bytes(int64_t rows, int n, int k);
int cmr_linear_bn_fwd_bf16_f32(const float* x, int64_t ldx, int k, const float* pro_stat, float pro_slope, const float* w, int64_t ldw,
                          const float* bias, int64_t bias_seg_rows, int64_t bias_stride, float* h, int64_t ldh, int64_t rows, int n, float eps,
                          float momentum, const float* gamma, const float* beta, float* running_mean, float* running_var, float* stat,
                          void* ws, int64_t ws_bytes, hipStream_t stream);
/* The elementwise glue of a vector-attention layer in training (PointNN.py:151-170, 219-226: `fc_gamma(q - k + pos)`, `v + pos`) in one pass
 * each way: a_in = q - k + pos, vp = v + pos (contiguous [rows][C] outputs);  backward dk = -da_in, dpos = da_in + dvp (dq and dv are the
 * incoming gradients themselves). */
int cmr_vecattn_mix_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* pos, int64_t ldp,
                        float* a_in, float* vp, int64_t rows, int C, hipStream_t stream);
int cmr_vecattn_mix_bwd_f32(const float* da, int64_t ldda, const float* dvp, int64_t lddv, float* dk, float* dpos, int64_t rows, int C,
                            hipStream_t stream);
/* dy = dz * LeakyReLU'(z) (+ add): activation backward where no BatchNorm sits in front (identity shortcut, PointNN.py:271). */
int cmr_act_bwd_f32(const float* dz, int64_t lddz, const float* z, int64_t ldz, float slope, const float* add, int64_t ldadd,
                    float* dy, int64_t lddy, int64_t rows, int C, hipStream_t stream);
/* Backward of [LeakyReLU -> AvgPool2d(ph, pw)] (CMRAgent.py:38-39,44-45,50-51,56-57): g [B,H/ph,W/pw,C] -> dc [B,H,W,C]
 * with d = the activation output. */
int cmr_pool_act_bwd_f32(const float* g, const float* d, float* dc, int B, int H, int W, int C, int ph, int pw, float slope,
                         hipStream_t stream);
/* per-batch column sum; per-batch column max with the arg-max row (first index on ties, as torch.max(dim) on the CPU);
 * backward of the max: dx[b, arg[b,c], c] += g[b,c]   (CMRAgent.py:95). */
int64_t cmr_colarg_workspace_bytes(int B, int N, int C);
int cmr_colsum_f32(const float* x, int64_t ldx, float* out, void* ws, int64_t ws_bytes, int B, int N, int C, hipStream_t stream);
int cmr_colmax_arg_f32(const float* x, int64_t ldx, float* out, int32_t* arg, void* ws, int64_t ws_bytes, int B, int N, int C,
                       hipStream_t stream);
int cmr_add_at_arg_f32(float* dx, int64_t lddx, const int32_t* arg, const float* g, int64_t ldg, int B, int N, int C,
                       hipStream_t stream);
/* Backward of y = act(x W^T + b) on a small row map (rows <= 4096; n % 32 == 0, n <= 128; k in {32, 64, 128}) in ONE launch -- the
 * autograd of nn.Linear / Conv1d(k=1) (+ ReLU / LeakyReLU) in Train_Geo.py:166-174's backward for the transformer / proxy layers:
 *   dYe = dy * (y > 0 ? 1 : slope) (y null: dYe = dy);  dw [n][k] (+)= dYe^T x;  db [n] (+)= column sums of dYe (optional);
 *   dx [rows][k] = dYe w (+ res) (optional; res may alias dx).  w [n][k] is the forward weight (no transposed copy needed).
 * Deterministic (fixed summation orders).  Returns -3 (unsupported) outside the shapes above: the caller composes cmr_act_bwd_f32,
 * cmr_linear_wgrad_f32 and cmr_linear_f32. */
int cmr_linear_bwd_rows_f32(const float* dy, int64_t lddy, const float* y, int64_t ldy, float slope, const float* x, int64_t ldx,
                            const float* w, int64_t ldw, int64_t rows, int n, int k, float* dw, int64_t lddw, int accumulate_dw,
                            float* db, int accumulate_db, const float* res, int64_t ldres, float* dx, int64_t lddx, hipStream_t stream);
/* nn.Linear / 1x1 conv backward on a handful of rows (<= 1024; the layers after the global pools, CMRAgent.py:57-59,70-86):
 * dYe = dY * LeakyReLU'(Y) (Y null: none); dW = dYe^T [X1|X2]; db = sum dYe; dX1 / dX2 (+)= dYe W. */
int cmr_linear_bwd_small_f32(const float* x1, int64_t ldx1, int k1, const float* x2, int64_t ldx2, int k2, const float* y,
                             int64_t ldy, float slope, const float* dy, int64_t lddy, const float* w, int64_t ldw, float* dw,
                             int64_t lddw, float* db, float* dx1, int64_t lddx1, float* dx2, int64_t lddx2, int acc_dx, int rows,
                             int n, hipStream_t stream);
/* Loss of one minibatch and its gradient w.r.t. logits / value (Train_Agent.py:268-302 with CMRAgent.py:129-144):
 * cross-entropy against the expert + alpha (PPO clip + w_value MSE - w_entropy entropy).  logits rows [B, d*S]; actions
 * int64 [B,d]; old_logprob [B, dr+dt]; returns / adv [B]; out [8] = (loss, clone, policy, value, entropy, ppo, 0, 0);
 * gradients are multiplied by grad_scale. */
int cmr_agent_loss_f32(const float* r_logits, int64_t ldr, const float* t_logits, int64_t ldt, const float* value, int64_t ldv,
                       const int64_t* expert_r, const int64_t* expert_t, const int64_t* act_r, const int64_t* act_t,
                       const float* old_logprob, const float* returns, const float* adv, float* d_r, int64_t lddr, float* d_t,
                       int64_t lddt, float* d_v, int64_t lddv, float* out, int B, int dr, int dt, int S, float alpha,
                       float clip_eps, float w_value, float w_entropy, float grad_scale, hipStream_t stream);
/* torch.optim.Adam step (Train_Agent.py:121-127, :305) over the flat parameter bucket: g <- grad_scale * g + wd * p;
 * m, v moments; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  n % 4 == 0 (the bucket pads every tensor).  grad_clip > 0
 * clamps the scaled gradient to [-clip, clip] first (nn.utils.clip_grad_value_, Train_Geo.py:172). */
int cmr_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, float bias_correction1, float bias_correction2, float grad_scale, float grad_clip,
                 hipStream_t stream);
/* torch.optim.SGD step (the 'SGD' branch of Train_Agent.py:111-117 / Train_Geo.py:65-71: momentum, L2 weight decay, dampening 0,
 * no Nesterov) over the flat parameter bucket: g <- grad_scale * g (clamped when grad_clip > 0) + wd * p; buf = g on the first
 * step, momentum * buf + g afterwards; p -= lr * buf.  n % 4 == 0. */
int cmr_sgd_f32(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                float grad_clip, int first_step, hipStream_t stream);
/* Transposed shadow of the matrix parameters of a flat bucket (operands of the data-gradient GEMMs): table [nslots][5] int64 =
 * (src offset, n, k, dst offset, first tile index), tiles of 32 x 32; dst[k][n] = src[n][k] for every slot, one launch. */
int cmr_transpose_slots_f32(const float* src, float* dst, const int64_t* table, int nslots, int64_t total_tiles,
                            hipStream_t stream);
/* nn.Conv2d(3x3, stride 1, pad 1) weight gradient on the matrix cores: dw [Cout][Cin][3][3] = sum over the minibatch
 * pixels of dy (x) shifted x (NHWC maps, W >= 2, Cin in {32,64,128}, Cout % 32 == 0). */
int64_t cmr_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
/* The same gradient with the products on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16: operands rounded to bf16, fp32 accumulate;
 * the bf16 training mode of BASELINE configs[2]).  x / dy stay fp32 NHWC; Cin in {64, 128}; workspace of
 * cmr_conv3x3_wgrad_workspace_bytes. */
int cmr_conv3x3_wgrad_bf16_f32(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dw, void* ws,
                               int64_t ws_bytes, hipStream_t stream);
/* The same launch + the bias gradient db [Cout] = sum of dy over all pixels (torch.nn.Conv2d's bias.grad; autograd of
 * Train_Agent.py:296-305): every dy element is staged by exactly one lane of the weight-gradient kernel, which keeps fp32 running
 * sums per channel -- replaces a cmr_colsum_f32 pass over dy.  db null: identical to the entry point above. */
int cmr_conv3x3_wgrad_bias_bf16_f32(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dw, float* db, void* ws,
                                    int64_t ws_bytes, hipStream_t stream);
/* The same with x given as the INPUT of a train-mode BatchNorm whose LeakyReLU(xslope) output was the convolution's operand and was never
 * stored (forward: cmr_conv3x3_bf16_pro_nhwc_f32; models/CMRAgent.py:34-56 conv -> BatchNorm -> LeakyReLU -> conv under Train_Agent.py:296-305):
 * the operand lrelu(x * xscale + xshift) (xscale, xshift [Cin] = stat[2], stat[3] of cmr_bn_stats_f32) is formed in the staging pass with the
 * arithmetic of cmr_affine_act_f32 -- bit-identical gradients to the call above on the stored map.  Cin = 128, Cout % 64 == 0, maps of
 * >= 32 768 pixels; CMR_EUNSUPPORTED (-3) otherwise. */
int cmr_conv3x3_wgrad_bias_bf16_pro_f32(const float* x, const float* xscale, const float* xshift, float xslope, const float* dy, int B, int H,
                                        int W, int Cin, int Cout, float* dw, float* db, void* ws, int64_t ws_bytes, hipStream_t stream);
int cmr_conv3x3_wgrad_f32(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dw, void* ws,
                          int64_t ws_bytes, hipStream_t stream);
/* The same gradient in the Winograd domain (round 6; Train_Geo.py:166-174 through models/ImageResNet.py:5-40: the forward and data-gradient
 * convolutions run on F(2x2,3x3), this is the transpose of that identity): dw = sum over the 2x2 output tiles of G^T[(A dy A^T) (.) (B^T x B)]G
 * -- 16 position GEMMs over the tiles (16 of the 36 multiplies of the direct sum) on v_mfma_f32_32x32x2_f32, fp32 accumulate, partial sums
 * reduced in double in a fixed order, the fold with G once per launch.  Served: Cin = Cout = 64, H and W even; CMR_EUNSUPPORTED (-3)
 * otherwise (the caller uses cmr_conv3x3_wgrad_f32).  Error against the float64 sum: 1.5 x the direct fp32 kernel's at K = 856 064 tiles
 * (tools/wino_wgrad_check.py). */
int64_t cmr_conv3x3_wgrad_wino_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int cmr_conv3x3_wgrad_wino_f32(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dw, void* ws,
                               int64_t ws_bytes, hipStream_t stream);
/* nn.Conv1d(k=1) / nn.Linear weight and bias gradient over a row map: dw [n][k] (+)= dy^T x, db [n] (+)= column sums of dy
 * (db optional), any n, k: one launch over (row slices) x (n blocks of 128) x (k blocks of 128) + one deterministic
 * reduction of the slices. */
int64_t cmr_linear_wgrad_workspace_bytes(int64_t rows, int n, int k);
int cmr_linear_wgrad_f32(const float* dy, int64_t lddy, int n, const float* x, int64_t ldx, int k, int64_t rows, float* dw,
                         int64_t lddw, int accumulate, float* db, int accumulate_db, void* ws, int64_t ws_bytes,
                         hipStream_t stream);
/* nn.Conv2d weight [Cout][Cin][3][3] -> operand layouts of the forward kernels (w9 [9][Co'][Ci'] and the Winograd
 * U fragments); transpose = 1 packs the data-gradient convolution W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx].  bf16_frag
 * (optional) receives the bf16 A fragments of cmr_conv3x3_bf16_nhwc_f32 for cout groups of 32 * bf16_nt. */
int cmr_pack_conv3x3_f32(const float* w, int Cout, int Cin, int transpose, float* w9, float* ufrag, void* bf16_frag, int bf16_nt,
                         hipStream_t stream);

/* ---- dataset-side geometry of one frame ------------------------------------------ */
/* dataset/KittiDataset.py:273-276, :284, :312-336 (same code in NuScenesDataset.py): velodyne -> camera transform of the
 * down-sampled cloud (choice = the np.random.choice indices, null = all points in order), projection with the 1/4-scale
 * intrinsics, round-half-even pixel, in-picture test, pc_mask, img_mask (coo_matrix(...).toarray() > 0), the random pose.
 * raw: planar float32 rows [>=3][ld_raw] as stored in the .npy; tr12 / k9 / prand12 are HOST arrays (float64, row-major
 * 3x4 / 3x3 / 3x4) copied by value; everything else is device memory.  Arithmetic in float64 like numpy.
 * Outputs: pc_cam / pc_out planar float32 [3][N], pc_mask int64 [N], xy float64 [2][N] (pc_[0:2]), img_mask int64 [h*w]. */
int cmr_dataset_project_f64(const float* raw, int64_t ld_raw, const int64_t* choice, const double* tr12, const double* k9,
                            const double* prand12, int w, int h, float* pc_cam, float* pc_out, int64_t* pc_mask, double* xy,
                            int64_t* img_mask, int64_t N, hipStream_t stream);
/* KittiDataset.py:338-345: pc_idx_for_circle_loss = np.where(is_in_picture)[0][perm[:nsel]] (ordered compaction by a
 * scan, compact_ws int32 [N]), the float32 pixel coordinates of those points and their np.round as int64.  count receives
 * the number of in-picture points; samples whose perm entry is >= count are marked with index -1. */
int cmr_dataset_circle_select_f64(const int64_t* pc_mask, const double* xy, const int64_t* perm, int nsel, int64_t N,
                                  int32_t* compact_ws, int64_t* count, int64_t* idx_out, float* xy_float, int64_t* xy_int,
                                  hipStream_t stream);

/* ---- bf16 matrix-core variant of the 3x3 convolution (BASELINE configs[2] / [3]) ---- */
/* Same contract as cmr_conv3x3_nhwc_f32 (fp32 NHWC in / out, stride 1|2, folded-BN bias, residual, LeakyReLU, positional
 * table, optional fused 2x2 average pool at stride 1) with the products on v_mfma_f32_32x32x16_bf16 (operands rounded to
 * bf16, fp32 accumulate).  wfrag: bf16 A fragments [Cout/(32 nt)][9][Cin/16][nt][64][8]
 * (cmr_agent_amd/models/_pack.py:conv_bf16_frags).  Served shapes: stride 1: (Cin 64, nt 1|2), (Cin 128, nt 1); stride 2:
 * (Cin 64, nt 1|2); anything else returns CMR_EUNSUPPORTED.  cu_budget: CUs the persistent two-team / matrix-class kernels may occupy
 * (0 = all), as for cmr_conv3x3_wino_nhwc_f32. */
int cmr_conv3x3_bf16_nhwc_f32(const float* x, int B, int H, int W, int Cin, const void* wfrag, int nt, const float* bias,
                              const float* res, const float* post, float* y, int Cout, int stride, float slope, int pool,
                              int cu_budget, hipStream_t stream);

/* ---- geometric-model update: backward pieces (reference Train_Geo.py:166-174) ---------------------- */
/* The training forward of MultiHeadModel is the op-level composition of the inference entry points above with BatchNorm
 * in batch-statistics mode (cmr_agent_amd/train/geo_update.py); these are the backward kernels of its ops.  `accumulate`
 * flags add into the destination (a value that feeds several consumers, a parameter used twice). */
int cmr_axpy_f32(float* y, int64_t ldy, const float* x, int64_t ldx, float alpha, int64_t rows, int C, hipStream_t stream);
/* y = act(x) (ReLU / LeakyReLU / erf-GELU / elu+1) and dx (+)= dy act'(x) with x the PRE-activation. */
int cmr_act_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int C, int act, float act_param, hipStream_t stream);
int cmr_act_bwd_x_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dx, int64_t lddx, int64_t rows, int C, int act,
                      float act_param, int accumulate, hipStream_t stream);
/* nn.LayerNorm(64) backward (ImageViT.py:140-141, IMGPCEncoder.py:86-87, LinearAttention.py:33-34). */
int64_t cmr_layernorm64_bwd_workspace_bytes(int64_t rows);
int cmr_layernorm64_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, float eps, float* dx,
                            int64_t lddx, int accumulate_dx, float* dgamma, float* dbeta, int accumulate_params, int64_t rows, void* ws,
                            int64_t ws_bytes, hipStream_t stream);
/* F.normalize(dim=1) backward over 64 channels (MultiHeadModel.py:233,241). */
int cmr_l2norm64_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dx, int64_t lddx, int accumulate, int64_t rows,
                         hipStream_t stream);
/* out[b,2y,2x,:] = g[b,y,x,:], zero elsewhere: a stride-2 convolution's data / weight gradients are the stride-1 ones of its
 * zero-inserted output gradient (ImageResNet.py:13,24-36). */
int cmr_zero_insert2_f32(const float* g, float* out, int B, int Ho, int Wo, int H, int W, int C, hipStream_t stream);
/* adjoints of cmr_patchify_nhwc_f32, of the nearest up-sampling half of cmr_upsample_concat_f32, and the 3-channel im2col pair
 * that turns the stem's convolutions (ImageResNet.py:5-40 with 3 input channels) into row GEMMs in the training path. */
int cmr_patchify_bwd_f32(const float* dpatches, float* dx, int B, int H, int W, int C, int P, int accumulate, hipStream_t stream);
int cmr_upsample_bwd_f32(const float* dcat, int64_t ldc, int coff, float* dproxy, int B, int H, int W, int C2, int scale, int accumulate,
                         hipStream_t stream);
int cmr_im2col3_f32(const float* x4, float* cols, int B, int H, int W, hipStream_t stream);
int cmr_col2im3_f32(const float* dcols, float* dx4, int B, int H, int W, int accumulate, hipStream_t stream);
/* softmax attention backward (forward cmr_mha_f32; ImageViT.py:81-108, IMGPCEncoder.py:36-58): ws = 16 floats per query row. */
int cmr_mha_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* o, int64_t ldo,
                    const float* dout, int64_t lddo, float* dq, int64_t lddq, int acc_dq, float* dk, int64_t lddk, int acc_dk, float* dv,
                    int64_t lddv, int acc_dv, float* ws, int64_t ws_bytes, int B, int Tq, int Tk, hipStream_t stream);
/* linear attention core backward (forward cmr_la_reduce_f32 + cmr_la_apply_f32; LinearAttention.py:53-60). */
int64_t cmr_la_bwd_workspace_bytes(int B, int L);
int cmr_la_bwd_f32(const float* qf, int64_t ldq, const float* kf, int64_t ldk, const float* v, int64_t ldv, const float* kvsum,
                   const float* dmsg, int64_t lddm, float* dqf, int64_t lddq, int acc_dq, float* dkf, int64_t lddk, int acc_dk, float* dv,
                   int64_t lddv, int acc_dv, void* ws, int64_t ws_bytes, int B, int L, int S, float eps, hipStream_t stream);
/* group / neighbourhood softmax backward (forward cmr_segment_softmax_f32; PointNN.py:171-182, :227-229). */
int cmr_segment_softmax_bwd_f32(const float* attn, const float* vp, const int32_t* order, const int32_t* offsets, int fixed_len, float scale,
                                const float* dout, float* dattn, float* dvp, int64_t nseg, hipStream_t stream);
/* focal / circle loss backward (forward cmr_focal_metrics_f32 / cmr_circle_loss_f32): gradients w.r.t. the 2-class logits rows; the
 * circle loss ADDS its gradient into the dense maps d_pc_feat [B*N,64] / d_img_feat [B,h,w,64] at the sampled positions. */
int cmr_focal_bwd_f32(const float* logits, int64_t ld, const int64_t* label, float alpha, int64_t rows, float grad_scale, float* dlogits,
                      int64_t ldd, hipStream_t stream);
int64_t cmr_circle_bwd_workspace_bytes(int B, int n);
int cmr_circle_loss_bwd_f32(const float* pc_feat, const float* img_feat, const int64_t* pc_idx, const int64_t* xy_int, const float* xy_float,
                            int B, int N, int h, int w, int n, float dist_thres, float pos_margin, float neg_margin, float log_scale,
                            float grad_scale, float* d_pc_feat, float* d_img_feat, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- IterModel: pose cost volume (models/IterModel.py:24-475) ------------------------------------------------
 * The reference warps the predicted-overlap points of ONE pair under nlabel^3 sampled poses, scatter-means their features onto the
 * 1/4-scale image grid, stacks [image features | warped features | occupancy | image overlap] per pose and runs a Conv3d chain with
 * (1, 3, 3) kernels.  Here the volume is a batch of P = nlabel^3 NHWC maps on cmr_conv3x3_*_nhwc_f32; these entry points are the
 * stages around the convolutions.
 * cmr_iter_sample_poses_f32 (IterModel.py:132-173): delta_r / delta_t [nlabel] = 2 amp / (nlabel - 1) * (-(nlabel-1)/2 .. (nlabel-1)/2),
 *   rt [P][3][4] = rows 0..2 of the inverse of [R_y(delta_r[i]) | (delta_t[j], 0, delta_t[k])], p = (i nlabel + j) nlabel + k.
 * cmr_iter_warp_scatter_f32 (IterModel.py:273-345): sel = mask if any(mask) else standby; for selected points in view of pose p,
 *   acc[p][y w + x][0:64] += feat[n], cnt += 1, occ += score[n] (pc planar [3][N], feat rows [N][64]; the accumulators are cleared here).
 * cmr_iter_finalize_f32 (IterModel.py:347-377 and the one-channel input halves of cost_volume_convs[0]): acc <- acc / max(cnt, 1) when
 *   acc is given; res[p][cell][0:64] = base[cell] + sum_taps w1[tap][c] plane[p][cell + tap] (zero padding), plane [P][h][w].
 * cmr_iter_head_f32 (IterModel.py:62-66): global average of channels 0..7 of x [P][cells][ldc], 1x1 conv 8 -> 4, LeakyReLU, 4 -> 1.
 * cmr_iter_decide_f32 (IterModel.py:175-193, 391-473): label_out [P] = label_r (x) (label_tx (x) label_tz); out_f = [cross entropy of
 *   logits vs arg-max(label_out), chosen ry, tx, tz]; out_i = [label, arg-max of the three softmax marginals, arg-max of the joint];
 *   matrix_i [4][4] = inverse of the chosen step.
 * cmr_iter_apply_f32 (IterModel.py:466-472): pc_out = matrix_i[0:3, 0:3] pc + matrix_i[0:3, 3]; acc_out = matrix_i acc_in. */
int cmr_iter_sample_poses_f32(const float* r_amp, const float* t_amp, int nlabel, float* delta_r, float* delta_t, float* rt,
                              hipStream_t stream);
int cmr_iter_warp_scatter_f32(const float* pc, const float* feat, const float* score, const uint8_t* mask, const uint8_t* standby,
                              uint8_t* sel, const float* rt, const float* Kmat, float* acc, float* cnt, float* occ, int N, int P,
                              int h, int w, hipStream_t stream);
/* cmr_iter_warp_bin_f32: cmr_iter_warp_scatter_f32 + the per-pose cmr_iter_finalize_f32 in one launch and without global atomics: a workgroup
 * bins the points of one pose that land in its band of map rows in LDS and writes warped [P][h*w][64] = scatter mean, occ [P][h*w] and
 * res [P][h*w][64] = base + 3x3 stencil of the occupancy plane with w1 [9][64], each once (w <= 384). */
int cmr_iter_warp_bin_f32(const float* pc, const float* feat, const float* score, const uint8_t* mask, const uint8_t* standby,
                          uint8_t* sel, const float* rt, const float* Kmat, const float* w1, const float* base, float* warped,
                          float* res, float* occ, int N, int P, int h, int w, hipStream_t stream);
int cmr_iter_finalize_f32(float* acc, const float* cnt, const float* plane, const float* w1, const float* base, float* res, int P,
                          int h, int w, hipStream_t stream);
int cmr_iter_head_f32(const float* x, int ldc, int cells, const float* w24, const float* b24, const float* w26, const float* b26,
                      float slope, float* logits, int P, hipStream_t stream);
int cmr_iter_decide_f32(const float* logits, int nlabel, const float* label_r, const float* label_tx, const float* label_tz,
                        const float* delta_r, const float* delta_t, float* label_out, float* out_f, int64_t* out_i,
                        float* matrix_i, hipStream_t stream);
int cmr_iter_apply_f32(const float* matrix_i, const float* pc, float* pc_out, int N, const float* acc_in, float* acc_out,
                       hipStream_t stream);

/* cmr_conv3x3_bf16_nhwc_f32 with the activations optionally STORED as bf16 NHWC (x_bf16 / y_bf16 != 0): for chains of bf16 convolutions
 * (conv a -> conv b of a ResidualBlock, ImageResNet.py:9-14; the eight convolutions of the agent's 2-D embedding, CMRAgent.py:34-56).  The
 * consumer rounds its fp32 input to bf16 (RNE) anyway, so a producer that writes those bf16 values gives bit-identical results with
 * half the bytes.  Served: stride 1 with any combination, stride 2 (64 -> 64 k) with fp32 or bf16 input; bias fp32; no table operand
 * with bf16 activations.  res_bf16 != 0: the residual is a bf16 NHWC map too (bf16-STORED towers, round 3: the input of a
 * ResidualBlock is then only ever read as bf16; 64 -> 64 k layers with a bf16 input, stride 1, plain epilogue) -- this one is NOT
 * bit-neutral: the residual enters the fp32 epilogue rounded to bf16.  Otherwise CMR_EUNSUPPORTED (-3). */
int cmr_conv3x3_bf16io_nhwc(const void* x, int x_bf16, int B, int H, int W, int Cin, const void* wfrag, int nt, const float* bias,
                            const void* res, int res_bf16, const float* post, void* y, int y_bf16, int Cout, int stride, float slope,
                            int pool, int cu_budget, hipStream_t stream);
/* Train-mode [BatchNorm -> LeakyReLU(in_slope) -> 3x3 convolution (+ bias, LeakyReLU(slope))] with the BatchNorm applied in the
 * convolution's own staging pass (models/CMRAgent.py:34-56 under Train_Agent.py:296-305; ImageResNet.py:5-40): x [B][H][W][Cin] is the
 * BatchNorm INPUT, in_scale / in_shift [Cin] its folded affine (stat[2], stat[3] of cmr_bn_stats_f32); the operand
 * lrelu(x * in_scale + in_shift) is formed while the halo is converted to bf16 (zero padding applied after it) with the fused
 * multiply-add and the select of cmr_affine_act_f32: bit for bit the result of cmr_affine_act_f32 + cmr_conv3x3_bf16_nhwc_f32, without the
 * activated map's write and read.  Stride 1, Cin = 128, Cout % 128 == 0, no residual / table / pool, maps of >= 128 8x32-pixel tiles
 * (x Cout / 128): the matrix-class kernel; CMR_EUNSUPPORTED (-3) otherwise (the caller materialises the activation). */
int cmr_conv3x3_bf16_pro_nhwc_f32(const float* x, const float* in_scale, const float* in_shift, float in_slope, int B, int H, int W, int Cin,
                                  const void* wfrag, int nt, const float* bias, float* y, int Cout, float slope, int cu_budget,
                                  hipStream_t stream);

/* ---- dropout (train mode; the reference trains MultiHeadModel with p = 0.1 in 141 nn.Dropout modules) --------------------------
 * Counter-based masks: element idx of site `site` is kept iff mix64(seed[0], site, idx) >= p 2^32 (csrc/cmr_common.h:cmr_keep); seed is
 * a DEVICE int64 (advanced once per optimizer step by the host, so that a captured hipGraph draws fresh masks on every replay).
 * cmr_dropout_f32: y = x * keep / (1 - p), idx = row * C + column (ImageViT.py:56, :107, :130-132, LinearAttention.py:27-29, :66,
 *   IMGPCEnDecoder.py:38, :54 ...); the backward pass is the same call on the gradient.
 * cmr_mha_dropout_f32 / cmr_mha_dropout_bwd_f32: cmr_mha_f32 / cmr_mha_bwd_f32 with dropout on the attention probabilities
 *   (ImageViT.py:100, PointViT.py:129, IMGPCEncoder.py:47), idx = ((b 8 + head) Tq + query) Tk + key. */
int cmr_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int C, float p, const int64_t* seed,
                    int64_t site, hipStream_t stream);
int cmr_mha_dropout_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* o,
                        int64_t ldo, int B, int Tq, int Tk, float p, const int64_t* seed, int64_t site, hipStream_t stream);
int cmr_mha_dropout_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* o,
                            int64_t ldo, const float* dout, int64_t lddo, float* dq, int64_t lddq, int acc_dq, float* dk,
                            int64_t lddk, int acc_dk, float* dv, int64_t lddv, int acc_dv, float* ws, int64_t ws_bytes, int B, int Tq,
                            int Tk, float p, const int64_t* seed, int64_t site, hipStream_t stream);

/* Weight gradient of a STRIDE-2 3x3 convolution (pad 1; ImageResNet.py:9-14, :24-27 under loss.backward()): x [B][H][W][Cin] (H, W even), dy
 * [B][H/2][W/2][Cout] -> dw [Cout][Cin][3][3].  Contracts over the OUTPUT pixels (cmr_conv3x3_wgrad_f32 on the zero-inserted gradient contracts
 * over all input pixels, three quarters of which multiply zeros).  Workspace: cmr_conv3x3_wgrad_workspace_bytes(B, H / 2, W / 2, Cin, Cout). */
int cmr_conv3x3_wgrad_s2_f32(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dw, void* ws, int64_t ws_bytes,
                             hipStream_t stream);
/* cmr_pack_conv3x3_f32 for EVERY 3x3 convolution of a training step, both orientations, in one launch: table = device [nslots][8] int64
 * {src offset in the flat parameter buffer, Cout, Cin, transpose, w9 offset in dst, U offset in dst (-1: none), bf16 fragment offset in
 * dst_bf16 in bf16 elements (-1: none), bf16_nt}; max_pairs = the largest Cout * Cin.  (Train_Geo.py:166-174 / Train_Agent.py:263-305: the
 * weights move every optimizer step, so the forward kernels' operand layouts are rebuilt per step -- one launch instead of one per
 * convolution and direction.) */
int cmr_pack_conv3x3_slots_f32(const float* src, float* dst, void* dst_bf16, const int64_t* table, int nslots, int64_t max_pairs,
                               hipStream_t stream);

/* ---- train-mode transformer block in fused launches (round 4; reference models/ImageViT.py:61-158, PointViT.py:96-183,
 * IMGPCEncoder.py:14-102 under model.train(), Train_Geo.py:166-174).  Replaces, per block and step, 16 forward and ~20 backward calls of
 * the op-level entry points above by 3 + 4: cmr_ln64_linear_f32, cmr_mha_dropout_f32, cmr_vit_out_ffn16_train_f32 forward;
 * cmr_vit_ffn_bwd16_f32, cmr_mha_dropout_bwd_f32, cmr_vit_lnqkv_bwd_f32, cmr_wgrad_group_f32 backward.  Dropout masks are those of
 * cmr_dropout_f32 (same (seed, site, row * width + column) -> same mask), p = 0 or seed null: no dropout. ---- */
/* Weights from the flat parameter bucket `src` into MFMA fragment order in `dst`, every slot of a step in ONE launch.  table: device
 * [nslots][10] int64 {src offset, n, k (shape of this slot's block of the packed matrix W'), row stride of the stored matrix, dst offset of
 * W' (multiple of 4), kind, transpose (the block is the transpose of the stored [k][n] matrix), elements (n k; kind 2: n rounded up to 4),
 * ktot (columns of the whole W'), koff (first column of the block inside W'; row blocks go through the dst offset)}; kind 0 = 32x32x2
 * fragments (_pack.frag_pack), 1 = 16x16x4 fragments (_pack.frag_pack16), 2 = plain copy of n floats.  max_elements = the largest
 * `elements`.  A stacked matrix ([Wq; Wk; Wv], or its transpose for the data gradient) is several slots writing one W'. */
int cmr_pack_frags_f32(const float* src, float* dst, const int64_t* table, int nslots, int64_t max_elements, hipStream_t stream);
/* x1 = x + drop_proj(ctx Wo^T + bo);  out = x1 + drop_fc2(W2 drop_act(gelu(W1 LN(x1) + b1)) + b2)   (ImageViT.py:103-108, 128-133, 150-157).
 * cmr_vit_out_ffn16_f32 with the three nn.Dropout sites applied in place and x1 written for the backward.  Weights: frag16 fragments. */
int cmr_vit_out_ffn16_train_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const float* wo_f16, const float* bo,
                                const float* ln_g, const float* ln_b, float eps, const float* w1_f16, const float* b1,
                                const float* w2_f16, const float* b2, float* out, int64_t ldo, float* x1, int64_t ldx1, int64_t rows,
                                float p_proj, float p_mlp, const int64_t* seed, int64_t site_proj, int64_t site_act, int64_t site_fc2,
                                hipStream_t stream);
/* Backward of that launch from d out: recomputes LN(x1), the fc1 pre-activations and the masks from x1;
 *   dm = drop_fc2(d out);  d hidden = dm W2;  du = drop_act(d hidden) gelu'(u);  d LN = du W1;  d x1 = d out + LayerNorm_bwd(d LN);
 *   da = drop_proj(d x1);  d ctx = da Wo.
 * Writes d x1, d ctx and the operands of the weight gradients: gs [rows][1024] (hidden activations as fc2 saw them), du [rows][1024],
 * h = LN(x1) [rows][64], dm [rows][64], da [rows][64]; lnpart [ceil(rows / 16)][128] = per-tile sums of (d gamma | d beta) of ffn_norm
 * (summed by cmr_wgrad_group_f32).  w2t / w1t / wot: frag16 fragments of W2^T, W1^T, Wo^T (cmr_pack_frags_f32, transpose = 1).  The
 * seven row outputs must have room for whole 16-row tiles (ceil(rows / 16) * 16 rows): rows past the end are written, never read. */
int cmr_vit_ffn_bwd16_f32(const float* dout, int64_t lddo, const float* x1, int64_t ldx1, const float* ln_g, const float* ln_b, float eps,
                          const float* w1_f16, const float* b1, const float* w2t_f16, const float* w1t_f16, const float* wot_f16,
                          float* dx1, int64_t lddx1, float* dctx, int64_t lddc, float* gs, float* du, float* h, float* dm, float* da,
                          float* lnpart, int64_t rows, float p_proj, float p_mlp, const int64_t* seed, int64_t site_proj,
                          int64_t site_act, int64_t site_fc2, hipStream_t stream);
/* Backward of attention_norm + the q / k / v projections for up to two row sets in one launch (self block: x with d = [dq | dk | dv],
 * k = 192; cross block: x with dq, k = 64, and y with [dk | dv], k = 128; IMGPCEncoder.py:93-94: both through the SAME LayerNorm):
 *   d LN(x) = d W_cat (W_cat = the projections' weights stacked, passed as frag32 fragments of W_cat^T);  dx = LayerNorm_bwd(d LN(x)) (+ res,
 * the gradient arriving on the residual stream; x set only).  Also writes LN(x) / LN(y) (operands of the projections' weight gradients)
 * and lnpart [tiles_x + tiles_y][128] (32-row tiles; per-tile sums of d gamma | d beta). */
int cmr_vit_lnqkv_bwd_f32(const float* d_x, int64_t ldd_x, int k_x, const float* wt_f_x, const float* x, int64_t ldx, const float* res,
                          int64_t ldres, float* dx, int64_t lddx, float* xn, int64_t ldxn, int64_t rows_x, const float* d_y,
                          int64_t ldd_y, int k_y, const float* wt_f_y, const float* y, int64_t ldy, float* dy, int64_t lddy, float* yn,
                          int64_t ldyn, int64_t rows_y, const float* gamma, const float* beta, float eps, float* lnpart,
                          hipStream_t stream);
/* Weight / bias gradients of up to 8 row-map linears (dw [n][k] (+)= dy^T x, db (+)= column sums of dy: cmr_linear_wgrad_f32's contract)
 * and up to 4 "vector jobs" (out_a | out_b [len] (+)= sums over nparts rows of part [nparts][2 len]: the LayerNorm parameter gradients the
 * row kernels left per tile) in ONE call of two kernels.  desc is a HOST array: nprob x 12 int64 {dy, lddy, n, x, ldx, k, rows, dw, lddw,
 * accumulate, db (0: none), accumulate_db}, then nvec x 6 int64 {part, nparts, len, out_a, out_b, accumulate}; pointers as integers.
 * Deterministic (fixed slices, fixed summation order, no atomics). */
int64_t cmr_wgrad_group_workspace_bytes(const int64_t* desc, int nprob, int nvec);
int cmr_wgrad_group_f32(const int64_t* desc, int nprob, int nvec, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- train-mode linear-attention layer in fused launches (round 4; reference models/LinearAttention.py:38-73 under model.train(),
 * Train_Geo.py:166-174): 2 forward + 4 backward calls per layer instead of ~16 + ~20 op-level ones. ---- */
/* cmr_la_kv_state_f32 that also writes kf = elu(Wk y) + 1 and v = Wv y [B S][64] for the backward. */
int cmr_la_kv_state_train_f32(const float* y, int64_t ldy, const float* wk, const float* wv, float* kvsum, float* kf, float* v,
                              void* workspace, int64_t workspace_bytes, int B, int S, hipStream_t stream);
/* cmr_la_query_layer_f32 with the layer's three nn.Dropout(p) sites applied (attention message after LayerNorm 1, MLP hidden activations,
 * MLP output; masks of cmr_dropout_f32, element index = row * width + column) and the activations the backward needs written once per row:
 * qf = elu(Wq x) + 1, msg, mm = Wm msg, d1 = drop(LN1(mm)), o = drop(W3 hid) [B L][64] and hid = drop(relu(W0 [x | d1])) [B L][128]; these six
 * buffers must have room for whole 32-row tiles (ceil(B L / 32) * 32 rows; rows past the end are written, never read). */
int cmr_la_query_layer_train_f32(const float* x, int64_t ldx, const float* kvsum, const float* wq, const float* wmerge,
                                 const float* ln1_g, const float* ln1_b, const float* w_mlp0, const float* w_mlp3,
                                 const float* ln2_g, const float* ln2_b, float* out, int64_t ldo, float* qf, float* msg, float* mm,
                                 float* d1, float* hid, float* o, int B, int L, int S, float eps, float ln_eps, float p,
                                 const int64_t* seed, int64_t site_att, int64_t site_hid, int64_t site_out, hipStream_t stream);
/* Backward of the query side's MLP half from d out (one pass over the rows): LayerNorm-2 backward, output dropout, W3^T, ReLU / hidden
 * dropout, W0^T, attention dropout, LayerNorm-1 backward, Wm^T.  Writes d_o [rows][64] (gradient at W3's output), d_hid [rows][128] (at
 * W0's output), d_mm [rows][64] (at Wm's output) -- the dy operands of the three weight gradients --, d_msg [rows][64] (gradient of the
 * attention message, input of cmr_la_bwd_f32), d_xa [rows][64] (gradient of x through the MLP) and lnpart1 / lnpart2 [min(256, ceil(rows / 256))][128]
 * (per-workgroup sums of d gamma | d beta of norm1 / norm2, summed by cmr_wgrad_group_f32).  The five row outputs must have room for whole
 * 32-row tiles (ceil(rows / 32) * 32 rows): rows past the end are written, so that no store is predicated. */
int cmr_la_mlp_bwd_f32(const float* dout, int64_t lddo, const float* o, const float* hid, const float* mm, const float* wmerge,
                       const float* w_mlp0, const float* w_mlp3, const float* ln1_g, const float* ln2_g, float* d_o, float* d_hid,
                       float* d_mm, float* d_msg, float* d_xa, float* lnpart1, float* lnpart2, int64_t rows, float ln_eps, float p,
                       const int64_t* seed, int64_t site_att, int64_t site_hid, int64_t site_out, hipStream_t stream);
/* Backward of the q / k / v projections for one or two row sets in one launch: per set dx = sum_i (d_i * elu1'(f_i)) W_i + res0 + res1, where
 * f_i is the SAVED activation elu(z) + 1 (derivative 1 where f > 1, else f; 0 = no activation) and W_i^T is passed as frag32 fragments
 * (cmr_pack_frags_f32).  desc: HOST array, 23 int64 per set: rows, nterm (1..3), dx, lddx, res0, ldr0, res1, ldr1, then 3 x {d, ldd, f, wt_f,
 * e_out}; e_out (0: none; may equal d) receives d_i * elu1'(f_i), the dy operand of W_i's weight gradient. */
int cmr_la_proj_bwd_f32(const int64_t* desc, int nprob, hipStream_t stream);

/* ---- raw scan -> prepared cloud: voxel-grid downsample and surface normals (csrc/cloud_prepare.hip) ------------------
 * Port extension: the reference reads clouds that an Open3D script of its lineage prepared (voxel_down_sample(0.1), estimate_normals(0.6))
 * and holds no code that makes them.  One cloud per call.  Every integer below follows from fp32 operations that are stated one by one,
 * so that a float32 restatement (tests/cloud_prepare_reference.py) reproduces keys, order, counts and the inverse map bit for bit.
 *
 * The grid.  A row is KEPT when its three coordinates are finite, else DROPPED.  Per axis the cell index of a kept row is
 *     c = floorf((x - origin) / cell)      one IEEE fp32 subtraction, one IEEE fp32 division (no reciprocal, no fused operation),
 * and its key is the int64  cz << 42 | cy << 21 | cx.  The caller guarantees 0 <= c < 2^21 on every axis for every kept row (the host
 * checks the two corners of cmr_cloud_bounds_f32, c being monotone in x, and raises before a key is used; a kernel handed anything else
 * clamps c into that range rather than forming a malformed key).  Dropped rows get the key 2^63 - 1, which sorts behind every cell.
 *
 * cmr_cloud_bounds_f32: bounds[0..2] / bounds[3..5] = per-axis minimum / maximum over the kept rows of points [N][ld >= 3] (+inf / -inf
 * when there is none), kept[0] = their number.  Workspace of cmr_cloud_bounds_workspace_bytes(N).  0 < N < 2^31 in all of these (the CSR
 * of cmr_segment_reduce_f32 is int32). */
int64_t cmr_cloud_bounds_workspace_bytes(int64_t N);
int cmr_cloud_bounds_f32(const float* points, int64_t ld, int64_t N, float* bounds, int64_t* kept, void* workspace,
                         int64_t workspace_bytes, hipStream_t stream);
/* keys[i] of every row, as above (voxel downsample: cell = the voxel size, origin = minimum - voxel / 2 in fp32 unless the caller names one;
 * normals: cell = the radius, origin = the minimum). */
int cmr_voxel_keys_f32(const float* points, int64_t ld, int64_t N, float ox, float oy, float oz, float cell, int64_t* keys,
                       hipStream_t stream);
/* Runs of equal keys -> CSR.  keys_sorted / order: the keys in ascending order and the row each came from (a STABLE sort: the rows of a
 * run are in ascending input index); the first `kept` of the N entries are kept rows (0 < kept <= N).  Run s = 0 .. nseg[0] - 1 in
 * ascending key order covers sorted positions offsets[s] .. offsets[s + 1] - 1; count[s] is its length; order32 [kept] is `order` as the
 * int32 row ids cmr_segment_reduce_f32 takes (mode 2 then gives each run's mean, summed in ascending input index and divided by the count);
 * inverse [N] (or null) = the run of every input row, -1 for dropped rows.  offsets has room for kept + 1 entries, count for kept; entries
 * past nseg[0] (+ 1) are not written.  The caller reads nseg[0] back: the number of runs is a result, so this step cannot be part of a
 * captured graph.  Workspace of cmr_segment_heads_workspace_bytes(N). */
int64_t cmr_segment_heads_workspace_bytes(int64_t N);
int cmr_segment_heads_i64(const int64_t* keys_sorted, const int64_t* order, int64_t N, int64_t kept, int32_t* order32, int32_t* offsets,
                          int32_t* count, int64_t* inverse, int64_t* nseg, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* Surface normals from fixed-radius neighbourhoods (Open3D estimate_normals with KDTreeSearchParamRadius + orient towards a viewpoint;
 * WITHOUT the max_nn cap of its hybrid search).  keys_sorted / order / kept: the rows' keys on the grid cell = radius, origin = (ox, oy, oz),
 * sorted as above.  Row i, kept:
 *   neighbours  the kept rows j (i included) with fp32  (dx dx + dy dy) + dz dz <= radius radius,  d = p_j - p_i, each product, sum and
 *               the square of the radius rounded on its own;  count[i] = their number k;
 *   sums        sum d and sum d d^T in fp32: every lane of a 16-lane group adds the neighbours it meets in sorted order, the 16 partial
 *               sums are added as a balanced tree -- a fixed order for a fixed input order, so two calls agree bit for bit;
 *   covariance  m = sum d / k,  C = sum d d^T / k - m m^T,  from those sums in fp64;
 *   normal      the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi in fp64, eight sweeps), sign such that
 *               n . (viewpoint - p_i) >= 0;  k < max(3, min_neighbors) gives the zero normal and zero eigenvalues;  a degenerate C gives
 *               some finite unit vector;
 *   eigenvalues [N][3] ascending (or null).
 * A dropped row gets the zero normal and count 0.  Outputs are in the input's row order.  points4: scratch of N float4 (16-byte
 * aligned), the kept rows gathered into key order.  The search reads, per (z, y) pair of cells round the query, ONE run of the sorted rows
 * (x is in the key's low bits): 9 runs, found by binary search; a query within rounding of a cell face also reads the cell after next on
 * that side, so that the neighbour set is exactly the one stated. */
int cmr_point_normals_f32(const float* points, int64_t ld, const int64_t* keys_sorted, const int64_t* order, int64_t N, int64_t kept,
                          float ox, float oy, float oz, float radius, float vx, float vy, float vz, int min_neighbors, float* points4,
                          float* normals, int32_t* count, float* eigenvalues, hipStream_t stream);
/* The first step of cmr_point_normals_f32 on its own: points4[i] = (x, y, z, 0) of row order[i], i < kept -- the kept rows in key order as
 * float4 (16-byte aligned).  With keys_sorted and order these are the rows of a GRID INDEX of the cloud (below).  0 < kept < 2^31. */
int cmr_cloud_gather4_f32(const float* points, int64_t ld, const int64_t* order, int64_t kept, float* points4, hipStream_t stream);

/* ---- cloud against cloud: nearest row and point-to-plane ICP on a grid index (csrc/cloud_icp.hip) --------------------
 * Port extension: every pose operation of the reference goes through a camera; these relate one cloud to another.
 *
 * The TARGET is handed over as a grid index, built once and searched by every call: keys_sorted / order = the keys of the target's rows
 * on the grid (origin (ox, oy, oz), cell) in ascending order and the row each came from (cmr_voxel_keys_f32 and a stable sort, as for
 * cmr_point_normals_f32), kept = the number of rows with finite coordinates, points4 = those rows in key order (cmr_cloud_gather4_f32).
 * Rows with a non-finite coordinate are not in the index and are never a match.
 *
 * cmr_cloud_nearest_f32.  Query row i of queries [M][ld >= 3], 0 < M < 2^31:
 *   q      with pose (fp32 [4][4], row-major; its upper 3 x 4 is read) q = R p + t in fp32, every operation rounded on its own, left to
 *          right:  q_x = ((R00 p_x + R01 p_y) + R02 p_z) + t_x  and likewise q_y, q_z;  with pose = null q = p;
 *   d2     of a target row c:  d = c - q in fp32,  d2 = (dx dx + dy dy) + dz dz,  each product and sum rounded on its own (the arithmetic
 *          of cmr_point_normals_f32's neighbour test);
 *   match  the target row with the least d2 among those with d2 <= max_dist max_dist (the square rounded on its own); on equal d2 the
 *          LOWEST row in the target's original order;
 *   idx[i] = that row in the target's original order and d2[i] = its d2;  idx[i] = -1 and d2[i] = NaN when there is none, or when q has a
 *          non-finite coordinate.
 * 0 < max_dist <= cell: a match then lies in the query's cell or one next to it.  One 16-lane group serves a query; per (z, y) pair of
 * cells it reads ONE run of the sorted rows, 9 runs, more for a query within rounding of a cell face, as for cmr_point_normals_f32, so the
 * candidate set holds every row within max_dist whatever the rounding of the cell coordinate.  Queries need not lie inside the target's
 * grid: per axis the cells searched are clamped to [0, 2^21), an empty range on any axis means no candidates, and no key is formed from
 * an index outside that range.  (d2, row) is ordered lexicographically and every output has one writer: the result is exact, and two
 * calls agree bit for bit. */
int cmr_cloud_nearest_f32(const float* queries, int64_t ld, int64_t M, const float* pose, const float* points4,
                          const int64_t* keys_sorted, const int64_t* order, int64_t kept, float ox, float oy, float oz, float cell,
                          float max_dist, int32_t* idx, float* d2, hipStream_t stream);
/* cmr_icp_point_to_plane_f32: the pose T (fp32 [4][4], maps source rows into the target's frame) that minimises the point-to-plane
 * distances of the source rows [M][ld >= 3] to their nearest target rows, by Gauss-Newton from pose_in; the whole loop runs on the device,
 * 2 iters + 2 launches whatever the data.  normals [n][3]: the target's normals in its ORIGINAL row order (n > every entry of order).
 * The working pose is float64.  Iteration k = 0 .. iters - 1 (0 <= iters <= 1000):
 *   match   the working pose rounded to fp32, then every source row as cmr_cloud_nearest_f32 states (q, the matched row c, fp32);
 *   pairs   the rows with a match whose normal n is not the zero vector;
 *   terms   in float64 from the fp32 q, c, n, each operation rounded on its own:  r = (nx (qx - cx) + ny (qy - cy)) + nz (qz - cz),
 *           J = [(q x n)^T, n^T],  w = 1, or with huber > 0:  w = 1 for |r| <= huber, huber / |r| above it  (huber >= 0; 0 = off);
 *   sums    H = sum w J^T J (21 upper-triangle entries, row by row, as (w J_a) J_b),  g = sum (w J) r,  cost = sum (w r) r,  the number of
 *           pairs -- float64 in a fixed order: the rows of a slice of 32 consecutive source rows in 16 interleaved sequences, those added
 *           in order, then the slices in order.  No atomics;
 *   step    H xi = -g by 6 x 6 Cholesky (a pivot must exceed 1e-13 of its diagonal entry), xi = (omega, v);  T <- [exp(omega) | v] T;
 *   stop    when |omega| < tol_rot and |v| < tol_trans: status 0, and every later launch of the call returns at once.
 * Outputs: pose;  trace float64 [iters][4] = {pairs, sqrt(cost / pairs) (0 without pairs), |omega|, |v|} of every executed iteration -- cost
 * and pairs are those of the pose the iteration STARTED from -- and zero rows after the last executed one;  system float64 [iters][28] (or
 * null) = H upper, g, cost per executed iteration, zero after;  status int32 [2] = {code, iterations executed}:
 *   0 converged;  1 iterations exhausted (iters = 0: pose = pose_in);  2 fewer than 6 pairs at some iteration;  3 non-finite sums, a failed
 *   factorisation or a non-finite update.  With 2 and 3 the pose is the one the failing iteration started from; that iteration counts as
 *   executed, its trace row holds pairs and the root mean square and zeros for the step.
 * Workspace of cmr_icp_point_to_plane_workspace_bytes(M), 16-byte aligned.  Two calls agree bit for bit. */
int64_t cmr_icp_point_to_plane_workspace_bytes(int64_t M);
int cmr_icp_point_to_plane_f32(const float* source, int64_t ld, int64_t M, const float* points4, const int64_t* keys_sorted,
                               const int64_t* order, int64_t kept, float ox, float oy, float oz, float cell, const float* normals,
                               const float* pose_in, float max_dist, float huber, int iters, float tol_rot, float tol_trans, float* pose,
                               double* trace, double* system, int32_t* status, void* workspace, int64_t workspace_bytes,
                               hipStream_t stream);

/* ---- registration without a start pose: FPFH descriptors, nearest descriptors, RANSAC over rigid hypotheses (csrc/cloud_fpfh.hip,
 * csrc/cloud_global.hip) ------------------------------------------------------------------------------------------------
 * Port extension.  cmr_icp_point_to_plane_f32 needs a start pose inside its basin; these three find one from the clouds alone.
 *
 * cmr_point_fpfh_f32: the FPFH descriptor (Rusu 2009; the definition is Open3D's ComputeFPFHFeature with a pure radius search) of every row
 * of a cloud handed over as a grid index (above: points4, keys_sorted, order, N rows of which kept are in the index, origin, cell) with its
 * normals [N][3] in the ORIGINAL row order.  0 < radius <= cell.
 *   rows        row i TAKES PART when it is in the index and its normal is finite and not the zero vector; any other row gets all-zero
 *               outputs and is nobody's neighbour;
 *   neighbours  of a row i that takes part: the rows j != i that take part with fp32  (dx dx + dy dy) + dz dz <= radius radius,  d = p_j - p_i
 *               (cmr_point_normals_f32's test); count[i] = their number k;
 *   pair        features in fp64 from the fp32 inputs, EVERY +, -, *, / and sqrt rounded on its own, a dot product summed as (x + y) + z:
 *               d = p_j - p_i, l = sqrt(d . d), l = 0 skips the pair;  a1 = n_i . d / l,  a2 = n_j . d / l;  when |a1| < |a2|:  n1 = n_j,
 *               n2 = n_i, d <- -d, f3 = -a2;  otherwise n1 = n_i, n2 = n_j, f3 = a1;  v = d x n1, |v| = sqrt(v . v), |v| = 0 skips the pair,
 *               v <- v / |v|;  w = n1 x v;  f2 = v . n2;  f1 = atan2(w . n2, n1 . n2)  (a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx));
 *   bins        min(10, max(0, floor(11 x)))  of  x = (f1 + pi) / (2 pi),  (f2 + 1) / 2,  (f3 + 1) / 2  with pi and 2 pi the nearest doubles;
 *   spfh        int32 [N][33] (or null): per row three groups of 11 INTEGER counts over its pairs that were not skipped;  the SPFH VALUE
 *               of a row is (100 count) / k in fp64 (k = 0: zero);
 *   fpfh        float [N][33]:  S[b] = sum over the neighbours j with d2_j > 0 of  value_j[b] / d2_j,  d2 the fp32 number of the
 *               neighbour test widened, the sum in fp64 in a fixed order (every lane of a 16-lane group adds what it meets in sorted
 *               order, then a balanced tree over the lanes; no atomics);  per group of 11  tot = the sum of its S in bin order,
 *               fpfh[b] = fp32(S[b] (100 / tot) + value_i[b]),  with 0 in place of 100 / tot when tot = 0.
 * Outputs are in the input's row order; two launches (SPFH, FPFH); two calls agree bit for bit.  Workspace of
 * cmr_point_fpfh_workspace_bytes(kept), 16-byte aligned: the SPFH table. */
int64_t cmr_point_fpfh_workspace_bytes(int64_t kept);
int cmr_point_fpfh_f32(const float* points4, const int64_t* keys_sorted, const int64_t* order, int64_t N, int64_t kept, float ox, float oy,
                       float oz, float cell, const float* normals, float radius, float* fpfh, int32_t* count, int32_t* spfh,
                       void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* cmr_descriptor_nearest_f32: for every row of queries [M][C] the nearest row of targets [N][C] by brute force, 0 < C <= 64
 * (CMR_EUNSUPPORTED above), M, N > 0.  query_mask / target_mask: bytes [M] / [N], non-zero = selected, null = every row.
 *   d2      in fp32 over c = 0 .. C - 1 in order:  acc = acc + (q_c - t_c) (q_c - t_c),  each operation rounded on its own, from acc = 0;
 *   idx[i]  the selected target row of least d2, the LOWEST row on equal d2;  a target whose d2 is NaN or infinite is no candidate;
 *   d2[i]   its d2;  idx = -1 and d2 = NaN for an unselected query, a query with a non-finite entry, and when no target is a candidate.
 * The targets pass through LDS in tiles; the four waves of a workgroup share 64 queries and split a tile's rows, a lane keeps the least
 * (d2, row) of its query while its rows go by in ascending order, and the four meet in a lexicographic minimum of (d2, row), so the result
 * does not depend on the tiling.  Every output is a plain store by its owner. */
int cmr_descriptor_nearest_f32(const float* queries, int64_t M, const float* targets, int64_t N, int C, const void* query_mask,
                               const void* target_mask, int32_t* idx, float* d2, hipStream_t stream);
/* cmr_ransac_rigid_f32: the rigid transform (R, t) with R a + t = b for most of the correspondences corr int32 [L][2] = (row of source
 * [M][3], row of target [N][3]), 0 < L <= 2^24, by RANSAC over n_hyp (<= 2^20) 3-point hypotheses.  Everything runs on the stream.
 *   list    the rows of corr with 0 <= source row < M, 0 <= target row < N and finite coordinates on both sides, in corr's order; the
 *           others are dropped before anything else;  fewer than 3: status 1;
 *   draws   hypothesis h takes 3 distinct list positions  hash(seed, 0, h, c) % count,  c = 0, 1, ... (at most 32), cmr_pnp_ransac_f32's
 *           hash;  all that follows is fp64 from the fp32 coordinates;
 *   checks  h is INVALID (inlier count -1) when it has no 3 distinct draws; when for one of its edges (0-1, 1-2, 2-0) the shorter of the two
 *           corresponding lengths is below edge_ratio (0 .. 1) times the longer (Open3D's CorrespondenceCheckerBasedOnEdgeLength); when
 *           the triple is collinear on either side:  |e1 x e2|^2 <= 1e-4 |e1|^2 |e2|^2  for e1, e2 the edges from its first point;
 *   fit     the (R, t) minimising sum |R a + t - b|^2 over the three pairs with det R = +1 (Horn's unit quaternion: the top eigenvector
 *           of a symmetric 4 x 4 by cyclic Jacobi, ten sweeps), t = mean b - R mean a;
 *   inlier  a list entry with  |R a + t - b|^2 <= thr thr,  residual and square in fp64 (thr > 0 widened first);
 *   best    the valid hypothesis with most inliers, the lowest h on ties;  none valid: status 2;
 *   refit   the same least squares over best's inlier set -- means, then the centred sums, fp64 in a fixed order without atomics -- and a
 *           recount of the whole list;  the refit is kept when its count is not below best's.
 * Outputs: pose fp32 [4][4];  result int32 [3] = {inliers, status, best h (-1 with status 1 or 2)};  hyp_inliers int32 [n_hyp] (or null).
 * status 0 ok; with 1 and 2 the pose is the identity and inliers 0.  Workspace of cmr_ransac_rigid_workspace_bytes(L, n_hyp), 16-byte
 * aligned.  Integer counts are added atomically (order free); two calls agree bit for bit. */
int64_t cmr_ransac_rigid_workspace_bytes(int64_t L, int n_hyp);
int cmr_ransac_rigid_f32(const float* source, int64_t M, const float* target, int64_t N, const int32_t* corr, int64_t L, int n_hyp,
                         float thr, float edge_ratio, uint32_t seed, float* pose, int32_t* result, int32_t* hyp_inliers, void* workspace,
                         int64_t workspace_bytes, hipStream_t stream);

/* ---- a voxel map of registered scans: insert, merge, forget (csrc/voxel_map.hip) -------------------------------------
 * Port extension.  A MAP is one row per occupied voxel of a fixed grid (origin (ox, oy, oz), voxel; the keys of the section "raw scan ->
 * prepared cloud" above): keys int64 [M] ascending and unique, points fp32 [M][3] and attr fp32 [M][C] = the running means of the rows
 * that fell into the voxel, count int32 [M] = their number, stamp int32 [M] = the stamp of the last insert that touched the voxel.  The
 * library keeps no state: an insert reads a map and a scan and writes a NEW map.  One insert is, in order: cmr_voxel_map_keys_f32, the
 * caller's stable sort of the keys, cmr_segment_heads_i64 and cmr_segment_reduce_f32 (mode 2) over the moved rows and over attr -- the
 * scan's own voxels in ascending key order, exactly as the voxel downsample makes them -- then cmr_voxel_map_plan_i64, a read of its
 * sizes, and cmr_voxel_map_write_f32.  No re-sort of the map and no atomics; every output has one writer; two calls agree bit for bit.
 *
 * cmr_voxel_map_keys_f32.  Row i of points [N][ld >= 3], 0 < N < 2^31, in one pass:
 *   q        with pose (fp32 [4][4], row-major, upper 3 x 4 read) q = R p + t as cmr_cloud_nearest_f32 states it, every operation rounded
 *            on its own;  with pose = null q = p;  moved[i] = q  (fp32 [N][3], written for every row);
 *   dropped  p or q has a non-finite coordinate:  keys[i] = -1;
 *   outside  else, on some axis  floorf((q - origin) / voxel)  -- one IEEE subtraction, one IEEE division, the arithmetic of the keys above --
 *            is below 0 or above 2^21 - 1, the comparison made on the float (so +-inf is outside):  keys[i] = -2;
 *   key      else cz << 42 | cy << 21 | cx of the three cells.
 * Both marks sort in FRONT of every cell (a key takes all 63 bits: 2^63 - 1 is the key of the last cell, so nothing sorts behind them):
 * after the sort the kept rows are the last N - dropped - outside entries, and those are what cmr_segment_heads_i64 is handed.
 * counts int64 [2] = {dropped, outside}, summed without atomics.  Workspace of cmr_voxel_map_keys_workspace_bytes(N). */
int64_t cmr_voxel_map_keys_workspace_bytes(int64_t N);
int cmr_voxel_map_keys_f32(const float* points, int64_t ld, int64_t N, const float* pose, float ox, float oy, float oz, float voxel,
                           int64_t* keys, float* moved, int64_t* counts, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* cmr_voxel_map_plan_i64: where the rows of a map (M >= 0 rows) and of a scan (S >= 0 voxels: run s of cmr_segment_heads_i64 over
 * keys_sorted, its key keys_sorted[offsets[s]]) go in the new map;  0 < M + S < 2^31.  0 <= stamp, min_stamp < 2^31.
 *   hit      a scan voxel whose key the map holds, and that map row;  every scan voxel is located in the map's keys and every map row in
 *            the scan's by binary search;  a scan voxel that is no hit is a MISS;
 *   stamps   after the insert a hit map row and a miss carry `stamp`, every other map row its own;
 *   kept     a map row or a miss whose stamp after the insert is not below min_stamp (min_stamp = 0 keeps everything);  the new map is
 *            the kept rows of both sides in ascending key order, a row's place the number of kept rows with a smaller key, from exclusive
 *            prefix sums of the keep flags of either side (tiles of 1024, int32, 64-bit row arithmetic);
 *   sizes    int64 [4] = {rows of the new map, new = misses, merged = hits, removed = M + new - rows}.
 * The caller reads sizes back to allocate the new map, so an insert cannot be part of a captured graph.  Workspace of
 * cmr_voxel_map_plan_workspace_bytes(M, S), 16-byte aligned; it holds the plan and is handed on, unchanged, to cmr_voxel_map_write_f32.
 * S = 0 with min_stamp > 0 is a pure prune.  The map's keys are taken as ascending and unique; whatever they are, no write of either
 * call leaves the new map's rows. */
int64_t cmr_voxel_map_plan_workspace_bytes(int64_t M, int64_t S);
int cmr_voxel_map_plan_i64(const int64_t* map_keys, const int32_t* map_stamp, int64_t M, const int64_t* keys_sorted, const int32_t* offsets,
                           int64_t S, int stamp, int min_stamp, int64_t* sizes, void* workspace, int64_t workspace_bytes,
                           hipStream_t stream);
/* cmr_voxel_map_write_f32: the new map's `rows` rows (sizes[0] of the plan in `workspace`; the other arguments as the plan took them),
 * each written once by the thread that owns it, with plain stores.  scan_points [S][3], scan_attr [S][C], scan_count int32 [S]: the scan's
 * voxels (means and run lengths).  C >= 0 attribute channels (attr pointers may be null when C = 0).
 *   a kept map row that is no hit     copied, with its count and stamp;
 *   a kept miss                       the scan voxel's means and count, and `stamp`;
 *   a kept hit (ca, ma | cb, mb)      n = min(ca + cb, 2^31 - 1) taken in int64,  w = (float) cb / (float) n  (one IEEE division),  and per
 *                                     component of points and attr  m' = ma + w (mb - ma):  a subtraction, a product and a sum, each
 *                                     rounded on its own (no fused operation);  count n, and `stamp`. */
int cmr_voxel_map_write_f32(const int64_t* map_keys, const float* map_points, const float* map_attr, const int32_t* map_count,
                            const int32_t* map_stamp, int64_t M, const float* scan_points, const float* scan_attr, const int32_t* scan_count,
                            int64_t S, int C, int stamp, int min_stamp, const void* workspace, int64_t workspace_bytes, int64_t rows,
                            int64_t* keys, float* points, float* attr, int32_t* count, int32_t* stamps, hipStream_t stream);

/* ---- free space in a voxel map: the rays of a scan cast through it (csrc/voxel_map_rays.hip) ---------------------------
 * Port extension.  Row i of points [N][ld >= 3], 0 < N < 2^31, is a beam from the sensor to its return; the cells of the map's grid
 * (origin (ox, oy, oz), voxel) between the two were empty when the scan was taken.  keys int64 [M], M >= 0: a map's keys, ascending and
 * unique.  Nothing in the map changes and the library keeps no state.  Everything below is fp32, every operation rounded on its own
 * (no fused operation), so that every integer is exact.
 *   ends      with pose (fp32 [4][4], row-major, upper 3 x 4 read) the sensor is o = t and the end q = R p + t, the moved row of
 *             cmr_voxel_map_keys_f32;  with pose = null  o = (0, 0, 0), q = p;
 *   dropped   p or q has a non-finite coordinate;
 *   outside   else, o or q lies off the grid on some axis: cmr_voxel_map_keys_f32's test, floorf((x - origin) / voxel) below 0 or above
 *             2^21 - 1, the comparison made on the float;
 *   per axis  a = (o - origin) / voxel,  b = (q - origin) / voxel,  start cell s = floorf(a),  end cell e = floorf(b),  d = b - a,
 *             left = |e - s|,  step = sign(e - s);
 *   long      else, left_x + left_y + left_z > max_cells (1 <= max_cells <= 65 536): the ray is not cast.  The cap bounds every
 *             lane's loop whatever the input;
 *   cast      else.  The walk starts in s and makes exactly left_x + left_y + left_z steps of one cell along one axis: the axis with the
 *             least tmax, ties going to x before y before z, where  tmax_i = +inf  once left_i = 0 and otherwise
 *             tmax_i = ((float) (c_i + (step_i > 0 ? 1 : 0)) - a_i) / d_i  of the cell c the walk is in -- recomputed from the integer
 *             cell after every step on axis i, never accumulated;  an axis with left_i = 0 is never divided on (d_i = 0 never divides,
 *             a ray of length zero makes no step).  The walk therefore ends in e whatever the rounding did on the way, and the key of e
 *             is, bit for bit, the key cmr_voxel_map_keys_f32 gives the row;
 *   hits      the map holds the key of e at row r:  hits[r] += 1;
 *   crossed   every cell c the walk visits other than e (s included) with  max_i |c_i - s_i| > start_margin  and
 *             max_i |c_i - e_i| > end_margin  (Chebyshev distances in cells; both margins >= 0) whose key the map holds at row r:
 *             crossed[r] += 1.
 * crossed, hits int32 [M] (may be null when M = 0): zeroed by the call, then integer sums by atomic add -- order free, two calls agree
 * exactly.  counts int64 [4] = {cast, dropped, outside, long}, per-workgroup totals added by one workgroup; they sum to N.  A row index
 * only ever comes out of a search over [0, M) that found an equal key there: whatever keys are handed over, no store leaves
 * crossed[0, M), hits[0, M) and counts.  Workspace of cmr_voxel_map_rays_workspace_bytes(N). */
int64_t cmr_voxel_map_rays_workspace_bytes(int64_t N);
int cmr_voxel_map_rays_f32(const int64_t* keys, int64_t M, float ox, float oy, float oz, float voxel, const float* points, int64_t ld,
                           int64_t N, const float* pose, int start_margin, int end_margin, int max_cells, int32_t* crossed, int32_t* hits,
                           int64_t* counts, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- place recognition between scans: ring-and-sector descriptors and their ring-shift match (csrc/scan_descriptor.hip) ----
 * Port extension.  Scan Context (Kim & Kim, IROS 2018) restated so that every integer follows from stated fp32 operations: no atan2, and
 * every operation below is rounded on its own (no fused operation).  1 <= R <= 64 rings, 4 <= S <= 256 sectors, S % 4 = 0, R S <= 4096;
 * any other (R, S) returns CMR_EUNSUPPORTED (-3).  The library keeps no state.
 *
 * cmr_scan_descriptor_f32: points [N][ld >= 3], 0 < N < 2^31 -> desc float [R][S] and counts int64 [3] = {binned, dropped, outside}, which
 * sum to N.  Two device tables, which the caller computes in fp64 and rounds to fp32:
 *   ring_edge2  float [R + 1]:        ring_edge2[j] = (min_range + (max_range - min_range) j / R)^2;
 *   sector_dir  float [S / 4 - 1][2]: sector_dir[k - 1] = (c_k, s_k) = (cos, sin)(k 2 pi / S), k = 1 .. S / 4 - 1 (may be null when S = 4).
 * Per row (x, y, z):
 *   dropped   x, y or z is not finite;
 *   ring      else r2 = fp32(fp32(x x) + fp32(y y));  the row is OUTSIDE when r2 < ring_edge2[0] or r2 >= ring_edge2[R];  otherwise its ring
 *             is the number of j in 1 .. R - 1 with r2 >= ring_edge2[j];
 *   quadrant  (u, v) = the row turned into the first quadrant by exact swaps and negations:  q = 0: x > 0 and y >= 0, (x, y);
 *             q = 1: x <= 0 and y > 0, (y, -x);  q = 2: x < 0 and y <= 0, (-x, -y);  q = 3: x >= 0 and y < 0, (-y, x);  x = y = 0: q = 0, (0, 0);
 *   sector    q S / 4 + m,  m = the number of k in 1 .. S / 4 - 1 with fp32(v c_k) >= fp32(u s_k); the value is that count, found by
 *             binary search (below);
 *   value     fp32(z + height)  (height: the sensor's height above the ground, finite);
 *   binned    every row that is neither dropped nor outside.
 * A cell of desc holds the largest value over its binned rows, and 0 when none of them is above 0: desc is zeroed by the call, then an
 * integer atomic max of the values' bit patterns (those of floats above 0 order like integers), per workgroup in LDS and then into desc;
 * the counts are integer atomic sums.  All of it is order free: two calls agree bit for bit.  The azimuth comparisons -- the sector's
 * here, the column's of cmr_range_image_f32 -- are monotone in the table index for a table made as above (an fp32 product is monotone in
 * each factor, c_k descends, s_k ascends, u, v >= 0): those that hold are the first m, so both entry points find m by bisecting the table
 * (csrc/cmr_scan_rows.h) instead of counting.  The ring is a count of at most R - 1 comparisons and m the lower end of a search over
 * [0, S / 4 - 1]: they lie in [0, R) and [0, S) whatever the rows and the tables hold, and no store leaves desc[0, R S) and counts[0, 3).
 *
 * cmr_scan_match_f32: queries float [Q][R][S] against cands float [N][R][S] (0 < Q, N < 2^31; values taken as finite) -> dist float [Q][N],
 * shift int32 [Q][N].  limit int32 [Q] or null: query q is compared with the candidates [0, limit[q]) only, 0 <= limit[q] <= N (null: all N;
 * a value outside that range acts as the nearer end of it).  1 <= min_cols <= S.
 *   unit columns  per descriptor and column  n2 = sum over r of fp32(a_r a_r),  from 0 in ring order, every sum rounded;  the column is EMPTY
 *                 when n2 == 0;  otherwise e_r = fp32(a_r / sqrtf(n2)),  square root and division correctly rounded;
 *   shift k       0 .. S - 1: over j = 0 .. S - 1 in order, query column j meets candidate column (j + k) mod S;  when neither is empty
 *                 dot = sum over r of fp32(eq_r ec_r)  from 0 in ring order, every sum rounded, then  sum = fp32(sum + dot)  and  cnt += 1;
 *                 the shift COUNTS when cnt >= min_cols, and its distance is then  fp32(1 - fp32(sum / fp32(cnt)));
 *   outputs       the least distance over the shifts that count and the lowest such shift on equal distances (a distance that is NaN, which
 *                 finite descriptors never give, is passed over);  NaN and -1 when no shift counts, and for every candidate at or beyond
 *                 limit[q].
 * Every output is written once, by the thread that owns it, with a plain store, and the order of every sum is the one above whatever the
 * tiling: two calls agree bit for bit.  Query and candidate indices are guarded at the stores: no store leaves dist, shift and the
 * workspace.  Workspace of cmr_scan_match_workspace_bytes(Q, N, R, S) (the unit columns and the empty flags of both sides), 16-byte aligned. */
int cmr_scan_descriptor_f32(const float* points, int64_t ld, int64_t N, int R, int S, const float* ring_edge2, const float* sector_dir,
                            float height, float* desc, int64_t* counts, hipStream_t stream);
int64_t cmr_scan_match_workspace_bytes(int64_t Q, int64_t N, int R, int S);
int cmr_scan_match_f32(const float* queries, int64_t Q, const float* cands, int64_t N, int R, int S, const int32_t* limit, int min_cols,
                       float* dist, int32_t* shift, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- a pose-graph solve over a chain of poses and its loop edges (csrc/pose_graph.hip) ----------------------------------
 * Port extension: the reference has no counterpart.  Everything is float64.
 *
 * NODES   poses [F][4][4] row-major, X_n = (R_n, t_n) maps frame n into the first frame; the upper 3 x 4 is read.
 * EDGES   edges int32 [E][2] = (i, j), meas [E][4][4] = Z_e, which maps frame i into frame j (Z ~ inv(X_j) X_i), weights [E][2] =
 *         (w_rot, w_trans), finite and >= 0.  An edge whose indices do not name two different nodes has zero terms.
 * RESIDUAL  R_D = R_Z^T R_j^T R_i,  t_D = R_Z^T (R_j^T (t_i - t_j) - t_Z);  r = (phi, rho), rho = t_D, phi = Log(R_D) from the
 *         antisymmetric part:  a = 1/2 (R32 - R23, R13 - R31, R21 - R12), s = |a|, c = (trace - 1) / 2, theta = atan2(s, c),
 *         phi = (theta / s) a, with theta / s = 1 + s^2 / 6 for s < 1e-8.  An edge with theta > 3 is WIDE: Log loses its digits near pi
 *         and such an edge is a wrong loop, not a measurement; wide edges are counted.
 * JACOBIAN  for the left increment X <- [Exp(w) | v] X, xi = (w, v):
 *           d r / d xi_i = J = [[Jr^-1(phi) R_i^T, 0], [-R_Z^T R_j^T [t_i]x, R_Z^T R_j^T]],  d r / d xi_j = -J,
 *         Jr^-1(phi) = I + 1/2 [phi]x + k [phi]x^2,  k = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta),  k = 1/12 for theta < 1e-4.
 * WEIGHT  chi^2 = w_rot |phi|^2 + w_trans |rho|^2.  huber = k > 0:  s_e = 1 and cost 1/2 chi^2 for chi <= k, s_e = k / chi and cost
 *         k chi - 1/2 k^2 above;  huber = 0: s_e = 1 always.  The cost is formed from the ROUNDED chi, every operation rounded on its
 *         own, as (0.5 chi) chi and k chi - (0.5 k) k: an edge's cost follows from its chi bit for bit.  A_e = s_e J^T W J (21 upper entries, row by row), b_e = s_e J^T W r,
 *         W = diag(w_rot x 3, w_trans x 3).
 *
 * cmr_pose_graph_linearize_f64: per edge r [E][6], chi [E], scale [E] = s_e, A [E][21], b [E][6]; cost [1] = the sum of the edges' costs
 * (the lanes of a workgroup of 256 consecutive edges by the wave butterfly and then in wave order, the workgroups' slots in slot order);
 * wide int32 [1].  0 < F, E with 6 F < 2^31 and 28 E < 2^31.  Workspace of cmr_pose_graph_linearize_workspace_bytes(E), 16-byte aligned.
 *
 * cmr_pose_graph_optimize_f64: Gauss-Newton from poses_in, the whole loop on the device and on the caller's stream, in
 * 2 (iters + 1) + iters (2 + 2 cg_iters) + 2 launches whatever the data (0 <= iters <= 100, 0 <= cg_iters <= 4096).
 *   system  J_j = -J_i, so H = sum_e (E_i - E_j) A_e (E_i - E_j)^T + damping I and g = sum_e (E_i - E_j) b_e: a graph Laplacian with 6 x 6
 *           weights.  Nodes with fixed[n] != 0 (bytes [F]) are removed: their rows of every vector are 0 and they do not move.
 *   sums    a node's incident edges are added in INCIDENCE order: inc_offsets int32 [F + 1] and inc_edges int32 [2 E] are the CSR of the
 *           incidence, a node's edge numbers ascending (which end of the edge the node is, is read from edges).  A dot product is six
 *           components in order per node, the nodes of a workgroup of 256 by the wave butterfly and then in wave order, the workgroups'
 *           slots in slot order.  No atomics, one writer per slot: two calls agree bit for bit.
 *   solve   H delta = -g by preconditioned conjugate gradients, matrix-free.  Preconditioner: M_n = sum_{e at n} A_e + damping I, inverted
 *           once per outer iteration (the 6 x 6 Cholesky of the pose refinement against the six unit vectors; a pivot must exceed 1e-13 of
 *           its diagonal entry).  x_0 = 0, r_0 = -g, z = M^-1 r, p = z; then q = H p (q_n = sum_{e at n} +- A_e (p_i - p_j), then
 *           + damping p_n), alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M^-1 r, beta = r.z / (previous r.z), p = z + beta p.
 *           It stops before iteration c when r.z <= cg_tol^2 (r_0.z_0), after cg_iters, or at a p.q that is not positive and finite.
 *   step    X_n <- [Exp(dw_n) | dv_n] X_n, delta_n = (dw_n, dv_n).
 *   rules   the cost is evaluated at the stepped poses.  A step with max_n |dw_n| <= tol_rot and max_n |dv_n| <= tol_trans stands and ends
 *           the loop (status 0) -- it changes the cost by less than the cost's rounding, so the costs are not compared.  Any other step
 *           whose cost is not below the cost before it is undone and ends the loop (status 0); else it stands and the loop goes on.  The
 *           last step's cost is evaluated too, so iters steps take iters + 1 linearisations.
 * Outputs: poses [F][4][4];  cost [1] = the cost at them;  trace [iters][5] = {cost the step started from, CG iterations used,
 * sqrt(r.z / r_0.z_0) at the end of CG, max |dw|, max |dv|} per executed step, zero rows after;  status int32 [3] = {code, steps executed
 * (an undone one counts), wide edges at the start}:
 *   0 converged, by either rule;  1 iterations exhausted;  2 a free node's block does not factor (a free node without edges at damping = 0
 *   is one), or a cost or an update is not finite: the poses are those the failing step started from;  3 wide edges at the start: nothing
 *   is solved, poses = poses_in.
 * Indices are guarded at every load and store that depends on them: whatever edges, inc_offsets and inc_edges hold, nothing outside the
 * arrays is touched.  Workspace of cmr_pose_graph_optimize_workspace_bytes(F, E), 16-byte aligned. */
int64_t cmr_pose_graph_linearize_workspace_bytes(int64_t E);
int cmr_pose_graph_linearize_f64(const double* poses, int64_t F, const int32_t* edges, const double* meas, const double* weights, int64_t E,
                                 double huber, double* r, double* chi, double* scale, double* A, double* b, double* cost, int32_t* wide,
                                 void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t cmr_pose_graph_optimize_workspace_bytes(int64_t F, int64_t E);
int cmr_pose_graph_optimize_f64(const double* poses_in, int64_t F, const int32_t* edges, const double* meas, const double* weights, int64_t E,
                                const int32_t* inc_offsets, const int32_t* inc_edges, const uint8_t* fixed, double huber, int iters,
                                int cg_iters, double cg_tol, double damping, double tol_rot, double tol_trans, double* poses, double* cost,
                                double* trace, int32_t* status, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- range images and virtual scans of a cloud from a sensor pose (csrc/range_image.hip) ---------------------------------
 * Port extension: what a spinning LiDAR standing at a pose would see of a cloud, as a spherical z-buffer.  Every integer follows from
 * stated fp32 operations: no atan2, no sqrt, and every operation below is rounded on its own (no fused operation).  1 <= rows <= 128,
 * 4 <= cols <= 4096, cols % 4 = 0, rows cols <= 2^19; any other shape returns CMR_EUNSUPPORTED (-3).  The library keeps no state.
 *
 * cmr_range_image_f32: points [N][ld >= 3], 0 < N < 2^31; pose float [4][4] row-major or null -> index int32 [rows][cols] (-1 where
 * empty), dist2 float [rows][cols] (the quiet NaN 0x7fc00000 where empty) and counts int64 [3] = {binned, dropped, outside}, which sum to
 * N.  min_range2 and max_range2 are the squared ranges, 0 < min_range2 < max_range2 < inf.  Two device tables, which the caller computes in
 * fp64 and rounds to fp32 (R = rows, C = cols):
 *   elev     float [R + 1][2]:     elev[j] = (s_j, q_j) = (sign(tan e_j) as -1, 0 or 1, tan^2 e_j) of the edge angle
 *                                  e_j = elev_lo + (elev_hi - elev_lo) j / R,  -pi/2 < elev_lo < elev_hi < pi/2;
 *   col_dir  float [C / 4 - 1][2]: col_dir[k - 1] = (c_k, s_k) = (cos, sin)(k 2 pi / C), k = 1 .. C / 4 - 1 (may be null when C = 4).
 * Per row (px, py, pz):
 *   pose      with a pose, (x, y, z) = R p + t as the cloud kernels move a row:  x = fp32(fp32(fp32(fp32(R00 px) + fp32(R01 py)) +
 *             fp32(R02 pz)) + t0), y and z alike;  without one, (x, y, z) = (px, py, pz);
 *   dropped   a coordinate that is not finite, before or after the pose;
 *   range     xx = fp32(x x), yy = fp32(y y), zz = fp32(z z), r2 = fp32(xx + yy), d2 = fp32(r2 + zz);  the row is OUTSIDE when
 *             d2 < min_range2 or d2 >= max_range2 (an infinite d2 is).  This test comes before any table is read;
 *   above(j)  "the elevation is at or above e_j", with rhs = fp32(r2 q_j):   s_j > 0:  z >= 0 and zz >= rhs;   s_j = 0:  z >= 0;
 *             s_j < 0:  z >= 0 or zz <= rhs;
 *   row       the row is OUTSIDE when above(0) fails or above(R) holds;  otherwise its image row is the number of j in 1 .. R - 1 for
 *             which above(j) holds: image row 0 is the lowest elevation;
 *   column    (u, v) and the quadrant q of (x, y) exactly as cmr_scan_descriptor_f32 takes them, x = y = 0 included;  m = the number of k
 *             in 1 .. C / 4 - 1 with fp32(v c_k) >= fp32(u s_k);  the column is q C / 4 + m;
 *   binned    every row that is neither dropped nor outside falls into the cell (image row, column).
 * A cell's winner is its binned row with the least d2, the lowest input row on equal d2: a 64-bit unsigned atomic minimum of
 * (bits of d2) << 32 | row, the bits of a float above 0 ordering like the float, over an image initialised to all ones; the counts are
 * integer atomic sums.  All of it is order free: two calls agree bit for bit, whatever the launch shape.  The column's comparisons are
 * monotone in the table index as cmr_scan_descriptor_f32's paragraph argues, and so are above(j) for a table made as above (an fp32
 * product is monotone in each factor, q_j descends where it is used), so the kernel finds the two counts by binary search; either way
 * they are bounded by R - 1 and C / 4 - 1 whatever the rows and the tables hold, and no store leaves index, dist2, counts and the
 * workspace.
 * Workspace of cmr_range_image_workspace_bytes(rows, cols) = 8 rows cols bytes (the packed image; 0 for a shape not served), 16-byte aligned.
 *
 * cmr_range_visible_f32: dist2 float [rows][cols] as above -> visible uint8 [rows][cols].  A cell that has a winner is visible iff
 * d2 <= fp32(m2 factor), m2 = the least dist2 over the cells (r + dr, (c + dc) mod cols) with |dr| <= radius_rows, |dc| <= radius_cols:
 * image rows are clipped at the border, columns wrap, empty cells (NaN) are passed over and the cell itself is included.  An empty cell is
 * not visible.  factor = fp32((1 + rel_tol)^2), formed by the caller in fp64, finite and >= 1.  The window a cell reads, after clipping
 * (min(2 radius_rows + 1, rows) rows of min(2 radius_cols + 1, cols) columns), holds at most 1024 cells.  One cell per thread, plain
 * stores by the owner. */
int64_t cmr_range_image_workspace_bytes(int rows, int cols);
int cmr_range_image_f32(const float* points, int64_t ld, int64_t N, const float* pose, int rows, int cols, const float* elev,
                        const float* col_dir, float min_range2, float max_range2, int32_t* index, float* dist2, int64_t* counts,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cmr_range_visible_f32(const float* dist2, int rows, int cols, int radius_rows, int radius_cols, float factor, uint8_t* visible,
                          hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CMR_HIP_H */
