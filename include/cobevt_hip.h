/*
 * cobevt_hip.h — C ABI of libcobevt_hip.so: the MI355X (gfx950) kernels behind the CoBEVT FAX hot path.
 *
 * The reference (DerrickXuNu/CoBEVT) has no FFI: its hot path is Python nn.Modules calling ATen.  The
 * drop-in boundary is therefore the nn.Module API (cobevt_amd/host/, same class names / constructor
 * arguments / state_dict keys / forward contracts); those modules bind the entry points below through
 * ctypes (cobevt_amd/lib.py).  Every entry point cites the reference code whose arithmetic it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C types only: device pointers (hipMalloc'ed / torch data_ptr()), ints, floats, a hipStream_t.
 *   - all work is enqueued asynchronously on `stream`; nothing is allocated, nothing synchronises.
 *   - return value: 0 = COBEVT_OK, otherwise an error code (see cobevt_strerror); on error nothing was launched.
 *   - dtype code: 0 = bf16 storage + bf16 MFMA + fp32 accumulate ; 1 = fp32 storage (parity modes); the matrix path of
 *     dtype 1 is a property of the LIBRARY - the same sources and the same ABI are built three times (cobevt_amd/build.py):
 *       libcobevt_hip.so       exact v_mfma_f32_32x32x2_f32
 *       libcobevt_hip_f32s.so  every product as two v_mfma_f32_32x32x16_bf16 over (hi, lo) bf16 halves (-DCOBEVT_F32_SPLIT=1; ~1e-5 end to end)
 *       libcobevt_hip_f32h.so  v_mfma_f32_32x32x16_f16 with fp16 operands, the weight-side operand as ONE fp16 term (-DCOBEVT_F32_SPLIT=2):
 *                              the ResNet encoder's library under host.set_compute_dtype("fp32_fast"), not meant for any other launch
 *     (csrc/common.hpp; dtype 0 is identical in all three).
 *   - activations are channels-last ("NHWC", token-major); weights are [Cout][Kpad] with
 *     k = (kh*Kw + kw)*Cin + c, zero padded to a multiple of 32 (bf16) / 16 (fp32) elements.
 */
#ifndef COBEVT_HIP_H
#define COBEVT_HIP_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COBEVT_OK 0
#define COBEVT_ERR_ARG 1
#define COBEVT_ERR_SHAPE 2
#define COBEVT_ERR_LAUNCH 3
#define COBEVT_ERR_UNSUPPORTED 4

int cobevt_abi_version(void);
const char* cobevt_strerror(int code);

/*
 * Implicit-GEMM convolution / linear layer with fused prologue + epilogue.
 * Replaces: torchvision ResNet convs + folded BatchNorm + ReLU + residual add called from
 *   opv2v/opencood/models/backbones/resnet_ms.py:67-74; nn.Linear / 1x1 convs of
 *   opv2v/opencood/models/sub_modules/fax_modules.py:107,114-117,189-193,281-292,311-312,472-489;
 *   opv2v/opencood/models/fusion_modules/swap_fusion_modules.py:45-53; base_transformer.py:112-124;
 *   naive_decoder.py:78-87 (nearest x2 up-sampling folded into the gather); bev_seg_head.py:35-61;
 *   nuscenes/cross_view_transformer/model/{encoder_pyramid_axial.py:515-526, decoder.py:12-34, cvt.py:29-33}.
 * dims (int32[21]): dtype, N, H, W, Cin, Ho, Wo, Cout, Kh, Kw, stride, pad, K, Kpad, upsample(0/1),
 *   pre_relu(0/1), act(0 none,1 ReLU,2 exact GELU), store_mode(0 NHWC dtype,1 PixelUnshuffle(2) NHWC dtype,
 *   2 NCHW fp32, 3 NHWC fp32), out_H, out_W (dims of a possibly zero-padded output map, modes 0/3),
 *   smallc (1: `in` is fp32 NHWC with tiny Cin, taps decoded through klut[Kpad] = kh<<20|kw<<10|c, -1 = pad).
 * pre_scale/pre_shift (fp32[Cin], nullable): a <- a*scale+shift (+ReLU if pre_relu) applied to the gathered
 *   input (pre-activation BatchNorm->ReLU->1x1 conv).  bias fp32[Cout] nullable.  residual: same dtype,
 *   (N,Ho,Wo,Cout), nullable, added before the activation.
 */
int cobevt_conv2d_nhwc(const void* in, const void* wgt, const float* bias, const void* residual,
                       const float* pre_scale, const float* pre_shift, const int* klut, void* out,
                       const int* dims, hipStream_t stream);

/*
 * Transposed convolution with kernel = stride = s (no overlapping taps) + folded eval BatchNorm + activation, written pixel-shuffled
 * into a channel slice of a wider NHWC map.  Replaces: the deblocks nn.ConvTranspose2d(Cin, Cout, s, stride=s, bias=False) ->
 * BatchNorm2d -> ReLU of opv2v/opencood/models/backbones/base_bev_backbone.py:58-69,85-90 and the torch.cat of their outputs (:113):
 *   out[n, s*y + dy, s*x + dx, c_off + co] = act(shift[co] + sum_ci in[n, y, x, ci] * wgt[(dy*s + dx)*Cout + co][ci])
 * in (N,H,W,Cin) NHWC and out (N, s*H, s*W, ldc) NHWC in the compute dtype; wgt [s*s*Cout][Kpad] in the compute dtype, tap-major rows
 * with the BatchNorm scale folded in, columns >= Cin zero; shift fp32[Cout].  One GEMM (M = N*H*W, K = Cin, s*s*Cout columns) on
 * the matrix path of the library it is linked into; every element of out[..., c_off : c_off + Cout] is written exactly once with
 * 16-byte stores, nothing else of `out` is touched (no atomics, no zero-fill needed).  s = 1 is a 1x1 convolution into a slice.
 * dims (int32[11]): dtype (0 bf16, 1 fp32), N, H, W, Cin, Cout, Kpad, s, c_off, ldc, act (0 none, 1 ReLU, 2 GELU, 3 swish, 4 sigmoid).
 * COBEVT_ERR_SHAPE unless 1 <= s <= 8, Cin % 8 == 0 (bf16) / % 4 == 0 (fp32), Cout % 32 == 0, Kpad >= Cin and Kpad % 32 == 0 (bf16) /
 * % 16 == 0 (fp32), c_off % 8 == 0, ldc % 8 == 0, c_off + Cout <= ldc, and N*H*W*s*s < 2^31.
 */
int cobevt_deconv_nhwc(const void* in, const void* wgt, const float* shift, void* out, const int* dims, hipStream_t stream);

/*
 * 3x3 / stride 1 / pad 1 convolution with an LDS-resident input patch (the fast path of cobevt_conv2d_nhwc for the
 * ResNet BasicBlocks resnet_ms.py:67-74, FAX Bottleneck / downsample convs fax_modules.py:472-489 and NaiveDecoder
 * naive_decoder.py:78-87).  Weights [Cout][Cin/cc][9][cc].  dims (int32[10]): dtype, N, H, W, Cin, Cout,
 * upsample(0/1: input is read through a nearest x2 up-sampling), act, store_mode (0 NHWC, 1 PixelUnshuffle(2)),
 * cc = channels per chunk (bf16: 64|32, fp32: 32|16; Cin % cc == 0).
 */
int cobevt_conv3x3_nhwc(const void* in, const void* wgt, const float* bias, const void* residual, void* out,
                        const int* dims, hipStream_t stream);

/*
 * The same 3x3 / stride 1 / pad 1 convolution (same reference call sites as cobevt_conv3x3_nhwc) with the weights
 * pre-ordered as MFMA B fragments, [Cout_p/32][Cin/cc][9 taps][4 k-groups][64 lanes][16 bytes] where lane = 32*half +
 * (cout % 32) holds bytes [32*kgroup + 16*half, +16) of that cout's 128-byte channel chunk and Cout_p >= Cout is the
 * zero-padded row count (multiple of 128): every weight operand is one coalesced 1-KB wave load from L2, LDS only holds
 * the input patch and there is one barrier per channel chunk instead of one per tap.  A workgroup owns MT strips of
 * 2 x 16 output pixels (numbered across image, row pair, column block) x 128 or 64 couts.  dims (int32[13]): dtype, N,
 * H, W, Cin, Cout, upsample, act, store_mode (0 NHWC, 1 PixelUnshuffle(2)), cc (bf16: 64, fp32: 32), Cout_p, variant =
 * 100 + 10*MT + (1 for 64-cout tiles; 3 = 32-cout tiles in four-wave workgroups, bf16 / stride 1, MT in 1..5), MT in 3..6
 * (0 = MT 5); the host picks MT so that the grid is a whole number of
 * workgroups per CU (cobevt_amd/ops.py conv3_tiling); stride (1, or 2 = the first conv of a down-sampling BasicBlock:
 * out (Ho, Wo) = ((H-1)/2+1, (W-1)/2+1), plain NHWC store, no up-sampling).  Needs N*H*W*Cin < 2^31.
 */
int cobevt_conv3x3_wfrag_nhwc(const void* in, const void* wfrag, const float* bias, const void* residual, void* out,
                              const int* dims, hipStream_t stream);

/*
 * The SECOND 3x3 convolution of a down-sampling BasicBlock together with the block's projection shortcut (torchvision
 * resnet.BasicBlock.forward with `downsample`, layer3.0 / layer4.0 as reached from resnet_ms.py:67-74), bf16:
 *     out = act(conv3x3(in; W2) + bias + bf16(conv1x1/stride2(in2; Wd) + bias2))      eval BatchNorms folded
 * in (N, H, W, Cin) = the block's first convolution's output, in2 (N, H2, W2, Cin2) = the block's input with
 * ((H2-1)/2+1, (W2-1)/2+1) = (H, W).  One launch instead of two (the shortcut's dense-row launch and its 2 x N*H*W*Cout
 * bytes of round trip go): behind the 3x3's channel chunks every wave computes the complete shortcut sum of some of its
 * output tiles from in2(2 oy, 2 ox), rounds it to bf16 as the separate launch stores it and adds it to its partial sum of
 * the 3x3 - the result differs from the two-launch path by fp32 summation order only.  wfrag: per
 * 32-cout tile the Cin/64 * 9 steps of cobevt_conv3x3_wfrag_nhwc's table followed by Cin2/64 steps of the same
 * [4 k-groups][64 lanes][16 bytes] shape built from Wd.  dims (int32[12]): dtype (0), N, H, W, Cin, Cout, act, Cout_p,
 * variant (100 + 10*MT + (1 for 64-cout tiles), MT in 3..5), H2, W2, Cin2; Cin % 64 == Cin2 % 64 == 0, Cin2 <= 256.
 */
int cobevt_conv3x3_ds_wfrag_nhwc(const void* in, const void* in2, const void* wfrag, const float* bias, const float* bias2, void* out,
                                 const int* dims, hipStream_t stream);

/*
 * Fused ResNet BasicBlock (stride 1, no downsample, C in {64, 128}): out = ReLU(conv2(ReLU(conv1(x) + b1)) + b2 + x) with
 * the eval BatchNorms folded into the weights / biases - torchvision resnet.BasicBlock.forward as reached from
 * resnet_ms.py:67-74 (layer1 / layer2 of the camera encoder).  One launch instead of two 3x3 launches: the intermediate
 * map stays in LDS (conv1 is recomputed on the 1-pixel halo conv2 needs) and is rounded to the storage type exactly as
 * the two-launch path stores it.  wfrag1 / wfrag2: the fragment-ordered tables of cobevt_conv3x3_wfrag_nhwc.
 * dims (int32[6]): dtype, N, H, W, C, tile_rows (0 = default; 8 | 16 pins the output tile height for C = 64 bf16).
 * Needs N*H*W*C < 2^31.
 */
int cobevt_basicblock_nhwc(const void* in, const void* wfrag1, const float* bias1, const void* wfrag2, const float* bias2,
                           void* out, const int* dims, hipStream_t stream);

/*
 * Fused down-sampling BasicBlock (ResNet layer2's first block: 64 -> 128 channels, stride 2, projection shortcut), bf16:
 * out = ReLU(conv2(ReLU(conv1/s2(x) + b1)) + b2 + conv1x1/s2(x) + b_ds) with the eval BatchNorms folded - torchvision
 * resnet.BasicBlock.forward with its `downsample` branch, as reached from resnet_ms.py:67-74.  One launch instead of three;
 * the intermediate map stays in LDS and is rounded to bf16 as the unfused path stores it, the shortcut is accumulated in
 * fp32 with conv2 (the unfused path rounds it to bf16 first).  wfrag1 / wfrag2: the fragment-ordered tables of
 * cobevt_conv3x3_wfrag_nhwc; wfrag_ds: the dense-row fragment table of cobevt_linear_rows_wfrag (K padded to 128).
 * dims (int32[6]): dtype (0 = bf16), N, H, W (even), Cin (64), Cout (128).  out: (N, H/2, W/2, 128).
 */
int cobevt_dsblock_nhwc(const void* in, const void* wfrag1, const float* bias1, const void* wfrag2, const float* bias2,
                        const void* wfrag_ds, const float* bias_ds, void* out, const int* dims, hipStream_t stream);

/*
 * ResNet stem: 7x7 / stride 2 / pad 3 conv on the fp32 3-channel channels-last image (+ folded BN, ReLU), computed as a
 * 4x4 stride-1 conv over the 2x2 space-to-depth image; torchvision resnet conv1/bn1/relu via resnet_ms.py:67-69.
 * wgt [Cout][16 taps][16] (12 real (dy,dx,c) channels + 4 zeros).  dims (int32[6]): dtype, N, H, W (even), Cout, act.
 */
int cobevt_stem_conv7x7s2(const float* in, const void* wgt, const float* bias, void* out, const int* dims,
                          hipStream_t stream);

/*
 * The stem followed by MaxPool2d(3, 2, 1) in one launch (torchvision resnet conv1/bn1/relu/maxpool, resnet_ms.py:67-71):
 * a workgroup computes the conv on the (2 R + 1) x 17 region an R x 8 tile of pooled pixels covers (R = 5 bf16, 3 fp32) and writes
 * the maxima, so the
 * (N, H/2, W/2, 64) stem map never reaches HBM.  Cout = 64, ReLU.  out (N, H/4, W/4, 64).
 * dims (int32[4]): dtype, N, H, W (multiples of 4).
 */
int cobevt_stem_conv7x7s2_pool(const float* in, const void* wgt, const float* bias, void* out, const int* dims,
                               hipStream_t stream);

/*
 * cobevt_stem_conv7x7s2_pool on the uint8 camera frames themselves: the ingest step of the reference's loop - RgbPreProcessor's
 * /255, (x - mean) / std on the host (opv2v/opencood/data_utils/pre_processor/rgb_preprocessor.py:14-31), the collate cast to
 * fp32 and `.to(device)` of the fp32 image (opv2v/opencood/tools/inference_camera.py:56-61) - folded into the stem's patch
 * gather.  in (N, H, W, 3) uint8; lut float[3][256]: lut[c][u] = the fp32 value the reference's pipeline gives byte u of channel c
 * (host/rgb_preprocessor.py: normalisation_table) - the kernel output is bit-identical to the fp32-image entry point fed lut[c][u].
 * A quarter of the bytes over PCIe and out of HBM.  dims as above.
 */
int cobevt_stem_conv7x7s2_pool_u8(const unsigned char* in, const float* lut, const void* wgt, const float* bias, void* out,
                                  const int* dims, hipStream_t stream);

/*
 * Dense-row GEMM with fused LayerNorm / pre-activation on the A operand and fused bias / residual / activation:
 * the fast path of every nn.Linear and 1x1 stride-1 convolution (fax_modules.py:189-193,281-292,309-313,411,435,472;
 * swap_fusion_modules.py:45-53; base_transformer.py:102-124).  wgt [N][Kp] (Kp = K rounded up to 128 bf16 / 64 fp32
 * elements).  dims (int64[16]): dtype, M, N, K, Kp, lda, pre_relu, act, src_H, src_W, out_H, out_W (these four remap
 * output rows into a zero-padded map; equal values = plain rows), ln (1 = normalise each A row over K first; the
 * LayerNorm affine is folded into wgt / bias by the host, or passed as ln_gamma/ln_beta fp32[K]; needs K <= one K-tile),
 * in_stride, in_H, in_W (in_stride s > 1: a 1x1 / stride-s convolution - the BasicBlock downsample path
 * resnet_ms.py:67-74 via torchvision resnet.py `downsample` - output row (n, oy, ox) of the (src_H, src_W) map reads
 * input pixel (n, s*oy, s*ox) of the (in_H, in_W) map; 1 = rows as stored).
 * pre_scale/pre_shift fp32[K] (nullable).
 */
int cobevt_linear_rows(const void* in, const void* wgt, const float* bias, const void* residual, const float* ln_gamma,
                       const float* ln_beta, const float* pre_scale, const float* pre_shift, void* out, const long* dims,
                       float ln_eps, hipStream_t stream);

/*
 * The same dense-row GEMM (same reference call sites and dims as cobevt_linear_rows) with the weights in MFMA fragment
 * order - rows zero-padded to a multiple of 128, [rows/32][Kp*esz/32 k-groups][64 lanes][16 bytes], lane = 32*half +
 * row%32 holding bytes [32*kgroup + 16*half, +16) of its row - and persistent workgroups: a workgroup walks the row tiles
 * of one 128-column tile with its weight fragments resident in registers (K <= one K-tile) and the next tile's rows in
 * flight under the current tile's MFMAs, epilogue and stores.  N % (8 bf16 | 4 fp32) == 0.  No ln_gamma / ln_beta
 * (the LayerNorm affine is folded into the weights by the host).
 */
int cobevt_linear_rows_wfrag(const void* in, const void* wfrag, const float* bias, const void* residual,
                             const float* pre_scale, const float* pre_shift, void* out, const long* dims, float ln_eps,
                             hipStream_t stream);

/*
 * Fused row-local chain after an attention (bf16 storage, or fp32 storage for C = 128 / hidden 256):  y = a.Wp^T (+bp) + skip ;  z = y + fc2(GELU(fc1'(norm(y)))) ;
 * out = post-LayerNorm(z) (optional) ;  out_next = act(norm?(out).Wn'^T + bn') (optional).  Replaces
 * fax_modules.py:240,246-247 + :411 / :435-437 and swap_fusion_modules.py:126,177 + base_transformer.py:102-124 in one
 * launch (hidden activations stay in LDS); the optional next projection is the row-local GEMM that reads `out` next in
 * the reference graph (to_qkv behind PreNormResidual.norm swap_fusion_modules.py:93, to_q of the second cross attention
 * fax_modules.py:201, the first 1x1 conv + BN + ReLU of the following ResNetBottleNeck fax_modules.py:472).
 * wp (C x 128), w1 (Hd x 128, LayerNorm affine folded in), w2 (C x Hdp), wnext (Nn x 128, LayerNorm affine / BN folded
 * in; nullable together with out_next [M][Nn]) are given in MFMA fragment order: rows zero-padded to a multiple of 128,
 * [rows/32][Kp/16][64 lanes][16 bytes] with lane = 32*half + row%32 holding bytes [32*kgroup + 16*half, +16) of its row,
 * so a wave's weight operand is one coalesced 1-KB load and no weight panel passes through LDS.  dims (int32[10]): dtype (0 bf16; 1 fp32
 * storage - round 6, csrc/row_chain_f32.hip: C == 128, Hd == Hdp == 256, fragments [rows/32][Kp/8][64 lanes][16 bytes] of fp32, the matrix
 * path of the library it is called from; other fp32 widths return COBEVT_ERR_UNSUPPORTED and the caller runs the GEMMs separately), M, C(<=128), Hd(<=256), Hdp, Nn (<= 768),
 * next_ln (1 = normalise the stored `out` rows first), next_act (0 none, 1 ReLU, 2 GELU), rows per workgroup (0 = 32; 64),
 * skip_rows (0 = M; a divisor of M: `skip` has that many rows and row m adds skip[m % skip_rows] - the learned prior
 * broadcast over the batch, fax_modules.py:509-510).
 */
int cobevt_attn_mlp_chain(const void* a, const void* skip, void* out, const void* wp, const float* bp, const void* w1,
                          const float* b1, const void* w2, const float* b2, const float* post_gamma,
                          const float* post_beta, const void* wnext, const float* bnext, void* out_next, const int* dims,
                          float eps1, float eps_post, float eps_next, hipStream_t stream);

/*
 * Fused gathered attention: window / dilated-grid partition -> QK^T -> (+relative position bias, key mask)
 * -> softmax -> PV -> (mean over query cameras) -> partition reverse, for projected token matrices.
 * Replaces: CrossWinAttention core, fax_modules.py:211-237,243 with the partitions of :399-404,:417-424 and
 *   reverses of :409,:433; swap Attention core, swap_fusion_modules.py:93-123 with :172-190;
 *   FAX global Attention core, fax_modules.py:137-171.
 * dims (int32[40]): dtype, B, L(windows), heads, ldq, ldk, ldv, ldo, qoff, koff, voff, ooff,
 *   bias_mode(0/1), bias_rows, bias_L, mean_q (0 none | 1 camera mean of per-camera query copies, fax_modules.py:243 | 2 per-camera
 *   query copies scored against their own camera's keys under ONE softmax over all cameras: CVT CrossAttention,
 *   cvt_modules.py:142-153), then three token maps {mode(0 window,1 grid,2 stored
 *   partitioned), ncam, HH, WW, w1, w2, X, Y} for q, k/v and out.  Head dim is 32.
 * bias_table fp32[bias_rows][heads] indexed ((dl+bias_L-1)(2w1-1)+(di+w1-1))(2w2-1)+(dj+w2-1);
 * mask fp32 (B,HH,WW,ncam) over the key map, 0 = masked (nullable).  `scale` multiplies QK^T.
 */
int cobevt_window_attention(const void* q, const void* k, const void* v, void* out, const float* bias_table,
                            const float* mask, const int* dims, float scale, hipStream_t stream);

/* Training slice (fp32 storage, dims[0] dtype = 1).  cobevt_window_attention_lse: the forward above that also stores the base-2
 * log-sum-exp of every query's logits, lse[B][L][heads][Nq] (mean_q must be 0).  cobevt_window_attention_bwd: given the forward
 * tensors, `out`, lse and dout (layout of out), writes dq, dk, dv (layouts of q, k, v; rows no window covers are left
 * untouched) and ADDS the bias-table gradient into dbias[bias_rows][heads] (zero-initialised; nullable without bias).  dlse (nullable,
 * layout of lse, drop_p must be 0): gradient w.r.t. the NATURAL log-sum-exp ln(2) * lse when the caller combines the lse further - CVT's
 * CrossAttention (cvt_modules.py:142-153: one softmax over all cameras' keys) trains as per-camera attentions merged by softmax(lse).
 * Replaces torch autograd through the einsum / softmax / einsum of fax_modules.py:219-237, swap_fusion_modules.py:100-121
 * (train_camera.py:143-179 loss.backward()). */
int cobevt_window_attention_lse(const void* q, const void* k, const void* v, void* out, float* lse, const float* bias_table,
                                const float* mask, const int* dims, float scale, float drop_p, unsigned drop_seed,
                                const unsigned* drop_seed_dev, hipStream_t stream);
int cobevt_window_attention_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse,
                                const void* dout, const float* dlse, void* dq, void* dk, void* dv, float* dbias, const float* bias_table,
                                const float* mask, const int* dims, float scale, float drop_p, unsigned drop_seed,
                                const unsigned* drop_seed_dev, hipStream_t stream);
/* drop_p > 0: nn.Dropout on the attention probabilities (FAX global attention in train mode, fax_modules.py:114,161): element
 * (query, key) is kept with probability 1 - drop_p and scaled by 1 / (1 - drop_p); the decision is a counter-based hash of
 * (seed, batch, window, head, query, key), regenerated by the backward kernels, seed = drop_seed + *drop_seed_dev (drop_seed_dev: a
 * nullable DEVICE word - a training step replayed from a captured HIP graph bumps it inside the graph, the scalar arguments being
 * frozen in the graph's nodes; forward and backward of one step must see the same value).  cobevt_attention_dropout_mask dumps
 * the mask of an effective seed (test hook): keep uint8 [B][L][heads][Nq][Nk]. */
int cobevt_attention_dropout_mask(int B, int L, int heads, int Nq, int Nk, float drop_p, unsigned drop_seed, unsigned char* keep,
                                  hipStream_t stream);

/* Row-local backward kernels of the training slice (fp32).  cobevt_layernorm_bwd: x, dy (rows, C) -> dx; ADDS the dy * xhat / dy
 * column sums into dgamma[C] / dbeta[C] (both nullable together; whatever they hold is kept: zero them for a plain gradient); gamma
 * nullable (= 1).  C % 4 == 0, 4 <= C <= 1024.  scratch: exactly cobevt_layernorm_bwd_scratch(rows, C) floats (one {dgamma, dbeta} record per
 * workgroup; 0 for a shape the entry points refuse), needed when dgamma / dbeta are given, not read or written otherwise: the records
 * are summed in fp64 and each word of dgamma / dbeta takes one fp32 rounding, in a fixed order (bit-reproducible).
 * cobevt_gelu: out = GELU(x) (dy null) or dy * GELU'(x) (exact erf form, nn.GELU()); n % 4 == 0.
 * (nn.LayerNorm / nn.GELU under autograd: base_transformer.py:102-124, swap_fusion_modules.py:275-279, fax_modules.py:189-191.) */
long cobevt_layernorm_bwd_scratch(int rows, int C);
int cobevt_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, int rows,
                         int C, float eps, float* scratch, hipStream_t stream);
int cobevt_gelu(const float* x, const float* dy, float* out, long n, hipStream_t stream);
/*
 * The same inside a bf16 autocast region (train_camera.py:157-160: torch's autocast runs layer_norm in fp32 and hands its result to the
 * bf16 projection that follows; nn.GELU runs in its input's bf16): every tensor fp32 or bf16 (dtype codes 0 = bf16, 1 = fp32), fp32
 * arithmetic.  cobevt_layernorm_fwd_t dtypes = [x, y]; cobevt_layernorm_bwd_t dtypes = [x, dy, dx]; cobevt_gelu_bf16: all bf16, n % 8 == 0.
 * The row mean is sum / C (a division), taken twice - of the row, then of the row shifted by it: a constant row has xhat = 0 and y = beta
 * exactly at every C, and a mean-dominated row loses nothing to the rounding of its mean.  cobevt_layernorm takes it the same way.
 */
int cobevt_layernorm_fwd_t(const void* x, const float* gamma, const float* beta, void* y, int rows, int C, float eps, const int* dtypes,
                           hipStream_t stream);
int cobevt_layernorm_bwd_t(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, int rows, int C,
                           float eps, const int* dtypes, float* scratch, hipStream_t stream);
int cobevt_gelu_bf16(const void* x, const void* dy, void* out, long n, hipStream_t stream);
/* Weight gradient of a k x k convolution, channels-last: dw fp32 (Cout, Cin, k, k) += sum over output pixels of dy (N, Ho, Wo, Cout)
 * x the tap-shifted x (N, H, W, Cin); dw must be zero-initialised (fp32 atomics).  dims (int32[11]): N, H, W, Cin, Ho, Wo, Cout, k,
 * stride, pad, storage type of x and dy (0 bf16 - the autocast path -, 1 fp32).  (cuDNN under autograd in the reference: every
 * nn.Conv2d on the path, train_camera.py:166-173.) */
int cobevt_conv_wgrad(const void* x, const void* dy, float* dw, const int* dims, hipStream_t stream);
/* Weight gradient of the transposed convolution z = ConvTranspose2d(kernel = stride = s, no bias) of x, channels-last, exact fp32 in
 * every library: dw[ci][co][dy][dx] = sum over (n, y, x) of x[n, y, x, ci] dz[n, s y + dy, s x + dx, co], with x (N, H, W, Cin) and
 * dz (N, sH, sW, Cout) contiguous fp32 and dw fp32 in the ConvTranspose2d layout (Cin, Cout, s, s), WRITTEN (not accumulated).  The
 * input pixels are the k dimension of v_mfma_f32_32x32x2_f32 and both operands are read as they lie; the pixel range is cut into
 * chunks whose accumulators go to `partial` (chunks x s s x Cin padded to 32 x Cout floats, plain stores), and a second launch adds
 * the chunks in order in fp64 and rounds once: no floating-point atomics, bit-reproducible.  dims (int32[7]): N, H, W, Cin, Cout, s,
 * chunks.  cobevt_deconv_wgrad_chunks reads dims[0..5] and returns the chunk count, a pure function of the shape (about 2048 one-wave
 * workgroups, at least 64 pixels per chunk, at most 64 MB of partials; not tuned), or MINUS an error code for a shape that is not
 * served; the launch returns COBEVT_ERR_SHAPE unless dims[6] is that count.  Served: 1 <= s <= 8, Cin % 4 == 0, Cout % 32 == 0,
 * N sH sW < 2^31 - 1, s s Cin (padded to 32) Cout floats <= 64 MB. */
int cobevt_deconv_wgrad_chunks(const int* dims);
int cobevt_deconv_wgrad(const float* x, const float* dz, float* partial, float* dw, const int* dims, hipStream_t stream);
/* The same weight gradient on the bf16 matrix path from BLOCKED bf16 copies of the operands (8 pixels of one channel = one 16-byte
 * piece, so a lane's matrix operand is one coalesced load and zero padding replaces every bounds test; cobevt_wgrad_block_operand
 * makes them): xb [N][Hp][XB][P][Cin][8] = x zero-padded by `pad` rows / columns, db [N][Ho][DB][Cout][8] = dy with rows zero-padded
 * to an even number DB of blocks; dw fp32 (Cout, Cin, k, k), zero-initialised.  Output row oy, tap row a reads padded row oy * sy + a
 * (Hp >= (Ho - 1) sy + k).  mode 0: stride 1, k = 1 / 3, P = 1, the taps of a row are pixel shifts (XB >= DB + (k > 1));
 * mode 1: stride 2 (sy = 2), k = 3 / pad 1 with P = 2 planes = even / odd padded columns (XB >= DB + 1), or k = 1 / pad 0 with the even
 * columns only (P = 1); mode 2: the k tap columns as P = k planes, k * Cin <= 32, k odd <= 7 (the 7x7 / stride 2 stem on 3 channels:
 * a tap row is one matrix instruction).  dims (int32[10]): N, Hp, XB, Cin, Ho, DB, Cout, k, sy, mode. */
int cobevt_conv_wgrad_blocked(const void* xb, const void* db, float* dw, const int* dims, hipStream_t stream);

/* out[b][i] = max over l of in[b][l][i] (F-Cooper max-out fusion over the max_cav agent slots, SpatialFusionMask,
 * opv2v/opencood/models/fusion_modules/f_cooper_fuse.py:30-36).  in (B, L, per) contiguous, dtype 0 bf16 / 1 fp32, per % 8 == 0. */
int cobevt_agent_max(const void* in, void* out, int dtype, int B, int L, long per, hipStream_t stream);

/* Fused torchvision Bottleneck(128, 32) (1x1 128->32, 3x3 32->32, 1x1 32->128, eval BatchNorms folded, ReLUs, identity skip) on
 * a channels-last bf16 map: ResNetBottleNeck(dim) of the FAX pyramid, fax_modules.py:10,472,512.  w1 / w2 / w3: MFMA fragment
 * tables [8][64][8] / [9][2][64][8] / [4][2][64][8] bf16 (layout: cobevt_amd/ops.py BottleneckPlan; w3's contraction index in
 * accumulator-register order), b1[32] / b2[32] / b3[128] fp32.  dims (int32[7]): dtype (0), N, H, W, C (128), mid (32),
 * tile rows (0 = automatic | 8 | 16). */
int cobevt_bottleneck_nhwc(const void* in, const void* w1, const void* w2, const void* w3, const float* b1, const float* b2,
                           const float* b3, void* out, const int* dims, hipStream_t stream);

/*
 * The same block for fp32 STORAGE (round 6, csrc/bottleneck_f32.hip; the matrix path is the library's): in (N, H, W, 128) fp32, out the same;
 * y1 (N, H, W, 32) = ReLU(conv1(x) + b1) when the producer of x already computed it (the row chain's `next` projection), else null and the
 * kernel computes conv1 on the tile's halo region itself.  w1frag / w3frag: the fp32 fragment tables of cobevt_linear_rows_small_k for the
 * folded 32 x 128 / 128 x 32 matrices ([rows/32][Kp/8][64 lanes][16 bytes], Kp = K rounded up to 64), w2frag: the table of
 * cobevt_conv3x3_wfrag_nhwc for the folded 3x3 ([tile][1 chunk][9 taps][4 k-groups][64 lanes][16 bytes]; tile 0 is used).
 * dims (int32[4]): N, H, W, w3 tile stride in 16-byte units (= Kp / 8 * 64).
 */
int cobevt_bottleneck_f32_nhwc(const void* in, const void* y1, const void* w1frag, const float* b1, const void* w2frag, const float* b2,
                               const void* w3frag, const float* b3, void* out, const int* dims, hipStream_t stream);

/* Test hooks for the integer part of the attention kernels (north-star: window index arithmetic bit-exact), computed by the
 * same device functions the attention kernels use.  cobevt_attention_index_map: rows[b][l][t] (int32, B * X*Y * ncam*w1*w2) =
 * row of token t of window l in the (B*ncam, HH, WW) token matrix, for one token map {mode, ncam, HH, WW, w1, w2, X, Y}:
 * the einops partitions of fax_modules.py:399-404 (window), :417-424 (grid), swap_fusion_modules.py:172-190.
 * cobevt_attention_bias_index: idx[tq][tk] (int32, Nq * Nk) = relative-position table row for query token tq / key token tk
 * (swap_fusion_modules.py:63-85 with bias_L = agent_size; fax_modules.py:123-130 with bias_L = 1). */
int cobevt_attention_index_map(const int* map8, int B, int* rows, hipStream_t stream);
int cobevt_attention_bias_index(const int* qmap8, const int* kmap8, int bias_L, int* idx, hipStream_t stream);

/* LayerNorm over channels (gamma/beta both null = normalisation only), optionally after a mean over `navg` slices (mlp_head).
 * Replaces: nn.LayerNorm of fax_modules.py:189-191,309-313,435-437; swap_fusion_modules.py:275-279;
 *   base_transformer.py:102-109. */
int cobevt_layernorm(const void* in, const float* gamma, const float* beta, void* out, int dtype, int rows, int C,
                     float eps, int navg, long avg_stride, long in_batch_stride, int rows_per_batch,
                     hipStream_t stream);

/* Camera-ray positional embedding, fax_modules.py:346-358.  out (BN, hw, D) channels-last. */
int cobevt_fax_ray_embed(const float* I_inv, const float* E_inv, const float* image_plane, const float* w_img,
                         const float* w_cam, void* out, int dtype, int BN, int hw, int D, hipStream_t stream);

/* BEV query embedding + prior, fax_modules.py:370-375,387-388.  out (B, n, hw, D).  x (B, hw, D), or with x_bcast = 1
 * one (hw, D) prior shared by every b (the first pyramid level, fax_modules.py:509-510 repeat of the learned prior). */
int cobevt_fax_bev_embed(const float* E_inv, const float* world, const float* w_bev, const float* b_bev,
                         const float* w_cam, const void* x, void* out, int dtype, int B, int n, int hw, int D,
                         int x_bcast, hipStream_t stream);

/*
 * BEV query embedding + prior fused with the to_q LayerNorm + Linear that consumes it (fax_modules.py:370-375,387-388
 * followed by CrossWinAttention.to_q :193-195,201): the (B, n, hw, D) query never reaches HBM - the dense-row GEMM
 * computes its A rows  x[b][pix] + L2norm_c(w_bev.world[pix] + b_bev - w_cam.E_inv[b,cam][:,3])  on the fly, rounds them
 * to the storage type exactly as cobevt_fax_bev_embed would have stored them, normalises (LayerNorm affine folded into
 * wgt / bias) and multiplies.  out (B*n*hw, N).  wgt [N][Kp] as for cobevt_linear_rows.  dims (int64[8]): dtype, B, n,
 * hw (multiple of 128), D (= K <= one K-tile), N, Kp, ln.
 */
int cobevt_bev_embed_linear_rows(const float* E_inv, const float* world, const float* w_bev, const float* b_bev,
                                 const float* w_cam, const void* x, const void* wgt, const float* bias, void* out,
                                 const long* dims, float ln_eps, hipStream_t stream);

/* MaxPool2d(3, 2, 1) channels-last; torchvision ResNet stem reached from resnet_ms.py:71. */
int cobevt_maxpool3x3s2(const void* in, void* out, int dtype, int N, int H, int W, int C, hipStream_t stream);

/* Strided (n,c,h,w) view <-> contiguous channels-last with dtype cast (module boundary; resnet_ms.py:62-65). */
int cobevt_to_nhwc(const void* in, int in_dtype, void* out, int out_dtype, int N, int C, int H, int W,
                   const long* strides, hipStream_t stream);
int cobevt_from_nhwc(const void* in, int in_dtype, void* out, int out_dtype, int N, int C, int H, int W,
                     const long* strides, hipStream_t stream);

/* Pairwise-warp fusion baselines (V2VNet fusion_modules/v2v_fuse.py:72-144, DiscoNet fusion_modules/disconet_fuse.py:106-168) on the
 * un-grouped channels-last agent batch x (sum(record_len), H, W, C), H == W; record_len device int32[B]; pairwise (B, L, L, 4, 4)
 * fp32 = batch['pairwise_t_matrix'] (intermediate_fusion_dataset.py:110-150).  All maps stay in their original orientation (the
 * reference's transpose + flip is folded into the kernels' indexing).
 * cobevt_pairwise_warp: nb[b][i][j] (B, L, L, H, W, C) = agent j's map warped into agent i's frame (zeros unless i, j <
 *   record_len[b]); roi (B, L, L, H, W) fp32 = get_rotated_roi's mask (torch_transformation_utils.py:77-105) at the position the
 *   reference multiplies that output pixel with.
 * cobevt_agent_message_reduce: out[off_b + i] = mean (mode 0) | max (mode 1) over j < record_len[b] of
 *   (msg[b][i][j] + ego[off_b + i]) * roi[b][i][j]   (v2v_fuse.py:108-119; ego = the ego half of msg_cnn + its bias).
 * cobevt_gru_zero_state: out[row] = sigmoid(in[row][0:C]) * tanh(in[row][C:2C]): the ConvGRU cell with the zero hidden state
 *   the fusions always pass (convgru.py:57-78, v2v_fuse.py:125-130).
 * cobevt_agent_softmax_sum: out[off_b + i] = sum_j softmax_j(score or -inf where roi == 0) * nb[b][i][j] * roi[b][i][j]
 *   (disconet_fuse.py:35-42,141-150); score = column 0 of a (B*L*L*H*W, lds) matrix. */
int cobevt_pairwise_warp(const void* x, const float* pairwise, const int* record_len, void* nb, float* roi, int dtype, int B, int L,
                         int H, int W, int C, float discrete_ratio, float downsample_rate, hipStream_t stream);
/* Adjoint of cobevt_pairwise_warp w.r.t. x (training; torch autograd through warp_affine in the reference): dnb (B, L, L, H, W, C) ->
 * dx fp32 (N, H, W, C), zero-initialised; the same bilinear sample positions, scattered with fp32 atomics. */
int cobevt_pairwise_warp_bwd(const void* dnb, const float* pairwise, const int* record_len, float* dx, int dtype, int B, int L, int H,
                             int W, int C, float discrete_ratio, float downsample_rate, hipStream_t stream);
int cobevt_agent_message_reduce(const void* msg, const void* ego, const float* roi, const int* record_len, void* out, int dtype,
                                int B, int L, int HW, int C, int mode, hipStream_t stream);
int cobevt_gru_zero_state(const void* in, void* out, int dtype, long rows, int C, hipStream_t stream);
int cobevt_agent_softmax_sum(const void* score, int lds, const void* nb, const float* roi, const int* record_len, void* out, int dtype,
                             int B, int L, int HW, int C, int use_mask, hipStream_t stream);

/* AttFusion (fusion_modules/self_attn.py:36-57) on channels-last maps, one launch: x (N, HW, C) and out (B, HW, C) contiguous in the
 * compute dtype (0 bf16, 1 fp32), N = sum(record_len).  For sample b with agents off .. off + n - 1 (off = sum record_len[:b]) and
 * every pixel p:  s_j = <x[off, p], x[off + j, p]> * scale;  out[b, p] = sum_j softmax_j(s) x[off + j, p]  - the ego's row of the
 * reference's n x n attention, the only one it keeps.  scale = 1 / sqrt(C), passed by the host.  fp32 arithmetic, online softmax
 * with a running maximum, one rounding to the storage type.  record_len (device int32[B]) is read on the device; n is clamped to
 * [0, N - off], so a wrong record_len reads nothing outside x, and a sample with n <= 0 gets zeros.  Every element of out is
 * written once.  COBEVT_ERR_SHAPE unless C = 8 * 2^k <= 512, 1 <= B <= 65535, N >= 1, HW >= 1. */
int cobevt_att_fuse_nhwc(const void* x, const int* record_len, void* out, int dtype, int B, int N, long HW, int C, float scale,
                         hipStream_t stream);
/* Its backward with respect to x (fp32 storage only): x (N, HW, C), dout (B, HW, C) -> dx (N, HW, C).  Nothing is saved by the forward;
 * per pixel the scores are recomputed: with g = dout[b, p], P = softmax_j(s), t_j = <g, x_j>, ds_j = P_j (t_j - sum_k P_k t_k):
 * dx_j = P_j g + scale ds_j x_0 for every agent j of the sample, and the ego's row additionally gets scale sum_j ds_j x_j.  Two
 * passes over the agents (statistics with a running maximum; rows), fp32 arithmetic, accurate expf, 16-byte accesses, the
 * forward's groups and grid.  record_len is read on the device and n is clamped to [0, N - off] as in the forward.  Every element of
 * dx is written exactly once (record_len >= 0): rows of agents that belong to no sample - off + j >= sum(record_len), or a sample
 * with n <= 0 - get 0; no atomics, no zero-fill needed.  A sample of one agent returns dx_0 = g (P_0 = 1 and ds_0 = 0 exactly).
 * The forward's shape rules: COBEVT_ERR_SHAPE unless C = 8 * 2^k <= 512, 1 <= B <= 65535, N >= 1, HW >= 1. */
int cobevt_att_fuse_bwd_nhwc(const float* x, const int* record_len, const float* dout, float* dx, int B, int N, long HW, int C, float scale,
                             hipStream_t stream);

/* Typed agent attention (HGTCavAttention, base_transformer.py:175-319) in three row-local launches: typed projection, attention,
 * typed output projection.  The 32 x 32 relation matrices are folded into the key / value projections by the host (ops.hgt_fold).
 *
 * cobevt_typed_linear:  y[row] = W[t] n(x[row]) + bias[t] (+ residual[row]).  The rows form G groups of R consecutive rows (one
 * agent's H W pixels); t = clamp(types[g], 0, T - 1) is read on the device from int32 types[G], so any value of it reads inside W
 * and bias.  n is the identity (ln = 0) or the LayerNorm normalisation (x - mean) rsqrt(var + ln_eps) without affine (ln = 1; the
 * affine is folded into W and bias), rounded once to the storage type.  x (G R, K), residual and out (G R, N), W (T, N, K) in
 * nn.Linear layout in the storage type (dtype 0 bf16 on v_mfma_f32_32x32x16_bf16, 1 fp32 on the exact v_mfma_f32_32x32x2_f32 in
 * every library), bias (T, N) fp32.  fp32 accumulation, bias and residual added in fp32, one rounding.  A 32-row tile never mixes two
 * groups and a tail tile stores nothing outside its group.  dims = [dtype, G, R, K, N, T, ln].
 * COBEVT_ERR_ARG: a null pointer (residual may be null), dtype or ln not 0 / 1, ln_eps negative or NaN.  COBEVT_ERR_SHAPE: K or N
 * not a positive multiple of 32, N > 2^20, G outside 1 .. 65535, R outside 1 .. 2^31 - 1, T outside 1 .. 65535, a pointer that is
 * not 16-byte aligned (types: 4-byte).
 * COBEVT_ERR_UNSUPPORTED: K > 512 with ln, K > 1024 without.  Everything is checked before the launch. */
int cobevt_typed_linear(const void* x, const void* w, const float* bias, const int* types, const void* residual, void* out,
                        const long* dims, float ln_eps, hipStream_t stream);
/* cobevt_hgt_attention_nhwc: proj (B, L, HW, (1 + 2 T) inner) with rows [q | k'_0 .. k'_(T-1) | v'_0 .. v'_(T-1)], inner = 32 heads
 * (dim_head = 32), types int32[B L] on the device, mask (B, HW, L) fp32 (0 = key masked) or null -> out (B, L, HW, inner).  Per
 * pixel, head and query agent i with a = clamp(types[b L + i], 0, T - 1):  s_j = scale <q_i, k'_a of agent j> over the unmasked
 * keys, out_i = sum_j softmax_j(s) v'_a of agent j.  fp32 arithmetic, accurate expf, running maximum, one rounding to the storage
 * type; no atomics, bit-reproducible.  A query whose keys are ALL masked writes zeros (the reference's softmax over -inf gives NaN
 * there).  COBEVT_ERR_ARG: a null pointer (mask may be null), dtype not 0 / 1.  COBEVT_ERR_SHAPE: B, L, HW, heads or T < 1,
 * B L > 65535, misaligned pointers.  COBEVT_ERR_UNSUPPORTED: L > 8, heads > 64, T > 64. */
int cobevt_hgt_attention_nhwc(const void* proj, const int* types, const float* mask, void* out, int dtype, int B, int L, long HW,
                              int heads, int T, float scale, hipStream_t stream);

/* regroup: split by record_len (device int32[B]), zero pad to max_cav, agent mask (B,max_cav) fp32.
 * Replaces fuse_utils.py:8-61 without its host synchronisation (:26). */
int cobevt_regroup(const void* in, const int* record_len, void* out, float* mask, int dtype, int B, int max_cav,
                   long elems_per_agent, hipStream_t stream);

/* STTF warp into the ego frame + ROI/agent mask.  x (B*L,H,W,C) -> out (B,L,H,W,C), com_mask (B,H,W,1,L).
 * Replaces corpbevt.py:28-64 and torch_transformation_utils.py:11-134,160-355. tmat: (B,L,4,4) fp32.
 * With record_len (device int32[B]) x is the un-grouped agent batch (sum(record_len),H,W,C) and regroup
 * (fuse_utils.py:8-61) happens inside: agent l of sample b is row sum(record_len[:b]) + l, absent agents warp to zeros and
 * get mask 0; cav_out (B,L) fp32 (nullable) receives the agent mask; cav_mask is then ignored. */
int cobevt_sttf_warp(const void* x, const float* tmat, const float* cav_mask, void* out, float* com_mask,
                     const int* record_len, float* cav_out, int dtype, int B, int L, int H, int W, int C,
                     float discrete_ratio, float downsample_rate, hipStream_t stream);

/* Batched inverse of n (dim x dim) fp32 matrices, dim in {3, 4}; fax_modules.py:500-501 (intrinsic.inverse()),
 * nuscenes encoder_pyramid_axial.py:538-539. */
int cobevt_invert_small(const float* in, float* out, int n, int dim, hipStream_t stream);

/* Channels-last resize: mode 0 nearest (F.interpolate default), mode 1 bilinear align_corners=True;
 * nuscenes/cross_view_transformer/model/decoder.py:12,31. */
int cobevt_resize_nhwc(const void* in, void* out, int dtype, int N, int H, int W, int C, int Ho, int Wo, int mode,
                       hipStream_t stream);

/* y = x*scale[c] + shift[c] on contiguous (N,C,HW) fp32; Normalize, nuscenes encoder_pyramid_axial.py:41-49. */
int cobevt_channel_affine(const float* in, const float* scale, const float* shift, float* out, long N, int C, long HW,
                          hipStream_t stream);

/*
 * Pull `bytes` (a multiple of 16) from pinned, device-visible HOST memory (hipHostMalloc / torch .pin_memory(): the host pointer is
 * the device pointer) into device memory with `blocks` (0 = 128; the captured step uses 16) workgroups of 256 lanes, each lane with eight
 * 8-byte SYSTEM-SCOPE relaxed atomic loads in flight (global_load_dwordx2 sc0 sc1 behind an acquire fence: a ring slot the host has
 * rewritten is never served out of the GPU's caches) and plain 8-byte stores: the ingest step of the reference's loop
 * (opv2v/opencood/tools/inference_camera.py:56-61 `.to(device)`) as a kernel that can be CAPTURED in the step's HIP graph and runs
 * beside the compute kernels (no LDS, 52 VGPRs) - host.pipeline.PipelinedCorpBEVT(host_ingest=True).
 */
int cobevt_host_fetch(const void* host_src, void* dst, long bytes, int blocks, hipStream_t stream);

/* ---- downstream of the hot path: the logits -> scored maps -------------------------------------- */

/* CameraBevPostprocessor.softmax_argmax, opv2v/opencood/data_utils/post_processor/camera_bev_postprocessor.py:55-59:
 * prob = Softmax(dim=1)(logits) (fp32) and map = argmax(prob, dim=1) (int64; the first maximum wins, and it is the
 * argmax of the rounded probabilities as in the reference, not of the logits).  logits (N, C, hw) planar, dtype 0 bf16 /
 * 1 fp32, C <= 8; prob (N, C, hw) fp32; map (N, hw) int64. */
int cobevt_softmax_argmax(const void* logits, float* prob, long long* map, int dtype, int N, int C, int hw,
                          hipStream_t stream);

/* The pixel counts mean_IU / mean_precision reduce their class masks to, opv2v/opencood/utils/seg_utils.py:6-50:
 * counts[n][c] = (n_ii = |pred==c & gt==c|, t_i = |gt==c|, n_ij = |pred==c|) for c < K, and counts[n][K] =
 * (|pred outside [0,K)|, |gt outside [0,K)|, 0).  pred, gt (N, hw) int64; counts (N, K + 1, 3) uint64, zeroed here. */
int cobevt_seg_class_counts(const long long* pred, const long long* gt, unsigned long long* counts, int N, int hw, int K,
                            hipStream_t stream);

/* Class-weighted cross entropy nn.CrossEntropyLoss(weight=w) computes in VanillaSegLoss (validation loss of
 * train_camera.py:182-196; opv2v/opencood/loss/vanilla_seg_loss.py:18-23,58-70): out[0] = sum_i w[y_i] (logsumexp(x_i) - x_i[y_i])
 * / sum_i w[y_i], out[1] / out[2] = numerator / denominator, out[3] = number of labels outside [0, C) other than -100 (the
 * ignore_index of nn.CrossEntropyLoss, which contributes to neither sum); the reference raises for such labels, so the caller
 * must refuse a result with out[3] != 0.  logits (N, C, hw) planar (dtype 0 bf16 / 1 fp32, 2 <= C <= 8), target (N, hw) int64,
 * weight [C] fp32, out >= 4 floats, scratch >= 3 * N * ceil(hw / 4096) floats (one {numerator, denominator, count} record per 4096 pixels
 * of an image; exactly that many are written), fixed summation order.  The sums are fp32: out[3] is exact below 2^24 bad labels.  With
 * every label -100 out[1] = out[2] = out[3] = 0 and out[0] = 0 / 0 = NaN, as nn.CrossEntropyLoss. */
int cobevt_weighted_cross_entropy(const void* logits, const long long* target, const float* weight, float* scratch, float* out,
                                  int dtype, int N, int C, int hw, hipStream_t stream);
/* Backward of the loss above for fp32 logits: dlogits (N, C, hw) = upstream[0] * w[y] (softmax_c - [c == y]) / sum w[y]; stats = the
 * forward's out[4]; upstream = the incoming gradient of the scalar loss (device fp32[1]).  train_camera.py:166-173 loss.backward().
 * A pixel labelled -100 gets exactly 0 in every class.  With stats[2] == 0 (every label ignored) every element is NaN (0 / 0, as torch). */
int cobevt_weighted_cross_entropy_bwd(const float* logits, const long long* target, const float* weight, const float* stats,
                                      const float* upstream, float* dlogits, int N, int C, int hw, hipStream_t stream);

/* 3x3 / stride 1 / pad 1 convolution with 1..4 output channels on a channels-last map -> fp32 NCHW logits: the BevSegHead heads
 * (bev_seg_head.py:20-33,44-58).  wgt fp32 [Cout][9 taps][Cin] (tap = kh * 3 + kw), bias fp32[Cout] nullable, Cin a multiple of
 * the 16-byte chunk with at most 256 bytes per pixel. */
int cobevt_conv3x3_head_nchw(const void* in, const float* wgt, const float* bias, float* out, int dtype, int N, int H, int W, int Cin,
                             int Cout, hipStream_t stream);

/* The same GEMM as cobevt_linear_rows for K <= 512 in bf16 (the to_q / to_k / to_v / to_qkv projections behind a LayerNorm,
 * feature_proj / feature_linear behind BN + ReLU, the Bottleneck 1x1 convs), on the row chain's structure: 32-row workgroups,
 * weights as MFMA fragments straight from L2.  wfrag: [N_p/32][8][64 lanes][16 bytes] as for cobevt_attn_mlp_chain (rows
 * zero-padded to a multiple of 128 columns K_p, K_p / 16 k-groups per tile, N_p = N rounded up to 128).  dims (int64[13]):
 * dtype (0), M, N (multiple of 8, <= 4096), K (multiple of 8, <= 512; ln needs K <= 128), lda, pre_relu, act (0..4), ln,
 * in_stride, src_H, src_W, in_H, in_W (strided row gather of a 1x1 / stride-2 conv as in cobevt_linear_rows; 1 = dense rows).
 * residual [M][N] (dense rows only), pre_scale / pre_shift [K], bias [N] nullable. */
int cobevt_linear_rows_small_k(const void* in, const void* wfrag, const float* bias, const void* residual, const float* pre_scale,
                               const float* pre_shift, void* out, const long* dims, float ln_eps, hipStream_t stream);

/* cobevt_bev_embed_linear_rows on the 32-row kernel: the BEV query  x[b][pix] + L2norm_c(w_bev . world[pix] + b_bev -
 * w_cam . E_inv[b, cam][:, 3])  (fax_modules.py:370-375,387-388) is produced while the A rows are staged, rounded as
 * cobevt_fax_bev_embed would have stored it, normalised and multiplied by to_q (fax_modules.py:193-195,201) - the
 * (B, n, hw, D) query never reaches HBM.  wfrag as cobevt_linear_rows_small_k.  dims (int64[8]): dtype (0), B, n, hw (multiple
 * of 32), D (= K <= 128), N, ln, x_bcast (1: x is one (hw, D) prior shared by every b).  out (B*n*hw, N). */
int cobevt_bev_embed_linear_rows_small_k(const float* E_inv, const float* world, const float* w_bev, const float* b_bev,
                                         const float* w_cam, const void* x, const void* wfrag, const float* bias, void* out,
                                         const long* dims, float ln_eps, hipStream_t stream);

/* Forward of BinarySegmentationLoss / CenterLoss, nuscenes/cross_view_transformer/losses.py:27-84: sigmoid focal loss (fvcore's
 * published definition) of pred (N, C, hw) fp32 logits against label_c = max over the label channels in label_mask[c]
 * (soft_label: label channel c itself, NL == C), over the pixels with visibility >= min_visibility (< 0: all), mean.
 * out[0] = mean, out[1] = sum, out[2] = count; scratch >= 2 * N * ceil(hw / 2048) floats (one {sum, count} record per 2048 pixels of an
 * image; exactly that many are written); fixed summation order.  The count is an fp32 sum of ones: exact below 2^24 kept elements.
 * With no pixel kept out[1] = out[2] = 0 and out[0] = 0 / 0 = NaN. */
int cobevt_sigmoid_focal_loss(const float* pred, const float* label, const unsigned char* visibility, const unsigned int* label_mask,
                              float* scratch, float* out, int N, int C, int NL, int hw, int min_visibility, float alpha,
                              float gamma, int soft_label, hipStream_t stream);

/* nuScenes IoU metric, nuscenes/cross_view_transformer/metrics.py:22-31,56-72: counts[t] += (tp, fp, fn) of
 * sigmoid(pred) >= thresholds[t] against label_c = any(label[l] != 0 for l in the bit mask label_mask[c]) over the pixels with
 * visibility >= min_visibility (min_visibility < 0: all pixels, visibility may be null).  pred (N, C, hw) fp32 logits, label
 * (N, NL <= 32, hw) fp32, visibility (N, hw) uint8, thresholds [T <= 8] fp32, counts (T, 3) uint64 - accumulated, not zeroed. */
int cobevt_iou_counts(const float* pred, const float* label, const unsigned char* visibility, const unsigned int* label_mask,
                      const float* thresholds, unsigned long long* counts, int N, int C, int NL, int hw, int T,
                      int min_visibility, hipStream_t stream);

/*
 * cobevt_resize_pil_u8 (csrc/image_ingest.hip; identical in every library): the camera side of the
 *   nuScenes LoadDataTransform (nuscenes/cross_view_transformer/data/transforms.py:118-149) on decoded frames in device memory -
 *   Image.resize((w_resize, h_resize), resample=BILINEAR) of Pillow's 8-bit path, the crop of the top `top_crop` rows, ToTensor.
 *   src (n, H, W, 3) uint8 contiguous, any alignment.  dims = [n, H, W, channels, h_resize, w_resize, top_crop, out is uint8] (host).
 *   out: (n, 3, h, w) fp32 = lut[byte] (out is uint8 = 0; lut[256] fp32 on the device, ToTensor's is i / 255), or (n, h, w, 3)
 *   uint8, the resized bytes themselves (out is uint8 = 1; lut may be null); h = h_resize - top_crop, w = w_resize.
 *   Per axis with n_in != n_out the caller passes Pillow's tap tables ON THE DEVICE (Resample.c precompute_coeffs +
 *   normalize_coeffs_8bpc, evaluated in float64 on the host): bounds (n_out, 2) int32 = [first source index, tap count] and coeffs
 *   (n_out, ksize) int32, 22-bit fixed point (the kernel multiplies in 24 bits: magnitudes below 2^23), ksize = 2 * ceil(max(n_in / n_out, 1)) + 1; hbounds / hcoeffs for W -> w_resize,
 *   vbounds / vcoeffs for H -> h_resize.  An axis that keeps its size is skipped as Pillow skips it (its tables may be null).
 *   One pass is clip((sum_t src[first + t] * coeffs[t] + 2^21) >> 22, 0, 255) in int32; the horizontal pass runs first and its
 *   result is rounded to a byte before the vertical pass reads it, as in Pillow: bit-exact.  Only rows the crop keeps are computed.
 *   Table entries are clamped to the image, so a wrong table gives wrong pixels and no access outside src.
 *   Code 2, before any launch: channels != 3, a down-scale above 8 on either axis (ksize > 17), n, a size or an output empty,
 *   n > 65535, top_crop outside [0, h_resize).  One launch, no atomics, no host read, no allocation.
 * cobevt_decode_bev: the label side (transforms.py:151-159 with data/common.py:69-78): labels (N, hw) int32 bit-packed ->
 *   out (N, num_classes <= 16, hw) fp32 of (x >> c) & 1, exactly 0.0 or 1.0.  One streaming launch.
 */
int cobevt_resize_pil_u8(const unsigned char* src, void* out, const int* hbounds, const int* hcoeffs, const int* vbounds,
                         const int* vcoeffs, const float* lut, const int* dims, hipStream_t stream);
int cobevt_decode_bev(const int* labels, float* out, int N, int hw, int num_classes, hipStream_t stream);

/* ---- upstream of the nuScenes path: MBConv pieces of the EfficientNet image backbone wrapped by
 * nuscenes/cross_view_transformer/model/backbones/efficientnet.py:24-96 (efficientnet-pytorch 0.7.1 MBConvBlock.forward;
 * the 1x1 convolutions of a block go through cobevt_linear_rows / cobevt_conv2d_nhwc with act 3 = swish) -------------- */

/* k x k depthwise convolution (groups == channels) + folded BatchNorm + activation on a channels-last map.  wgt [k*k][C]
 * fp32 (BN scale folded), bias [C] fp32.  dims (int32[12]): dtype, N, H, W, C (multiple of 8), k (<= 7), stride, pad_top,
 * pad_left (the TensorFlow-"same" extra row / column at the bottom / right is implicit: taps outside the map read zero),
 * Ho, Wo, act (0 none, 1 ReLU, 2 GELU, 3 swish, 4 sigmoid). */
int cobevt_depthwise_conv_nhwc(const void* in, const float* wgt, const float* bias, void* out, const int* dims,
                               hipStream_t stream);

/* Squeeze: out[n][c] = mean over the hw pixels of in (N, hw, C), fp32, fixed summation order. */
int cobevt_spatial_mean_nhwc(const void* in, float* out, int dtype, int N, int hw, int C, hipStream_t stream);

/* Excitation: gate (N, C) = sigmoid(w_expand (C x Cs) . swish(w_reduce (Cs x C) . mean (N, C) + b_reduce) + b_expand), fp32. */
int cobevt_se_gate(const float* mean, const float* w_reduce, const float* b_reduce, const float* w_expand,
                   const float* b_expand, float* gate, int N, int C, int Cs, hipStream_t stream);

/* out (N, hw, C) = in * gate (N, C). */
int cobevt_channel_gate_nhwc(const void* in, const float* gate, void* out, int dtype, int N, int hw, int C,
                             hipStream_t stream);

/* SwapFusionEncoder.mlp_head in one launch (swap_fusion_modules.py:275-281: mean over the agents, LayerNorm, Linear): out (B * R, N) =
 * act(LayerNorm?(mean over j < L of in[b][j][r][:]) . W^T + bias), in (B, L, R, K) bf16, K <= 128; the dense-row kernel of
 * cobevt_linear_rows_small_k with the agent mean taken while the A rows are staged.  Weights in MFMA fragment order, the LayerNorm
 * affine folded in.  dims (int64[8]): dtype (0), B, L, R, K, N, ln, act. */
int cobevt_mean_linear_rows_small_k(const void* in, const void* wfrag, const float* bias, void* out, const long* dims,
                                    float ln_eps, hipStream_t stream);

/* cobevt_window_attention with the KEYS of every window shared out over `ksplit` (2..16) workgroups per query tile and a merge
 * pass (same reference code: fax_modules.py:211-237, 137-171): for launches whose grid leaves the chip idle while every query
 * walks a long key list (FAX level 2 / global attention: 1024 keys, 160 workgroups; the nuScenes CVT encoder's camera-paired
 * level-1 attention: 625 queries x 6 x 6720 keys, 20 workgroups unsplit).  Inference attention without camera mean, lse or
 * dropout; camera-paired (mean_q = 2, cvt_modules.py:142-153 / nuscenes encoder.py:142-153) allowed - its partial rows follow
 * the output map.  Bias table and mask as there.  COBEVT_ERR_SHAPE when a split would get no key tile (64 keys; camera-paired:
 * tiles never mix cameras).  part_out: [ksplit][out_rows][heads * 32] in the storage dtype, part_lse: fp32 [ksplit][out_rows]
 * [heads] - scratch; out_rows = rows of `out` (ld = dims' ldo). */
int cobevt_window_attention_ksplit(const void* q, const void* k, const void* v, void* out, const float* bias_table,
                                   const float* mask, void* part_out, float* part_lse, const int* dims, float scale,
                                   int ksplit, long out_rows, hipStream_t stream);

/*
 * Projection chain (bf16, 128 channels): the key / value side of a FAX cross-view level in one launch per operand -
 *   y = ReLU?(a * pre_scale[c] + pre_shift[c]) . Wp^T + bp + skip     pre-activation BatchNorm -> ReLU -> 1x1 conv (feature_proj /
 *                                                                     feature_linear, fax_modules.py:281-292,377-396) + the ray embedding
 *   next = act(LayerNorm?(y) . Wn'^T + bn')                           to_k / to_v of BOTH cross attentions stacked (fax_modules.py:201-205)
 * with y (the "key" / "val" map of the reference) kept in LDS: it is written to `out` only when out != null.  The row_chain
 * kernel without its MLP phases (csrc/row_chain.hip).  Weights in MFMA fragment order as for cobevt_attn_mlp_chain.
 * dims (int32[9]): dtype (0), M, C (128), Nn (<= 768), next_ln, next_act, skip_rows (0 = M), pre_relu, variant (0 = automatic:
 * maps of >= 32768 rows run as independent waves with the rows in registers and the weights in LDS, csrc/proj_chain128.hip;
 * 1 = always the barrier-phased kernel).
 */
int cobevt_proj_chain(const void* a, const float* pre_scale, const float* pre_shift, const void* skip, const void* wp,
                      const float* bp, void* out, const void* wnext, const float* bnext, void* out_next, const int* dims,
                      float eps_next, hipStream_t stream);

/*
 * Key AND value side of a FAX pyramid level whose image features are wider than the level, one launch (csrc/proj_chain_k.hip):
 *   key = ReLU(BN(feature)) . Wk^T + ray embedding, val = ReLU(BN'(feature)) . Wv^T   (feature_proj / feature_linear, fax_modules.py:281-292,392-396)
 *   kk = LN(key) . [to_k of attention 1 | attention 2]^T, vv = LN(val) . [to_v | to_v]^T            (fax_modules.py:201-205)
 * for K = 256 / 384 / 512 feature channels and 128 level channels; the key / value maps stay in LDS.  a (M, K) bf16.  ptrs: host
 * array of 18 device pointers, side s (0 key, 1 value) at [9 s ..]: pre_scale, pre_shift (float[K] or null), wp (fragment-ordered
 * [4][K/16]), bp (float[128] or null), skip ((skip_rows, 128) bf16 or null), wn (fragment-ordered stacked next projection), bn
 * (float[Nn]), out ((M, 128) or null), out_next (M, Nn).  dims (int32[10]): dtype (0), M, K, Nn, next_ln, nsides (1 | 2),
 * pre_relu_0, skip_rows_0 (0 = M), pre_relu_1, skip_rows_1.
 */
int cobevt_proj_chain_kv(const void* a, const void* const* ptrs, const int* dims, float eps_next, hipStream_t stream);

/*
 * One half of a SwapFusionBlock in ONE launch (bf16 mode, 128 channels = 4 heads of 32): PreNormResidual(Attention) +
 * PreNormResidual(FeedForward) over the window (map mode 0) or dilated-grid (mode 1) partition of (B, L, H, W, 128) agent maps
 * = opv2v/opencood/models/fusion_modules/swap_fusion_modules.py:87-128 (attention with the 3-D relative position bias and the
 * key mask), :126,172-190 (to_out, residuals, rearranges) and base_transformer.py:102-124 (PreNormResidual / FeedForward), plus
 * the LayerNorm + to_qkv (:93) of the NEXT half while the rows are in LDS.  A workgroup carries 32 query tokens of one
 * window / grid group through attention (one wave per head, K rows straight from L2, V^T in LDS) and the row chain; the
 * attention output never reaches memory (csrc/swap_stage.hip).
 * qkv [rows][384] = to_qkv(LayerNorm(x)) (q | k | v), x / out [rows][128], qkv_next [rows][Nn] (nullable with wn / bn);
 * rows = (b, l, h, w).  map (int32[8]): mode, L, H, W, w1, w2, X, Y as for cobevt_window_attention.  bias_table: the
 * relative-position table one column per head, [4][bias_rows rounded up to a multiple of 4] fp32, multiplied by log2(e) (the
 * kernel's softmax runs in the base-2 domain) and zero-padded to 10240 floats (copied whole), bias_rows = (2L-1)(2w1-1)(2w2-1); mask (B, H, W, L) fp32 (0 = key masked out) or null.  Weights in MFMA fragment order as for
 * cobevt_attn_mlp_chain (wp: to_out, w1 / b1: fc1 with the LayerNorm affine folded in, w2 / b2: fc2, wn / bn: next to_qkv
 * with its LayerNorm folded in).  dims (int32[9]): dtype (0), B, C (128), heads (4), Hd, Hdp, Nn, bias_rows, bias_L.
 */
int cobevt_swap_fusion_stage(const void* qkv, const void* x, void* out, void* qkv_next, const int* map,
                             const float* bias_table, const float* mask, const void* wp, const float* bp, const void* w1,
                             const float* b1, const void* w2, const float* b2, const void* wn, const float* bn,
                             const int* dims, float scale, float eps1, float eps_next, hipStream_t stream);

/* ---- training glue, both directions (csrc/train_glue.hip): what torch autograd + cuDNN run between the convolutions under
 * opv2v/opencood/tools/train_camera.py:143-179.  Channels-last maps flattened to (rows, C) / (N, H, W, C); dtype 0 bf16, 1 fp32;
 * C a multiple of 8 (<= 2048) except where noted. --------------------------------------------------------------------------- */

/* sum[c] = sum over rows of (x - shift[c]) and (sumsq nullable; must be sum + C) sumsq[c] = sum of its squares, fp64 (shift nullable
 * = 0; a shift near the mean keeps the variance from being a cancellation); out_f (nullable): the same values as fp32.
 * scratch: fp64 [scratch_blocks][2][C] for per-workgroup partial sums (no atomics: they serialise on the C result words).
 * BatchNorm batch statistics (torchvision BasicBlock / Bottleneck bn1-3 reached from resnet_ms.py:67-74, fax_modules.py:10,472-489,
 * naive_decoder.py:78-87) and bias gradients (any C: channel counts off the 8-channel piece take a scalar kernel, without shift /
 * out_f). */
int cobevt_channel_sums(const void* x, const float* shift, double* sum, double* sumsq, float* out_f, double* scratch,
                        int scratch_blocks, int dtype, long rows, int C, hipStream_t stream);
int cobevt_f64_to_f32(const double* in, float* out, int n, hipStream_t stream);
/* nn.BatchNorm2d statistics -> per-channel scale / shift (scale = gamma rstd, shift = beta - mean scale), mean / rstd for backward.
 * training != 0: batch statistics from the sums (shifted != 0: they were taken of x - running_mean), running_mean / running_var
 * (nullable) updated in place with `momentum` and the unbiased variance; training == 0: the frozen running statistics.
 * batches_tracked (nullable): the module's int64 num_batches_tracked word, incremented by one. */
int cobevt_bn_finalize(const double* sum, const double* sumsq, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float* scale, float* shift, float* mean, float* rstd, int C, long rows, float eps,
                       float momentum, int training, int shifted, long long* batches_tracked, hipStream_t stream);
/* cobevt_channel_sums (x and x^2, taken about row 0 of x: a pivot inside the data whether or not a running mean exists or is near
 * the batch) + cobevt_bn_finalize(training = 1) as two launches instead of three: the batch statistics of a training BatchNorm2d
 * incl. the running-stat update; running_mean / running_var nullable together; 8 | C. */
int cobevt_bn_batch_stats(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* scale,
                          float* shift, float* mean, float* rstd, double* scratch, int scratch_blocks, int dtype, long rows, int C,
                          float eps, float momentum, long long* batches_tracked, hipStream_t stream);
/* y = act(x * scale[c] + shift[c] (+ residual)), act 0 none / 1 ReLU. */
int cobevt_bn_apply(const void* x, const void* residual, const float* scale, const float* shift, void* y, int dtype, long rows,
                    int C, int act, hipStream_t stream);
/* Backward of cobevt_bn_apply behind the statistics: g = dy [y > 0 when act == 1]; dgamma_dbeta (fp64 [2][C], written) = sum g xhat,
 * sum g; grads_f (nullable) the same as fp32; dx = gamma rstd (g - (dbeta + xhat dgamma) / rows) with batch statistics, gamma rstd g
 * with frozen ones; dres (nullable) = g.  scratch: fp64 [scratch_blocks][2][C], 16-byte aligned or COBEVT_ERR_ARG (the fp32 coefficients
 * of the dx pass are left in its first 2 C words). */
int cobevt_bn_backward(const void* x, const void* y, const void* dy, const float* mean, const float* rstd, const float* gamma,
                       double* dgamma_dbeta, float* grads_f, double* scratch, int scratch_blocks, void* dx, void* dres, int dtype,
                       long rows, int C, int act, int training, hipStream_t stream);
/* nn.MaxPool2d(3, 2, 1) backward (resnet_ms.py:70): dx fp32 (N, H, W, C), every element written; first maximum of a window wins. */
int cobevt_maxpool3x3s2_bwd(const void* x, const void* dy, float* dx, int dtype, int N, int H, int W, int C, hipStream_t stream);
/* the same with dx in the maps' own type (dtype 0 bf16 | 1 fp32): one thread per 2 x 2 input block and 8 channels */
/*
 * Training forms of the FAX BEV query (CrossViewSwapAttention, fax_modules.py:344-372), channels-last, d = 128:
 *   v = W grid + bias - c[b, cam];  query[b, cam, pixel] = v / (||v|| + 1e-7) + x[b, pixel]
 * grid (K, H, W) - or (B, K, H, W): the per-camera homogeneous ray directions of the key-side image embedding (fax_modules.py:330-343,
 * K = 4, n = 1, x null) - w (d, K), bias (d) | null, c (B * n, d), x (B, H, W, d) | null, out / dq (B, n, H, W, d), all fp32; n <= 8.
 * dims (int32[8]): B, n, H, W, d, round_bf16 (1 inside a bf16 autocast region: W, grid, W grid + bias and v rounded to bf16 like torch's
 * autocast conv / subtraction), K (2 | 4), per_batch_grid (0 | 1).  The backward WRITES dx (B, H, W, d) (nullable) and ADDS into
 * dw (d, K), dbias (d) | null, dc (B * n, d).
 * What torch autograd does with a K = 2 convolution, sub, norm, div, add and a permute over the (B, n, d, H, W) tensor
 * (train_camera.py:143-179).
 */
int cobevt_fax_bev_query_train(const float* grid, const float* w, const float* bias, const float* c, const float* x, float* out,
                               const int* dims, hipStream_t stream);
int cobevt_fax_bev_query_train_bwd(const float* grid, const float* w, const float* bias, const float* c, const float* dq, float* dx,
                                   float* dw, float* dbias, float* dc, const int* dims, hipStream_t stream);
/* mean over the n slabs of a contiguous (B, n, inner) tensor -> (B, inner) (backward = 0), or its backward: (B, inner) -> (B, n, inner),
 * every slab = in / n (backward = 1); dtype 0 bf16 | 1 fp32, 8 | inner.  The camera mean of CrossWinAttention (fax_modules.py:243) under
 * train_camera.py:143-179. */
int cobevt_group_mean(const void* in, void* out, int dtype, long B, int n, long inner, int backward, hipStream_t stream);
int cobevt_maxpool3x3s2_bwd_t(const void* x, const void* dy, void* dx, int dtype, int N, int H, int W, int C, hipStream_t stream);
/* nn.PixelUnshuffle(2) (fax_modules.py:479) on channels-last maps: inverse 0: (N, 2Ho, 2Wo, C) -> (N, Ho, Wo, 4C); 1: back. */
int cobevt_pixel_unshuffle2_nhwc(const void* in, void* out, int dtype, int N, int Ho, int Wo, int C, int inverse,
                                 hipStream_t stream);
/* nearest x2 up-sampling (naive_decoder.py:84): backward 0: (N, H, W, C) -> (N, 2H, 2W, C); 1: dy (N, 2H, 2W, C) -> dx (N, H, W, C). */
int cobevt_upsample_nearest2_nhwc(const void* in, void* out, int dtype, int N, int H, int W, int C, int backward,
                                  hipStream_t stream);
/* Input gradient of cobevt_sttf_warp (corpbevt.py:28-64, torch_transformation_utils.py:317-355): dout (B, L, H, W, C) fp32 ->
 * dx (agents, H, W, C) fp32 (zeroed by the caller), scattered through the same sample positions; record_len as there. */
int cobevt_sttf_warp_bwd(const float* dout, const float* tmat, const int* record_len, float* dx, int B, int L, int H, int W, int C,
                         float discrete_ratio, float downsample_rate, hipStream_t stream);

/* Operand preparation of the training convolutions (what cuDNN does internally for the reference's nn.Conv2d / nn.Linear under
 * train_camera.py:143-179; csrc/train_prep.hip).  cobevt_conv_weight_rows: fp32 master weight (Cout, Cin, kh, kw) -> the weight rows
 * cobevt_conv2d_nhwc reads, in the compute type dims[0] (0 bf16, 1 fp32): rows_fwd [Cout][Kpad_fwd] with k = (r * kw + s) * Cin + c,
 * rows_dgrad [Cin][Kpad_dgrad] with k = (r * kw + s) * Cout + o of w[o][c][kh-1-r][kw-1-s] (the input gradient = the same
 * convolution, taps flipped, channel roles swapped); columns past K are zero; either output may be null.
 * dims: [dtype, Cout, Cin, kh, kw, Kpad_fwd, Kpad_dgrad]. */
int cobevt_conv_weight_rows(const float* w, void* rows_fwd, void* rows_dgrad, const int* dims, hipStream_t stream);
/*
 * The same for a 3x3 / pad-1 convolution with 64 | channel counts that runs on the inference kernels in training (bf16): the fp32
 * master weight (Cout, Cin, 3, 3) -> `frag` (cobevt_conv3x3_wfrag_nhwc's fragment table, [Op/32][I/64][9][4][64 lanes][8], Op = O
 * rounded up to 128) and / or `rows3` (cobevt_conv3x3_nhwc's [O][I/64][9][64]); either nullable.  dims (int32[3]): Cout, Cin, dgrad.
 * dgrad = 0: the forward convolution (O = Cout, I = Cin); dgrad = 1: its input gradient, i.e. the convolution with the channel
 * roles swapped and the taps flipped (O = Cin, I = Cout) - what cuDNN's backward-data does under train_camera.py:143-179.
 */
int cobevt_conv3_weight_operands(const float* w, void* frag, void* rows3, const int* dims, hipStream_t stream);
/* ... both directions from one launch: outs[4] = {forward frag, forward rows3, input-gradient frag, input-gradient rows3}, each nullable;
 * dims (int32[2]): Cout, Cin. */
int cobevt_conv3_weight_operands2(const float* w, void* const* outs, const int* dims, hipStream_t stream);
/* The same for a dense projection / 1x1 stride-1 convolution on the inference row-GEMM kernel (cobevt_linear_rows_small_k) in training:
 * fp32 master weight (N, K) -> the bf16 fragment tables of cobevt_linear_rows_small_k ([Rp/32][Cp/16][64 lanes][8], both padded to 128):
 * `frag` for the projection (rows N, contraction K), `frag_t` for its input gradient dx = dy W (rows K, contraction N); either nullable,
 * one launch.  dims (int32[2]): N, K. */
int cobevt_linear_weight_frags(const float* w, void* frag, void* frag_t, const int* dims, hipStream_t stream);
/*
 * Weight gradient of a 3x3 / stride-1 / pad-1 convolution from the channels-last bf16 maps themselves (csrc/wgrad3.hip: the
 * pixel-major operands of the matrix instruction come out of LDS through ds_read_b64_tr_b16, no blocked copies, no atomics):
 * dw (Cout, Cin, 3, 3) fp32 is WRITTEN (not accumulated).  x (N, H, W, Cin), dy (N, H, W, Cout) bf16, 32 | Cin, 32 | Cout, 16 | W.
 * cobevt_conv_wgrad3_chunks(dims[5]: N, H, W, Cin, Cout) returns the number of partial copies of dw the launch writes (scratch must hold
 * that many x Cout * Cin * 9 floats), or minus an error code when the shape is not served (the caller then takes
 * cobevt_conv_wgrad_blocked); cobevt_conv_wgrad3 takes dims (int32[6]): N, H, W, Cin, Cout, that chunk count.
 * cuDNN's backward-filter under train_camera.py:143-179.
 */
int cobevt_conv_wgrad3_chunks(const int* dims);
int cobevt_conv_wgrad3(const void* x, const void* dy, float* dw, float* scratch, const int* dims, hipStream_t stream);
/*
 * The same for a dense projection / 1x1 stride-1 convolution: dw (Cout, Cin) fp32 = dy^T x over R bf16 rows (x (R, Cin), dy (R, Cout),
 * 128 | Cin, 128 | Cout), written, not accumulated - nn.Linear's backward-filter under train_camera.py:143-179.
 * cobevt_linear_wgrad_chunks(dims[3]: R, Cin, Cout) -> partial copies of dw in `scratch` (or minus an error code);
 * cobevt_linear_wgrad dims (int64[4]): R, Cin, Cout, that chunk count.
 */
int cobevt_linear_wgrad_chunks(const long* dims);
int cobevt_linear_wgrad(const void* x, const void* dy, float* dw, float* scratch, const long* dims, hipStream_t stream);
/* bf16 channels-last map (N, H, W, C) -> the blocked operand of cobevt_conv_wgrad_blocked, dst [N][Hp][NB][C][8]: pixel x of input
 * row y sits in block (x + pad_left) / 8 of row y + pad_top; everything else is zero.  In general dst is [N][Hp][NB][P][C][8] and slot j
 * of plane q of block b holds input pixel sx (8 b + j) + q - pad_left (P = 1, sx = 1 above; P = 2, sx = 2: even / odd columns of a
 * stride-2 convolution; P = k, sx = stride: the k tap columns of a tap row as planes).
 * dims: [N, H, W, C, Hp, NB, pad_top, pad_left, P, sx]. */
int cobevt_wgrad_block_operand(const void* src, void* dst, const int* dims, hipStream_t stream);

/* Backward pieces of the nuScenes SinBEVT training path (csrc/train_nusc.hip; torch autograd + cuDNN in the reference:
 * nuscenes/cross_view_transformer/model/model_module.py:35-60 over backbones/efficientnet.py:85-96, decoder.py:27-36, losses.py:27-84).
 * cobevt_swish: dy == NULL: out = x sigmoid(x) (efficientnet-pytorch's MemoryEfficientSwish); else out = dy d/dx; n elements (multiple of 8),
 * dtype 0 bf16 / 1 fp32. */
int cobevt_swish(const void* x, const void* dy, void* out, int dtype, long n, hipStream_t stream);
/* Weight gradient of the depthwise k x k convolution (k = 3 / 5): dw fp32 [k * k][C] += sum over output pixels of dy (N, Ho, Wo, C) x the
 * tap-shifted x (N, H, W, C); ADDED to what dw holds (zero it for a plain gradient): a workgroup's share is summed in fp64 and added with one
 * fp32 atomic per entry, at most 256 per entry.  dims (int32[11]): dtype, N, H, W, C, k, stride, pad_top, pad_left, Ho, Wo.  (The input
 * gradient is cobevt_depthwise_conv_nhwc on the flipped taps, on the zero-stuffed gradient when strided.) */
int cobevt_depthwise_wgrad(const void* x, const void* dy, float* dw, const int* dims, hipStream_t stream);
/* Adjoint of cobevt_resize_nhwc mode 1 (align_corners bilinear; nn.Upsample of decoder.py:12): dy (N, Ho, Wo, C) -> dx fp32 (N, H, W, C),
 * ADDED with fp32 atomics to what dx holds (zero it first).  Both kernels take source row floor(fp32(oh * scale)), scale = fp32((H - 1) / (Ho - 1))
 * (0 when Ho == 1), clamp the next row to H - 1 and weigh it by fma(oh, scale, -floor), the fraction of the unrounded product; columns alike. */
int cobevt_resize_bilinear_bwd(const void* dy, float* dx, int dtype, int N, int H, int W, int C, int Ho, int Wo, hipStream_t stream);
/* Gradient of cobevt_sigmoid_focal_loss's mean w.r.t. the logits: dpred (N, C, hw) fp32 = gscale[0] / count x d loss / d logit on the kept
 * elements, 0 elsewhere.  stats = the forward's out[3] (mean, sum, count) and gscale (the upstream gradient) are DEVICE words: no host sync.
 * With count == 0 (no pixel kept) every element is 0. */
int cobevt_sigmoid_focal_loss_bwd(const float* pred, const float* label, const unsigned char* visibility, const unsigned int* label_mask,
                                  const float* stats, const float* gscale, float* dpred, int N, int C, int NL, int hw, int min_visibility,
                                  float alpha, float gamma, int soft_label, hipStream_t stream);

/* ---- multi-GPU: the V2V feature-sharing step in front of FuseBEVT.  The reference keeps all agents in one
 * process (opv2v/opencood/models/corpbevt.py:112-124, sub_modules/fuse_utils.py:8-61: agents are a batch dimension up to
 * `regroup`); its only collective call sites are the DDP set-up in opv2v/opencood/tools/multi_gpu_utils.py:32-37 and
 * train_camera.py:105-110.  With one agent per GPU the (32, 32, 128) per-agent blocks (256 KiB bf16) are exchanged once per
 * frame: either by RCCL (torch.distributed.all_gather_into_tensor, cobevt_amd/dist.py) or by the one-shot direct exchange
 * below - every rank owns a WINDOW of uncached device memory mapped by all peers through hipIpc, and one launch pair per
 * frame stores the local blocks straight into the destination windows over xGMI (csrc/peer_gather.hip). ------------------ */

/* Allocate this rank's window: `bytes` of block storage (multiple of 16) followed by the flag words, zero-filled; writes the
 * device pointer and the 64-byte hipIpc handle peers open with cobevt_peer_window_open.  Synchronous (set-up time only). */
int cobevt_peer_window_alloc(long bytes, void** dptr, void* handle64);
/* Map a peer's window into this process (hipIpcOpenMemHandle with lazy peer access). */
int cobevt_peer_window_open(const void* handle64, void** dptr);
int cobevt_peer_window_close(void* dptr);
int cobevt_peer_window_free(void* dptr);
/* Synchronise `stream`, then read the local window's status (0 = every bounded wait so far completed, 1 = a peer's
 * "window free" acknowledgement timed out, 2 = a peer's data-ready flag timed out) and the count of completed exchanges. */
int cobevt_peer_window_status(const void* window, long bytes, int* status, int* epoch, hipStream_t stream);
/* The same read in stream order, no synchronisation: the window's 32 flag words (status at [18], completed exchanges at [16]) are copied
 * to `host_words` (pinned host memory); look at them after an event recorded behind this call has completed. */
int cobevt_peer_window_status_async(const void* window, long bytes, unsigned int* host_words, hipStream_t stream);
/* One exchange, two launches on `stream` (capturable in a HIP graph: the epoch lives in the window).  windows: HOST array
 * of `world` (<= 8) device pointers = this process's mappings of every rank's window, the own window at [rank].  local:
 * n_local (<= 16) contiguous blocks of block_bytes; block j is stored at block slot dest_block[j] of rank dest_rank[j]'s
 * window, or of every rank's window when dest_rank[j] < 0 (all-gather).  When the second launch retires, every block
 * addressed to this rank has landed in its window.  spin_limit: bound on the flag polls (<= 0: default, ~30 s). */
int cobevt_peer_exchange(const void* local, void* const* windows, int world, int rank, int n_local, long block_bytes,
                         const int* dest_rank, const int* dest_block, long window_bytes, long spin_limit,
                         hipStream_t stream);

/*
 * Box calibration (bench.py `box_calibration`; no reference counterpart - the reference's benchmark protocol,
 * nuscenes/scripts/benchmark.py:42-55, reports wall time only).  cobevt_calibrate_mfma: `blocks` workgroups of 4 waves issue
 * 4 * iters independent v_mfma_f32_32x32x16_bf16 each (no operand traffic): 2 * 32*32*16 * 16 * iters flops per workgroup;
 * clk[0] / clk[1] (device int64[2]) = shader-clock / 100-MHz wall-clock ticks workgroup 0 spent in the loop.  out: fp32
 * [blocks * 256].  cobevt_calibrate_copy: streaming copy of `bytes` (multiple of 16) src -> dst.
 */
int cobevt_calibrate_mfma(float* out, long long* clk, int blocks, int iters, hipStream_t stream);
int cobevt_calibrate_copy(const void* src, void* dst, long bytes, hipStream_t stream);
/* rate of the wall clock behind clk[1] and the device's maximum shader clock (kHz), of the current device */
int cobevt_calibrate_clock_khz(int* wall_khz, int* sclk_max_khz);

/*
 * LiDAR pillar front end (csrc/pillar_vfe.hip): PillarVFE with ONE PFN layer of 64 channels (pillar_vfe.py:10-53, 105-146), fused with
 * PointPillarScatter (point_pillar_scatter.py:14-47) and regroup (fuse_utils.py:8-61).  fp32 VALU arithmetic in every library; only
 * the store converts to `dtype`.
 *   voxel_features (P, T, 4) fp32, T <= 32; voxel_num_points (P) int32; voxel_coords (P, 4) int32 as [n, z, y, x];
 *   w (K, 64) / shift (64) fp32: the eval BatchNorm1d folded into the bias-free Linear (or the Linear's weight^T and bias);
 *   dims  = [P, T, F = 4, K, use_absolute_xyz, with_distance, dtype, rows, N, B, max_cav, ny, nx] (host), K = (4 | 1) + 6 + (1 | 0);
 *   geom  = [voxel x, y, z, offset x, y, z] (host), offset = voxel / 2 + range minimum.
 * rows = 0: `out` is the channels-last canvas - (B, max_cav, ny, nx, 64) with record_len (device int32 (B)), which also writes
 * cav_mask (B, max_cav) fp32 as cobevt_regroup does, or (N, ny, nx, 64) when record_len is NULL.  Two launches: every 16-byte chunk of
 * the canvas <- 0, then one 64-channel row per pillar at cell z + y * nx + x of its agent's slot.  A pillar is skipped (never
 * written) when its batch index is negative, >= N or regroups to a slot >= max_cav, when y or x lies outside the grid, or when
 * voxel_num_points <= 0.  Coordinates are unique per agent (the voxel generator's contract).  No atomics, no host synchronisation.
 * rows = 1: `out` is (P, 64), destination row = p (a pillar with voxel_num_points <= 0 gives a zero row); N .. nx are ignored.
 */
int cobevt_pillar_vfe(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, const float* w,
                      const float* shift, const int* record_len, void* out, float* cav_mask, const int* dims, const float* geom,
                      hipStream_t stream);
/* PointPillarScatter on given rows: rows (P, C) in `dtype` (C * element size a multiple of 16) -> out (N, ny, nx, C), every chunk
 * zeroed first; the skip rules of the fused operator without the point count. */
int cobevt_scatter_rows(const void* rows, const int* voxel_coords, void* out, int dtype, long P, int C, int N, int ny, int nx,
                        hipStream_t stream);

/*
 * Train mode of the pillar front end (csrc/train_pillar.hip): Linear -> BatchNorm1d on BATCH statistics -> ReLU -> max over T
 * (pillar_vfe.py:31-53 in train()).  The statistics run over the rows of exactly the pillars cobevt_pillar_vfe writes (rows form:
 * voxel_num_points > 0), masked all-zero rows included, and are formed from sum(f) and the K x K Gram matrix of the decorated features
 * in fp64 - no (P, T, 64) tensor.  dims / geom as for cobevt_pillar_vfe (dims[6], the dtype, is ignored: fp32).  No host read, no
 * floating-point atomics: results are bitwise reproducible and do not depend on where skipped rows sit in the batch.
 *
 * cobevt_pillar_train_scratch: element counts of `partial` (fp64) for _stats and of `partial` (fp32) for _bwd at P pillars.
 *
 * cobevt_pillar_train_stats, mode 0 batch statistics | 1 frozen running statistics | 2 no norm (gamma NULL, beta = the Linear's bias):
 *   w (64, K) the Linear's weight; order (P) int32, dst (P) int64, count (1) int32: the valid pillars in index order, their
 *   destination rows and their number (written in every mode); w_folded (K, 64), shift_folded (64): the operands cobevt_pillar_vfe
 *   takes for the forward; stat (512) fp64: M = count x T, sum(f), the Gram matrix, mean, rstd, biased variance, for the backward.
 *   Mode 0 also updates running_mean / running_var (the latter with M / (M - 1)) at `momentum` and adds 1 to num_batches_tracked
 *   (int64), all three optional; with zero valid pillars nothing is updated.
 *
 * cobevt_pillar_train_bwd: dout = gradient of the canvas (or of the dense rows), fp32, read at every valid pillar's destination row
 *   where its maximum is positive, applied at the winning row (lowest index on ties).  dw (64, K), dgamma (64), dbeta (64; d bias in
 *   mode 2) fp32; the other arguments as _stats left them.
 */
int cobevt_pillar_train_scratch(long P, long* stats_doubles, long* bwd_floats);
int cobevt_pillar_train_stats(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, const int* record_len,
                              const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                              long* num_batches_tracked, int* order, long* dst, int* count, double* partial, float* w_folded,
                              float* shift_folded, double* stat, const int* dims, const float* geom, int mode, float eps, float momentum,
                              hipStream_t stream);
int cobevt_pillar_train_bwd(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, const int* order,
                            const long* dst, const int* count, const float* w_folded, const float* shift_folded, const float* w,
                            const float* gamma, const double* stat, const float* dout, float* partial, float* dw, float* dgamma,
                            float* dbeta, const int* dims, const float* geom, int mode, hipStream_t stream);
/* backward of cobevt_scatter_rows: rows (P, C) <- the canvas gradient (N, ny, nx, C) at each row's cell; zero for skipped rows */
int cobevt_gather_rows(const void* canvas, const int* voxel_coords, void* rows, int dtype, long P, int C, int N, int ny, int nx,
                       hipStream_t stream);

/*
 * Voxelisation of raw LiDAR points (csrc/voxelize.hip): spconv's points_to_voxel with OpenCOOD's collate, producing the voxel dict
 * cobevt_pillar_vfe reads.  fp32 / int32 only, identical in every library.
 *   points (M, 4) fp32 [x, y, z, intensity], the agents' points concatenated; point_offsets (N + 1) int32 ON THE DEVICE: agent a
 *   owns rows offsets[a] .. offsets[a + 1], rows at or past offsets[N] are ignored (M can stay fixed under graph replay);
 *   dims  = [M, N, T, max_voxels, nx, ny, nz, range_mask, ego_mask] (host), T in 1 .. 32, nz = 1, max_voxels per agent;
 *   geom  = [x0, y0, z0, x1, y1, z1, voxel x, y, z] (host).
 * Per agent, in input order: a point is dropped when a coordinate is not finite, when range_mask is set and the strict inequalities
 * of pcd_utils.mask_points_by_range fail, when ego_mask is set and it lies in the box of pcd_utils.mask_ego_points, or when
 * floor((p - lo) / voxel) (fp32, correctly rounded subtract and divide) is outside the grid on any axis.  The first kept point of a
 * cell opens a voxel; voxels are numbered in order of their first point; once an agent has max_voxels, cells that would open
 * another are dropped with all their points while open cells keep accepting points.  A voxel keeps the first T points of its cell.
 * Outputs, Pcap = N * max_voxels rows, agent a's voxels from row a * max_voxels: voxel_features (Pcap, T, 4) - slots past the
 * point count zero; voxel_coords (Pcap, 4) = [a, 0, y, x]; voxel_num_points (Pcap); num_voxels (N).  Rows without a voxel get
 * voxel_coords [-1, 0, 0, 0] and voxel_num_points 0 (the padding rows cobevt_pillar_vfe skips); their voxel_features are NOT
 * written.  Seven launches, integer atomics only, no workgroup waits on another, no host read, no allocation; the result does not
 * depend on scheduling (bitwise reproducible).  workspace: cobevt_voxelize_scratch(dims) ints, contents irrelevant on entry.
 * points, voxel_features and voxel_coords must be 16-byte aligned.
 */
int cobevt_voxelize_scratch(const long* dims, long* workspace_ints);
int cobevt_voxelize_points(const float* points, const int* point_offsets, float* voxel_features, int* voxel_coords,
                           int* voxel_num_points, int* num_voxels, int* workspace, const long* dims, const float* geom,
                           hipStream_t stream);
/*
 * The same on a 3-D grid (csrc/voxelize.hip): cells (z, y, x), voxel_coords (Pcap, 4) = [a, z, y, x] - the voxel dict cobevt_mean_vfe
 * and cobevt_sparse_index read.  Pointers, geom, drop rules, numbering, cap, outputs and padding rows exactly as
 * cobevt_voxelize_points, with floor((p.z - z0) / voxel z) in [0, nz) in place of its single cell over the height; on an nz = 1 grid
 * the four outputs are bit-identical to cobevt_voxelize_points'.
 *   dims  = [M, N, T, max_voxels, nx, ny, nz, range_mask, ego_mask, slots] (host), T in 1 .. 32, nx, ny, nz in 1 .. 2^24 each (every
 *   cell index exact in fp32) and N nx ny nz <= 2^62; slots: the entries of the hash table below - a power of two, M < slots <= 2^31 -
 *   or 0 for the default, the smallest power of two >= max(2 M, 64).
 * The per-cell tables of cobevt_voxelize_points are indexed by the slot that the cell's 64-bit key agent * (nx ny nz) + (z ny + y) nx
 * + x holds in an open-addressed table (64-bit compare-and-swap on the key word, linear probing, at most `slots` probes, no thread
 * waits on another; slots > M leaves an empty slot at all times), so time and workspace follow M, slots and N max_voxels and not the
 * grid.  Which slot a key gets depends on scheduling and stays inside the workspace; the outputs do not (bitwise reproducible).
 * Seven launches, integer atomics only, no host read, no allocation.  workspace: cobevt_voxelize3d_scratch(dims) ints (6 slots +
 * N max_voxels + 2 M + ...), contents irrelevant on entry, 8-byte aligned (the keys lead it); points, voxel_features and voxel_coords
 * 16-byte aligned.  A null pointer is COBEVT_ERR_ARG; a T, grid, slots, alignment or voxel size outside the above COBEVT_ERR_SHAPE,
 * before any launch.
 */
int cobevt_voxelize3d_scratch(const long* dims, long* workspace_ints);
int cobevt_voxelize3d_points(const float* points, const int* point_offsets, float* voxel_features, int* voxel_coords,
                             int* voxel_num_points, int* num_voxels, int* workspace, const long* dims, const float* geom,
                             hipStream_t stream);

/*
 * LiDAR detection output (csrc/detect_post.hip): OpenCOOD's VoxelPostprocessor.post_process - box decode, box filters, the cut at
 * the 1000 best-scored candidates, rotated NMS, range mask - and its pieces.  fp32 / int32 data, fp64 only inside the quad clip;
 * identical in every library.
 *
 * cobevt_detect_post: ncav in 1 .. 16 agents ("cavs").  psm, rm, anchors: HOST arrays of ncav DEVICE pointers - cav c's psm
 *   (1, A, H, W) and rm (1, 7A, H, W) in NCHW fp32 (channel a * 7 + k of rm = delta k of anchor a) and anchors (H, W, A, 7) fp32;
 *   matrices (ncav, 4, 4) fp32 ON THE DEVICE; cav_dims = [H, W, A] per cav (host); hwl != 0: the box order 'hwl' (size columns read
 *   as [5, 4, 3]), otherwise as they stand.  The global anchor index counts cav 0's anchors in (h, w, a) order, then cav 1's, ...
 *   score = sigmoid(psm); box = delta_to_boxes3d (x, y scaled by the anchor diagonal sqrt(a4^2 + a5^2), z by a3, exp on the sizes,
 *   yaw added); corners as boxes_to_corners_3d, projected by the cav's matrix.  A candidate survives when score > score_threshold,
 *   x extent <= 6, y extent <= 6, y extent != 0 (the reference's z_len is computed from the y column and used as a truth value),
 *   min z >= -3, max z <= 1 and every coordinate is finite.  The 1000 best-scored survivors of all cavs (no cap before that cut;
 *   equal scores: lower global index first) go through greedy NMS on the IoU of corners 0 .. 3 in xy (fp64 clip of the fp32 corners,
 *   suppressed when (float)iou > nms_thresh); picked boxes with all 8 corners in x [-140, 140], y [-40, 40] are written in pick
 *   order: boxes (1000, 8, 3), scores (1000), index (1000) = global anchor index, count (1).  Rows at and past count are zero.
 *   One 8-byte memset node and four launches (decode, select + sort, mask, greedy), integer atomics only, no workgroup waits on
 *   another, no host read, no allocation, bitwise reproducible.  workspace: cobevt_detect_scratch(total anchors) BYTES, 8-byte
 *   aligned, contents irrelevant on entry.  Skip rules: none - every anchor of every cav is decoded.
 *
 * cobevt_nms_rotated: the same selection, mask and greedy pass on N given boxes - box_corners (N, 8, 3) (corner_floats = 24) or
 *   (N, 4, 2) (corner_floats = 8, written back as corners 0 .. 3 with z = 0) and box_scores (N), any sign - without filters and
 *   without the range mask: box_utils.nms_rotated.  index = the kept boxes' input rows in pick order.  workspace:
 *   cobevt_detect_scratch(N).  N = 0 gives count 0.
 *
 * cobevt_delta_to_boxes3d: rm (N, 7A, H, W), anchors (H, W, A, 7) -> boxes3d (N, H W A, 7), N >= 1.  One launch.
 * cobevt_rotated_iou: a (N, 4, 2), b (M, 4, 2) fp32 -> iou (N, M) fp64 by the same device function (either winding; a pair whose
 *   union has no area gives 0).  One launch; N = 0 or M = 0 launches nothing.
 */
int cobevt_detect_scratch(long total_anchors, long* workspace_bytes);
int cobevt_detect_post(const float* const* psm, const float* const* rm, const float* const* anchors, const float* matrices,
                       const int* cav_dims, int ncav, int hwl, float score_threshold, float nms_thresh, float* boxes, float* scores,
                       int* index, int* count, void* workspace, hipStream_t stream);
int cobevt_nms_rotated(const float* box_corners, const float* box_scores, long N, int corner_floats, float nms_thresh, float* boxes,
                       float* scores, int* index, int* count, void* workspace, hipStream_t stream);
int cobevt_delta_to_boxes3d(const float* rm, const float* anchors, float* boxes3d, int N, int H, int W, int A, hipStream_t stream);
int cobevt_rotated_iou(const float* a, const float* b, double* iou, long N, long M, hipStream_t stream);

/*
 * LiDAR detection targets and loss (csrc/detect_targets.hip): OpenCOOD's
 * VoxelPostprocessor.generate_label with the box_overlaps.bbox_overlaps it needs, and the PointPillar detection loss with its
 * gradient.  fp32 / int32 data, fp64 only in the loss sums; identical in every library.
 *
 * cobevt_boxes_standup: boxes (n, 7) fp32 in 'hwl' order -> standup (n, 4) fp32 [x1, y1, x2, y2], the axis-aligned hull of the four
 *   rotated footprint corners (boxes_to_corners_3d + corner2d_to_standup_box; length = column 5, width = column 4), every product
 *   and sum a separately rounded fp32 operation.  standup 16-byte aligned.  One launch; n = 0 launches nothing.
 *
 * cobevt_detect_targets: anchors (H, W, A, 7) fp32 and their standup boxes (H W A, 4); gt_boxes (B, G, 7), gt_standup (B, G, 4),
 *   mask (B, G) fp32, G <= 128 (more: code 2; G = 0 or a mask without a 1 is valid: everything negative).  A slot is valid when its
 *   mask == 1; column k of the IoU matrix is the k-th VALID box and targets are taken from that same box (the reference indexes the
 *   unfiltered array with the filtered index: the same thing for a prefix mask).  IoU = bbox_overlaps on the standup boxes with the
 *   `+1` convention, bit-identical to the compiled reference: float coordinate differences, the `+ 1.0` sums, both areas and the
 *   union in double (Cython emits the literal as a double), rounded to float once, then a float division - no fused multiply-add,
 *   correctly rounded division.  Per valid gt the
 *   highest anchor = the lowest anchor index of maximal IoU, kept when that IoU > 0.  Positive: any IoU > pos_threshold, or a kept
 *   highest anchor; matched gt = the lowest k with IoU > pos_threshold if there is one, else the lowest k it is the kept highest
 *   of.  Negative: every IoU < neg_threshold, cleared for kept highest anchors.  Outputs, all elements written: pos_equal_one and
 *   neg_equal_one (B, H, W, A) fp32 0 / 1, targets (B, H, W, 7A) fp32 [(gx - ax) / d, (gy - ay) / d, (gz - az) / a3, log(g3 / a3),
 *   log(g4 / a4), log(g5 / a5), g6 - a6] with d = sqrt(a4^2 + a5^2) for positives and 0 elsewhere, num_pos (B) int32.
 *   Two memset nodes and two launches (one when G = 0); the per-gt maximum crosses workgroups by atomicMax on 64-bit integer keys
 *   (IoU bits, inverted anchor index): integer atomics only, bitwise reproducible, no host read, no allocation.
 *   workspace: 8 * B * max(G, 1) bytes, 8-byte aligned, contents irrelevant on entry; the standup boxes 16-byte aligned.
 *
 * cobevt_pointpillar_loss: psm (B, A, H, W) and rm (B, 7A, H, W) NCHW fp32 (channel a * 7 + k of rm = component k of anchor a),
 *   pos_equal_one (B, H, W, A), targets (B, H, W, 7A), num_pos (B) int32 or NULL (then counted as pos_equal_one > 0, one more
 *   launch with integer atomics) -> loss (3) fp32 = [total, conf_loss, reg_loss] and, when dpsm and drm are given (both or
 *   neither), d total / d psm and d total / d rm in the maps' own layouts, from the same launch.  With p_b = max(1, num_pos[b]) and
 *   t = pos_equal_one: conf_loss = cls_weight / B * sum [0.25 t + 0.75 (1 - t)] pt^2 bce / p_b, bce = max(x, 0) - x t +
 *   log1p(exp(-|x|)), pt = t (1 - sigmoid(x)) + (1 - t) sigmoid(x); reg_loss = reg / B * sum over t > 0 of smooth_l1(d_k) / p_b with
 *   beta = 1 / 9, d_k = rm_k - tgt_k (k < 6), d_6 = sin(rm_6) cos(tgt_6) - cos(rm_6) sin(tgt_6), a NaN target counting as d = 0;
 *   total = conf_loss + reg_loss.  Per-element arithmetic fp32, sums fp64 in a fixed order (one partial pair per workgroup, then
 *   one finishing workgroup): no floating-point atomics, bitwise reproducible.
 *   workspace: 16 * ceil(H W / 256) * A * B + 4 * B bytes, 8-byte aligned.
 */
int cobevt_boxes_standup(const float* boxes, float* standup, long n, hipStream_t stream);
int cobevt_detect_targets(const float* anchors, const float* anchor_standup, const float* gt_boxes, const float* gt_standup,
                          const float* mask, float pos_threshold, float neg_threshold, float* pos_equal_one, float* neg_equal_one,
                          float* targets, int* num_pos, void* workspace, int B, int H, int W, int A, int G, hipStream_t stream);
int cobevt_pointpillar_loss(const float* psm, const float* rm, const float* pos_equal_one, const float* targets, const int* num_pos,
                            float* loss, float* dpsm, float* drm, void* workspace, int B, int H, int W, int A, float cls_weight,
                            float reg, hipStream_t stream);

/*
 * LiDAR BEV maps, the PIXOR formulation: OpenCOOD's BevPreprocessor (csrc/bev_points.hip) and
 * LidarBevPostprocessor (labels: csrc/bev_labels.hip; post_process: the bev mode of csrc/detect_post.hip).  Identical in every library.  No timing of these entry
 * points has been measured yet.
 *
 * cobevt_bev_points: points (M, 4) fp32 [x, y, z, intensity] of N agents and point_offsets (N + 1) int32 ON THE DEVICE, with the
 *   conventions of cobevt_voxelize_points (rows at or past offsets[N] are ignored) -> bev (N, C, nx, ny) fp32, or (N, nx, ny, C) when
 *   channels_last is set: channels 0 .. C - 2 the binary occupancy of the height slices, channel C - 1 the mean intensity.
 *   dims = [M, N, nx, ny, C, range_mask, ego_mask, channels_last] (host), C >= 2;
 *   geom = [x0, y0, z0, x1, y1, z1 (cav_lidar_range, for range_mask), L1, W1, H1, res] (host, DOUBLES).
 *   Index per axis: trunc(((double)p - origin) / res) - fp64 on the fp32 point, truncation toward zero, not floor: a point in
 *   (origin - res, origin) falls into cell 0.  Skip rules: a point is dropped when a coordinate or its intensity is not finite, when
 *   |intensity| >= 2^8, when a mask removes it (same rules as cobevt_voxelize_points) or when its index is outside [0, nx) x [0, ny)
 *   x [0, C - 1) - a deliberate deviation: the reference wraps negative indices and writes iz = C - 1 into the intensity channel.
 *   Every kept point sets bev[ix, iy, iz] = 1; the intensity channel is the mean intensity of the cell's kept points, 0 without one.
 *   Order independence: per cell a 32-bit count and a 64-bit fixed-point sum (quantum 2^-32) in separate arrays, integer atomics
 *   only, then a finalise pass that divides in fp64 and rounds to fp32 once.  Intensities with 2^-9 <= |i| < 2^8 are summed exactly,
 *   smaller ones with a per-point error <= 2^-33: |out - mean| <= 2^-33 + 2^-24 |mean| (1 + 2^-20).  Bitwise identical under any
 *   permutation of the points and from run to run.  Two memset nodes (bev, workspace) and two launches (points, finalise; M = 0: one);
 *   no host read, no allocation.  workspace: cobevt_bev_points_scratch(dims) ints, 8-byte aligned, contents irrelevant on entry;
 *   points 16-byte aligned.
 *
 * cobevt_bev_labels: LidarBevPostprocessor.generate_label for a batch.  gt_boxes (B, G, 7) fp32 in 'lwh' order, mask (B, G) fp32
 *   (valid when == 1), G <= 128 (more: code 2; G = 0 is valid) -> label_map (B, 7, lx, ly) fp32, bev_corners (B, G, 4, 2) fp32 (valid
 *   boxes compacted to the front in slot order, zero rows behind them) and num_valid (B) int32.  dims = [B, G, lx, ly] (host);
 *   params = [L1, W1, res, downsample_rate, target_mean (6), target_std_dev (6)] (host, doubles; res, rate > 0, std != 0).
 *   Corners 0 .. 3 of boxes_to_corners_3d in separately rounded fp32 (cos / sin: the fp64 functions rounded to fp32); everything
 *   after that in fp64 in the reference's operation order: pixel (i, j) belongs to a box when (p_rel . e) / (e . e) is in [0, 1]
 *   inclusive for both edges c1 - c0 and c3 - c0 of the corners in label-pixel units; targets [1, cos yaw, sin yaw, x - px, y - py,
 *   log dx, log dy] with (px, py) from dist_to_continuous.  Tie rule: where boxes overlap the LAST valid box wins.  Channels 1 .. 6 of
 *   every pixel, background included, are (v - mean) / std; one cast to fp32.  Skip rule: a box with an edge of squared norm <= 1e-6
 *   (the reference asserts) marks no pixel.  One launch, no atomics, no host read, no allocation.
 *
 * cobevt_bev_post: LidarBevPostprocessor.post_process.  cls, reg: HOST arrays of ncav (1 .. 16) DEVICE pointers - cav c's cls
 *   (1, 1, lx, ly) and reg (1, 6, lx, ly) fp32; matrices (ncav, 4, 4) fp32 ON THE DEVICE; cav_dims = [lx, ly] per cav (host); params as
 *   for cobevt_bev_labels.  prob = sigmoid(cls) in fp32; a pixel is a candidate when prob > score_threshold and every decoded value
 *   is finite.  reg * std + mean, atan2, exp, the cell centre (float)(L1 + i res rate) + x and the corner template are fp64; the
 *   rotation, the `+= centre` (one fp64 add rounded to fp32) and the projection by the cav's matrix are rounded to fp32 where the
 *   reference rounds.  Then cobevt_detect_post's own select + sort, mask and greedy launches: the 1000 best of all cavs (equal
 *   scores: lower global pixel index first), suppression when (float)iou > nms_thresh, and the GT_RANGE test on the four corners, x
 *   in [-140, 140] and y in [-40, 40], after suppression.  Outputs in pick order: boxes (1000, 4, 2), scores (1000), index (1000) =
 *   the global pixel index (cav 0's pixels in (i, j) order, then cav 1's), count (1); rows at and past count are zero.  One 8-byte
 *   memset node and four launches (bev decode, select + sort, mask, greedy); integer atomics only, no host read, no allocation,
 *   bitwise reproducible.  workspace: cobevt_detect_scratch(total pixels) BYTES, 8-byte aligned.  Skip rules: none.
 */
/*
 * cobevt_prepare_points (csrc/cloud_prep.hip; identical in every library): per-agent SENSOR-frame clouds and
 *   their matrices -> one compact ego-frame cloud, the input of cobevt_voxelize_points / cobevt_bev_points.  What the reference's
 *   datasets do in NumPy: pcd_utils.mask_ego_points, lidar_project, DataAugmentor (world flip / rotation / scaling),
 *   mask_points_by_range and the vstack.
 *   points (M, 4) fp32 and point_offsets (N + 1) int32 ON THE DEVICE with the conventions of cobevt_voxelize_points (rows at or past
 *   offsets[N] are ignored); transforms (N, 4, 4) fp64 on the device or null (no projection); order (M) int32 on the device or null:
 *   row i reads points[order[i]] - it must map each agent's row range onto itself, which is NOT checked (an entry outside [0, M)
 *   drops the row); out (M, 4) fp32, not overlapping points; out_offsets (N + 1) int32: each agent's start in out.
 *   dims = [M, N, G, ego_mask, range_mask, flip_x, flip_y, rotate, scale, boxes are fp64] (host), G <= 128 (more: code 2);
 *   geom = [x0, y0, z0, x1, y1, z1 (for range_mask), cos, sin (fp32 values of the fp32 angle), angle, scale] (host, DOUBLES).
 *   Per agent, in input (or `order`) order:
 *     1 ego mask (ego_mask) on the sensor-frame fp32 point, the rule of cobevt_voxelize_points;
 *     2 projection (transforms): ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] in fp64, this association, no contraction;
 *     3 augmentation: flip_x negates y, flip_y negates x; rotate rounds x, y, z to fp32, forms x c - y s and x s + y c in fp64 from
 *       the fp32 values and rounds each to fp32; scale is fl32(v * fl32(scale)) - the reference where its points are fp32 at that
 *       step; after a projection without a rotation it multiplies its fp64 array by the fp64 scale, up to one fp32 ulp away; the
 *       intensity is copied bitwise;
 *     4 the point is rounded to fp32;
 *     5 range mask (range_mask): strict inequalities against the limits rounded to fp32, on the fp32 OUTPUT point - a deliberate
 *       deviation where the reference still holds fp64 points (140.7999999 against 140.8 is kept there and dropped here);
 *     6 stable compaction.  Rows of out at or past out_offsets[N] are NOT written.
 *   Skip rules: none for non-finite values, IEEE comparisons decide (a NaN survives the ego mask and fails the range mask).
 *   boxes (G, 7) and box_mask (G), both fp32 or both fp64, or null with G = 0: rows with mask == 1 get stage 3 in place as
 *   augment_utils applies it to boxes, in fp64 - flip_x: y, heading negated; flip_y: x negated, heading <- -(h + pi); rotate: x, y, z
 *   rounded to fp32 and rotated as the points, heading += angle; scale: columns 0 .. 5 times the fp64 scale - and are rounded to
 *   their dtype once; other rows are untouched.
 *   Three launches (classify: a flag bit per point and a count per 1024 points; scan: one workgroup, and one more for the boxes;
 *   scatter: one 16-byte store per kept point), M = 0: the scan launch alone.  No atomics, no workgroup waits on another, no host
 *   read, no allocation, bitwise reproducible.  workspace: cobevt_prepare_points_scratch(dims) ints, 8-byte aligned, contents
 *   irrelevant on entry; points and out 16-byte aligned.  Measured: 38.8 us per eager call for 5 x 65,536 points with every stage on.
 */
int cobevt_prepare_points_scratch(const long* dims, long* workspace_ints);
int cobevt_prepare_points(const float* points, const int* point_offsets, const double* transforms, const int* order, float* out,
                          int* out_offsets, void* boxes, const void* box_mask, int* workspace, const long* dims, const double* geom,
                          hipStream_t stream);
int cobevt_bev_points_scratch(const long* dims, long* workspace_ints);
int cobevt_bev_points(const float* points, const int* point_offsets, float* bev, int* workspace, const long* dims, const double* geom,
                      hipStream_t stream);
int cobevt_bev_labels(const float* gt_boxes, const float* mask, float* label_map, float* bev_corners, int* num_valid, const int* dims,
                      const double* params, hipStream_t stream);
int cobevt_bev_post(const float* const* cls, const float* const* reg, const float* matrices, const int* cav_dims, int ncav,
                    const double* params, float score_threshold, float nms_thresh, float* boxes, float* scores, int* index, int* count,
                    void* workspace, hipStream_t stream);

/*
 * The sparse 3-D voxel backbone (csrc/sparse_conv.hip; identical in every library): OpenCOOD's MeanVFE,
 * VoxelBackBone8x (spconv's SubMConv3d / SparseConv3d + BatchNorm1d + ReLU) and HeightCompression (SparseConvTensor.dense).
 * dtype: 0 = bf16 storage (bf16 MFMA, fp32 accumulation), 1 = fp32 storage (the exact fp32 MFMA, in all three libraries).  Every
 * `dims` is a host array of longs.  All of them: no host read, no allocation, no floating-point atomics, bitwise reproducible; scalar
 * arguments are validated before anything is launched (null: code 1; shape, alignment, unsupported layer: code 2).
 *
 * A LEVEL is a sparse shape (N, D, H, W), N D H W < 2^31 - 32768, with an active set.  Its index is one int32 workspace of
 * cobevt_sparse_scratch([N, D, H, W]) ints, 16-byte aligned, contents irrelevant on entry (a bit per cell, a popcount prefix per
 * 32-bit word, the scan's partials), plus caller-owned indices (capacity, 4) int32 [b, z, y, x] and num (2) int32 = [live rows,
 * dropped rows].  Rows are ordered by the cell index ((b D + z) H + y) W + x.  Active cells past the capacity are dropped from the
 * high end of that order - never written, inactive to every later lookup - and counted in num[1]; num[0] = min(active, capacity).
 * Launches are sized by capacities and read num on the device.
 *
 * cobevt_mean_vfe: voxel_features (P, T, C) fp32, voxel_num_points (P) int32, voxel_coords (P, 4) int32 or null -> out (P, Cpad) in
 *   dtype: the sum of the first n = voxel_num_points point slots in slot order, divided by max(n, 1) (correctly rounded); channels
 *   C .. Cpad - 1 and rows with voxel_coords[p][0] < 0 (padding rows) are 0.  dims = [dtype, P, T, C, Cpad], C <= Cpad <= 64.  One launch.
 * cobevt_sparse_index: voxel_coords (P, 4) int32 [b, z, y, x] -> the level's index, and source (capacity) int32: source[row] = the
 *   LOWEST input row of that cell (rows >= num[0]: not meaningful).  Rows with b < 0 or a coordinate outside the shape are ignored.
 *   dims = [N, D, H, W, P, capacity].  Six launches (clear, mark, count, scan, emit, source), no memset node.
 * cobevt_sparse_downsample: the output level of SparseConv3d(kernel, stride, pad) over an input level's (in_indices, in_num):
 *   output shape floor((n + 2 pad - kernel) / stride) + 1 per axis, a cell active when any input of its receptive field is.
 *   `workspace`, indices, num are the OUTPUT level's.  dims = [N, D, H, W of the input, input capacity, output capacity, kernel z y x,
 *   stride z y x, pad z y x]; kernel 3 3 3 or 3 1 1 (pad 0 only), stride 1 1 1 / 2 2 2 / 2 1 1, pad 1 1 1 / 0 1 1 / 0 0 0.
 * cobevt_sparse_conv: out[r] = relu(bias + sum over taps k of W'[k] in[row(stride o_r - pad + k)]), r < out_num[0], for SubMConv3d
 *   (the output level IS the input level: pass its indices / num as out_indices / out_num, kernel 3, stride 1, pad 1) and SparseConv3d
 *   (out_indices / out_num from cobevt_sparse_downsample).  in (input feature rows, input row) in dtype, rows ordered as the input
 *   level's - or, with row_map (source of cobevt_sparse_index), in the caller's order: row r of the level reads in[row_map[r]].
 *   in_workspace / in_num: the INPUT level's.  weight [taps][Cout padded to 32][input row] in dtype, tap = (kz KY + ky) KX + kx, with the
 *   BatchNorm scale folded in; bias (Cout padded to 32) fp32; out (output capacity, Cout) in dtype, rows >= out_num[0] NOT written.
 *   dims = [dtype, N, D, H, W of the input, input feature rows, output capacity, input row in channels, Cout, kernel, stride, pad].
 *   Channel pairs (input row -> Cout): bf16 16 -> 16 | 32, 32 -> 32 | 64, 64 -> 64 | 128; fp32 the same and 8 -> 16 | 32 (narrower
 *   inputs are zero-padded to the 32-byte row by the caller).  One launch: 128 output rows per workgroup, the rows x taps neighbour
 *   table in LDS, one ballot per tap and 32-row tile skips absent taps.
 * cobevt_sparse_dense: rows -> out (N, H, W, C D) in dtype, channel index c D + d, zero elsewhere (NHWC of dense().view(N, C D, H, W)).
 *   dims = [dtype, N, D, H, W, capacity, C]; out 16-byte aligned.  Two launches (clear, scatter), no memset node.
 */
int cobevt_mean_vfe(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, void* out, const long* dims,
                    hipStream_t stream);
int cobevt_sparse_scratch(const long* dims, long* workspace_ints);
int cobevt_sparse_index(const int* voxel_coords, int* workspace, int* indices, int* num, int* source, const long* dims, hipStream_t stream);
int cobevt_sparse_downsample(const int* in_indices, const int* in_num, int* workspace, int* indices, int* num, const long* dims,
                             hipStream_t stream);
int cobevt_sparse_conv(const void* in, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                       const int* out_num, const void* weight, const float* bias, void* out, const long* dims, hipStream_t stream);
int cobevt_sparse_dense(const void* features, const int* indices, const int* num, void* out, const long* dims, hipStream_t stream);

/*
 * Training of the sparse backbone (csrc/sparse_conv.hip; fp32 rows only, the exact fp32 MFMA).  A layer's training forward is
 * z = conv(x) (cobevt_sparse_conv_raw), the BatchNorm statistics of z over the live rows and y = relu(z scale + shift)
 * (cobevt_sparse_bn_relu); its backward is cobevt_sparse_bn_relu_bwd (dy -> dz, dgamma, dbeta), cobevt_sparse_conv_dgrad (dz -> dx) and
 * cobevt_sparse_conv_wgrad (dz, x -> dW).  As above: every row count is the level's device word num[0], no host read, no allocation, no
 * floating-point atomics, bitwise reproducible, arguments validated before any launch (null: code 1; shape, alignment, unsupported pair,
 * scratch too small: code 2).  Reductions over rows are cut into a fixed number of row chunks (64) whose length,
 * ceil(ceil(num[0] / 64) / 32) * 32 rows, comes from num[0] on the device: the summation order does not depend on a capacity.
 * Channel pairs (input row -> Cout): 8 -> 16, 16 -> 16 | 32, 32 -> 32 | 64, 64 -> 64 | 128; kernel / stride / pad as cobevt_sparse_conv.
 *
 * cobevt_sparse_train_scratch: dims = [input row in channels, Cout, taps (27 | 3)] -> sizes[0] = floats of cobevt_sparse_conv_wgrad's
 *   `partial` (64 x taps x Cout padded to 32 x input row), sizes[1] = doubles of the `partial` of the two BatchNorm entries (64 x 2 x 128).
 * cobevt_sparse_conv_raw: cobevt_sparse_conv's arguments without bias, weight [taps][Cout padded to 32][input row] fp32 UNfolded, ->
 *   out (output capacity, Cout) = the plain sums; rows in [out_num[0], capacity) are written as 0.
 *   dims = [N, D, H, W of the input, input feature rows, output capacity, input row in channels, Cout, kernel, stride, pad].  One launch.
 * cobevt_sparse_bn_relu: z (capacity, C), C = 16 | 32 | 64 | 128 -> stat (4, C) fp32 = [mean, rstd, scale = gamma rstd,
 *   shift = beta - mean scale] over the n = num[0] live rows (biased variance; fp64 sums about the pivot z[0], per chunk, added in
 *   chunk order), and y (capacity, C) = relu(z scale + shift), 0 at and past num[0]; y null: the statistics alone.  mode 0: batch
 *   statistics; with running_mean, running_var (fp32) and num_batches_tracked (int64) given and n > 1 they are updated in place
 *   (momentum, the variance with n / (n - 1); + 1); n = 0: mean 0, variance 0, n = 1: variance 0, neither updates anything.  mode 1: the
 *   running statistics as they are.  dims = [capacity, C, mode, doubles of partial].  Two launches + one for y (mode 1: one + one).
 * cobevt_sparse_bn_relu_bwd: with g = dy [y > 0], xhat = (z - mean) rstd: dgamma = sum g xhat, dbeta = sum g (fp64, chunk order),
 *   coef (3, C) = [k = gamma rstd, A = k rstd dgamma / n, B = k dbeta / n] (mode 1 or n = 0: A = B = 0), dz = k g - (B + (z - mean) A),
 *   0 at and past num[0], where dy is never read.  dims as cobevt_sparse_bn_relu.  Three launches.
 * cobevt_sparse_conv_dgrad: dz (output capacity, Cout) by the OUTPUT level's rows (out_workspace, out_num) -> dx (input capacity, Cin) by
 *   the input level's rows (in_indices, in_num): dx[i] = sum over taps k of W[k]^T dz[row((i + pad - k) / stride)] where the division
 *   is exact, the cell lies in the output shape and its row is live; 0 without any, and 0 at and past in_num[0].
 *   weight_t [taps][Cin padded to 32][Cout] fp32.  dims = [N, D, H, W of the INPUT level, input capacity, output capacity, Cin, Cout,
 *   kernel, stride, pad], Cin = 16 | 32 | 64.  One launch (cobevt_sparse_conv's kernel with the transposed neighbour rule).
 * cobevt_sparse_conv_wgrad: x as cobevt_sparse_conv_raw's `in` (row_map honoured), dz (output capacity, Cout) ->
 *   dw (Cout, kz, ky, kx, Cin) fp32, real channels only.  One wave per (row chunk, tap) with the rows as the MFMA's k dimension writes
 *   partial [chunk][tap][Cout padded to 32][input row]; a second launch adds the chunks in order in fp64.
 *   dims = [N, D, H, W of the input, input feature rows, output capacity, Cin, input row in channels, Cout, kernel, stride, pad, floats
 *   of partial].
 * cobevt_sparse_dense_bwd: dcanvas (N, H, W, C D) fp32 -> dfeatures (capacity, C): the cell of every live row, 0 at and past num[0].
 *   dims = [N, D, H, W, capacity, C].  One launch.
 */
int cobevt_sparse_train_scratch(const long* dims, long* sizes);
int cobevt_sparse_conv_raw(const float* in, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                           const int* out_num, const float* weight, float* out, const long* dims, hipStream_t stream);
int cobevt_sparse_bn_relu(const float* z, const int* num, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          long* num_batches_tracked, float* stat, double* partial, float* y, const long* dims, float eps, float momentum,
                          hipStream_t stream);
int cobevt_sparse_bn_relu_bwd(const float* dy, const float* y, const float* z, const int* num, const float* gamma, const float* stat,
                              double* partial, float* dgamma, float* dbeta, float* coef, float* dz, const long* dims, hipStream_t stream);
int cobevt_sparse_conv_dgrad(const float* dz, const int* out_workspace, const int* out_num, const int* in_indices, const int* in_num,
                             const float* weight_t, float* dx, const long* dims, hipStream_t stream);
int cobevt_sparse_conv_wgrad(const float* x, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                             const int* out_num, const float* dz, float* partial, float* dw, const long* dims, hipStream_t stream);
int cobevt_sparse_dense_bwd(const float* dcanvas, const int* indices, const int* num, float* dfeatures, const long* dims, hipStream_t stream);

/*
 * Multi-tensor Adam / AdamW (csrc/train_glue.hip; torch.optim.Adam / AdamW without amsgrad / maximize, fp32 contiguous tensors only).
 * The tensor lists are HOST arrays of device pointers, copied by value into the kernel arguments: no pointer table in device memory
 * and no host -> device copy, so both entry points may be captured into a HIP graph.  What changes between replays is read from
 * device memory: the step counters, lr_dev, grad_scale, found_inf.  Arguments are validated before any launch (null: code 1; count,
 * range, alignment: code 2).
 *
 * cobevt_adam_prepare: n >= 1 step counters (fp32 words) and coef, device fp32 [n][4], 16-byte aligned.  lr_dev (nullable, a device
 *   fp64 word, 8-byte aligned) replaces lr when given; grad_scale and found_inf (nullable, device fp32 words) are torch.amp.GradScaler's.
 *   found_inf != 0: no counter moves and every row is [0, 0, 0, -1] = "skip".  Otherwise step += 1 and row i =
 *   [adamw ? 1 - lr weight_decay : weight_decay, lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step), grad_scale ? 1 / grad_scale : 1],
 *   each computed in fp64 and rounded to fp32 once.  0 <= beta < 1, weight_decay >= 0, lr >= 0.  One launch per 448 tensors.
 * cobevt_multi_adam: 1 <= n <= 64 tensors of numels[i] >= 1 elements and the n rows of coef written for them.  Per element, every line
 *   one rounded fp32 operation (no contraction; division and square root correctly rounded), c = the tensor's row:
 *     g = g c[3];  adamw ? p = p c[0] : g = g + c[0] p;  m = m + (g - m) (1 - beta1);  v = beta2 v + ((1 - beta2) g) g;
 *     p = p - c[1] (m / (sqrt(v) c[2] + eps))
 *   with (1 - beta1), beta2, (1 - beta2) and eps rounded from fp64 once.  A "skip" row leaves p, m and v untouched, bit for bit; grads
 *   are never written.  One launch of sum ceil(numels[i] / 4096) workgroups (< 2^31); tensors whose four pointers are not all 16-byte
 *   aligned are served element by element.
 */
int cobevt_adam_prepare(float* const* steps, int n, float* coef, int adamw, double beta1, double beta2, double weight_decay, double lr,
                        const double* lr_dev, const float* grad_scale, const float* found_inf, hipStream_t stream);
int cobevt_multi_adam(void* const* params, const void* const* grads, void* const* exp_avgs, void* const* exp_avg_sqs, const long* numels,
                      int n, const float* coef, int adamw, double beta1, double beta2, double eps, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* COBEVT_HIP_H */
