/*
 * segmif_hip.h — C ABI of libsegmif_hip.so: the MI355X (gfx950) kernels behind SegMiF's
 * fusion + segmentation hot path.
 *
 * The upstream reference (JinyuanLiu-CV/SegMiF) is pure Python: it has no FFI of its own and
 * delegates all arithmetic to aten ops.  The entry points below are therefore what a binding
 * for this path binds *instead of* those aten calls; each one cites the reference call site(s)
 * it replaces (paths relative to the reference root).  segmif_amd/_lib.py is the ctypes binding;
 * INTEGRATION.md shows how the reference's core/ package is swapped for segmif_amd.core.
 *
 * Conventions
 *  - all tensors are fp32, device-resident, activation layout NHWC == tokens (B, H*W, C);
 *    a "row" is one pixel/token; leading dimensions (ld*) are in floats.
 *  - no allocation, no global state, re-entrant per stream; work is enqueued on `stream`
 *    (a hipStream_t passed as void*).  Returns 0 on success, a hipError_t / negative
 *    SEGMIF_E* code otherwise.
 *  - pointers must be 16-byte aligned where a vector path applies (documented per call).
 */
#ifndef SEGMIF_HIP_H
#define SEGMIF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGMIF_ABI_VERSION 4
#define SEGMIF_EINVAL (-22)
#define SEGMIF_ENOSYS (-38)

/* activation codes for fused epilogues */
enum { SEGMIF_ACT_NONE = 0, SEGMIF_ACT_RELU = 1, SEGMIF_ACT_PRELU = 2, SEGMIF_ACT_GELU = 3 };

int segmif_abi_version(void);
/* name of the device the library sees (debug aid); returns 0 and fills buf. */
int segmif_device_name(char* buf, int len);

/*
 * Implicit-GEMM convolution / linear on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *
 *   out[z][m][n] = epi( sum_k A(m,k) * Wt[z][n][k] + bias[n] )
 *   epi(y) = act(y)                      res == NULL
 *          = res[z][m][n] + act(y)       res != NULL
 *
 * A(m,k) is gathered on the fly (no im2col buffer):
 *   conv:  m = (b, oy, ox) over B*OH*OW, k = (ky, kx, c) tap-major / channel-minor,
 *          A = in[b][oy*stride - pad + ky*dil][ox*stride - pad + kx*dil][c]  (0 outside),
 *          `in` is NHWC with pixel pitch lda (lets a conv read the first Cin channels of a
 *          wider concat buffer) ;
 *   dense: A = in[m*lda + k]  (KH = KW = 1, stride 1, pad 0 — nn.Linear / 1x1 conv);
 *   dense, two sources (k < K1 from in, k >= K1 from in2 with pitch lda2) when in2 != NULL.
 * Wt is [N][Kp] row-major, Kp = K rounded up to 16 and zero-filled (see segmif_pack_conv_weight).
 * out pitch ldo (lets a conv write its channels in place into a concat buffer).
 * A pitch covers what a row holds: lda >= Cin (conv) or K (dense; K1 and lda2 >= K - K1 with two sources), ldo >= N,
 * ldr >= N; act is one of SEGMIF_ACT_*.  Anything else is SEGMIF_EINVAL.
 *
 * Replaces: nn.Conv2d / nn.Linear / F.conv2d call sites on the path —
 *   core/mix_transformer.py:47,51 (fc1/fc2), :96,102,112 (q/kv/proj), :100 (sr conv), :193 (patch
 *   embed); core/segformer_head.py:23,77,80; core/model_fusion.py:135-155 (DRDB convs, with the
 *   torch.cat of :137-153 folded into ldo), :351-353,:359-360 (CrossPath linears), :1051-1065
 *   (conv1/2/21/22/3/4 with the shared PReLU of :1038).
 */
typedef struct SegmifIgemm {
  const float* in;     /* activations */
  const float* in2;    /* optional second dense source (NULL otherwise) */
  const float* wt;     /* packed weights [N][Kp] */
  const float* bias;   /* [N] or NULL */
  const float* res;    /* residual [M][ldr] or NULL */
  const float* prelu;  /* device scalar slope, used when act == SEGMIF_ACT_PRELU */
  float* out;
  int64_t M;           /* rows per z-slice: B*OH*OW */
  int32_t N, K;        /* K = KH*KW*Cin (un-padded) */
  int32_t lda, lda2, K1, ldo, ldr;
  /* conv geometry (dense: KH=KW=1, stride=1, pad=0, dil=1, H=OH, W=OW, Cin=K) */
  int32_t H, W, Cin, KH, KW, stride, pad, dil, OH, OW;
  int32_t act;
  /* batching over gridDim.z (e.g. per-image weights): element strides, 0 = shared */
  int32_t nz;
  int64_t in_zstride, in2_zstride, wt_zstride, out_zstride, res_zstride;
  int32_t tile;        /* -1 = auto; otherwise index into the tile table (bench / tests) */
  /* optional second batching level: z = zb * nz2 + z2 (e.g. zb = image, z2 = attention head) */
  int32_t nz2;         /* 0 / 1 = unused */
  int32_t ldw;         /* weight row pitch in floats; 0 = Kp (packed). Lets K / V slices of a kv tensor act as weights */
  int64_t in_zstride2, wt_zstride2, out_zstride2, res_zstride2;
  /* optional split-K scratch: segmif_igemm_workspace_floats(desc) floats (0 = none needed). Without it the
   * same problem runs un-split. Partials are summed in a fixed order: results do not depend on the split. */
  float* workspace;
  int64_t workspace_floats;
  /* optional fused LayerNorm over the output row (N must be 64, act NONE): out = LN(res + A.W^T + bias)
   * — CrossPath's norm(x + end_proj(...)) (core/model_fusion.py:359-360) in the GEMM epilogue */
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  /* optional second copy of the output as "planes" chunks (see segmif_planes_* below): conv output (B, OH, OW, N) with
   * N % 16 == 0 written as chunks [planes_chunk0, planes_chunk0 + N/16) of a planes buffer of planes_chunks chunk
   * images per batch element, geometry of segmif_planes_dims(OH, OW).  Needs the 16-byte epilogue (N, ldo multiples of 4,
   * aligned out), nz <= 1 and a convolution (not a plain 1x1 / Linear problem); conv1 of Fusion_Network3_ac hands its
   * result to the first DRDB this way.
   * planes_f16 != 0: the buffer is an f16x3 one (segmif_planes16_*), max |output| is folded into planes_amax[image]
   * (planes_amax_images == B: one range slot per batch element) or into planes_amax[0] (planes_amax_images <= 1). */
  void* planes_out;
  int32_t planes_chunks, planes_chunk0;
  int32_t planes_f16;
  uint32_t* planes_amax;   /* or NULL */
  int32_t planes_amax_images;
  /* optional ReLU mask applied LAST (after the residual): out = relu_mask[m][n] > 0 ? act(A.W^T + bias) + res : 0.
   * The DRDB backward in gather form (core/model_fusion.py:134-157 differentiated): the conv that completes a block's
   * gradient writes it through that block's ReLU mask (relu_mask = the block's forward output) straight into the slot
   * the next conv reads - no separate mask pass.  Served by the split 3x3 tile (14) and by the 16-byte epilogue of the
   * implicit-GEMM tiles (N, ldo, ld_mask multiples of 4, aligned pointers, no fused LayerNorm / planes copy / second batch
   * level; a masked problem is never split along K): CrossPath's backward writes each gradient through the ReLU of the
   * channel_proj half it belongs to (core/model_fusion.py:351-353).  Anything else is SEGMIF_EINVAL. */
  const float* relu_mask;  /* [M][ld_mask] or NULL */
  int32_t ld_mask;
  /* split 3x3 tile (14) on f16x3 arithmetic (r4, the training path): wt = segmif_conv3x3_split16_pack image, activations split
   * into half pairs in the kernel after scaling by the power of two that puts max |input| in [2^13, 2^14).  split_in_amax:
   * split_in_amax_n (1..64) device words holding the IEEE bit pattern of max |x| per channel block of the input (written by
   * split_out_amax of the producing launches or by segmif_amax_f32; the kernel takes their maximum; all zero = scale 1;
   * inf / NaN = every output NaN).  split_out_amax (either arithmetic, or NULL): split_out_amax_n words (a power of two
   * <= 64; 0 = 1) receiving the atomic max of |output| bit patterns, one atomic per workgroup spread over the words by
   * workgroup index - the consumer passes all of them as (part of) its split_in_amax. */
  int32_t split_f16;
  const uint32_t* split_in_amax;
  int32_t split_in_amax_n;
  uint32_t* split_out_amax;
  int32_t split_out_amax_n;
  /* segmif_wgrad_f32 with split_f16 != 0 (3x3 stride-1 convs, the two-team kernel): the same f16x3 arithmetic for the weight
   * gradient - split_in_amax covers the input's channel blocks, wgrad_dy_amax those of dY */
  const uint32_t* wgrad_dy_amax;
  int32_t wgrad_dy_amax_n;
  int64_t mask_zstride;    /* relu_mask with nz > 1 (per-image weights): element stride between batch slices */
} SegmifIgemm;

int segmif_igemm_f32(const SegmifIgemm* desc, void* stream);
int64_t segmif_igemm_workspace_floats(const SegmifIgemm* desc);
/* number of tile configurations and a printable name for each (bench / tests) */
int segmif_igemm_num_tiles(void);
const char* segmif_igemm_tile_name(int tile);

/*
 * Repack an OIHW conv weight (Cout, Cin, KH, KW) — or a Linear weight (N, K) with KH=KW=1 — into
 * the [N][Kp] tap-major/channel-minor layout segmif_igemm_f32 consumes. dst holds N*Kp floats,
 * Kp = ((KH*KW*Cin + 15) / 16) * 16; the tail is zero-filled.
 */
int segmif_pack_conv_weight(const float* src_oihw, float* dst, int N, int Cin, int KH, int KW, void* stream);

/*
 * Split-bf16 ("bf16x6") form of a packed 3x3 weight, for tile 14 of segmif_igemm_f32: every fp32
 * weight becomes three bf16 planes (w = w0 + w1 + w2, 24 significand bits), laid out
 * [n-tile][16-channel chunk][tap][n][plane][16] so a workgroup streams one chunk's nine taps as one
 * contiguous block.  The kernel splits the activations the same way on the fly and sums the six
 * products >= 2^-16 on v_mfma_f32_32x32x16_bf16: fp32-class accuracy at 2.7x the fp32 MFMA rate
 * (DRDB convs, core/model_fusion.py:121-157).  `packed` is the segmif_pack_conv_weight image
 * (row pitch ldw floats); `out` holds segmif_conv3x3_split_weight_bytes(N, Cin) bytes.  Cin % 16 == 0.
 * With tile = 14 the descriptor's `wt` points at this image; geometry limits are those of the halo
 * tiles (3x3, stride 1, dilation 1|2, pad = dilation, N <= 256), anything else returns SEGMIF_EINVAL.
 */
int64_t segmif_conv3x3_split_weight_bytes(int N, int Cin);
int segmif_conv3x3_split_pack(const float* packed, int N, int Cin, int ldw, void* out, void* stream);
/* f16x3 form of the same image (r4): rows scaled by a power of two, planes W0 | Wl | 2^-11 W0 as halves, then one float per
 * padded output channel (the scale's inverse).  Re-packed per call on the training path (weights change every step). */
int64_t segmif_conv3x3_split16_weight_bytes(int N, int Cin);
int segmif_conv3x3_split16_pack(const float* packed, int N, int Cin, int ldw, void* out, void* stream);
/* max |x| of a rows view (rows x C floats, pitch ld; C, ld multiples of 4, 16-byte aligned) folded into slots[0 .. nslots)
 * (nslots a power of two <= 64: one atomic per block, spread over the words by block index; the maximum over the words
 * is the tensor's) as IEEE bit patterns by atomic integer max (a NaN stays on top); the caller zeroes the words first */
int segmif_amax_f32(const float* x, int64_t rows, int C, int ld, uint32_t* slots, int nslots, void* stream);

/*
 * Dense GEMM with bf16x6 arithmetic (csrc/gemm_split.hip): out = res + act(A W^T + bias), A (M, K) fp32 rows (pitch lda,
 * 16-byte aligned), K % 32 == 0, any M, N % 4 == 0; out / res rows of N floats with pitches ldo / ldr >= N (multiples of 4,
 * 16-byte aligned); act one of SEGMIF_ACT_* (PRELU needs `prelu`); anything else is SEGMIF_EINVAL.
 * `w` is the segmif_gemm_split_pack image of the (N, K) weight (row pitch ldw floats), segmif_gemm_split_weight_bytes(N, K)
 * bytes.  fp32-class accuracy (three bf16 terms per operand, six products) at 2.7x the fp32 MFMA rate: the MiT encoder's and
 * SegFormer head's nn.Linear layers
 * (core/mix_transformer.py:46-53, :94-115; core/segformer_head.py:23).
 */
typedef struct SegmifGemmSplit {
  const float* a; const void* w; const float* bias; const float* res; const float* prelu; float* out;
  int64_t M; int32_t N, K, lda, ldo, ldr, act;
  /* patch mode (patch_k > 0): a k x k convolution with stride patch_st and zero padding patch_pad as this GEMM with no gather
   * pass - Attention's spatial-reduction conv (core/mix_transformer.py:73-75, :98-101; k = stride = sr, pad 0) and the
   * overlapping patch embeds of stages 2-4 (:171-172; k 3, stride 2, pad 1).  `a` is a dense NHWC image batch
   * (B, patch_H, patch_W, C) with lda = C, C % 32 == 0; row m = (b, oy, ox) of A is the patch at (st oy - pad, st ox - pad) in
   * (ky, kx, c) order, taps outside the image read as zeros; K = k * k * C, M = B * OH * OW with OH = (H + 2 pad - k) / st + 1;
   * `w` is the image of the conv weight in the same order (segmif_pack_conv_weight's [N][Kp] rows).  0 = plain rows. */
  int32_t patch_k, patch_st, patch_pad, patch_H, patch_W;
} SegmifGemmSplit;
int64_t segmif_gemm_split_weight_bytes(int N, int K);
int segmif_gemm_split_pack(const float* w, int N, int K, int ldw, void* out, void* stream);
int segmif_gemm_split_f32(const SegmifGemmSplit* desc, void* stream);
/*
 * (r5) The f16x3 GEMM with BOTH operands pre-split (csrc/gemm_pairs.hip): out = res + act(A W^T + bias) where A arrives in
 * PAIRS format - a row of K values is K / 16 groups of 64 bytes, [16 hi halves | 16 lo halves], x = hi + 2^-11 lo - written
 * once by its producer (segmif_layernorm_pairs_f32, segmif_dwconv3x3_gelu_pairs_f32, the attention kernel's pairs output,
 * segmif_pairs_from_f32) with the same byte count as fp32, and W is the two-plane image of segmif_gemm_pairs_pack.  Both go
 * HBM -> LDS by LDS-DMA; the kernel does no vector arithmetic on its operands.  Replaces the aten addmm of nn.Linear in
 * core/mix_transformer.py:46-53 (fc1 / fc2), :94-115 (q / kv / proj) and, in patch mode, Attention's spatial-reduction conv
 * (:73-75, :98-101) for the tall problems of stages 2-4.  Range: the PRODUCER of A folds max |x| into the guard slots.
 *   lda_bytes: row pitch of A in bytes (>= 4 K, a multiple of 16); patch mode (patch_k > 0): A is a dense NHWC pairs image
 *   (B, patch_H, patch_W, patch_C), patch_C % 16 == 0, row m = (b, oy, ox) the k x k patch at (st oy - pad, st ox - pad) in
 *   (ky, kx, c) order, taps outside the image read as zeros, K = k k C;  tile_rows: 0 = chosen by size, 128 | 256 forces one,
 *   any other value is SEGMIF_EINVAL, as are ldo or ldr < N (both multiples of 4) and an act outside SEGMIF_ACT_*.
 */
typedef struct SegmifGemmPairs {
  const void* a; const void* w; const float* bias; const float* res; const float* prelu; float* out;
  int64_t M; int64_t lda_bytes;
  int32_t N, K, ldo, ldr, act;
  int32_t patch_k, patch_st, patch_pad, patch_H, patch_W, patch_C;
  int32_t tile_rows;
} SegmifGemmPairs;
int64_t segmif_gemm_pairs_weight_bytes(int N, int K);
int segmif_gemm_pairs_pack(const float* w, int N, int K, int ldw, void* out, void* stream);
int segmif_gemm_pairs_f32(const SegmifGemmPairs* desc, void* stream);
/* fp32 rows (rows x C, pitch ldx floats) <-> pairs rows (pitch in bytes); C % 16 == 0.  amax (or NULL): range slots receiving
 * max |x| (planes16 patterns), amax_images whole images of rows / amax_images rows each. */
int segmif_pairs_from_f32(const float* x, int64_t ldx, void* y, int64_t ldy_bytes, int64_t rows, int C, uint32_t* amax,
                          int amax_images, void* stream);
int segmif_pairs_to_f32(const void* x, int64_t ldx_bytes, float* y, int64_t ldy, int64_t rows, int C, void* stream);
/*
 * (r5) Backward of the spatial-reduction attention without the score matrix (csrc/attention_bwd.hip; the autograd of
 * core/mix_transformer.py:107-111 - softmax(q k^T scale) v): q, out, dout, dq are (B, N, heads * 64) rows, k / v the two
 * halves of a (B, Nk, ldkv >= 2 heads 64) tensor, dkv receives (B, Nk, 2 heads 64) = (dk | dv).  Scores are recomputed per
 * 32 x 32 tile on the exact-fp32 matrix pipe; dk / dv are formed per chunk of queries (segmif_sr_attention_bwd_chunks of them:
 * about one round of workgroups on the chip) and summed in a fixed order
 * (deterministic).  workspace: segmif_sr_attention_bwd_workspace_floats floats (row statistics + the chunk partials).
 */
int segmif_sr_attention_bwd_chunks(int B, int heads, int N, int Nk);
int64_t segmif_sr_attention_bwd_workspace_floats(int B, int heads, int N, int Nk, int C);
int segmif_sr_attention_bwd_f32(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq,
                                float* dkv, float* workspace, int B, int heads, int N, int Nk, int hd, int ldkv, float scale,
                                void* stream);

/* Producers of PAIRS rows (r5): LayerNorm (core/mix_transformer.py:152-155 norm1 / norm2, :113 the norm after the sr conv),
 * depthwise 3x3 + bias + GELU (:46-53, :376-387) and the fused attention kernel (:107-111) with their result written as half
 * pairs - 16-channel groups of [16 hi | 16 lo], the fp32 row's byte count - and max |y| folded into the f16x3 range slot of the
 * row's image (amax: amax_images words, rows / amax_images rows per image; NULL = no report).  Same arithmetic as
 * segmif_layernorm_f32 / segmif_dwconv3x3_gelu_f32 / segmif_sr_attention_split16_f32; C % 16 == 0.  The LayerNorm's waves are
 * short and numerous: it takes amax_sub (a power of two) consecutive ROWS of slots, amax_pitch words apart (>= amax_images: the
 * guard's own image count, which differs from amax_images when the launch reports to column 0 only), and spreads its
 * reports over them (a slot access serialises on its memory channel).  Pitches as segmif_layernorm_f32: ldx, ldy >= C. */
int segmif_layernorm_pairs_f32(const float* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, int ldx,
                               int ldy, float eps, uint32_t* amax, int amax_images, int amax_sub, int amax_pitch, void* stream);
int segmif_dwconv3x3_gelu_pairs_f32(const float* x, const float* w9, const float* bias, void* y, int B, int H, int W, int C,
                                    uint32_t* amax, int amax_images, void* stream);
int segmif_sr_attention_split16_pairs_f32(const float* q, const float* k, const float* v, void* out, void* workspace, int B,
                                          int heads, int N, int Nk, int hd, int ldq, int ldkv, int ldo, float scale,
                                          uint32_t* amax, uint32_t* out_amax, int amax_images, void* stream);

/* The same GEMM with f16x3 arithmetic (half pairs x three products, see segmif_planes16_* below): A is split in the kernel,
 * max |A| of the staged rows is folded into the range slots amax[0 .. amax_images) (NULL = off): the M rows are
 * amax_images whole images of M / amax_images rows, image i reports to amax[i] (amax_images = 1: one slot) - the caller
 * must re-run the images whose slot left [2^-13, 65504) on segmif_gemm_split_f32; `w` is the segmif_gemm_split16_pack
 * image (the bf16 image's layout with scaled half planes, then one float 2^-e(n) per padded output column). */
int64_t segmif_gemm_split16_weight_bytes(int N, int K);
int segmif_gemm_split16_pack(const float* w, int N, int K, int ldw, void* out, void* stream);
int segmif_gemm_split16_f32(const SegmifGemmSplit* desc, uint32_t* amax, int amax_images, void* stream);

/*
 * "Planes" activations: the bf16x6 operand split done ONCE by the producer instead of in every
 * consumer (csrc/conv3x3_planes.hip).  A planes buffer holds `chunks` 16-channel chunk images per batch
 * element, [b][chunk][Hp][Wp][plane 0..2][16] bf16 (x = p0 + p1 + p2, 24 significand bits), with
 * Hp = ceil(H/8)*8 + 4, Wp = ceil(W/32)*32 + 4 (segmif_planes_dims): a zero border of 2 pixels plus the
 * round-up to whole 8 x 32 patches, which segmif_planes_zero_border clears once per buffer (kernels only
 * ever write the H x W interior).  Position j of a chunk holds channel 16*chunk + (j&3) + 4*(j>>3) +
 * 8*((j>>2)&1) (the MFMA accumulator's hand-out order).  segmif_planes_from_f32 converts `nconv` chunks
 * (16*nconv leading channels of the fp32 rows x, pixel pitch ldx floats, 16-byte aligned) into chunks
 * [chunk0, chunk0 + nconv).  segmif_planes_pack_weight turns a segmif_pack_conv_weight image (row pitch
 * ldw floats; taps = 9 for a 3x3 conv, 1 for a 1x1 conv / Linear; N % 32 == 0, Cin % 16 == 0) into the
 * matching split weight image of segmif_planes_weight_bytes(N, Cin, taps) bytes.
 *
 * segmif_conv3x3_planes_bf16x6: 3x3 stride-1 "same" convolution (dilation 1 | 2) with 32 output channels
 * over the first `cin` channels of a planes buffer: bias + act (NONE | RELU | PRELU), written as two more
 * planes chunks (planes_out / out_chunk0; may be the input buffer, chunks >= cin/16) and / or as fp32 rows
 * (out, pitch ldo).  Six bf16 MFMA products per fp32-equivalent MAC: fp32-class accuracy.  With w1 != NULL
 * the kernel also evaluates   out1 = res + act1( W1 . [in(cin) | act(conv)(32)] + bias1 )   — a 1x1 conv with
 * 64 outputs over the input channels and the conv's own result (w1: segmif_planes_pack_weight(N = 64,
 * Cin = cin + 32, taps = 1)) — i.e. a whole DRDB tail (core/model_fusion.py:153-157: Dcov5, torch.cat,
 * conv 224 -> 64, ReLU, residual) in one launch, the concat never reaching HBM.  Pitches: ldo >= 32, ldo1 >= 64, ldr >= 64,
 * multiples of 4; act1 NONE | RELU.  Every argument is checked before the runtime is asked for anything.
 * Replaces core/model_fusion.py:135-157 in inference.
 */
typedef struct SegmifConvPlanes {
  const void* planes_in;
  void* planes_out;    /* or NULL */
  const void* wt;      /* segmif_planes_pack_weight(N = 32, Cin = cin, taps = 9) */
  const float* bias;   /* [32] or NULL, 16-byte aligned */
  const float* prelu;
  float* out;          /* optional fp32 rows [B*H*W][ldo] */
  int32_t ldo;
  int32_t B, H, W, cin, dil;
  int32_t in_chunks;   /* chunk images per batch element in planes_in */
  int32_t out_chunks, out_chunk0;
  int32_t act;
  const void* w1;      /* fused 1x1 tail (NULL = off) */
  const float* bias1;  /* [64] or NULL */
  const float* res;    /* [B*H*W][ldr] or NULL */
  float* out1;         /* [B*H*W][ldo1], 64 channels */
  int32_t ldr, ldo1, act1;
  /* f16x3 fused tail with res == NULL: != 0 takes the residual from the conv's OWN input, chunks 0..3 of planes_in
   * (x = hi + 2^-11 lo: the DRDB's input as its producer split it, 23 significand bits) - the fp32 copy of that tensor then
   * needs no writer and no reader (core/model_fusion.py:157: out = conv(cat) + x).  Ignored by the bf16x6 entry point. */
  int32_t res_from_planes;
} SegmifConvPlanes;

int segmif_planes_dims(int H, int W, int* Hp, int* Wp);
int64_t segmif_planes_bytes(int B, int H, int W, int chunks);
int segmif_planes_zero_border(void* planes, int B, int H, int W, int chunks, void* stream);
int segmif_planes_from_f32(const float* x, int ldx, void* planes, int B, int H, int W, int chunks, int chunk0, int nconv,
                           void* stream);
int64_t segmif_planes_weight_bytes(int N, int Cin, int taps);
int segmif_planes_pack_weight(const float* packed, int N, int Cin, int taps, int ldw, void* out, void* stream);
int segmif_conv3x3_planes_bf16x6(const SegmifConvPlanes* desc, void* stream);

/*
 * "f16x3" planes: the same buffers, kernels and descriptor with HALF-precision pairs instead of bf16 triples -
 * [b][chunk][Hp][Wp][plane 0..1][16] halves, x = p0 + 2^-11 p1 (p0 = RN16(x), p1 = RN16(2^11 (x - p0)): 23 significand
 * bits + rounding, one bit short of fp32) - and weight rows scaled by a power of two into the half's range and stored as
 * W0 | W - W0 | 2^-11 W0 followed by the N row factors (segmif_planes16_weight_bytes = the bf16 image + 4 N bytes).
 * THREE MFMA products per fp32-equivalent MAC instead of six and 2/3 of the activation bytes, at the error level of
 * the bf16x6 kernels (tests/test_gpu_kernels.py) - provided the activations lie in the half's exponent range: every
 * producer (segmif_planes16_from_f32, the conv's own planes / fused-tail output) folds max |x| of what it wrote into
 * a range slot (atomic max on the IEEE bit pattern of a non-negative float - NaN compares above inf; NULL = off):
 * amax[b] for batch element b when amax_images == B, amax[0] when amax_images == 1.  The caller must read the slots
 * back and re-run, on the bf16x6 entry points, the images whose value left [2^-13, 65504) (0 = an all-zero tensor is
 * fine): above, a half overflows; below, the pair keeps fewer than 23 bits.  segmif_amd.ops.run_guarded does this once
 * per pair forward, per image (ops.Planes16Guard).
 * Same geometry (segmif_planes_dims), channel order and argument rules as the bf16 entry points above.
 */
int64_t segmif_planes16_bytes(int B, int H, int W, int chunks);
int segmif_planes16_zero_border(void* planes, int B, int H, int W, int chunks, void* stream);
int segmif_planes16_from_f32(const float* x, int ldx, void* planes, int B, int H, int W, int chunks, int chunk0, int nconv,
                             uint32_t* amax, int amax_images, void* stream);
/* (r6) The fusion net's first convs, conv1_ir / conv1_vis (core/model_fusion.py:1029-1030, applied at :1051-1053 / :1055-1057 to
 * ir[:, 0:1] / vis[:, 0:1]): 3 x 3 'same' conv from ONE channel to 64 + bias + activation (SEGMIF_ACT_*; prelu = the shared scalar
 * slope) as a store-bound stencil.  x: (B, H, W) fp32, w: the raw (64, 1, 3, 3) weight, bias: 64 floats or NULL.  Outputs, at least
 * one: `planes` - an f16x3 planes buffer of `chunks` chunks per image receiving chunks [chunk0, chunk0 + 4) (half pairs, max |y|
 * folded into the range slots `amax`: amax_images = B words, one per image, or 1) - and / or `out`, (B, H, W, 64) fp32 rows with
 * pixel pitch ldo.  Replaces the scalar-gather implicit GEMM for Cin = 1. */
int segmif_conv3x3_c1_f16x3(const float* x, const float* w, const float* bias, const float* prelu, int act, void* planes,
                            int chunks, int chunk0, float* out, int ldo, int B, int H, int W, uint32_t* amax, int amax_images,
                            void* stream);
int64_t segmif_planes16_weight_bytes(int N, int Cin, int taps);
int segmif_planes16_pack_weight(const float* packed, int N, int Cin, int taps, int ldw, void* out, void* stream);
int segmif_conv3x3_planes_f16x3(const SegmifConvPlanes* desc, uint32_t* amax, int amax_images, void* stream);

/*
 * Weight gradient of the same problem: dW[n][k] = sum_m dY[m][n] * A(m,k), contraction over rows on
 * fp32 MFMA, deterministic two-pass reduction (per-chunk partials, then an fp64 sum) written in the
 * parameter's own layout: dw[n*dw_sn + k'*...] — OIHW for convs, (N, K) for linears; for dense
 * problems the output element (n, k) goes to dw[n*dw_sn + k*dw_sk] (dw_sn = K, dw_sk = 1 normally;
 * other strides let attention backward write dK / dV in place).  `desc` describes the FORWARD problem
 * (in, lda, geometry, M, N, K; nz / in_zstride / out_zstride reused as batch count, input and dW batch
 * strides).  workspace: segmif_wgrad_workspace_size(M, N, K) * max(nz,1) floats.  accumulate: dw += .
 * ldy >= N and lda >= Cin (conv) / K (dense), as in the forward; anything else is SEGMIF_EINVAL.
 * Backward of every nn.Conv2d / nn.Linear listed under segmif_igemm_f32.
 */
int64_t segmif_wgrad_workspace_size(int64_t M, int N, int K);
int segmif_wgrad_f32(const SegmifIgemm* desc, const float* dy, int ldy, int64_t dy_zstride, float* dw,
                     int64_t dw_sn, int64_t dw_sk, float* dbias /* optional [N]: sum_m dY, fused */,
                     float* workspace, int accumulate, void* stream);
/* The same for a dense problem batched over TWO levels (batch z = z1 * desc->nz2 + z2; e.g. image x attention head):
 * input / dY / dW offsets z1 * {in_zstride, dy_zstride, out_zstride} + z2 * {in_zstride2, dy_zstride2, out_zstride2}.
 * One launch forms dK^T (or dV^T) of every head of every image in the spatial-reduction attention's backward
 * (core/mix_transformer.py:107-111 under autograd).  workspace: segmif_wgrad_workspace_size(M, N, K) * nz * nz2 floats. */
int segmif_wgrad_batched2_f32(const SegmifIgemm* desc, const float* dy, int ldy, int64_t dy_zstride, int64_t dy_zstride2,
                              float* dw, int64_t dw_sn, int64_t dw_sk, float* workspace, int accumulate, void* stream);
/* column sums of a rows x N matrix (bias gradients), two-pass, fp64 accumulation.
 * workspace: segmif_colsum_blocks(rows) * N doubles, 8-byte aligned. */
int segmif_colsum_blocks(int64_t rows);
int segmif_colsum_f32(const float* x, float* out, double* workspace, int64_t rows, int N, int ldx,
                      int accumulate, void* stream);
/* dx = dy * act'(.): ref = activation OUTPUT for ReLU / PReLU (slope > 0), PRE-activation for GELU.  act is one of SEGMIF_ACT_*
 * (NONE copies), every pitch >= C; anything else is SEGMIF_EINVAL. */
int segmif_act_bwd_f32(const float* dy, const float* ref, float* dx, int64_t rows, int C, int ldy, int ldr,
                       int ldx, int act, const float* slope, void* stream);
/* the same with the activation output given as ref - ref2 (r4: a DRDB keeps x and x + relu(.) - the mask source is their
 * difference, formed in registers instead of by a full-resolution subtraction pass; core/model_fusion.py:153-157) */
int segmif_act_bwd2_f32(const float* dy, const float* ref, const float* ref2, float* dx, int64_t rows, int C, int ldy,
                        int ldr, int ldr2, int ldx, int act, const float* slope, void* stream);

/*
 * LayerNorm over the last dimension: y = (x - mean) / sqrt(var + eps) * gamma + beta,
 * biased variance, two-pass in registers.  rows x C, pitches ldx/ldy >= C (multiples of 4). C % 4 == 0, C <= 1024.
 * Replaces nn.LayerNorm at core/mix_transformer.py:101,152-153,196,320,328,336,344 and
 * core/model_fusion.py:359-360 (eps 1e-6 / 1e-5: SURVEY F6).
 */
int segmif_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y,
                         int64_t rows, int C, int ldx, int ldy, float eps, void* stream);
/* Residual form of the training path (r4; core/mix_transformer.py:171-177: x = x + drop_path(f(norm(x)))):
 *   sum = x + scale[row / rows_per_image] * branch  (scale NULL = 1: the per-sample stochastic-depth factor mask / keep)
 *   y   = LayerNorm(sum)
 * in one pass - the residual add, the DropPath multiply and the next LayerNorm were three.  Every pitch (ldx, ldb, lds, ldy)
 * is >= C and a multiple of 4. */
int segmif_add_layernorm_f32(const float* x, const float* branch, const float* scale, int64_t rows_per_image,
                             const float* gamma, const float* beta, float* sum, float* y, int64_t rows, int C, int ldx,
                             int ldb, int lds, int ldy, float eps, void* stream);

/*
 * Mix-FFN middle: depthwise 3x3 (pad 1) + bias + exact-erf GELU on tokens viewed as an
 * NHWC image (B, H, W, C); w9 is the depthwise weight repacked to [9][C].  C % 4 == 0.
 * Replaces DWConv.forward + nn.GELU: core/mix_transformer.py:48-49, :381-387.
 */
int segmif_dwconv3x3_gelu_f32(const float* x, const float* w9, const float* bias, float* y,
                              int B, int H, int W, int C, void* stream);
/* DWConv.forward called on its own (core/mix_transformer.py:381-387): depthwise 3x3 + bias, no activation. */
int segmif_dwconv3x3_bias_f32(const float* x, const float* w9, const float* bias, float* y,
                              int B, int H, int W, int C, void* stream);

/*
 * 3x3 stride-1 "same" convolution from 32 channels to ONE + bias + act (NONE | RELU | PRELU): conv22 of Fusion_Network3_ac
 * (core/model_fusion.py:1042, :1065), a bandwidth-bound stencil on the vector ALU (the matrix-pipe kernels pad the single
 * output channel to a 32-wide tile).  x: (B, H, W, >= 32) rows with pixel pitch ldx (16-byte aligned, ldx % 4 == 0);
 * wt: [9][32] tap-major = the segmif_pack_conv_weight image of the (1, 32, 3, 3) weight; y: (B, H, W) dense.
 */
int segmif_conv3x3_c32to1_f32(const float* x, int ldx, const float* wt, const float* bias, const float* prelu, int act, float* y,
                              int B, int H, int W, void* stream);

/*
 * Bilinear resize, align_corners=False, NHWC: (B, IH, IW, C) -> (B, OH, OW, C) written with
 * pixel pitch ldo at channel offset 0 of `y` (lets the SegFormer head write straight into its
 * concat buffer).  16-byte vector path when C, ldx, ldo are multiples of 4; scalar otherwise (9-class logits).
 * Replaces F.interpolate at core/mix_transformer.py:364-373, core/segformer_head.py:67-73,
 * core/model_fusion.py:1095 and test_segmentation.py:170.
 */
int segmif_bilinear_nhwc_f32(const float* x, float* y, int B, int IH, int IW, int OH, int OW, int C,
                             int ldx, int ldo, void* stream);
/* out = act(base + bias + sum of up to three bilinear resizes (align_corners=False) to OH x OW), all NHWC with C
 * channels (C % 4 == 0; the sources are dense, base / out may be pitched); act NONE or RELU; NULL base / bias /
 * x_i are skipped.  The SegFormer head with linear_fuse applied per scale before the resize
 * (segformer_head.py:67-77 commuted: a 1x1 conv commutes with a bilinear resize) ends in this kernel. */
int segmif_upsum_act_nhwc_f32(const float* base, int ldb, const float* x0, int ih0, int iw0, const float* x1, int ih1,
                              int iw1, const float* x2, int ih2, int iw2, const float* bias, float* out, int ldo, int B,
                              int OH, int OW, int C, int act, void* stream);

/*
 * Fused spatial-reduction attention: O = softmax(Q K^T * scale) V per (batch, head), never
 * materialising the N x Nk score matrix.  q: (B, N, ldq) with head h at columns [h*hd, (h+1)*hd);
 * k and v: (B, Nk, ldkv) (the kv Linear output: k = kv, v = kv + C); out: (B, N, ldo).
 * hd in {32, 64}.  QK^T and PV run on fp32 MFMA, softmax is per-lane (online, exact expf).
 * ldq, ldo >= heads * hd and ldkv >= 2 * heads * hd (multiples of 4; the split entry points below: ldkv even), else SEGMIF_EINVAL.
 * Replaces core/mix_transformer.py:107-111.
 */
int segmif_sr_attention_f32(const float* q, const float* k, const float* v, float* out,
                            int B, int heads, int N, int Nk, int hd, int ldq, int ldkv, int ldo,
                            float scale, void* stream);
/* The same function on the bf16 matrix pipe (csrc/attention_split.hip): operands split three ways into bf16, six MFMA
 * products per fp32 product (fp32-class, like segmif_conv3x3_planes_bf16x6).  hd == 64 only.  K and V are split once per
 * call into `workspace` (segmif_sr_attention_split_workspace(B, heads, Nk) bytes, 16-byte aligned, device memory),
 * which the attention workgroups then read by LDS-DMA. */
int64_t segmif_sr_attention_split_workspace(int B, int heads, int Nk);
int segmif_sr_attention_split_f32(const float* q, const float* k, const float* v, float* out, void* workspace,
                                  int B, int heads, int N, int Nk, int hd, int ldq, int ldkv, int ldo,
                                  float scale, void* stream);
/* The same with f16x3 arithmetic (half pairs x three f16 MFMA products, see segmif_planes16_*): K and V^T are packed as
 * scaled half planes with one power-of-two scale per (key tile, head, image), Q and the probabilities are split in registers.
 * amax[image] (amax_images == B) or amax[0] (1) receives max |scale log2(e) Q| (NULL = off): the caller re-runs images whose
 * slot left [2^-13, 65504) on segmif_sr_attention_split_f32.  Same workspace size. */
int segmif_sr_attention_split16_f32(const float* q, const float* k, const float* v, float* out, void* workspace, int B,
                                    int heads, int N, int Nk, int hd, int ldq, int ldkv, int ldo, float scale,
                                    uint32_t* amax, int amax_images, void* stream);

/*
 * Linear ("efficient") cross attention context, step 1: per (batch, head) partial sums of
 * K^T V over row blocks.  kv: (B, N, 2*C), C = heads*d <= 64, d <= 8: k = cols [0,C), v = [C,2C).  heads = d = 8 (C = 64: the
 * configuration Fusion_Network3_ac instantiates) has a partial-sum kernel with 16-byte loads; any other geometry - the ablation
 * networks' dim-32 modules, core/model_fusion.py:363-429, :626-661 - one with scalar loads and the same arithmetic; step 2 is
 * one kernel for all of them.
 * partial: (B, nblk, heads*d*d) DOUBLES with nblk = segmif_linattn_num_blocks(N) (fp32 inside a
 * 32-row run, fp64 across runs: the sum feeds a softmax).
 * Step 2 (segmif_linattn_fold_f32) reduces the partials in fp64, applies
 * softmax over the k-index (dim=-2) of (K^T V)*scale, and folds the block-diagonal context into
 * the following end_proj weight:  Weff[b][n][kofs + h*d + i] = sum_j ctx[b][h][i][j] * Wend[n][wofs + h*d + j].
 * Both folds need wofs, kofs >= 0, ldw >= wofs + C, ldweff >= kofs + C and `partial` 8-byte aligned (SEGMIF_EINVAL otherwise).
 * Replaces core/model_fusion.py:281-286 and :316-326 (ctx and q@ctx) together with the cat +
 * end_proj of :357-360, which becomes one dense igemm over [y3 | u_i] with per-image weights.
 */
int segmif_linattn_num_blocks(int64_t N);
int segmif_linattn_partial_f32(const float* kv, double* partial, int B, int64_t N, int heads, int d,
                               int ldkv, void* stream);
/* Fused form of (kv Linear without bias) + segmif_linattn_partial_f32: y is the (B, N, 64) input of the
 * kv projection (pitch ldy), wkv its raw (128, 64) row-major weight; kv is never written to HBM. */
int segmif_linattn_kvpartial_f32(const float* y, const float* wkv, double* partial, int B, int64_t N,
                                 int heads, int d, int ldy, void* stream);
int segmif_linattn_fold_f32(const double* partial, const float* wend, float* weff, int B, int nblk,
                            int heads, int d, int Nout, int ldw, int wofs, int ldweff, int kofs,
                            float scale, void* stream);
/* Backward of segmif_linattn_fold_f32 (training path) at any geometry the forward takes: C = heads * d <= 64, C % 16 == 0, d <= 8
 * (Fusion_Network3_ac: 8 heads of 8; the ablation networks' interaction modules: dim 32 = 8 heads of 4).  ktv (B, heads, d, d) = the
 * per-head K^T V the fold read (fp64; the sum of its partials), wend / wofs / kofs / scale as in the forward, dweff (B, Nout, ldweff)
 * the gradient of the folded weight: its columns [kofs, kofs + C) and wend's [wofs, wofs + C) are the fold's.  Writes dktv
 * (B, heads, d, d) fp64 - through the softmax over the k index - and, per image, this fold's share of d end_proj:
 * dwend_part[b][n][wofs + c] (c < C, pitch ldp floats; the caller sums over b).  fp64 where the forward is.  EINVAL for a geometry
 * outside the above, a pitch narrower than wofs + C / kofs + C, or fp64 pointers not 8-byte aligned.  Replaces the torch softmax /
 * einsum / cat of the training path's context fold (core/model_fusion.py:281-286, :316-326, :357-360 under autograd). */
int segmif_linattn_fold_bwd_f32(const double* ktv, const float* wend, int ldw, int wofs, const float* dweff, int ldweff, int kofs,
                                float scale, double* dktv, float* dwend_part, int ldp, int B, int Nout, int heads, int d,
                                void* stream);

/*
 * CrossPath in inference without its 128-wide intermediates (csrc/crosspath.hip; core/model_fusion.py:329-361).
 *  - segmif_crosspath_gram_f32: per-image Gram matrix G = sum_n y_n y_n^T of y_n = ReLU(W x_n + bias), W: 64 rows x 64
 *    (row-major, the needed half of a channel_proj weight), x: (B, N, 64) rows with pixel pitch ldx.  Written as
 *    segmif_crosspath_gram_blocks(N) partial matrices per image, 3072 doubles each (tiles (0,0), (0,1), (1,1) of the
 *    symmetric 64 x 64 matrix, 32 x 32 row-major); fp32 inside a 32-pixel run, fp64 across runs.
 *  - segmif_crosspath_fold_f32: K^T V = Wk G Wv^T per head from the Gram partials ([Wk; Wv] = the raw (128, 64) kv
 *    weight), softmax over the k index of (K^T V) * scale, folded into end_proj exactly like segmif_linattn_fold_f32.
 *    cond (or NULL): B words, one per image; the launch raises cond[b] (integer atomic max over fp32 bit patterns) to
 *    kappa = max over its 64 softmax columns of max_i |p_i (dL_i - sum_k p_k dL_k)|, dL the derivative of the logits with
 *    respect to a relative perturbation G -> G o (1 + eps S) of the Gram entries under one fixed symmetric +-1 pattern S - how
 *    far this softmax moves per unit RELATIVE error of its input.  The host's f16x3 guard reads it beside the range slots: an
 *    image whose kappa passes a calibrated bound is computed again with the 3x3 convs in exact fp32 (round 5;
 *    core/model_fusion.py:281-286, :316-326).
 *  - segmif_crosspath_tail_f32: out = LayerNorm_64(x_i + Weff_b . [ReLU(W3 x_3 + b3) | ReLU(Wi x_i + bi)] + bend):
 *    channel_proj halves, the context-folded end_proj (Weff: (B, 64, 128)), residual and norm in one pass over the
 *    tokens; optionally also emits out as planes chunks 0..3 (conv3x3_planes format, H * W == N) for the next DRDB.
 *    ln_gamma and ln_beta are required (NULL is SEGMIF_EINVAL); segmif_crosspath_fold_f32's pitches and offsets follow
 *    segmif_linattn_fold_f32's rule with C = 64.
 * Replaces core/model_fusion.py:351-360 together with :281-286 / :316-326 (the three kv Linears and K^T V).
 */
typedef struct SegmifCrossTail {
  const float* x3; const float* xi;     /* (B, N, 64) rows, pitches ld3 / ldi */
  const float* w3; const float* b3;     /* 64 x 64 rows of channel_proj3 (y half) and their bias (or NULL) */
  const float* wi; const float* bi;     /* 64 x 64 rows of channel_proj_i (u half) and their bias (or NULL) */
  const float* weff;                    /* (B, 64, 128) */
  const float* bend;                    /* end_proj bias [64] or NULL */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  float* out;                           /* may be NULL when planes_out is the only consumer (no fp32 copy is written) */
  int32_t ld3, ldi, ldo;
  int32_t B; int64_t N;
  void* planes_out; int32_t H, W, planes_chunks;   /* optional planes copy of out (NULL = off) */
  int32_t planes_f16;                               /* != 0: an f16x3 buffer (segmif_planes16_*) */
  uint32_t* planes_amax;                            /* f16x3: range slot(s) for max |out|, or NULL */
  int32_t planes_amax_images;                       /* == B: planes_amax[image]; <= 1: planes_amax[0] */
  /* (r5) x3_ih > 0: x_3 is NOT a full-resolution tensor.  x3 then points at the (B, x3_ih * x3_iw, ld3) LOW-resolution map
   * of channel_proj3's y half ALREADY APPLIED (w3 x + b3, no ReLU; w3 / b3 here are ignored), and the kernel resizes it to
   * H x W (bilinear, align_corners = False: segmif_bilinear_nhwc_f32's arithmetic) row by row as it consumes it - a resize
   * is a convex combination per channel, so it commutes with the Linear.  H, W must be set (H * W == N).  Replaces
   * F.interpolate at core/mix_transformer.py:364-373 for this consumer: the resized tensor never exists. */
  int32_t x3_ih, x3_iw;
  /* (r6) arith_f16 != 0: the kernel's own contractions on f16x3 operands (half pairs x power-of-two-scaled half planes, three MFMA
   * products per MAC instead of six bf16 ones) - for the lazy (x3_ih > 0), planes-only (out == NULL), f16x3-planes launch, inside a
   * guarded scope: arith_amax = the range slot(s) receiving max |x_i| and max |interpolated y_3| (arith_amax_images == B: one per
   * image; <= 1: arith_amax[0]). */
  int32_t arith_f16; uint32_t* arith_amax; int32_t arith_amax_images;
} SegmifCrossTail;

int segmif_crosspath_gram_blocks(int64_t N);
int segmif_crosspath_gram_f32(const float* x, int ldx, const float* w, const float* bias, double* partial, int B, int64_t N,
                              void* stream);
/* (r5) the Gram partials of relu(resize(s_low -> H x W)) for s_low = the (B, ih * iw, lds) low-resolution map of a channel_proj
 * half ALREADY APPLIED (W x + c, no ReLU): same (B, segmif_crosspath_gram_blocks(H * W), 3072) fp64 output as
 * segmif_crosspath_gram_f32 on the resized tensor (bilinear, align_corners = False), which is never formed.  Needs
 * W % 4 == 0 and an enlargement by three or more (3 iw <= W), else SEGMIF_EINVAL (the caller resizes first).  Replaces
 * F.interpolate (core/mix_transformer.py:364-373) + channel_proj3 (core/model_fusion.py:353) for cross_attn's context. */
int segmif_crosspath_gram_lazy_f32(const float* s_low, int lds, int ih, int iw, int H, int W, double* partial, int B, void* stream);
/* (r6) total (B, 3072) = the sum over an image's nblk Gram partials, in a fixed order, by 12 workgroups per image; the result is a
 * one-partial image (nblk = 1) for segmif_crosspath_fold_f32, whose single workgroup per image otherwise spends its launch pulling
 * 1.5 - 3 MB of partials through one CU. */
int segmif_crosspath_gram_sum_f64(const double* partial, int nblk, double* total, int B, void* stream);
int segmif_crosspath_fold_f32(const double* partial, int nblk, const float* wkv, const float* wend, float* weff, int B,
                              int Nout, int ldw, int wofs, int ldweff, int kofs, float scale, uint32_t* cond, void* stream);
int segmif_crosspath_tail_f32(const SegmifCrossTail* desc, void* stream);

/*
 * Pointwise helpers (bandwidth-bound, NCHW <-> NHWC at the module boundary).
 *  - segmif_seg_normalize: (x*255 - mean_c)/std_c on a (B,3,H,W) NCHW image -> NHWC (B,H,W,3)
 *    (core/model_fusion.py:1083-1085).
 *  - segmif_nchw_to_nhwc / segmif_nhwc_to_nchw: layout transposes (B, C, HW) <-> (B, HW, C).
 *  - segmif_fuse_ycrcb: fused RGB = clamp01(YCrCb2RGB([Yf, Cr(vis), Cb(vis)])) with
 *    vis NCHW RGB, yf (B,1,H,W); out NCHW (core/model_fusion.py:69-111 + test_fusion.py:102-111).
 */
int segmif_seg_normalize_f32(const float* x_nchw, float* y_nhwc, int B, int H, int W, void* stream);
int segmif_nchw_to_nhwc_f32(const float* x, float* y, int B, int C, int64_t HW, int ldo, void* stream);
int segmif_nhwc_to_nchw_f32(const float* x, float* y, int B, int C, int64_t HW, int ldx, void* stream);
int segmif_fuse_ycrcb_f32(const float* vis_nchw, const float* yf, float* out_nchw, int B, int64_t HW, void* stream);
/* (r6) two-source pointwise pass over rows views (rows x C, pitches in floats and >= C, C % 4 == 0, 16-byte aligned) - the glue of the
 * reference's ablation networks: mode 0 y = a + b (Fusion_Network3_Add, core/model_fusion.py:745-752); mode 1
 * y = silu(a) + silu(b) (Fusion_Network3_Average's att_i(x) + att_j(seg): AttentionModule ends in sigmoid(z) * z, :769-770,
 * :807-813); mode 2 y = silu(a) (AttentionModule alone; b may be NULL) */
int segmif_pointwise2_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int64_t rows, int C, int mode,
                          void* stream);
/* Backward of modes 1 and 2 of segmif_pointwise2_f32 from the saved pre-activations: mode 1 da = dy * silu'(a) and
 * db = dy * silu'(b); mode 2 da only (b, db may be NULL); silu'(z) = sigmoid(z) (1 + z (1 - sigmoid(z))).  Rows views in and out
 * (rows x C, pitches in floats, C % 4 == 0, every pointer 16-byte aligned): the gradients may land in channel slices of wider
 * buffers.  Mode 0 (a + b) has no kernel: its gradient passes through to both inputs. */
int segmif_pointwise2_bwd_f32(const float* dy, int ldy, const float* a, int lda, const float* b, int ldb, float* da, int ldda,
                              float* db, int lddb, int64_t rows, int C, int mode, void* stream);
/* RGB2YCrCb / YCrCb2RGB themselves (core/model_fusion.py:69-91, :93-111; called at train.py:355, :365) and their backward, on
 * planar (B, 3, HW) images: mode 0 RGB -> YCrCb; mode 1 YCrCb -> RGB (ysrc != NULL supplies channel 0 from a (B, 1, HW)
 * tensor: train.py:362-364's clone + slice assignment folded in); mode 2 backward of 0 (in = d/dYCrCb -> d/dRGB); mode 3
 * backward of 1 (in = d/dRGB -> d/d[Y, Cr, Cb], nout = 1: d/dY only, (B, 1, HW)).  nout = 3 otherwise. */
int segmif_color3_f32(const float* in, const float* ysrc, float* out, int B, int64_t HW, int mode, int nout, void* stream);
/* argmax over C of NHWC logits -> int32 labels (test_segmentation.py:174); ties -> lowest index */
int segmif_argmax_nhwc_i32(const float* x, int32_t* labels, int64_t rows, int C, int ldx, void* stream);
/* (r6) test_segmentation.py:169-174 in one pass: labels = argmax_c bilinear(x -> OH x OW) for NHWC logits x (B, IH, IW, C), pixel pitch
 * ldx (align_corners = False, segmif_bilinear_nhwc_f32's arithmetic; ties -> lowest index): the resized logits are never written.
 * OH and B <= 65535 (grid dimensions), as for segmif_bilinear_nhwc_f32. */
int segmif_bilinear_argmax_i32(const float* x, int32_t* labels, int B, int IH, int IW, int OH, int OW, int C, int ldx, void* stream);
/* Multi-scale + flip inference (the protocol SegFormer's tables are quoted under; the reference evaluates one view only,
 * test_segmentation.py:169-174), combined in one pass (csrc/tta.hip).  A view is the NHWC logits (B, ih, iw, C), pixel pitch
 * ldx >= C, of one forward on a resized and, with flip != 0, mirrored input. */
typedef struct { const float* x; int ih, iw, ldx, flip; } SegmifTtaView;
/* For every output pixel and every view v of the HOST table `views`, in table order: r_v = bilinear(view v -> OH x OW)
 * (align_corners = False, segmif_bilinear_nhwc_f32's arithmetic) sampled at column ox, or OW - 1 - ox when the view is mirrored
 * (= flip(interpolate(x))); p_v = softmax_c(r_v) (max-subtracted, expf); mean = (sum_v p_v) / n_views;
 * labels = argmax_c mean (ties -> lowest index).  probs_or_null, when given, receives mean as (B, OH, OW, C); nothing else of
 * that size is read or written.  One thread owns a pixel and sums in table order: no atomics, bitwise reproducible,
 * independent of B.  The table travels in the kernel arguments (no device allocation, no copy).  1 <= n_views <= 16,
 * 1 <= C <= 32, ldx >= C, OH and B <= 65535; anything else is SEGMIF_EINVAL. */
int segmif_tta_vote_f32(const SegmifTtaView* views, int n_views, int32_t* labels, float* probs_or_null, int B, int OH, int OW, int C,
                        void* stream);
/* y = flip?(interpolate(x, (OH, OW), bilinear, align_corners = False)) for `planes` = B * C contiguous (IH, IW) planes (NCHW):
 * a view's network input in one pass (resize, then torch.flip, would be two).  The same coordinate arithmetic; a mirrored
 * output column ox holds the resize's column OW - 1 - ox.  OH and planes <= 65535. */
int segmif_resize_flip_nchw_f32(const float* x, float* y, int planes, int IH, int IW, int OH, int OW, int flip, void* stream);
/* conf[t*K + p] += #{i : label[i] == t, pred[i] == p}, both inside [0, K) (K <= 32) — the accumulation of
 * test_segmentation.py:176-177 (sklearn confusion_matrix with labels=[0..K-1]: rows = ground truth,
 * columns = prediction, samples outside the label set ignored); conf is NOT cleared */
int segmif_confusion_i32(const int32_t* pred, const int64_t* label, int64_t* conf, int64_t n, int K, void* stream);
/* test_fusion.py:112-120 on device: a = uint8(255 x), min / max of a over the WHOLE batch, then
 * uint8(255.0 * ((a - min) / (max - min))) in float64, written NHWC (the reference's transpose(0,2,3,1));
 * x is (B, C, HW) fp32 already clamped to [0, 1]; minmax: 2 int32 of scratch (returns {min, max}) */
int segmif_quantize_u8(const float* x_nchw, uint8_t* out_nhwc, int32_t* minmax, int B, int C, int64_t HW, void* stream);
/* the way back, as test_segmentation.py's loader reads those PNGs (TaskFusion_dataset2.py:84-88): NHWC uint8 ->
 * NCHW fp32 = float(u) / 255 with an IEEE division (PairForward(uint8_roundtrip=True)) */
int segmif_dequantize_u8(const uint8_t* in_nhwc, float* out_nchw, int B, int C, int64_t HW, void* stream);
/* Fusion-quality statistics of fused_rgb / vis_rgb (B, H, W, 3) uint8 and ir (B, H, W) uint8, PER IMAGE, all integers:
 * f = L(fused), v = L(vis), a = ir with L(R, G, B) = (299 R + 587 G + 114 B + 500) / 1000 (integer division).
 *   joint_fa[b][f][a], joint_fv[b][f][v]   (B, 256, 256) int64 counts
 *   sums[b][0..3]   int64: sum a v; sum_{x >= 1} (f[y][x] - f[y][x-1])^2; sum_{y >= 1} (f[y][x] - f[y-1][x])^2; H W
 *   ag[b]           fp64: sum_{y < H-1, x < W-1} sqrt((dx^2 + dy^2) / 2), forward differences; the fp32 terms are summed
 *                   exactly (as integers in units of 2^-24), so the value is bitwise reproducible and batch independent
 * accumulate == 0: the call clears all four outputs itself (memset nodes when captured); != 0: it adds to them.  workspace:
 * segmif_fusion_stats_workspace_bytes(B, H, W) bytes of 8-byte aligned scratch (0 = invalid sizes).  H, W >= 2, B >= 1,
 * H W <= 2^30; nothing allocates or synchronises. */
int64_t segmif_fusion_stats_workspace_bytes(int B, int H, int W);
int segmif_fusion_stats_u8(const uint8_t* fused_rgb, const uint8_t* vis_rgb, const uint8_t* ir, int64_t* joint_fa, int64_t* joint_fv,
                           int64_t* sums, double* ag, void* workspace, int B, int H, int W, int accumulate, void* stream);
/* Local-window fusion scores of the same three planes (f = L(fused), v = L(vis), a = ir), PER IMAGE, all fp64:
 *   qabf[b][0..1]            Xydeas-Petrovic (L = 1): sum (Q_AF gA + Q_VF gV) and sum (gA + gV) over the pixels; 3 x 3 Sobel as
 *                            true convolutions with zero padding, the gS / gF comparison decided on the integers sx^2 + sy^2
 *   ssim[b][0..1]            sum over the H W pixels of the SSIM map of (f, a) and of (f, v): 11 x 11 Gaussian, sigma 1.5, zero
 *                            padding of 5, images taken as x / 255, C1 = 0.01^2, C2 = 0.03^2 (pytorch_ssim.ssim's map)
 *   vif[b][src][scale][0..1] pixel-domain VIF, sigma_nsq = 2, src 0 = a, 1 = v as the reference image and f as the distorted
 *                            one, scale 0 .. 3 with N = 17, 9, 5, 3 ("valid" Gaussians of sd = N / 5, decimation by 2):
 *                            sum log10(1 + g^2 s1 / (sv + 2)) and sum log10(1 + s1 / 2)
 * Every output is overwritten.  Sums are combined in a fixed order without floating-point atomics: bitwise reproducible and
 * batch independent.  workspace: segmif_structural_stats_workspace_bytes(B, H, W) bytes of 8-byte aligned scratch (0 = invalid
 * sizes).  H, W >= 41 (the fourth VIF scale), 1 <= B <= 65535, H W <= 2^30; a null pointer or an invalid size returns
 * SEGMIF_EINVAL before any launch; nothing allocates or synchronises, so the call can be captured in a graph. */
int64_t segmif_structural_stats_workspace_bytes(int B, int H, int W);
int segmif_structural_stats_u8(const uint8_t* fused_rgb, const uint8_t* vis_rgb, const uint8_t* ir, double* qabf, double* ssim,
                               double* vif, void* workspace, int B, int H, int W, void* stream);
/* out[i] = palette[labels[i]] for labels int32 (n), palette uint8 (K, 3), 1 <= K <= 256; a label outside 0 .. K-1 gives
 * (0, 0, 0) (util/util.py:21-29 leaves unmatched pixels zero) */
int segmif_palette_u8(const int32_t* labels, const uint8_t* palette, uint8_t* out, int64_t n, int K, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training data on the device: the loader's augmentation (datasets/voc_fusion3.py:169-216 with
 * datasets/imutils.py) over uint8 frames resident in device memory - ir, mask, label (N, h, w),
 * vis (N, h, w, 3).  The host draws the random parameters; the kernels read every geometry value
 * from one record per sample, so a batch is one upload and two launches, without a host sync.
 * ---------------------------------------------------------------------------------------------- */
#define SEGMIF_AUGMENT_MAX_SIDE 4096
/* One sample of a batch.  `tab` (the second device buffer of a batch, int32 words) holds, at the word offsets below,
 *   tab_x:  nw entries of (2 + taps_x) words: first source column, tap count n <= taps_x, n coefficients  } Pillow's bilinear
 *   tab_y:  nh entries of (2 + taps_y) words, the same for rows                                            } tables, 22 bits
 *   near_x: nw source columns, near_y: nh source rows (Pillow's nearest resize, for the label)
 * A dimension that keeps its size has the identity table (one tap of 2^22).  A pixel of a pass is
 * clip8((2^21 + sum k_i p_i) >> 22); the horizontal pass runs first and is rounded to uint8.  in / out <= 4 per axis. */
typedef struct {
  int32_t src, h, w;               /* frame index and the frames' size (must equal the h, w of the call) */
  int32_t nw, nh;                  /* scaled size (int(ratio w), int(ratio h)) */
  int32_t flip;                    /* np.fliplr after the resize */
  int32_t bright_on; float beta;   /* visible image only: uint8(clip(float32(v) + beta, 0, 255)), then */
  int32_t contrast_on; float alpha;/*                     uint8(clip(float32(v) * alpha, 0, 255)) */
  int32_t pad_h, pad_w;            /* where the image sits in the padded canvas */
  int32_t H, W;                    /* canvas: max(crop_h, nh), max(crop_w, nw) */
  int32_t cand[20];                /* ten candidate crop origins (row, column) on the canvas */
  int32_t box_h, box_w, chosen;    /* the kept origin and its index: written by segmif_augment_pick_u8 (or by the host) */
  int32_t ticket, accept_mask;     /* pick's scratch: zero on entry, zero again on exit */
  int32_t accepted;                /* written by pick: bit c set = candidate c passed the class-balance test */
  int32_t tab_x, tab_y, near_x, near_y, taps_x, taps_y;
  int32_t reserved[2];             /* zero.  segmif_augment_pick_class_u8 uses the pair as one 64-bit scratch word: zero on entry and on exit */
} SegmifAugmentRec;
int segmif_augment_record_bytes(void);
/* imutils.py:223-238 for every sample: counts the classes of each candidate window of the virtual label (nearest-resized,
 * flipped, padded with 255) and keeps the first with a non-ignore pixel and 4 max_count < 3 sum_count (= max / sum < 0.75
 * in float64 for counts below 2^18; `len(cnt > 1)` there is len(cnt)), else the tenth.  Writes box_h, box_w, chosen, accepted. */
int segmif_augment_pick_u8(const uint8_t* label, int N, int h, int w, SegmifAugmentRec* rec, const int32_t* tab, int64_t tab_words,
                           int B, int crop_h, int crop_w, void* stream);
/* The same pick with a second acceptance rule, for rare-class sampling (Hoyer et al. 2022, DAFormer; NOT the reference's
 * loader).  want (B, 2) int32 on the device: per sample a class c and a threshold t.
 *   c < 0:         segmif_augment_pick_u8's rule and exactly its record words; got[b] = -1.
 *   0 <= c <= 254: with n_k the pixels equal to c in candidate k's window of the virtual label, candidate k is accepted iff
 *                  n_k > t (strict; the 0.75 test is not applied).  chosen = the first accepted candidate, else the one with
 *                  the largest n_k, the lowest index on ties (candidate 0 when the class is in no window); accepted = the mask
 *                  of accepted candidates; got[b] = n_chosen.  With tally (n_class_tally, 2) int64 given and c < n_class_tally:
 *                  tally[c][0] += 1 (drawn), tally[c][1] += 1 if a candidate was accepted (hit).  The call does not zero tally.
 * c > 254 or t < 0 is the caller's to refuse (the values live on the device); such a sample is treated as c < 0.  rec and tally
 * must be 8-byte aligned.  A record that fails the geometry checks is left alone, its got[b] too. */
int segmif_augment_pick_class_u8(const uint8_t* label, int N, int h, int w, SegmifAugmentRec* rec, const int32_t* tab, int64_t tab_words,
                                 int B, int crop_h, int crop_w, const int32_t* want, int32_t* got, int64_t* tally, int n_class_tally,
                                 void* stream);
/* The batch itself: ir3, vis3, mask3 (B, 3, crop_h, crop_w) fp32 = value / 255 (IEEE division) and label_out (B, crop_h, crop_w)
 * int64, from box_h / box_w of the records.  Outside the image: float32(123.675 | 116.28 | 103.53) / 255 per channel in all
 * three images (random_crop2 pads the grey ones the same way) and label 255.  crop_w % 4 == 0, outputs 16-byte aligned. */
int segmif_augment_apply_u8(const uint8_t* ir, const uint8_t* vis, const uint8_t* mask, const uint8_t* label, int N, int h, int w,
                            const SegmifAugmentRec* rec, const int32_t* tab, int64_t tab_words, int B, int crop_h, int crop_w,
                            float* ir3, float* vis3, float* mask3, int64_t* label_out, void* stream);

/* Class statistics of label maps: counts (N, 257) int64, counts[n][v] = pixels of frame n equal to v for v in 0..255, column
 * 256 = values outside 0..255 (always 0 for the uint8 entry).  Frame n is the `pixels` elements at label + n * pixels.  The
 * call zeroes counts itself, on `stream`; exact integers (LDS and global integer atomics, no float arithmetic).  Any
 * pixels >= 1; the uint8 pointer may have any alignment (a slice of a larger tensor).  SEGMIF_EINVAL: a null pointer, N < 1,
 * pixels < 1, counts not 8-byte aligned. */
int segmif_label_stats_u8(const uint8_t* label, int N, int64_t pixels, int64_t* counts, void* stream);
int segmif_label_stats_i64(const int64_t* label, int N, int64_t pixels, int64_t* counts, void* stream);

/* ClassMix (Olsson et al. 2021; the mixing step of DAFormer, Hoyer et al. 2022): classes of one crop of an augmented batch
 * pasted into another.  NOT the reference's loader, which mixes nothing.  The rule:
 *
 * Inputs: an augmented batch ir3, vis3, mask3 (B, 3, h, w) fp32 and label (B, h, w) int64 (what segmif_augment_apply_u8
 * writes; w % 4 == 0), a per-sample table of int32 rows (donor, force, key[0], ..., key[n_class-1]), width 2 + n_class,
 * n_class in 1..255 and min_pixels >= 0.  For receiver b with d = donor[b]:
 *   - If d == b, the sample is not mixed.  Its output is its input, nothing is selected, and pasted[b] = 0.
 *   - n_c is the number of pixels of crop d's label equal to c, for c in 0..n_class-1.  The value 255 never counts.  Any other
 *     value outside 0..n_class-1 never counts either, whatever its low byte: negative values, 256 and 2^40 + 3 all stay out.
 *   - present = {c : n_c > min_pixels}.  The comparison is strict.
 *   - If force >= 0: selected = {force} when force is in present, else empty.
 *   - If force < 0: selected is the k = ceil(|present| / 2) classes of present with the smallest key.  The keys of a row are a
 *     permutation of 0..n_class-1, so there are no ties.  This is ClassMix's "half of the classes present, at random"; the count
 *     is (n + n % 2) / 2, as ClassMix and DAFormer's get_class_masks compute it.
 *   - M(y, x) = [label_d(y, x) in selected].  At every pixel, every channel of ir3, vis3, mask3 and the label take the donor's
 *     value where M is set and the receiver's elsewhere.  Float values are copied bit for bit: NaN payloads and -0.0 survive,
 *     no arithmetic is done.
 *   - Donors are always the UNMIXED inputs: a chain 0 <- 1 <- 2 <- 0 pastes original pixels.  The call is out of place and
 *     leaves its inputs untouched (the outputs must not overlap the inputs).
 * Outputs: four new tensors; sel (B, 8) int32, bit c & 31 of word c >> 5 set for each selected class; pasted (B,) int64, the
 * sum of n_c over the selected classes, which equals the number of set pixels of M; and, when tally (n_class, 2) int64 is
 * given, tally[c][0] += 1 per sample that selected c and tally[c][1] += n_c.  The call does not zero tally.
 *
 * segmif_class_mix_select: counts (B, 257) int64 is segmif_label_stats_i64 over the batch's label; writes sel and pasted, adds
 * to tally (null: none) through integer atomics.  segmif_class_mix_apply_f32: reads sel and writes the four outputs.  Values
 * that live on the device are not checked by the entry points: a donor outside 0..B-1 is treated as donor == b, keys are taken
 * as they are (equal keys rank by class), a force >= n_class selects nothing.  SEGMIF_EINVAL: a null pointer (tally may be
 * null), B < 1 (apply: B > 65535), n_class outside 1..255, min_pixels < 0, h < 1, w % 4, a float or label pointer not 16-byte
 * aligned, counts, sel, pasted or tally not 8-byte aligned. */
int segmif_class_mix_select(const int64_t* counts, const int32_t* table, int B, int n_class, int64_t min_pixels, int32_t* sel,
                            int64_t* pasted, int64_t* tally, void* stream);
int segmif_class_mix_apply_f32(const float* ir3, const float* vis3, const float* mask3, const int64_t* label, const int32_t* table,
                               const int32_t* sel, int B, int h, int w, int n_class, float* ir3_out, float* vis3_out,
                               float* mask3_out, int64_t* label_out, void* stream);

/* Contour scores of a segmentation: the integer tables behind Boundary IoU (Cheng et al., CVPR 2021), the trimap-band mIoU
 * (Kohli et al. 2009) and the boundary F-score (Csurka et al., BMVC 2013), in one pass over a prediction and its ground truth
 * (csrc/boundary_stats.hip).  NOT the reference's evaluation, which reports the plain mIoU only.  The rule:
 *
 * Inputs: pred (B, H, W) int32, label (B, H, W) int64, K in 1..32 classes, the band half-width d in 1..32 and the contour
 * tolerance theta in 0..31.  All distances are Chebyshev distances: every window is a square.
 *   - g(y, x) = label(y, x) when that value lies in 0..K-1, compared on the full 64 bits; otherwise IGN.  255, -1, 256 and
 *     2^40 + 3 are all IGN.
 *   - p(y, x) = pred(y, x) when g(y, x) != IGN and pred(y, x) lies in 0..K-1; otherwise IGN: the prediction is blanked wherever
 *     the ground truth is ignored.
 *   - IGN is a value like any other when two positions are compared; a position that holds it is never counted.
 *   - uniform_d(m; y, x) holds iff every (y', x') with |y' - y| <= d and |x' - x| <= d lies inside the frame and m(y', x') ==
 *     m(y, x).  A window that leaves the frame is not uniform.
 *   - band_d(m) = {(y, x) : m(y, x) != IGN and not uniform_d(m; y, x)}.  For a class c, band_d(m) intersected with {m == c} is
 *     mask_c - erode(mask_c) with a 3 x 3 structuring element of ones, d iterations and the frame padded with zeros: the
 *     mask_to_boundary of the Boundary IoU authors.
 *   - contour(m) = {(y, x) : m(y, x) != IGN and some position INSIDE the frame within distance 1 holds a different value}.
 *     Positions outside the frame are skipped: the frame's own border is not a contour.
 *   - near_theta(S) = the positions that have a member of S within distance theta inside the frame.
 * Outputs, per frame, both int64 and both zeroed by the call on `stream`:
 *   cls (B, K, 8), row c: [0] g_band = |band_d(g) & {g = c}|, [1] p_band = |band_d(p) & {p = c}|, [2] band_inter = the size
 *     of the intersection of those two sets, [3] g_contour = |GC_c| with GC_c = contour(g) & {g = c}, [4] p_contour = |PC_c|
 *     with PC_c = contour(p) & {p = c}, [5] g_matched = |GC_c & near_theta(PC_c)|, [6] p_matched = |PC_c & near_theta(GC_c)|,
 *     [7] reserved, 0.
 *   trimap (B, K, K): trimap[t][q] = #{(y, x) in band_d(g) : g = t, p = q}; rows = ground truth, as segmif_confusion_i32 has them.
 * Exact integers (LDS and global integer atomics, no floating point), so the tables are the same in every run; frame b's tables
 * depend on frame b only.  One workgroup per SEGMIF_BOUNDARY_TILE x SEGMIF_BOUNDARY_TILE tile of a frame.  Any H, W >= 1,
 * frames smaller than the window included; nothing is demanded of W.  SEGMIF_EINVAL before any launch: a null pointer, B, H or
 * W < 1, K outside 1..32, d outside 1..32, theta outside 0..31, cls or trimap not 8-byte aligned (label: 8, pred: 4), more than 2^31 - 1 tiles in the batch. */
#define SEGMIF_BOUNDARY_TILE 64
int segmif_boundary_stats_i32(const int32_t* pred, const int64_t* label, int B, int H, int W, int K, int d, int theta,
                              int64_t* cls, int64_t* trimap, void* stream);

/* Pseudo-labels for self-training (the EMA teacher of DAFormer, Hoyer et al. 2022; mean teacher, Tarvainen & Valpola 2017), in one
 * pass from the teacher's NHWC logits x (B, IH, IW, C), pixel pitch ldx >= C, to full resolution (csrc/pseudo_label.hip).  NOT the
 * reference's training, which uses labelled frames only.  The (B, OH, OW, C) resized logits are never written.  The rule, per
 * output pixel:
 *   - v_c is the bilinear resize of channel c (align_corners = False), segmif_bilinear_argmax_i32's expression: source coordinate
 *     max(0, s (dst + 0.5) - 0.5) with s = in / out, and hy (hx p00 + lx p01) + ly (hx p10 + lx p11).
 *   - label = argmax_c v_c; ties go to the lowest index.  The labels are segmif_bilinear_argmax_i32's.
 *   - p_max = 1 / sum_c exp(v_c - v_max) in float32: the softmax probability of the label.
 *   - The pixel is confident iff p_max > tau.  The comparison is strict; a NaN p_max (a NaN or infinite logit among the four
 *     source pixels) is not confident.
 *   - labels (B, OH, OW) int64: the argmax everywhere when below_ignore == 0 (DAFormer: the weight carries the confidence);
 *     when below_ignore != 0 a pixel that is not confident holds ignore_index instead (per-pixel thresholding, FixMatch style).
 *   - conf_or_null (B, OH, OW) float32 receives p_max; NULL: not written.
 *   - count (B,) int64: the confident pixels of each sample.  The call zeroes it on `stream` first.  Exact: a ballot and popcount
 *     per wave, one partial per block, one integer atomic per block; integer sums do not depend on their order, so the count is
 *     the same in every run.  count[b] / (OH OW) is DAFormer's per-image pseudo_weight.
 * No host synchronisation, no floating-point atomics: capturable in a hipGraph.  SEGMIF_EINVAL before any launch: a null pointer
 * (conf_or_null may be null), a size < 1, C outside 1..32, ldx < C, B or OH > 65535, tau NaN or outside [0, 1]. */
int segmif_pseudo_label_f32(const float* x, int64_t* labels, float* conf_or_null, int64_t* count, int B, int IH, int IW, int OH,
                            int OW, int C, int ldx, float tau, int below_ignore, int ignore_index, void* stream);

/* Strong augmentation of the student's unlabelled batch in self-training (DAFormer's strong_transform, Hoyer et al. 2022: colour
 * jitter, then a Gaussian blur; csrc/strong_augment.hip).  NOT the reference's training.  The constants a policy draws are
 * DAFormer's; the formulas are this project's and are stated here.  The rule:
 *
 * Input x (B, 3, h, w) fp32, contiguous, 16-byte aligned, w % 4 == 0, values nominally in [0, 1] (what segmif_augment_apply_u8 and
 * segmif_class_mix_apply_f32 write, mean-colour padding included).  Output y, the same shape, a new tensor (out of place; y must
 * not overlap x), and mean (B,) fp32.  One record per sample, 16 words; `reserved` is zero.
 *
 * Jitter (jitter_on != 0).  All arithmetic is float32, every product and sum rounded on its own (no fused multiply-add).
 * Channels are r, g, b; clamp is to [0, 1]; luma(v) = (0.299 r + 0.587 g) + 0.114 b, its three constants rounded to float32 (they
 * are part of the rule, as the record's factors and taps are).  Four operations in this fixed order
 * (kornia's, which DAFormer uses), with torchvision's float formulas:
 *   1. Brightness: v = clamp(fb v).
 *   2. Contrast:   v = clamp(fc v + (1 - fc) m_b).  m_b is the sum of luma(v) over the h w pixels of the brightness-adjusted
 *      sample, taken in double, divided by h w, rounded to float32.  The sum runs in one fixed order (a fixed walk per thread, a
 *      shuffle tree per wave, the waves of a block and then the sample's segmif_strong_augment_blocks(h, w) blocks in index
 *      order) and uses no float atomics: m_b is the same bits in every run and does not depend on the other samples of the
 *      batch.  mean[b] = m_b, and 0 for a sample without jitter.
 *   3. Saturation: v = clamp(fs v + (1 - fs) luma(v)).
 *   4. Hue, RGB to HSV: mx, mn the max and min of the three channels; eq = (mx == mn), cr = mx - mn; s = cr / (eq ? 1 : mx),
 *      d = eq ? 1 : cr; (rc, gc, bc) = (mx - (r, g, b)) / d; h = bc - gc where mx == r, (2 + rc) - bc where mx == g and mx != r,
 *      (4 + gc) - rc otherwise; h = frac(h / 6 + 1), then h = frac(h + fh) with frac(t) = t - floor(t); V = mx.
 *   5. Hue, HSV to RGB: i = floor(6 h) mod 6, f = 6 h - floor(6 h); p = clamp(V (1 - s)), q = clamp(V (1 - s f)),
 *      t = clamp(V (1 - s (1 - f))); (r, g, b) = (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q) for i = 0..5.  A sample with
 *      fh == 0 still goes through the conversion: one rule, no special case.
 *
 * Blur (radius in 1..8), after the jitter: every channel is filtered with the separable symmetric kernel w_k = taps[|k|],
 * |k| <= radius, first along the rows, then along the columns, each pass rounded to float32 and summed as
 * taps[0] v_0 + taps[1] (v_-1 + v_1) + ... + taps[radius] (v_-radius + v_radius), left to right.  The border is reflected without
 * repeating the edge: index -i -> i and n - 1 + i -> n - 1 - i (torch's `reflect`, scipy's `mirror`).  A record whose radius lies
 * outside 0..min(8, h - 1, w - 1) is treated as radius = 0: the kernel never indexes by an unchecked radius.
 *
 * A sample with jitter_on == 0 and an effective radius of 0 is copied bit for bit: NaN payloads and -0.0 survive.  Non-finite
 * input is not special-cased: outputs that depend on it are unspecified, nothing else is affected and nothing faults.
 *
 * segmif_strong_augment_blocks(h, w): the partial sums per sample (1..32; SEGMIF_EINVAL for sizes the call refuses).
 * segmif_strong_augment_f32: partial is a scratch of B * segmif_strong_augment_blocks(h, w) doubles.  Two launches on `stream` (the
 * mean pass, then one workgroup per SEGMIF_STRONG_TILE_H x SEGMIF_STRONG_TILE_W output tile), no host synchronisation, no atomics.
 * The factors live on the device and are not checked by the entry point.  SEGMIF_EINVAL before any launch: a null pointer, B < 1
 * or B > 65535, h < 1, w < 4, w % 4 != 0, x or y not 16-byte aligned, partial not 8-byte aligned, rec or mean not 4-byte aligned. */
#define SEGMIF_STRONG_TILE_H 32
#define SEGMIF_STRONG_TILE_W 64
typedef struct {
  int32_t jitter_on;
  float fb, fc, fs, fh;            /* brightness, contrast, saturation factors (>= 0) and the hue shift (|fh| <= 0.5) */
  int32_t radius;                  /* 0: no blur */
  float taps[9];                   /* taps[0..radius] */
  int32_t reserved;                /* zero */
} SegmifStrongAugRec;
int segmif_strong_augment_blocks(int h, int w);
int segmif_strong_augment_f32(const float* x, float* y, const SegmifStrongAugRec* rec, double* partial, float* mean, int B, int h, int w,
                              void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training path (backward of the ops above; autograd in the reference: loss.backward() at
 * train.py:226, :384).  Contractions reuse segmif_igemm_f32 (input gradients, with transposed /
 * rotated weights) and segmif_wgrad_f32; the entries below cover the rest.  Every reduction is
 * two-pass and deterministic.
 * ---------------------------------------------------------------------------------------------- */

/* LayerNorm backward: dx, plus per-block partial rows [dgamma | dbeta] (nblk x 2C floats) that the
 * caller sums with segmif_colsum_f32.  nblk = segmif_layernorm_bwd_blocks(rows, C).  Pitches (ldx, ldy, lddx; lddres / lddbr of the
 * residual form when their pointer is given) are >= C and multiples of 4. */
int segmif_layernorm_bwd_blocks(int64_t rows, int C);
int segmif_layernorm_bwd_f32(const float* x, const float* dy, const float* gamma, float* dx, float* partial,
                             int64_t rows, int C, int ldx, int ldy, int lddx, float eps, void* stream);
/* backward of segmif_add_layernorm_f32: dx = LayerNorm-backward(dy at x = the saved sum) + dres (the gradient arriving at the
 * sum itself; NULL = none), dbranch = scale[row / rows_per_image] * dx (NULL with scale NULL: the branch's gradient IS dx).
 * dx may alias dres. */
int segmif_layernorm_bwd_add_f32(const float* x, const float* dy, const float* gamma, const float* dres, int lddres,
                                 const float* scale, int64_t rows_per_image, float* dx, float* dbranch, int lddbr,
                                 float* partial, int64_t rows, int C, int ldx, int ldy, int lddx, float eps, void* stream);

/* Mix-FFN middle backward.  Part 1: z = dwconv(h)+b is recomputed, dz = dy * gelu'(z) is stored and
 * per-block partials [9 taps | bias][C] are written (segmif_dwconv_bwd_partial_rows rows x 10C floats;
 * sum with segmif_colsum_f32).  Part 2: dh = segmif_dwconv3x3_plain_f32(dz, taps flipped; C % 4 == 0, x / w9 / y 16-byte aligned).
 * C % 128 == 0. */
int64_t segmif_dwconv_bwd_partial_rows(int B, int H, int W);
int segmif_dwconv3x3_gelu_bwd_f32(const float* h, const float* w9, const float* bias, const float* dy, float* dz,
                                  float* partial, int B, int H, int W, int C, void* stream);
int segmif_dwconv3x3_plain_f32(const float* x, const float* w9, float* y, int B, int H, int W, int C, void* stream);
/* parameter-gradient partials of the bare depthwise conv (segmif_dwconv3x3_bias_f32): same [9 taps | bias][C] rows as above
 * with dz = dy; the input gradient is segmif_dwconv3x3_plain_f32(dy, taps flipped). */
int segmif_dwconv3x3_bias_bwd_f32(const float* h, const float* w9, const float* dy, float* partial, int B, int H, int W,
                                  int C, void* stream);

/* adjoint of segmif_bilinear_nhwc_f32 (gather form): dy (B,OH,OW,C) -> dx (B,IH,IW,C) */
int segmif_bilinear_nhwc_bwd_f32(const float* dy, float* dx, int B, int IH, int IW, int OH, int OW, int C,
                                 int lddy, int lddx, void* stream);

/* attention training path (scores materialised): p = softmax(s*scale) in place; ds = p*(dp - sum(p*dp))*scale in place.
 * Columns [L, ld) of every row (ld <= 1024: pitch padding a later GEMM contracts over) are set to zero by both. */
int segmif_row_softmax_f32(float* s, int64_t rows, int L, int ld, float scale, void* stream);
int segmif_row_softmax_bwd_f32(const float* p, float* dp, int64_t rows, int L, int ld, float scale, void* stream);

/* softmax cross-entropy with ignore_index over NHWC logits (train.py:156,224; model_fusion.py:1096):
 * partial[2*blk] = sum of losses, partial[2*blk+1] = valid count (doubles, segmif_softmax_ce_blocks(rows)
 * blocks); dlogits (optional) = softmax - onehot, 0 for ignored rows, NOT divided by the count. */
int segmif_softmax_ce_blocks(int64_t rows);
int segmif_softmax_ce_f32(const float* logits, const int64_t* labels, float* dlogits, double* partial,
                          int64_t rows, int C, int ld, int ldd, int ignore_index, void* stream);

/* input gradient of a strided convolution of any dilation (gather form, vector ALU); wd = weight as [tap][n][c]:
 * dx[iy][ix] sums the taps with (iy + pad - ky dil) and (ix + pad - kx dil) multiples of the stride.  The training path
 * takes it for stride > 1 with dil > 1 only (dilation 1: GEMM + segmif_col2im_f32 below). */
int segmif_conv_dgrad_strided_dil_f32(const float* dy, const float* wd, float* dx, int B, int H, int W, int Cin, int N,
                                      int KH, int KW, int stride, int pad, int dil, int OH, int OW, int lddy, int lddx,
                                      void* stream);

/* second half of the same gradient computed as GEMM + gather: cols (B, OH, OW, k*k*C) = dY . W^T with columns ordered
 * (ky, kx, c) -> dx (B, H, W, C), dx[y][x] = sum of the taps ky = (y + pad) mod stride (+ stride ..), likewise kx, read from
 * output pixel ((y + pad - ky) / stride, (x + pad - kx) / stride).  Replaces the scalar kernel above at dilation 1
 * (every strided conv of the networks: overlap patch embeds, sr convs). */
int segmif_col2im_f32(const float* cols, float* dx, int B, int H, int W, int C, int k, int stride, int pad, int OH, int OW,
                      void* stream);

/* Train-mode BatchNorm2d on NHWC rows (segformer_head.py:50-55: linear_fuse.bn with batch statistics).
 * segmif_bn_colstats_f32: mode 0 -> out[C] = sum_rows (x - mu)^2 ; mode 1 -> out[2C] = [sum dz | sum dz*xhat]
 * (fp64; partial holds ceil(rows/256) * (mode ? 2C : C) doubles).  segmif_bn_apply_f32: y = relu?(x*scale + shift).
 * segmif_bn_bwd_apply_f32: dx = scale * (dz - a - xhat * b) with a = mean dz, b = mean dz*xhat. */
int segmif_bn_colstats_f32(const float* x, const float* dz, const float* mu, const float* rstd, double* partial,
                           double* out, int64_t rows, int C, int mode, void* stream);
int segmif_bn_apply_f32(const float* x, const float* scale, const float* shift, float* y, int64_t rows, int C,
                        int relu, void* stream);
int segmif_bn_bwd_apply_f32(const float* x, const float* dz, const float* mu, const float* rstd, const float* scale,
                            const float* a, const float* b, float* dx, int64_t rows, int C, void* stream);

/* 11-tap separable Gaussian blur, zero padded, over (planes, H, W): the SSIM window of
 * pytorch_ssim/__init__.py:8-43 (five of these per SSIM evaluation; self-adjoint, so also its backward).
 * taps11 is a HOST pointer to the 11 window weights. */
int segmif_gauss_blur11_f32(const float* x, float* y, int planes, int H, int W, const float* taps11, void* stream);

/* Fusion losses of train_fusion as fused kernels (csrc/losses.hip), single-channel images of n = planes*H*W pixels:
 *  Fusionloss_grad3 (core/loss.py:506-517) = MSE + 1.1 (1 - SSIM), SSIM of pytorch_ssim/__init__.py:19-43:
 *    segmif_ssim_prep_f32   stack5 = [gen, mask, gen^2, mask^2, gen*mask]  (then segmif_gauss_blur11_f32 over 5*planes)
 *    segmif_ssim_map_f32    sums2 = {sum of the SSIM map, sum (mask - gen)^2} (partial: 2*segmif_loss_blocks(n) doubles)
 *                           and, if der3 != NULL, the planes dS/dmu1, dS/dE[gen^2], dS/dE[gen*mask] for the backward
 *    segmif_ssim_grad_f32   grad = upstream * (coef_ssim * (B0 + 2 gen B1 + mask B2) + coef_mse * (gen - mask)), B = the
 *                           blurred der3 planes (the Gaussian window is symmetric: its adjoint is the same blur)
 *  Fusionloss3 (core/loss.py:459-476, Sobelxy :634-650) = L1(mask, gen) + L1(Sobel(mask), Sobel(gen)):
 *    segmif_sobel_l1_f32    sums2 = {sum |mask - gen|, sum |S(mask) - S(gen)|}; pxy2 (optional) = the backward's two planes
 *    segmif_sobel_l1_bwd_f32  grad = upstream / n * (sign(gen - mask) + adjoint Sobel stencils of pxy2)
 * `upstream` is a device scalar (d loss / d this term). */
int segmif_loss_blocks(int64_t n);
int segmif_ssim_prep_f32(const float* gen, const float* mask, float* stack5, int64_t n, void* stream);
int segmif_ssim_map_f32(const float* blurred5, const float* gen, const float* mask, float* der3, double* partial, double* sums2,
                        int64_t n, void* stream);
int segmif_ssim_grad_f32(const float* blurred_der3, const float* gen, const float* mask, float* grad, int64_t n,
                         const float* upstream, float coef_ssim, float coef_mse, void* stream);
int segmif_sobel_l1_f32(const float* gen, const float* mask, float* pxy2, double* partial, double* sums2, int planes, int H, int W,
                        void* stream);
int segmif_sobel_l1_bwd_f32(const float* pxy2, const float* gen, const float* mask, float* grad, int planes, int H, int W,
                            const float* upstream, void* stream);

/* LapLoss2 (lap_loss.py:100-118, built by Fusionloss_grad3 at core/loss.py:509): d_k(img) = img - G_k * img for the three
 * zero-padded Gaussians G_3, G_5, G_7 (sigma 2, lap_loss.py:39-80), loss = 10 (L1_3 + L1_5) + L1_7,
 * L1_k = mean | d_k(gen) - max(d_k(ir), d_k(vis)) | over n = planes*H*W pixels.
 *   segmif_laploss2_f32      sums2[0] = sum of 10 |a_3| + 10 |a_5| + |a_7| (divide by n); sign3 (optional, [3][n]) = sign(a_k)
 *   segmif_laploss2_bwd_f32  grad = upstream / n * sum_k c_k (s_k - G_k * s_k)   (gradient w.r.t. gen only)
 * partial: 2*segmif_loss_blocks(n) doubles. */
int segmif_laploss2_f32(const float* gen, const float* ir, const float* vis, float* sign3, double* partial, double* sums2,
                        int planes, int H, int W, void* stream);
int segmif_laploss2_bwd_f32(const float* sign3, float* grad, int planes, int H, int W, const float* upstream, void* stream);

/* The other fusion objectives of core/loss.py (:386-397 new_loss_sobel, :423-457 Fusionloss / Fusionloss2, :479-505, :518-603) as one
 * table-driven kernel pair (csrc/fusion_objective.hip).  gen, ir, vis: single-channel planes (planes, H, W); mask: (planes,
 * mask_planes, H, W), mask_planes in 1..4.  Term k of a descriptor is
 *     s_k = sum over pixels of rho( w * (L(gen) - t) )
 *   op      L: identity, or Sobelxy = |gx| + |gy| (zero padding, core/loss.py:634-650)
 *   target  t = L(a_ir ir + a_vis vis + a_mask mask_0) (LINEAR), or max(L(ir), L(vis)) (MAX: the a_* are not read)
 *   weight  w = 1, mask_c or |1 - mask_c|; a weighted term sums over its first mask_channels (1..4, <= mask_planes) mask planes c,
 *           as torch's broadcast of (B, 3, H, W) * (B, 1, H, W) does.  mask_0 is the plane a_mask reads.
 *   rho     |.| or (.)^2
 * ir / vis / mask may be NULL when no term reads them.
 *   segmif_fusion_objective_f32      sums8[k] = s_k for k < n_terms (0 above); one launch, then a fixed-order sum: deterministic.
 *                                    partial: 8 * segmif_fusion_objective_blocks(planes, H, W) doubles.
 *   segmif_fusion_objective_bwd_f32  grad = sum_k coef8[k] ds_k/dgen, recomputed from the inputs (sign(0) = 0); coef8: 8 device
 *                                    floats, which the caller forms from sums8 and the upstream gradient on the device.
 * 16-byte row loads when W % 4 == 0 and the planes are 16-byte aligned, scalar ones otherwise.  A descriptor with n_terms
 * outside 1..8, an unknown enum value or mask_channels outside 1..4 (or above mask_planes) returns SEGMIF_EINVAL; nothing is
 * launched. */
#define SEGMIF_OBJ_MAX_TERMS 8
enum { SEGMIF_OBJ_IDENTITY = 0, SEGMIF_OBJ_SOBEL = 1 };
enum { SEGMIF_OBJ_TARGET_LINEAR = 0, SEGMIF_OBJ_TARGET_MAX = 1 };
enum { SEGMIF_OBJ_WEIGHT_ONE = 0, SEGMIF_OBJ_WEIGHT_MASK = 1, SEGMIF_OBJ_WEIGHT_INV_MASK = 2 };
enum { SEGMIF_OBJ_RHO_ABS = 0, SEGMIF_OBJ_RHO_SQUARE = 1 };

typedef struct {
  int32_t op, target, weight, rho;
  float a_ir, a_vis, a_mask;
  int32_t mask_channels;
} SegmifObjTerm;

typedef struct {
  int32_t n_terms;
  SegmifObjTerm term[SEGMIF_OBJ_MAX_TERMS];
} SegmifFusionObjective;

int segmif_fusion_objective_blocks(int planes, int H, int W);
int segmif_fusion_objective_f32(const SegmifFusionObjective* desc, const float* gen, const float* ir, const float* vis,
                                const float* mask, int mask_planes, double* partial, double* sums8, int planes, int H, int W,
                                void* stream);
int segmif_fusion_objective_bwd_f32(const SegmifFusionObjective* desc, const float* gen, const float* ir, const float* vis,
                                    const float* mask, int mask_planes, const float* coef8, float* grad, int planes, int H, int W,
                                    void* stream);

/* The segmentation objectives of core/loss.py (:342-383 OhemCELoss, SoftmaxFocalLoss, NormalLoss) and torch's class-weighted /
 * label-smoothed cross entropy as one kernel pair (csrc/seg_objective.hip) over NHWC logits (rows x C, pitch ld >= C, C <= 32) and
 * int64 labels.  With p = softmax(x), y the label, w = class_weight (C device floats; NULL: all 1) and q = 1 - p_y, formed as
 * sum_{c != y} e_c / sum_c e_c (the subtraction cancels as p_y -> 1), the per-pixel loss is
 *   gamma == 0   l = (1 - eps) (-w_y log p_y) + (eps / C) sum_c (-w_c log p_c)      torch's F.cross_entropy(weight, label_smoothing)
 *   gamma > 0    l = -w_y q^gamma log p_y  (eps must be 0)                           SoftmaxFocalLoss
 *                dl/dx_c = w_y (delta_cy - p_c) q^gamma (gamma p_y log(p_y) / q - 1), log(p_y) / q = log1p(-q) / q with the limit
 *                -1 at q = 0: finite for gamma < 1
 * A pixel whose label equals ignore_index or lies outside [0, C) is ignored: l = 0 and gradient 0 (segmif_softmax_ce_f32's rule).
 * Reductions:
 *   SEGMIF_SEG_MEAN_VALID  sum l / sum_valid w_y   nn.CrossEntropyLoss / nn.NLLLoss 'mean'; NaN when no pixel is valid, as torch
 *   SEGMIF_SEG_MEAN_ALL    sum l / rows            NormalLoss: torch.mean of reduction='none', ignored zeros count
 *   SEGMIF_SEG_OHEM        OhemCELoss.forward without the sort; ohem_t = -log(thresh) in float32 as the reference forms it.
 *                          n_gt = #{l > ohem_t}; n_gt >= ohem_n_min: the mean of {l > ohem_t}; otherwise the mean of the ohem_n_min
 *                          largest l over ALL rows (ignored pixels' zeros included, as the reference sorts the whole view(-1)) =
 *                          (sum_{l > kappa} l + (n_min - #{l > kappa}) kappa) / n_min, kappa the n_min-th largest l, found by an
 *                          exact radix select on the device (integer atomics only).
 * Ties at kappa: pixels with l == kappa share the n_min - #{l > kappa} remaining slots equally (a fractional weight; 1 when the
 * value is unique; of no effect at kappa = 0, where ignored pixels have gradient 0).  The VALUE is the reference's exactly; the
 * GRADIENT differs from the reference's arbitrary sort order only when two valid pixels have bit-equal losses.
 *   segmif_seg_objective_workspace_bytes  bytes of `workspace` (0: rows < 1 or an unknown reduction)
 *   segmif_seg_objective_f32      record4 = {loss, 1 / denominator, kappa (ohem_t on the threshold branch), tie weight} (device
 *                                 floats).  For OHEM the workspace keeps the per-pixel l: hand the same workspace to the backward.
 *   segmif_seg_objective_bwd_f32  dlogits (pitch ldd >= C) = upstream[0] * d loss / d logits, recomputed from the logits, already
 *                                 scaled; upstream and record4 are read on the device.  workspace may be NULL unless OHEM.
 * No host synchronisation, no floating-point atomics, fixed-order sums: bit-identical from run to run, capturable in a hipGraph;
 * every launch is issued whichever OHEM branch the data takes.  16-byte loads when ld == C and the base is 16-byte aligned,
 * scalar ones otherwise.  SEGMIF_EINVAL before any launch: C < 1 or C > 32, ld < C, gamma < 0, eps outside [0, 1), gamma > 0 with
 * eps > 0, an unknown reduction, OHEM with n_min < 1, n_min > rows or ohem_t not finite. */
enum { SEGMIF_SEG_MEAN_VALID = 0, SEGMIF_SEG_MEAN_ALL = 1, SEGMIF_SEG_OHEM = 2 };

typedef struct {
  float gamma, label_smoothing, ohem_t;
  int32_t reduction, ignore_index;
  int32_t reserved;
  int64_t ohem_n_min;
} SegmifSegObjective;

int64_t segmif_seg_objective_workspace_bytes(int64_t rows, int reduction);
int segmif_seg_objective_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels, const float* class_weight,
                             void* workspace, float* record4, int64_t rows, int C, int ld, void* stream);
int segmif_seg_objective_bwd_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                 const float* class_weight, const void* workspace, const float* record4, const float* upstream,
                                 float* dlogits, int64_t rows, int C, int ld, int ldd, void* stream);
/* The same pair with a weight per pixel and / or per sample (self-training: the confidence of a pseudo-label).  NOT the
 * reference's objective.  pixel_weight: `rows` device floats, NULL: all 1; sample_weight: rows / rows_per_sample device floats,
 * NULL: all 1; row i belongs to sample i / rows_per_sample.  With u_i = pixel_weight[i] * sample_weight[i / rows_per_sample] the
 * per-pixel loss becomes u_i l_i, l_i exactly as above (gamma, label smoothing, class weights, the ignore rule).  THE DENOMINATORS
 * DO NOT CONTAIN u: SEGMIF_SEG_MEAN_VALID divides by sum_valid w_y, SEGMIF_SEG_MEAN_ALL by rows - what mmsegmentation / DAFormer
 * compute with a pixel weight, (loss * weight).mean().  A uniform weight q therefore scales value and gradient by q; it does not
 * cancel.  The weights are data: they are read as given (any float; 0 gives the row an all-zero gradient) and receive no
 * gradient.  With both weights NULL the calls ARE the unweighted ones, and an all-ones weight gives their bits (a product with
 * 1.0f is exact).  Hand the backward the weights the forward had.  SEGMIF_EINVAL in addition to the cases above:
 * SEGMIF_SEG_OHEM with a weight; with sample_weight given, rows_per_sample < 1 or rows % rows_per_sample != 0. */
int segmif_seg_objective_weighted_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                      const float* class_weight, const float* pixel_weight, const float* sample_weight,
                                      int64_t rows_per_sample, void* workspace, float* record4, int64_t rows, int C, int ld,
                                      void* stream);
int segmif_seg_objective_weighted_bwd_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                          const float* class_weight, const float* pixel_weight, const float* sample_weight,
                                          int64_t rows_per_sample, const void* workspace, const float* record4, const float* upstream,
                                          float* dlogits, int64_t rows, int C, int ld, int ldd, void* stream);

/* The region objectives that go with them (csrc/region_objective.hip): Lovasz-Softmax (Berman et al. 2018, the batch as one set)
 * and soft Dice over the same rows (rows x C, pitch ld >= C, C <= 32, int64 labels).  Neither is the reference's.  A row is valid
 * when its label lies in [0, C) and is not ignore_index; invalid rows take no part and get gradient 0.  With p = softmax(x),
 * fg_ic = [y_i == c] and the sums over the P valid rows:
 *   SEGMIF_REGION_LOVASZ  e_ic = |fg_ic - p_ic|, for the labelled class formed as q = sum_{k != y} e_k / sum e_k.  The errors of a
 *                         class are sorted in descending order, rows with bit-equal float32 errors by ASCENDING ROW INDEX.  With
 *                         G = sum fg and F_k the foreground rows among the first k: J_k = 1 - (G - F_k) / (G + k - F_k), J_0 = 0,
 *                         g_k = J_k - J_{k-1}, loss_c = sum_k e_(k) g_k (an absent class: max_i p_ic).  The gradient takes g as
 *                         constant: d loss_c / d e_i = g_rank(i), chained through sign(p_ic - fg_ic) and the softmax.
 *   SEGMIF_REGION_DICE    I_c = sum p_ic fg_ic, S_c = sum p_ic, G_c = sum fg_ic, D_c = 1 - (2 I_c + smooth) / (S_c + G_c + smooth).
 * The result is the mean over the classes with G > 0 (SEGMIF_REGION_PRESENT) or over all C (SEGMIF_REGION_ALL); with no class to
 * average, or no valid row, it is 0 with gradient 0.
 *   segmif_region_objective_workspace_bytes  bytes of `workspace` (16-byte aligned); 0: rows < 1, C outside 1..32, rows * C beyond
 *                                    2^31 - 1 (the kernels' index type), an unknown kind.  Lovasz keeps two (key, row) pairs per
 *                                    row and class for its sort: 16 rows C bytes and a little more.
 *   segmif_region_objective_f32      record4 = {loss, 1 / n, n, P}, n the classes averaged (device floats).  Lovasz: a stable LSD
 *                                    radix sort of every class's errors (ranks from ballots and prefix sums, never from atomics:
 *                                    the tie order, and with it the gradient, is the same in every run), an integer scan of the
 *                                    sorted foreground flags, g_k in double from (k, F_k, G); the workspace keeps g per row and class.
 *   segmif_region_objective_bwd_f32  dlogits (pitch ldd >= C) = upstream[0] * d loss / d logits, the softmax recomputed, already
 *                                    scaled; workspace (the forward's), record4 and upstream are read on the device.
 * No host synchronisation, no floating-point atomics, fixed-order sums, a launch sequence that does not depend on the data:
 * bit-identical from run to run, capturable in a hipGraph.  SEGMIF_EINVAL before any launch: the size query's zero cases, ld < C,
 * ldd < C, an unknown kind or classes, smooth negative or not finite, a NULL or misaligned workspace. */
enum { SEGMIF_REGION_LOVASZ = 0, SEGMIF_REGION_DICE = 1 };
enum { SEGMIF_REGION_PRESENT = 0, SEGMIF_REGION_ALL = 1 };

typedef struct {
  int32_t kind, classes, ignore_index;
  float smooth;
  int32_t reserved[4];
} SegmifRegionObjective;

int64_t segmif_region_objective_workspace_bytes(int64_t rows, int C, int kind);
int segmif_region_objective_f32(const SegmifRegionObjective* desc, const float* logits, const int64_t* labels, void* workspace,
                                float* record4, int64_t rows, int C, int ld, void* stream);
int segmif_region_objective_bwd_f32(const SegmifRegionObjective* desc, const float* logits, const int64_t* labels,
                                    const void* workspace, const float* record4, const float* upstream, float* dlogits,
                                    int64_t rows, int C, int ld, int ldd, void* stream);

/* The fusion net's shared scalar PReLU (core/model_fusion.py:1038) on the training path, kept apart from the conv so
 * that the backward reads the branch off the pre-activation z (any slope, also <= 0): y = z > 0 ? z : a z;
 * dz = dy (z > 0 ? 1 : a), dslope[0] = sum over z <= 0 of dy z (fp64 two-pass).  16-byte path when n % 4 == 0 and the
 * pointers are aligned, scalar otherwise.  partial: 2 * (segmif_prelu_bwd_blocks(n) + 1) doubles. */
int segmif_prelu_f32(const float* z, const float* slope, float* y, int64_t n, void* stream);
int segmif_prelu_bwd_blocks(int64_t n);
int segmif_prelu_bwd_f32(const float* dy, const float* z, const float* slope, float* dz, double* partial, float* dslope,
                         int64_t n, void* stream);
/* the same with dy a rows view (rows x C, pitch lddy floats): a channel slice of a wider gradient buffer, read in place */
int segmif_prelu_bwd_rows_f32(const float* dy, int64_t lddy, const float* z, const float* slope, float* dz, double* partial,
                              float* dslope, int64_t rows, int C, void* stream);

/* multi-tensor AdamW (utils/optimizer.py:6 -> torch.optim.AdamW arithmetic). table: device array of
 * {float* p; const float* g; float* m; float* v; int64 n; float lr; float wd;} entries
 * (segmif_adamw_entry_bytes() each); chunk_entry / chunk_off map each block to (entry, offset).
 * bias_corr1 = 1 - beta1^step and bias_corr2_sqrt = sqrt(1 - beta2^step) are evaluated by the caller in double. */
int segmif_adamw_entry_bytes(void);
int segmif_adamw_f32(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks,
                     int chunk_elems, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2_sqrt,
                     void* stream);

/* The guarded step (csrc/grad_guard.hip): gradient norm, clipping and skip-on-non-finite decided on the device, over the SAME
 * table and chunk arrays as segmif_adamw_f32 (chunk_elems a multiple of 4; the chunks of an entry are neighbours, in offset order).
 * Neither the reference nor its optimizer has any of this.  Nothing allocates or synchronises; no floating-point atomics: every
 * sum has one fixed order (lanes, waves, chunks of an entry, entries of the table), so the record is bitwise reproducible.
 *   record     one SegmifGradGuardRecord on the device, zeroed once by the caller; the counters run on from call to call
 *   per_entry  nentries SegmifGradEntryStat, rewritten by every call
 *   entry_slot / param_count (both or neither): entry i of the table is parameter entry_slot[i] of a persistent per-parameter
 *              array; a skipped step adds 1 to `skipped` of every parameter in the table, a parameter whose gradient held a
 *              non-finite element adds 1 to its `offended`. */
typedef struct {
  double sumsq;               /* sum of g^2 over the FINITE elements of every gradient (squares exact in double) */
  float norm;                 /* (float)sqrt(sumsq) */
  float coef;                 /* min(1, max_norm / (norm + 1e-6)): torch.nn.utils.clip_grad_norm_; 1 for max_norm = +inf */
  uint32_t nonfinite;         /* inf / NaN elements met (not part of sumsq) */
  uint32_t skip_now;          /* nonfinite != 0 && skip_nonfinite: the guarded update and the scale leave everything untouched */
  uint32_t attempts, applied, skipped, clipped; /* running: calls; calls not skipped; skipped; applied with coef < 1 */
  uint32_t consecutive_skips; /* skipped calls since the last applied one */
  uint32_t reserved;
} SegmifGradGuardRecord;
typedef struct { double sumsq; uint32_t nonfinite, reserved; } SegmifGradEntryStat;
typedef struct { uint32_t skipped, offended; } SegmifGradParamCount;
int segmif_grad_guard_record_bytes(void);
int segmif_grad_entry_stat_bytes(void);
int segmif_grad_param_count_bytes(void);
/* bytes of `workspace` for a table of nchunks chunks (8-byte aligned; 0: nchunks < 1) */
int64_t segmif_grad_norm_workspace_bytes(int nchunks);
/* Two launches: one block per chunk (partials into the workspace), then one block that fills per_entry and the record.
 * max_norm > 0 (+inf: never clip). */
int segmif_grad_norm_f32(const void* table, int nentries, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks,
                         int chunk_elems, void* workspace, SegmifGradEntryStat* per_entry, SegmifGradGuardRecord* record,
                         const int32_t* entry_slot, SegmifGradParamCount* param_count, float max_norm, int skip_nonfinite,
                         void* stream);
/* segmif_adamw_f32's arithmetic on g * record->coef (exact for coef == 1); with record->skip_now set no block touches p, m or v.
 * chunk_entry / chunk_off / nchunks may address a sub-range of the table's chunks (one hyper-parameter group).  `step` is the
 * group's count of ATTEMPTED steps; the kernel takes t = step - param_count[slot].skipped, the applied steps, and forms
 * 1 - beta1^t and sqrt(1 - beta2^t) in double on the device. */
int segmif_adamw_guarded_f32(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks, int chunk_elems,
                             double beta1, double beta2, float eps, int step, const SegmifGradGuardRecord* record,
                             const int32_t* entry_slot, const SegmifGradParamCount* param_count, void* stream);
/* g *= record->coef in place for every gradient of the table; nothing when record->skip_now is set (or coef == 1). */
int segmif_grad_scale_f32(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks, int chunk_elems,
                          const SegmifGradGuardRecord* record, void* stream);

/* Exponential moving average of the parameters (csrc/weight_ema.hip), one launch AFTER segmif_adamw_f32 / segmif_adamw_guarded_f32 over
 * the same table and chunk arrays (a sub-range of the chunks is allowed, as for the guarded update); of an entry only p and n are
 * read, and p is the value the update before it left.  Neither the reference nor its optimizer has any of this.
 *   ema        device array of 2 * nentries pointers indexed by the table's entry: ema[2 i] = hi, ema[2 i + 1] = lo, n floats each.
 *              The average is the pair hi + lo; hi is its float32 rounding (what a model loads), lo the remainder.
 *   record     NULL, or the guard's record of this step: with record->skip_now set no block touches hi or lo.
 *   entry_slot / param_count (both or neither): t = step - param_count[entry_slot[entry]].skipped, the parameter's applied steps
 *              with this one included, floored at 1 - the count the guarded bias correction uses.  Without them t = step.
 * Per block, in double: d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay, a = 1 - d_t.  Per element, in double:
 *   e = hi + lo;  e += a * (p - e);  hi = (float)e;  lo = (float)(e - hi)
 * A float32 average updated as ema += a * (p - ema) loses increments under half an ulp - at decay 0.9999 and learning rates around
 * 1e-4 that is most of them - and stalls; the pair keeps 48 bits.  Non-finite values are not special-cased: a p that is inf or NaN
 * makes its average NaN from then on.  Element-wise only, no atomics, no reductions: bitwise reproducible.  16-byte accesses where
 * p, hi and lo of the chunk are 16-byte aligned.  decay inside (0, 1), chunk_elems a multiple of 4, step >= 1. */
int segmif_weight_ema_f32(const void* table, float* const* ema, const int32_t* chunk_entry, const int64_t* chunk_off,
                          int nchunks, int chunk_elems, double decay, int warmup, int step,
                          const SegmifGradGuardRecord* record, const int32_t* entry_slot,
                          const SegmifGradParamCount* param_count, void* stream);

/*
 * Mix-FFN of a MiT block as ONE kernel (csrc/mixffn.hip), C = 64 | 128 (stages 1-2 of mit_b1 .. b5):
 *     out = x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x)))))     core/mix_transformer.py:46-53, :376-387, :152-155
 * on (B, H*W, C) tokens; a workgroup owns a 12 x 16 pixel tile, the 4C-wide hidden tensor stays in its LDS / registers.
 * f16x3 arithmetic (half pairs x three products, see segmif_planes16_*): `wimg` is the segmif_mixffn_pack image
 * (segmif_mixffn_weight_bytes(C) bytes) of everything per hidden channel - the fc1 (4C, C) and fc2 (C, 4C) weights, fc1's bias,
 * the depthwise weight as [9][4C] (tap-major) and its bias -, one contiguous block per 32 hidden channels;
 * amax_a / amax_g: range slots of the two tensors the kernel splits (LN(x) and the GELU output), indexed by image when
 * amax_images == B (NULL = off); the caller re-runs tripped images on the bf16x6 chain (segmif_layernorm_f32,
 * segmif_gemm_split_f32, segmif_dwconv3x3_gelu_f32).  out must not alias x.
 */
typedef struct SegmifMixFfn {
  const float* x; float* out; const void* wimg;
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  const float* b2;   /* fc2 bias [C] */
  int32_t B, H, W, C;
  uint32_t* amax_a; uint32_t* amax_g; int32_t amax_images;
} SegmifMixFfn;
int64_t segmif_mixffn_weight_bytes(int C);
int segmif_mixffn_pack(const float* w1 /* (4C, C) */, const float* b1, const float* dw9 /* [9][4C] */, const float* dw_bias,
                       const float* w2 /* (C, 4C) */, int C, void* out, void* stream);
int segmif_mixffn_f16x3(const SegmifMixFfn* desc, void* stream);

/*
 * Gradient exchange of the data-parallel training steps behind the C ABI (SURVEY.md section 8(b) lists
 * segmif_comm_{init, allreduce, destroy}; section 8(e): one fp32 sum / average all-reduce per step over RCCL / xGMI; the
 * reference has no distributed code at all).  Thin entry points over RCCL for a host that is not Python - this
 * repo's Python host uses torch.distributed (backend "nccl" IS RCCL) in segmif_amd/parallel.py and does not route through
 * them.  librccl is looked up at first use (the copy the process already holds first), never at load time.
 *   segmif_comm_available   0 when RCCL could be resolved (version = ncclGetVersion), SEGMIF_ENOSYS otherwise
 *   segmif_comm_unique_id   rank 0 obtains the 128-byte rendezvous id; the host hands it to every rank by its own means
 *   segmif_comm_init        one communicator per process / GPU (binds to the caller's current HIP device)
 *   segmif_comm_allreduce_f32  recv = sum (average != 0: mean) over ranks of send, in place allowed, on `stream`
 * Return 0, SEGMIF_EINVAL / SEGMIF_ENOSYS, or 1000 + ncclResult_t.
 */
int segmif_comm_available(int* version);
int segmif_comm_unique_id(void* id, int64_t bytes /* >= 128 */);
int segmif_comm_init(void** comm, int world, int rank, const void* id, int64_t bytes);
int segmif_comm_world(void* comm, int* world, int* rank);
int segmif_comm_allreduce_f32(void* comm, const float* send, float* recv, int64_t count, int average, void* stream);
int segmif_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* SEGMIF_HIP_H */
