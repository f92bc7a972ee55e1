/*
 * segmif_distill.h — the distillation objectives of libsegmif_hip.so (csrc/distill_objective.hip): a frozen large teacher
 * supervises a small student on the nets' quarter-resolution logits.  This project's addition, NOT the reference's training: its
 * train.py trains one net on labels alone.  A header of its own beside segmif_hip.h (whose conventions hold here: fp32,
 * device-resident, NHWC rows, pitches in floats, work enqueued on `stream`, 0 on success); the same library exports the symbols,
 * segmif_amd/_lib.py binds them from DISTILL_SIGNATURES, and segmif_abi_version() does not count them.
 *
 * Inputs: student logits s and teacher logits t, both rows x C float32 at the same resolution (no bilinear step), pitches
 * lds, ldt >= C, 1 <= C <= 32.  rows = B * P, P = rows_per_sample >= 1 the positions of one sample; row i belongs to sample i / P.
 * Temperature T, finite and > 0.  z = x / T, lse the log-sum-exp over the stated axis, log softmax = z - lse.
 *
 *   SEGMIF_DISTILL_PIXEL    per-pixel KD (Hinton et al. 2015), softmax over the C classes of a row i:
 *                             k_i = sum_c p_ic ((zt_ic - lse_t,i) - (zs_ic - lse_s,i)),  p = softmax(zt_i)
 *                             loss = T^2 sum_i k_i / rows            dloss/ds_ic = (T / rows) (q_ic - p_ic),  q = softmax(zs_i)
 *   SEGMIF_DISTILL_CHANNEL  channel-wise distillation on the logit maps (CWD, Shu et al., ICCV 2021), per sample b and class c a
 *                           softmax over that sample's P positions j:
 *                             k_bc = sum_j p_bcj ((zt - lse_t,bc) - (zs - lse_s,bc))
 *                             loss = T^2 sum_{b,c} k_bc / (B C)      dloss/ds_bjc = (T / (B C)) (q_bcj - p_bcj)
 *
 * The teacher is data: it gets no gradient.  Every maximum is subtracted before exp; a probability is exp(z - max) / sum.  The KL
 * term is formed from z - lse = (z - max) - log sum, never from log(p): a teacher probability that underflows to 0 contributes 0,
 * not NaN.  NaN or inf in either input propagates as it does through a softmax written with torch operators; nothing is
 * special-cased.
 *
 *   segmif_distill_workspace_bytes    bytes of `workspace` (8-byte aligned is enough); 0 for anything refused below.
 *   segmif_distill_objective_f32      record4 = {loss, the gradient scale T / rows (pixel) or T / (B C) (channel), T, the mean
 *                                     before the T^2 factor = loss / T^2} (device floats).
 *                                     Pixel: one launch over blocks of SEGMIF_DISTILL_BLOCK_ROWS rows (the block's teacher rows,
 *                                     then its student rows, go through LDS; a thread keeps its row's two softmaxes in registers)
 *                                     that writes one double per block, then one block that sums them in a fixed order.
 *                                     Channel: a statistics launch on a grid (blocks per sample, B) - blocks per sample =
 *                                     min(ceil(P / SEGMIF_DISTILL_BLOCK_ROWS), SEGMIF_DISTILL_MAX_BLOCKS_PER_SAMPLE), fixed by the
 *                                     shapes alone; block j of a sample takes its tiles j, j + blocks, ... - that leaves
 *                                     (max, sum exp) per block, class and tensor; one small block per sample that combines those
 *                                     in block order into {max, sum, log sum} per (b, c) and tensor - the table at the head of
 *                                     the workspace, B x 6 x 32 floats, what the loss pass and the backward read; a loss launch on
 *                                     the statistics' grid that writes one double per block; then the same one-block sum.
 *   segmif_distill_objective_bwd_f32  one launch; recomputes from the logits (channel: with the workspace's table) and writes
 *                                     dstudent (pitch ldd >= C) = upstream[0] * record4[1] * (q - p); upstream and record4 are
 *                                     read on the device.  Hand it the workspace and the record of the forward on the same inputs.
 *
 * No host synchronisation, no floating-point atomics (no atomics at all), launch counts that do not depend on the data, every sum
 * in a fixed order: bit-identical from run to run.  In channel mode a sample's k_bc and its gradient's direction q - p depend on
 * that sample only.  16-byte accesses when a tensor's pitch equals C, its base is 16-byte aligned and (channel mode) P * C is a
 * multiple of 4, so that every sample starts aligned; scalar accesses otherwise.
 *
 * SEGMIF_EINVAL (-22) before any launch: a NULL desc, student, teacher, workspace or record4 (backward: also upstream, dstudent);
 * C outside 1..32; lds, ldt (backward: ldd) below C; T not finite or <= 0; an unknown mode; rows < 1; rows_per_sample < 1;
 * rows % rows_per_sample != 0; a batch beyond what the grid takes: in channel mode B = rows / rows_per_sample > 65535 (the grid's
 * second dimension), in pixel mode more than 2^31 - 1 blocks of rows.
 */
#ifndef SEGMIF_DISTILL_H
#define SEGMIF_DISTILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SEGMIF_DISTILL_PIXEL = 0, SEGMIF_DISTILL_CHANNEL = 1 };

#define SEGMIF_DISTILL_BLOCK_ROWS 256            /* rows of a block's tile */
#define SEGMIF_DISTILL_MAX_BLOCKS_PER_SAMPLE 64  /* channel mode: cap of the grid's first dimension */
#define SEGMIF_DISTILL_MAX_BATCH 65535           /* channel mode: the grid's second dimension */

typedef struct {
  float temperature;
  int32_t mode;
  int32_t reserved[2];
} SegmifDistill;

int64_t segmif_distill_workspace_bytes(int64_t rows, int64_t rows_per_sample, int C, int mode);
int segmif_distill_objective_f32(const SegmifDistill* desc, const float* student, const float* teacher, void* workspace,
                                 float* record4, int64_t rows, int64_t rows_per_sample, int C, int lds, int ldt, void* stream);
int segmif_distill_objective_bwd_f32(const SegmifDistill* desc, const float* student, const float* teacher, const void* workspace,
                                     const float* record4, const float* upstream, float* dstudent, int64_t rows,
                                     int64_t rows_per_sample, int C, int lds, int ldt, int ldd, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGMIF_DISTILL_H */
