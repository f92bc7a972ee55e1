/*
 * segmif_calib.h — confidence calibration statistics of libsegmif_hip.so (csrc/calibration_stats.hip): reliability tables, the
 * counts above confidence thresholds and the sums of NLL and Brier score of the segmentation net's softmax, over a grid of
 * temperatures, in one gather pass.  This project's addition, NOT the reference's evaluation (its test_segmentation.py scores
 * labels only).  A header of its own beside segmif_hip.h (whose conventions hold here: fp32, device-resident, NHWC rows, pitches
 * in floats, work enqueued on `stream`, 0 on success); the same library exports the symbols, segmif_amd/_lib.py binds them from
 * CALIB_SIGNATURES, and segmif_abi_version() does not count them.
 *
 * The rule, per output pixel (b, oy, ox) of label (B, OH, OW) int64:
 *   y = label.  The pixel is labelled iff 0 <= y < C on the full 64 bits; every other value (255, -1, 256, 2^40 + 3) is `ignored`,
 *   one counter, and nothing else is done with the pixel.
 *   v_c, c < C = the bilinear interpolation (align_corners = False) of x (B, IH, IW, C) NHWC, pitch ldx >= C, 1 <= C <= 32, with
 *   segmif_pseudo_label_f32's expressions: sy = (float)IH / (float)OH, fy = max(sy (oy + 0.5) - 0.5, 0),
 *   y0 = min((int)fy, IH - 1) (the clamp, which this kernel adds, never binds for oy < OH up to rounding: it keeps every read in bounds),
 *   y1 = min(y0 + 1, IH - 1), ly = fy - y0, hy = 1 - ly (x alike), v = hy (hx p00 + lx p01) + ly (hx p10 + lx p11).
 *   If any v_c of a labelled pixel is not finite the pixel counts as `nonfinite` and nothing else; otherwise it is `valid`.
 *   pred = argmax_c v_c, ties to the lowest index; it does not depend on the temperature.  correct = (pred == y).
 *   For each temperature T_t, with r = 1 / T_t formed once in float32 (on the host):
 *     e_c = exp((v_c - v_pred) r), the maximum's own term exactly 1;  s = sum_c e_c in ascending c;  conf = 1 / s;
 *     nll = log(s) - (v_y - v_pred) r;   brier = sum_c (e_c / s - [c == y])^2, e_c / s formed as e_c conf.
 *   bin = the number of interior edges with conf >= edge (a float32 compare), 0 <= bin < M = NE + 1.
 *
 * Outputs; the call does NOT zero them, it adds to them (a data set is summed in place):
 *   counts (NT, M, 3) int64   {n, correct, conf_q} per temperature and bin, conf_q = sum of conf * 2^32.  conf >= 1 / 32 up to
 *                             rounding and conf * 2^32 is an exact integer for every float32 conf >= 2^-9, so conf_q is an exact
 *                             integer sum that does not depend on the order of the pixels.
 *   above  (NT, NK, 2) int64  {n, correct} of the valid pixels with conf > tau_k (strict, as segmif_pseudo_label_f32's compare).
 *   totals (3) int64          {valid, ignored, nonfinite}; their sum grows by B OH OW per call.
 *   sums   (NT, 2) float64    the sums of nll and of brier over the valid pixels (each pixel's value a float32).
 *   conf_or_null (NT, B, OH, OW) float32 and pred_or_null (B, OH, OW) int32, both optional and overwritten: the kernel's own conf
 *   and pred; NaN and -1 at ignored and non-finite pixels.
 *
 *   segmif_calibration_workspace_bytes  bytes of `workspace` (8-byte aligned): one double per block, temperature and sum;
 *                                       0 for anything refused below.  blocks = ceil(OW / SEGMIF_CALIB_BLOCK_COLUMNS) x
 *                                       ceil(OH / SEGMIF_CALIB_BLOCK_ROWS) x B.
 *   segmif_calibration_stats_f32        two launches.  The gather kernel, grid (column blocks, row blocks, B): one thread per
 *                                       pixel interpolates its v_c once into registers (instantiations C <= 12 and C <= 32, no
 *                                       scratch) and walks the temperatures; a wave combines its lanes' contributions per bin
 *                                       (ballots, a fixed shuffle tree), the block sums them in LDS with integer atomics and
 *                                       sends one 64-bit integer atomic per non-zero counter to the tables; nll and brier are
 *                                       summed per wave in a fixed shuffle tree, per block in wave order -> the workspace.  The
 *                                       final kernel sums the blocks' partials in a fixed order and adds the call's total to the
 *                                       running value of `sums` with one add.
 *
 * Integer atomics only, no floating-point atomics, no host synchronisation, launch counts that follow from the shapes alone,
 * every floating-point sum in a fixed order: bit-identical from run to run.  64-bit offsets throughout.
 *
 * SEGMIF_EINVAL (-22) before any launch: a NULL desc, x, label, counts, totals, sums or workspace; a NULL above with NK > 0;
 * C outside 1..32; ldx < C; NT outside 1..16, NE outside 0..31, NK outside 0..8; a temperature that is not finite or <= 0; edges
 * that are not strictly ascending or not inside the open interval (0, 1) (NaN included); a threshold outside [0, 1] (NaN
 * included); B, IH, IW, OH or OW below 1; B or OH above SEGMIF_CALIB_MAX_GRID (the grid's dimensions).
 */
#ifndef SEGMIF_CALIB_H
#define SEGMIF_CALIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGMIF_CALIB_MAX_TEMPERATURES 16
#define SEGMIF_CALIB_MAX_EDGES 31
#define SEGMIF_CALIB_MAX_THRESHOLDS 8
#define SEGMIF_CALIB_BLOCK_COLUMNS 256 /* output columns of a block */
#define SEGMIF_CALIB_BLOCK_ROWS 4      /* output rows of a block */
#define SEGMIF_CALIB_MAX_GRID 65535    /* B and OH */

typedef struct {
  int32_t n_temperatures; /* NT, 1..16 */
  int32_t n_edges;        /* NE, 0..31; M = NE + 1 bins */
  int32_t n_thresholds;   /* NK, 0..8 */
  int32_t reserved0;
  float temperatures[SEGMIF_CALIB_MAX_TEMPERATURES];
  float edges[SEGMIF_CALIB_MAX_EDGES + 1]; /* the first NE are read */
  float thresholds[SEGMIF_CALIB_MAX_THRESHOLDS];
  int32_t reserved[4];
} SegmifCalib;

int64_t segmif_calibration_workspace_bytes(int B, int OH, int OW, int NT);
int segmif_calibration_stats_f32(const SegmifCalib* desc, const float* x, const int64_t* label, int64_t* counts, int64_t* above,
                                 int64_t* totals, double* sums, void* workspace, float* conf_or_null, int32_t* pred_or_null, int B,
                                 int IH, int IW, int OH, int OW, int C, int ldx, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGMIF_CALIB_H */
