/*
 * segmif_objects.h — object-level statistics of libsegmif_hip.so (csrc/objects.hip): the connected components of the predicted
 * and of the ground-truth label map, and per frame, side, class and size bucket the number of components by the decile of their
 * coverage by the other map.  This project's addition, NOT the reference's evaluation (its test_segmentation.py reports the plain
 * mIoU only).  A header of its own beside segmif_hip.h (whose conventions hold here: device-resident, work enqueued on `stream`,
 * 0 on success); the same library exports the symbols, segmif_amd/_lib.py binds them from OBJECT_SIGNATURES, and
 * segmif_abi_version() does not count them.
 *
 * The rule.
 *
 * Inputs and validity.  Inputs are pred (B, H, W) int32 and label (B, H, W) int64.  K is in 1..32 and connectivity conn is 4 or 8.
 * These are boundary_stats' conventions:
 *   g = label where it lies in 0..K-1 on the full 64 bits.  Otherwise g = IGN; 255, -1, 256 and 2^40 + 3 are all IGN.
 *   p = pred where g != IGN and pred is in 0..K-1.  Otherwise p = IGN.
 *   The prediction is blanked where the ground truth is ignored.
 *   IGN pixels belong to no component and count in nothing.
 *
 * Components.  Two valid pixels of a map are joined iff they are conn-neighbours INSIDE THE FRAME and hold the same value.
 * A component's ROOT is the smallest linear index y * W + x of its pixels.  This does not depend on how it is computed, so it can be
 * compared for equality with any other labeller.  root_g and root_p are (B, H, W) int32.  They hold that index at valid pixels and
 * -1 at IGN.  Frames are independent of each other.
 *
 * Per-component sums.  Per component Q of class c:
 *   area(Q) is its pixel count.
 *   On side 0, Q is a component of g.  hit(Q) is the number of its pixels with p == c.
 *   On side 1, Q is a component of p.  hit(Q) is the number of its pixels with g == c.
 *
 * Buckets.
 *   Size bucket s is the number of size_edges (0..3 ascending int64 values) with area >= edge, so S = n_edges + 1.  The default
 *   edges are COCO's, (1024, 9216).  They give small below 32^2, medium, and large from 96^2 upward.
 *   Coverage decile j is (10 * hit) / area in integer arithmetic, so 0..10, with j = 10 iff hit == area.  So "at least k / 10 of
 *   the object is covered" is exactly j >= k.
 *
 * Outputs.  The call adds to its outputs and does not zero them, as calibration_stats does.
 *   obj  (B, 2, K, S, 11) int64: the number of components per frame, side, class, size bucket and decile.
 *   mass (B, 2, K, S, 2) int64:  {sum of area, sum of hit} over those components.
 *   status (2) int32:            {a loop reached its iteration cap, reserved}.
 * Everything is an exact integer: two runs give equal bits; frame b's tables depend on frame b only; the tables do not depend on
 * the order in which components are merged.
 *
 * Scores.  These are formed on the host in float64 from tables summed over the data set.  The sum comes first and the ratio
 * after, as with mIoU and the boundary scores.  With a coverage tau = k / 10:
 *   obj_recall[c] = #(side 0, class c, j >= k) / #(side 0, class c).
 *   obj_precision[c] is the same expression on side 1.
 *   obj_f1 = 2 P R / (P + R).  It is NaN when either denominator is empty and 0 when P + R = 0.
 *   obj_recall_by_size (K, S) and obj_precision_by_size (K, S).
 *   n_gt_objects (K, S) and n_pred_objects (K, S).
 *   mObjRecall, mObjPrecision and mObjF1 = mean(nan_to_num(.)), the convention every mean here follows.
 * This is coverage-based detection, the Pd / false-alarm convention of IR small-target work.  It is not a one-to-one IoU matching
 * as panoptic quality does: a blob that swallows three pedestrians detects all three and counts as one correct prediction.
 *
 * How it is computed (csrc/objects.hip); four launches whatever the maps hold, both sides through the same kernels (the side is
 * the low bit of the grid's z):
 *   local    one workgroup per SEGMIF_OBJECTS_TILE x SEGMIF_OBJECTS_TILE tile and map.  The map is narrowed to bytes (the 64-bit
 *            range test first); the parents are an LDS array of local indices in which a pixel starts at the first pixel of its
 *            horizontal run (a wave holds a row: one ballot joins the W neighbours), then each pixel unites with its N (conn 8: NW
 *            and NE too) neighbour of equal value inside the tile through LDS atomicMin unless a neighbour joins the same two runs,
 *            the tile is flattened, and every pixel writes the GLOBAL index of its local root to parent[] and zeroes its area /
 *            hit entries.  Raster order inside a tile is the frame's raster order restricted to it, so parent <= child holds on
 *            the frame: the invariant the min-index root needs.
 *   border   the pixels of a tile's top row and left column unite with their equal-valued neighbours in the adjacent tiles (the
 *            diagonal ones across a corner included) on the global array with the lock-free step a = find(a), b = find(b); stop
 *            if equal; order a > b; old = atomicMin(&parent[a], b); stop if old == a, else a = old and repeat.  Every read of
 *            parent[] in this kernel is an agent-scope relaxed atomic load and every write an agent-scope atomic; no thread
 *            waits for another.
 *   count    after the kernel boundary, plain loads: every pixel walks to its root and writes root_* if asked; a thread carries
 *            (root, area, hit) over SEGMIF_OBJECTS_RUN consecutive pixels, the lanes of a wave that hold the same root combine,
 *            and one lane adds to area[root] / hit[root] with int32 atomics.
 *   tally    the pixels with parent == own index are the components: each forms s and j and adds into its workgroup's LDS table
 *            with integer atomics; a workgroup sends one 64-bit atomic per non-zero counter.
 * Every find and union loop carries an iteration cap of H * W + 1.  Indices strictly decrease along a walk, so a correct kernel
 * never reaches it; a loop that does sets status[0] and leaves (as does a walk that meets an index outside the frame).  No
 * floating point at all, no host synchronisation, launch counts that follow from the shapes alone.
 *
 *   segmif_object_workspace_bytes  bytes of `workspace` (8-byte aligned): per frame, side and pixel three int32 (parent, area, hit)
 *                                  and one byte (the narrowed map), SEGMIF_OBJECTS_WORKSPACE_PER_PIXEL in all, rounded up to a
 *                                  multiple of 8; 0 for anything refused below.
 *   segmif_object_stats_i32        root_g_or_null and root_p_or_null (B, H, W) int32 are optional and overwritten.
 *
 * SEGMIF_EINVAL (-22) before any launch: a NULL desc, pred, label, obj, mass, status or workspace; K outside 1..32; connectivity
 * other than 4 or 8; n_edges outside 0..3; edges not strictly ascending or below 1; B, H or W below 1; H * W >= 2^31; a grid
 * dimension over its limit (B above SEGMIF_OBJECTS_MAX_FRAMES: the grid's z holds 2 B).
 */
#ifndef SEGMIF_OBJECTS_H
#define SEGMIF_OBJECTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGMIF_OBJECTS_TILE 64                /* a workgroup's tile is TILE x TILE pixels */
#define SEGMIF_OBJECTS_RUN 8                  /* consecutive pixels a thread of the count pass carries */
#define SEGMIF_OBJECTS_MAX_EDGES 3            /* so at most 4 size buckets */
#define SEGMIF_OBJECTS_DECILES 11             /* j = 0..10 */
#define SEGMIF_OBJECTS_MAX_FRAMES 32767       /* B: the grid's z holds 2 B <= 65535 */
#define SEGMIF_OBJECTS_WORKSPACE_PER_PIXEL 26 /* bytes per pixel and frame: 2 sides x (3 int32 + 1 byte) */

typedef struct {
  int32_t connectivity; /* 4 or 8 */
  int32_t n_edges;      /* 0..3; S = n_edges + 1 size buckets */
  int64_t edges[4];     /* the first n_edges are read: strictly ascending, each >= 1 */
  int32_t reserved[4];
} SegmifObjects;

int64_t segmif_object_workspace_bytes(int B, int H, int W);
int segmif_object_stats_i32(const SegmifObjects* desc, const int32_t* pred, const int64_t* label, int64_t* obj, int64_t* mass,
                            int32_t* status, void* workspace, int32_t* root_g_or_null, int32_t* root_p_or_null, int B, int H, int W,
                            int K, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGMIF_OBJECTS_H */
