/*
 * segmif_paste.h — instance copy-paste of libsegmif_hip.so (csrc/copy_paste.hip): an object bank cut from the resident frames along
 * their connected components, and the paste of banked objects into an augmented batch (Ghiasi et al., CVPR 2021, "Simple
 * Copy-Paste").  This project's addition, NOT the reference's loader, which pastes nothing.  A header of its own beside
 * segmif_hip.h (whose conventions hold here: device-resident, work enqueued on `stream`, 0 on success); the same library exports
 * the symbols, segmif_amd/_lib.py binds them from PASTE_SIGNATURES, and segmif_abi_version() does not count them.
 *
 * Records.  Every record is SEGMIF_PASTE_RECORD_WORDS (8) int32 values.
 *   an object   {frame, root, cls, area, x0, y0, bw, bh}: the frame's index in the set, the component's root (the smallest linear
 *               index y * W + x of its pixels, as segmif_objects.h defines it), its class, its pixel count and its tight bounding box.
 *   a slot      {obj, dx, dy, ow, oh, sx, sy, flip}: see "Paste" below.
 *   a pixel     8 BYTES {ir, v0, v1, v2, mask, alpha, 0, 0} of the patch store.
 *
 * 1. Boxes (segmif_object_boxes_i32).  root (n, H, W) int32 is what connected_components returns for the frames' labels: the root at
 * the pixels of a component, -1 outside every component (a value outside 0..H*W-1 is read as -1).  label (n, H, W) uint8 are the same
 * frames' labels.  For every component area, x0, y0, bw, bh (the TIGHT bounding box) and cls = label[root] are formed.  One record is
 * appended iff cls < K, bit cls of class_mask is set, area >= min_area and bw * bh <= max_box; its frame is frame0 + the frame's
 * index in this call, so that a set can be walked in chunks.  The record goes to the position an integer atomicAdd on *counter
 * returns.  The caller zeroes the counter; the counter is added to across calls.  A position at or past `capacity` is not written but
 * the counter still rises: the host sees the overflow in the counter and repeats with a larger list.
 *   Determinism.  The append order is ARRIVAL order and differs from run to run.  The set of records does not: the host sorts them by
 *   (frame, root), a key that is unique, so the bank is a function of the data only.
 *   How.  Three launches, integers only, no host synchronisation: init (the pixels with root == own index reset their five workspace
 *   words), gather (a thread carries {root, area, xmin, xmax} over SEGMIF_PASTE_RUN consecutive pixels of a row; the lanes of a wave
 *   that hold the same root combine and one lane sends int32 atomicAdd / atomicMin / atomicMax to the root's words), emit (the pixels
 *   with root == own index test and append).  The workspace is indexed by pixel and initialised by the call itself.
 *
 * 2. Pack (segmif_object_pack_u8).  records (M, 8) are the SORTED objects on the device, offsets (M + 1) int64 their first pixel in the
 * patch store (so offsets[m + 1] - offsets[m] >= bw * bh and offsets[M] = store_pixels).  root (n, H, W) are the root maps of frames
 * frame0 .. frame0 + n - 1; ir, mask (n, H, W) and vis (n, H, W, 3) uint8 the same frames.  Object m owns bw * bh pixel records,
 * row-major over its box.  alpha = 1 exactly where the frame's root equals the record's root, and the pixel then holds the frame's
 * ir, vis[0..2] and mask bytes; a pixel with alpha = 0 is eight zero bytes.  The store therefore depends on the object alone: a
 * second component of the same class inside the box leaves no trace.  An object of another frame than the call's, or whose box or
 * offsets do not lie inside the frame / the store, is skipped.  One launch, a workgroup per object.
 *
 * 3. Paste (segmif_copy_paste_f32).  ir3, vis3, mask3 (B, 3, h, w) fp32 and label (B, h, w) int64, w % 4 == 0, are an augmented batch
 * (segmif_augment_apply_u8 or segmif_class_mix_apply_f32).  table (B, P, 8) int32 with P in 0..SEGMIF_PASTE_MAX_SLOTS holds P slots
 * per sample:
 *   obj      indexes the bank.
 *   dx, dy   the top-left corner in the crop; negative or past the edge is legal, what falls outside is dropped.
 *   ow, oh   the pasted size.
 *   sx, sy   16.16 fixed-point source steps: nearest-neighbour scaling, all in integers.
 *   flip     bit 0 mirrors the object horizontally.
 * A slot is EMPTY when obj lies outside 0..M-1, ow or oh outside 1..SEGMIF_PASTE_MAX_SIZE (4096), or sx or sy outside
 * 1..SEGMIF_PASTE_MAX_STEP (2^24).  These clamps are part of the rule, not a debugging aid: no value in a device table can make the
 * kernel read outside the bank.  (A bank record whose patch does not lie inside the store makes its slots EMPTY too.)
 *   Per output pixel (y, x) of receiver b, walk the slots from P - 1 down to 0.  With u = x - dx and v = y - dy a slot is a candidate
 *   iff 0 <= u < ow and 0 <= v < oh.  Then, in 64-bit integers, su = min(bw - 1, (u * sx + (sx >> 1)) >> 16); if flip & 1,
 *   su = bw - 1 - su; sv = min(bh - 1, (v * sy + (sy >> 1)) >> 16), never flipped.  The pixel record is
 *   patch[offsets[obj] + sv * bw + su].  The first candidate whose record has alpha = 1 wins, so later slots lie on top.
 *   The winner's values: all three channels of ir3 become __fdiv_rn((float)ir, 255.0f), mask3 likewise from mask, vis3[c] from v_c,
 *   label = cls as int64.  This is the expression csrc/augment.hip uses, so a pasted value equals what augment_apply gives that byte
 *   WITHOUT photometric distortion: the receiver's brightness / contrast draw is NOT applied to the object.
 *   Where no slot wins every value is the receiver's, copied bit for bit: NaN payloads, -0.0 and labels such as 255, -1 and
 *   2^40 + 3 survive.
 *   Outputs.  Out of place, the inputs are untouched: ir3_out, vis3_out, mask3_out, label_out.  pasted (B) int64 is ZEROED by the call
 *   and then holds the pixels that took a slot's values.  tally_or_null (n_class, 2) int64 is ADDED to: +1 in [cls][0] per non-empty
 *   slot, the pixels that took the slot's values in [cls][1] (a cls outside 0..n_class-1 is not tallied).
 *   How.  One launch (after the memset of pasted): the sample in blockIdx.y, a thread per group of 4 pixels of a row, a workgroup per
 *   1024 consecutive pixels.  The sample's slots are read once per workgroup, validated and culled against the workgroup's rows.  A
 *   group no slot's rectangle touches is a straight 16-byte copy (nine plane loads and stores, two label loads and stores);
 *   otherwise one 8-byte patch load per candidate pixel.  Counts go by ballot and popcount per wave and integer atomics per
 *   workgroup.  No float arithmetic but the divisions, no float atomics, 64-bit offsets.  Everything is exact: two runs give equal bits.
 *
 * SEGMIF_EINVAL (-22) before any launch:
 *   boxes  a NULL root, label, counter or workspace; NULL records with capacity > 0; K outside 1..32; min_area or max_box below 1;
 *          capacity or frame0 below 0; n, H or W below 1; n above SEGMIF_PASTE_MAX_FRAMES; H * W >= 2^31; frame0 + n > 2^31 - 1;
 *          records not 16-byte aligned (a record is written by two 16-byte stores); root, counter or workspace not 4-byte aligned.
 *          segmif_object_boxes_workspace_bytes answers 0 for the extents refused here.
 *   pack   a NULL pointer; M below 1 or above 2^31 - 1 (the grid's x holds M); store_pixels below 0; n, H, W as above; frame0 below 0;
 *          frame0 + n > 2^31 - 1; offsets or patches not 8-byte aligned; records or root not 4-byte aligned.
 *   paste  a NULL tensor, records, offsets, patches or pasted; NULL table with P > 0; P outside 0..8; B outside 1..65535; h or w below
 *          1; w % 4; n_class outside 1..255; M below 1; store_pixels below 1; one of the eight tensors not 16-byte aligned;
 *          offsets, patches, pasted or the tally not 8-byte aligned; records or table not 4-byte aligned; h * w / 1024 above 2^31 - 1.
 */
#ifndef SEGMIF_PASTE_H
#define SEGMIF_PASTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGMIF_PASTE_RECORD_WORDS 8         /* int32 values per object record and per slot; bytes per patch pixel */
#define SEGMIF_PASTE_MAX_SLOTS 8            /* P */
#define SEGMIF_PASTE_MAX_SIZE 4096          /* ow, oh */
#define SEGMIF_PASTE_MAX_STEP (1 << 24)     /* sx, sy: 256 source pixels per pasted pixel */
#define SEGMIF_PASTE_RUN 8                  /* consecutive pixels a thread of the gather pass carries */
#define SEGMIF_PASTE_MAX_FRAMES 32767       /* n: the grid's y */
#define SEGMIF_PASTE_WORKSPACE_PER_PIXEL 20 /* bytes per pixel and frame: area, xmin, xmax, ymin, ymax as int32 */

int64_t segmif_object_boxes_workspace_bytes(int n, int H, int W);
int segmif_object_boxes_i32(const int32_t* root, const uint8_t* label, int n, int H, int W, int K, uint32_t class_mask, int64_t min_area,
                            int64_t max_box, int frame0, int32_t* records, int64_t capacity, int32_t* counter, void* workspace,
                            void* stream);
int segmif_object_pack_u8(const int32_t* records, const int64_t* offsets, int64_t M, int64_t store_pixels, const int32_t* root,
                          const uint8_t* ir, const uint8_t* vis, const uint8_t* mask, int frame0, int n, int H, int W, uint8_t* patches,
                          void* stream);
int segmif_copy_paste_f32(const float* ir3, const float* vis3, const float* mask3, const int64_t* label, int B, int h, int w,
                          const int32_t* records, const int64_t* offsets, const uint8_t* patches, int64_t M, int64_t store_pixels,
                          const int32_t* table, int P, int n_class, float* ir3_out, float* vis3_out, float* mask3_out,
                          int64_t* label_out, int64_t* pasted, int64_t* tally_or_null, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGMIF_PASTE_H */
