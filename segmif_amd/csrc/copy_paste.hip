// Instance copy-paste (Ghiasi et al. 2021): the object bank's boxes and patch store from the connected components of the resident
// labels, and the paste of banked objects into an augmented batch.  The rule is stated in include/segmif_paste.h.  Integers and
// copied float bits throughout; the only float arithmetic is the byte / 255 division csrc/augment.hip makes.
//
//   boxes_init_kernel    the pixels with root == own index reset their five workspace words
//   boxes_gather_kernel  a thread carries {root, area, xmin, xmax} over RUN consecutive pixels of a row; the lanes of a wave that hold
//                        the same root combine and one lane sends int32 atomics to the root's words
//   boxes_emit_kernel    the pixels with root == own index test class, area and box and append a record at atomicAdd(counter)
//   pack_kernel          a workgroup per object: its box's pixels as 8-byte records, alpha where the frame's root is the object's
//   paste_kernel         grid (blocks, B), a thread per group of 4 pixels; the sample's slots validated and culled once per
//                        workgroup in LDS; untouched groups are 16-byte copies; counts by ballot / popcount and integer atomics
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "segmif_hip.h"
#include "segmif_paste.h"

namespace {

constexpr int THREADS = 256;
constexpr int RUN = SEGMIF_PASTE_RUN;
constexpr int WORDS = SEGMIF_PASTE_RECORD_WORDS;
constexpr int MAX_SLOTS = SEGMIF_PASTE_MAX_SLOTS;

typedef uint32_t Quad __attribute__((ext_vector_type(4)));            // four floats' bits, or four record words
typedef uint32_t Duo __attribute__((ext_vector_type(2)));             // one patch pixel
typedef unsigned long long Pair __attribute__((ext_vector_type(2)));  // two labels

// ---- boxes --------------------------------------------------------------------------------------------------------------------------

struct BoxArgs {
  const int* root;             // (n, N)
  const unsigned char* label;  // (n, N)
  int *area, *xmin, *xmax, *ymin, *ymax;  // (n, N) each
  int N, W, K, frame0;
  uint32_t class_mask;
  long long min_area, max_box, capacity;
  int* records;
  int* counter;
};

__global__ __launch_bounds__(THREADS) void boxes_init_kernel(BoxArgs a) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.N) return;
  const long long at = (long long)blockIdx.y * a.N + i;
  if (a.root[at] != (int)i) return;
  a.area[at] = 0;
  a.xmin[at] = INT_MAX, a.ymin[at] = INT_MAX;
  a.xmax[at] = -1, a.ymax[at] = -1;
}

// The lanes with `flush` set hand {root, area, x0, x1, y} over; those that hold the same root combine and one lane sends the
// atomics.  Called by whole waves.  `base` is the frame's first workspace word.
__device__ __forceinline__ void box_flush(bool flush, int root, int area, int x0, int x1, int y, const BoxArgs& a, long long base,
                                          int lane) {
  unsigned long long todo = __ballot(flush);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(root, lead);
    const bool in = flush && root == r0;
    const unsigned long long m = __ballot(in);
    int s = in ? area : 0, lo_x = in ? x0 : INT_MAX, hi_x = in ? x1 : -1, lo_y = in ? y : INT_MAX, hi_y = in ? y : -1;
    if (m & (m - 1)) {  // (more than one lane holds it; the same in every lane)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        lo_x = min(lo_x, __shfl_xor(lo_x, off)), hi_x = max(hi_x, __shfl_xor(hi_x, off));
        lo_y = min(lo_y, __shfl_xor(lo_y, off)), hi_y = max(hi_y, __shfl_xor(hi_y, off));
      }
    }
    if (lane == lead) {  // r0 is in 0..N-1: the gather pass carries no other root
      atomicAdd(a.area + base + r0, s);
      atomicMin(a.xmin + base + r0, lo_x), atomicMax(a.xmax + base + r0, hi_x);
      atomicMin(a.ymin + base + r0, lo_y), atomicMax(a.ymax + base + r0, hi_y);
    }
    todo &= ~m;
  }
}

__global__ __launch_bounds__(THREADS) void boxes_gather_kernel(BoxArgs a) {
  const int lane = threadIdx.x & 63;
  const long long base = (long long)blockIdx.y * a.N;
  const int* root = a.root + base;
  const long long i0 = ((long long)blockIdx.x * THREADS + threadIdx.x) * RUN;
  int y = (int)(i0 / a.W), x = (int)(i0 - (long long)y * a.W);
  int carry_root = -1, c_area = 0, c_x0 = 0, c_x1 = 0, c_y = 0;
#pragma unroll 1
  for (int j = 0; j < RUN; ++j) {  // (no early exit: box_flush is called by whole waves)
    const long long i = i0 + j;
    int r = i < a.N ? root[i] : -1;
    if ((unsigned)r >= (unsigned)a.N) r = -1;
    const bool flush = carry_root >= 0 && (r != carry_root || y != c_y);
    box_flush(flush, carry_root, c_area, c_x0, c_x1, c_y, a, base, lane);
    if (flush || carry_root < 0) carry_root = r, c_area = 0, c_x0 = x, c_y = y;
    if (r >= 0) ++c_area, c_x1 = x;
    if (++x == a.W) x = 0, ++y;
  }
  box_flush(carry_root >= 0, carry_root, c_area, c_x0, c_x1, c_y, a, base, lane);
}

__global__ __launch_bounds__(THREADS) void boxes_emit_kernel(BoxArgs a) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.N) return;
  const long long at = (long long)blockIdx.y * a.N + i;
  if (a.root[at] != (int)i) return;
  const int cls = a.label[at], area = a.area[at];
  const int x0 = a.xmin[at], y0 = a.ymin[at], bw = a.xmax[at] - x0 + 1, bh = a.ymax[at] - y0 + 1;
  if (area < 1 || bw < 1 || bh < 1) return;  // (cannot be: a root counts itself)
  if (cls >= a.K || !((a.class_mask >> cls) & 1u)) return;
  if (area < a.min_area || (long long)bw * bh > a.max_box) return;
  const long long pos = atomicAdd(a.counter, 1);
  if (pos < 0 || pos >= a.capacity) return;  // (the counter still rose: the host sees the overflow)
  Quad* out = reinterpret_cast<Quad*>(a.records + pos * WORDS);
  out[0] = Quad{(uint32_t)(a.frame0 + (int)blockIdx.y), (uint32_t)i, (uint32_t)cls, (uint32_t)area};
  out[1] = Quad{(uint32_t)x0, (uint32_t)y0, (uint32_t)bw, (uint32_t)bh};
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void pack_kernel(const int* __restrict__ records, const long long* __restrict__ offsets,
                                                       long long store_pixels, const int* __restrict__ root,
                                                       const unsigned char* __restrict__ ir, const unsigned char* __restrict__ vis,
                                                       const unsigned char* __restrict__ mask, int frame0, int n, int H, int W,
                                                       Duo* __restrict__ patches) {
  const long long m = blockIdx.x;
  const int* rec = records + m * WORDS;
  const int frame = rec[0], r = rec[1], x0 = rec[4], y0 = rec[5], bw = rec[6], bh = rec[7];
  const long long off = offsets[m], next = offsets[m + 1];
  if (frame < frame0 || frame >= frame0 + n || x0 < 0 || y0 < 0 || bw < 1 || bh < 1 || bw > W - x0 || bh > H - y0) return;
  const long long count = (long long)bw * bh;
  if (off < 0 || next > store_pixels || count > next - off) return;
  const long long N = (long long)H * W, fb = (long long)(frame - frame0) * N;
  for (long long p = threadIdx.x; p < count; p += THREADS) {
    const int py = (int)(p / bw), px = (int)(p - (long long)py * bw);
    const long long src = fb + (long long)(y0 + py) * W + (x0 + px);
    Duo v = Duo{0u, 0u};
    if (root[src] == r) {
      const unsigned char* c = vis + 3 * src;
      v[0] = (uint32_t)ir[src] | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 24);
      v[1] = (uint32_t)mask[src] | (1u << 8);
    }
    patches[off + p] = v;
  }
}

// ---- paste --------------------------------------------------------------------------------------------------------------------------

struct Slot {
  int dx, dy, ow, oh, sx, sy, flip, bw, bh, cls;
  long long off;
};

struct PasteArgs {
  const float* in[3];  // ir3, vis3, mask3
  float* out[3];
  const long long* label;
  long long* label_out;
  const int* records;
  const long long* offsets;
  const Duo* patches;
  const int* table;
  long long M, store_pixels, hw;
  int w, P, n_class;
  unsigned long long* pasted;
  unsigned long long* tally;
};

__device__ __forceinline__ uint32_t unit_bits(uint32_t byte) { return __float_as_uint(__fdiv_rn((float)byte, 255.0f)); }

__global__ __launch_bounds__(THREADS) void paste_kernel(PasteArgs a) {
  __shared__ Slot s_slot[MAX_SLOTS];
  __shared__ int s_live[MAX_SLOTS];
  __shared__ unsigned s_cnt[MAX_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  const long long groups = a.hw >> 2;
  const long long g0 = (long long)blockIdx.x * THREADS;
  if (tid < MAX_SLOTS) {
    s_live[tid] = 0, s_cnt[tid] = 0u;
    if (tid < a.P) {
      const int* row = a.table + ((long long)b * a.P + tid) * WORDS;
      Slot s;
      const int obj = row[0];
      s.dx = row[1], s.dy = row[2], s.ow = row[3], s.oh = row[4], s.sx = row[5], s.sy = row[6], s.flip = row[7];
      s.bw = s.bh = 1, s.cls = -1, s.off = 0;
      bool ok = obj >= 0 && obj < a.M && s.ow >= 1 && s.ow <= SEGMIF_PASTE_MAX_SIZE && s.oh >= 1 && s.oh <= SEGMIF_PASTE_MAX_SIZE &&
                s.sx >= 1 && s.sx <= SEGMIF_PASTE_MAX_STEP && s.sy >= 1 && s.sy <= SEGMIF_PASTE_MAX_STEP;
      if (ok) {
        const int* rec = a.records + (long long)obj * WORDS;
        s.cls = rec[2], s.bw = rec[6], s.bh = rec[7], s.off = a.offsets[obj];
        ok = s.bw >= 1 && s.bh >= 1 && s.off >= 0 && s.off <= a.store_pixels && (long long)s.bw * s.bh <= a.store_pixels - s.off;
      }
      if (ok) {
        if (blockIdx.x == 0 && a.tally && s.cls >= 0 && s.cls < a.n_class) atomicAdd(a.tally + 2 * s.cls, 1ull);
        // the rows and columns this workgroup's pixels lie in
        const long long last = min(groups, g0 + THREADS) * 4 - 1;
        const long long r0 = (g0 * 4) / a.w, r1 = last / a.w;
        const long long top = s.dy, bottom = (long long)s.dy + s.oh - 1, left = s.dx, right = (long long)s.dx + s.ow - 1;
        s_live[tid] = top <= r1 && bottom >= r0 && left < a.w && right >= 0;
        s_slot[tid] = s;
      }
    }
  }
  __syncthreads();

  const long long g = g0 + tid;
  const bool active = g < groups;
  int win[4] = {-1, -1, -1, -1};
  if (active) {
    const long long p = g << 2;
    const int y = (int)(p / a.w), x = (int)(p - (long long)y * a.w);
    Quad plane[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) plane[q][ch] = *reinterpret_cast<const Quad*>(a.in[q] + ((long long)b * 3 + ch) * a.hw + p);
    Pair l0 = *reinterpret_cast<const Pair*>(a.label + (long long)b * a.hw + p);
    Pair l1 = *reinterpret_cast<const Pair*>(a.label + (long long)b * a.hw + p + 2);
    unsigned touched = 0u;
    for (int s = 0; s < a.P; ++s) {
      if (!s_live[s]) continue;
      const long long v = (long long)y - s_slot[s].dy, left = s_slot[s].dx;
      if (v >= 0 && v < s_slot[s].oh && left <= x + 3 && left + s_slot[s].ow > x) touched |= 1u << s;
    }
    if (touched) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        for (int s = a.P - 1; s >= 0; --s) {
          if (!((touched >> s) & 1u)) continue;
          const Slot& t = s_slot[s];
          const long long u = (long long)(x + j) - t.dx, v = (long long)y - t.dy;
          if (u < 0 || u >= t.ow) continue;
          long long su = min((long long)t.bw - 1, (u * t.sx + (t.sx >> 1)) >> 16);
          if (t.flip & 1) su = t.bw - 1 - su;
          const long long sv = min((long long)t.bh - 1, (v * t.sy + (t.sy >> 1)) >> 16);
          const Duo px = a.patches[t.off + sv * t.bw + su];
          if (((px[1] >> 8) & 255u) != 1u) continue;
          const uint32_t fi = unit_bits(px[0] & 255u), fm = unit_bits(px[1] & 255u);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            plane[0][ch][j] = fi;
            plane[1][ch][j] = unit_bits((px[0] >> (8 + 8 * ch)) & 255u);
            plane[2][ch][j] = fm;
          }
          const unsigned long long lab = (unsigned long long)(long long)t.cls;
          if (j < 2)
            l0[j & 1] = lab;
          else
            l1[j & 1] = lab;
          win[j] = s;
          break;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<Quad*>(a.out[q] + ((long long)b * 3 + ch) * a.hw + p) = plane[q][ch];
    *reinterpret_cast<Pair*>(a.label_out + (long long)b * a.hw + p) = l0;
    *reinterpret_cast<Pair*>(a.label_out + (long long)b * a.hw + p + 2) = l1;
  }

  // counts: per live slot one ballot per pixel of the group, one LDS atomic per wave, one global atomic per workgroup
  for (int s = 0; s < a.P; ++s) {
    if (!s_live[s]) continue;  // (the same in every thread of the workgroup)
    unsigned n = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) n += (unsigned)__popcll(__ballot(win[j] == s));
    if (lane == 0 && n) atomicAdd(&s_cnt[s], n);
  }
  __syncthreads();
  if (tid < a.P && s_cnt[tid]) {
    const int cls = s_slot[tid].cls;
    atomicAdd(a.pasted + b, (unsigned long long)s_cnt[tid]);
    if (a.tally && cls >= 0 && cls < a.n_class) atomicAdd(a.tally + 2 * cls + 1, (unsigned long long)s_cnt[tid]);
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

bool extents_ok(int n, int H, int W) {
  return n >= 1 && H >= 1 && W >= 1 && n <= SEGMIF_PASTE_MAX_FRAMES && (long long)H * W < (1ll << 31);
}

}  // namespace

extern "C" int64_t segmif_object_boxes_workspace_bytes(int n, int H, int W) {
  if (!extents_ok(n, H, W)) return 0;
  return (int64_t)n * H * W * SEGMIF_PASTE_WORKSPACE_PER_PIXEL;
}

extern "C" int segmif_object_boxes_i32(const int32_t* root, const uint8_t* label, int n, int H, int W, int K, uint32_t class_mask,
                                       int64_t min_area, int64_t max_box, int frame0, int32_t* records, int64_t capacity, int32_t* counter,
                                       void* workspace, void* stream) {
  if (!root || !label || !counter || !workspace) return SEGMIF_EINVAL;
  if (K < 1 || K > 32 || min_area < 1 || max_box < 1 || capacity < 0 || frame0 < 0 || !extents_ok(n, H, W)) return SEGMIF_EINVAL;
  if ((capacity > 0 && !records) || (long long)frame0 + n > INT_MAX) return SEGMIF_EINVAL;
  if (misaligned(root, 4) || misaligned(records, 16) || misaligned(counter, 4) || misaligned(workspace, 4)) return SEGMIF_EINVAL;
  BoxArgs a;
  const long long N = (long long)H * W, all = N * n;
  a.root = root, a.label = label;
  a.area = (int*)workspace, a.xmin = a.area + all, a.xmax = a.xmin + all, a.ymin = a.xmax + all, a.ymax = a.ymin + all;
  a.N = (int)N, a.W = W, a.K = K, a.frame0 = frame0, a.class_mask = class_mask;
  a.min_area = min_area, a.max_box = max_box, a.capacity = capacity, a.records = records, a.counter = counter;
  hipStream_t s = (hipStream_t)stream;
  const unsigned per_pixel = (unsigned)((N + THREADS - 1) / THREADS), per_run = (unsigned)((N + THREADS * RUN - 1) / (THREADS * RUN));
  hipLaunchKernelGGL(boxes_init_kernel, dim3(per_pixel, (unsigned)n), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(boxes_gather_kernel, dim3(per_run, (unsigned)n), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(boxes_emit_kernel, dim3(per_pixel, (unsigned)n), dim3(THREADS), 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int segmif_object_pack_u8(const int32_t* records, const int64_t* offsets, int64_t M, int64_t store_pixels, const int32_t* root,
                                     const uint8_t* ir, const uint8_t* vis, const uint8_t* mask, int frame0, int n, int H, int W,
                                     uint8_t* patches, void* stream) {
  if (!records || !offsets || !root || !ir || !vis || !mask || !patches) return SEGMIF_EINVAL;
  if (M < 1 || M > INT_MAX || store_pixels < 0 || frame0 < 0 || !extents_ok(n, H, W) || (long long)frame0 + n > INT_MAX) return SEGMIF_EINVAL;
  if (misaligned(records, 4) || misaligned(offsets, 8) || misaligned(root, 4) || misaligned(patches, 8)) return SEGMIF_EINVAL;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)M), dim3(THREADS), 0, (hipStream_t)stream, records,
                     reinterpret_cast<const long long*>(offsets), (long long)store_pixels, root, ir, vis, mask, frame0, n, H, W,
                     reinterpret_cast<Duo*>(patches));
  return (int)hipGetLastError();
}

extern "C" int segmif_copy_paste_f32(const float* ir3, const float* vis3, const float* mask3, const int64_t* label, int B, int h, int w,
                                     const int32_t* records, const int64_t* offsets, const uint8_t* patches, int64_t M, int64_t store_pixels,
                                     const int32_t* table, int P, int n_class, float* ir3_out, float* vis3_out, float* mask3_out,
                                     int64_t* label_out, int64_t* pasted, int64_t* tally_or_null, void* stream) {
  if (!ir3 || !vis3 || !mask3 || !label || !records || !offsets || !patches || !ir3_out || !vis3_out || !mask3_out || !label_out || !pasted)
    return SEGMIF_EINVAL;
  if (P < 0 || P > MAX_SLOTS || (P > 0 && !table) || B < 1 || B > 65535 || h < 1 || w < 1 || w % 4) return SEGMIF_EINVAL;
  if (n_class < 1 || n_class > 255 || M < 1 || store_pixels < 1) return SEGMIF_EINVAL;
  if (misaligned(ir3, 16) || misaligned(vis3, 16) || misaligned(mask3, 16) || misaligned(label, 16) || misaligned(ir3_out, 16) ||
      misaligned(vis3_out, 16) || misaligned(mask3_out, 16) || misaligned(label_out, 16) || misaligned(records, 4) ||
      misaligned(offsets, 8) || misaligned(patches, 8) || misaligned(table, 4) || misaligned(pasted, 8) || misaligned(tally_or_null, 8))
    return SEGMIF_EINVAL;
  const long long hw = (long long)h * w, groups = hw >> 2, blocks = (groups + THREADS - 1) / THREADS;
  if (blocks > INT_MAX) return SEGMIF_EINVAL;
  PasteArgs a;
  a.in[0] = ir3, a.in[1] = vis3, a.in[2] = mask3, a.out[0] = ir3_out, a.out[1] = vis3_out, a.out[2] = mask3_out;
  a.label = reinterpret_cast<const long long*>(label), a.label_out = reinterpret_cast<long long*>(label_out);
  a.records = records, a.offsets = reinterpret_cast<const long long*>(offsets), a.patches = reinterpret_cast<const Duo*>(patches);
  a.table = table, a.M = M, a.store_pixels = store_pixels, a.hw = hw, a.w = w, a.P = P, a.n_class = n_class;
  a.pasted = reinterpret_cast<unsigned long long*>(pasted), a.tally = reinterpret_cast<unsigned long long*>(tally_or_null);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(pasted, 0, sizeof(int64_t) * (size_t)B, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(paste_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(THREADS), 0, s, a);
  return (int)hipGetLastError();
}
