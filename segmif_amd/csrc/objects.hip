// Object-level statistics of two label maps (include/segmif_objects.h has the rule): connected components of the ground truth
// (side 0) and of the prediction (side 1) with their minimum linear index as the root, and per frame, side, class and size bucket
// the number of components by the decile of their coverage by the other map.  This project's addition, NOT the reference's
// evaluation.  Four launches; the side is the low bit of blockIdx.z, the frame the rest.
//
//   objects_local_kernel   one workgroup per 64 x 64 tile and map: narrow to bytes, LDS parents (local raster index) that start at
//                          the head of the pixel's horizontal run, unions with the row above (atomicMin), flatten, write the global
//                          index of the local root to parent[] and zero area / hit
//   objects_border_kernel  the top row and left column of every tile unite with their neighbours in the adjacent tiles on the
//                          global array: lock-free, agent-scope atomics only, nobody waits
//   objects_count_kernel   plain loads after the kernel boundary: walk to the root, write root_*, add area and hit to the root's
//                          entries - carried over a thread's run of 8 pixels, combined over the lanes of a wave that hold the root
//   objects_tally_kernel   the roots form (size bucket, decile) and add into an LDS table; one 64-bit atomic per non-zero counter
//
// Workspace, per frame and side N = H * W entries each: parent, area, hit (int32), then the narrowed maps (bytes).  Integer
// arithmetic only; no float atomics, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"
#include "segmif_objects.h"

namespace {

constexpr int TILE = SEGMIF_OBJECTS_TILE;
constexpr int TILE_PIXELS = TILE * TILE;
constexpr int THREADS = 256;
constexpr int RUN = SEGMIF_OBJECTS_RUN;
constexpr int BORDER_THREADS = 128;  // 64 of the top row + 63 of the left column (the corner once)
constexpr int MAXS = SEGMIF_OBJECTS_MAX_EDGES + 1;
constexpr int DEC = SEGMIF_OBJECTS_DECILES;
constexpr int IGN = 255;

static_assert(TILE == 64 && THREADS * 16 == TILE_PIXELS, "the local pass walks 16 pixels per thread in rows of 64");
static_assert(64 * RUN < 65536, "a wave's combined {area, hit} is packed into 16 + 16 bits");

struct ObjArgs {
  const int* pred;
  const long long* label;
  unsigned long long* obj;
  unsigned long long* mass;
  int* status;
  int* parent;  // [2 B][N]
  int* area;    // [2 B][N]
  int* hit;     // [2 B][N]
  unsigned char* val;  // [2 B][N]
  int* root_g;
  int* root_p;
  int B, H, W, K, N, tiles_x, conn8, S, cap;
  long long edge[MAXS];
};

// ---- local pass ------------------------------------------------------------------------------------------------------------------

// Termination: lp[x] <= x always (a parent is only ever replaced by a smaller index), so x strictly decreases along the walk and it
// ends within TILE_PIXELS <= cap steps; the cap (H * W + 1) only turns a defect into status[0] instead of a hung card.
__device__ __forceinline__ int find_lds(int* lp, int x, int cap, int* status) {
  for (int n = 0; n < cap; ++n) {
    const int p = __hip_atomic_load(lp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
  atomicOr(status, 1);
  return -1;
}

// Termination: after a failed atomicMin, old < a, so the larger of the two roots strictly decreases from one turn to the next: at
// most TILE_PIXELS <= cap turns.  Nobody is waited for: a turn either links, finds the two already joined, or goes on with a
// smaller index that another thread's link handed it.
__device__ __forceinline__ void unite_lds(int* lp, int a, int b, int cap, int* status) {
  for (int n = 0; n < cap; ++n) {
    a = find_lds(lp, a, cap, status);
    b = find_lds(lp, b, cap, status);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(lp + a, b);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, 1);
}

__global__ __launch_bounds__(THREADS) void objects_local_kernel(ObjArgs a) {
  __shared__ int lp[TILE_PIXELS];
  __shared__ unsigned char lv[TILE_PIXELS];
  const int tid = threadIdx.x;
  const int side = blockIdx.z & 1, b = blockIdx.z >> 1;
  const int tx0 = ((int)blockIdx.x % a.tiles_x) * TILE, ty0 = ((int)blockIdx.x / a.tiles_x) * TILE;
  const long long base = ((long long)b * 2 + side) * a.N;

#pragma unroll 4
  for (int k = 0; k < TILE_PIXELS / THREADS; ++k) {
    const int i = tid + k * THREADS;
    const int x = tx0 + (i & (TILE - 1)), y = ty0 + (i >> 6);
    int v = IGN;
    if (x < a.W && y < a.H) {
      const long long o = (long long)b * a.N + (long long)y * a.W + x;
      const long long l = a.label[o];
      const bool labelled = (unsigned long long)l < (unsigned long long)a.K;  // the full 64 bits, before narrowing
      if (side == 0) {
        v = labelled ? (int)l : IGN;
      } else {
        const int p = a.pred[o];
        v = labelled && (unsigned)p < (unsigned)a.K ? p : IGN;
      }
    }
    // A wave holds one row of the tile (lane = column): every pixel starts at the first pixel of its horizontal run, so the W
    // neighbours are joined without a union and the trees start flat.  (Whole waves get here: the loads above are predicated.)
    const int lx = i & (TILE - 1);
    const int vprev = __shfl_up(v, 1);
    const bool same = lx > 0 && v != IGN && vprev == v;
    const unsigned long long starts = ~__ballot(same);  // (bit 0 is always set)
    const int start = 63 - __clzll((long long)(starts & (~0ull >> (63 - lx))));
    lv[i] = (unsigned char)v;
    lp[i] = i - lx + start;
  }
  __syncthreads();

#pragma unroll 1
  for (int k = 0; k < TILE_PIXELS / THREADS; ++k) {
    const int i = tid + k * THREADS;
    const int v = lv[i];
    if (v == IGN) continue;  // (pixels outside the frame are IGN: nothing joins across the frame's edge)
    const int lx = i & (TILE - 1), ly = i >> 6;
    const bool w = lx > 0 && lv[i - 1] == v;
    const bool n = ly > 0 && lv[i - TILE] == v;
    // (W is joined by the runs; with W and NW equal too, the W pixel joins the same two runs)
    if (n && !(w && lv[i - TILE - 1] == v)) unite_lds(lp, i, i - TILE, a.cap, a.status);
    if (a.conn8 && ly > 0 && !n) {  // (with N equal, NW and NE are N's own W and E neighbours: joined through it)
      if (!w && lx > 0 && lv[i - TILE - 1] == v) unite_lds(lp, i, i - TILE - 1, a.cap, a.status);
      if (lx < TILE - 1 && lv[i - TILE + 1] == v) unite_lds(lp, i, i - TILE + 1, a.cap, a.status);
    }
  }
  __syncthreads();

  // flatten: the trees no longer change, a pixel replaces its own parent by its root (shortening the others' walks meanwhile)
#pragma unroll 1
  for (int k = 0; k < TILE_PIXELS / THREADS; ++k) {
    const int i = tid + k * THREADS;
    if (lv[i] == IGN) continue;
    const int r = find_lds(lp, i, a.cap, a.status);
    if (r >= 0) __hip_atomic_store(lp + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();

#pragma unroll 4
  for (int k = 0; k < TILE_PIXELS / THREADS; ++k) {
    const int i = tid + k * THREADS;
    const int x = tx0 + (i & (TILE - 1)), y = ty0 + (i >> 6);
    if (x >= a.W || y >= a.H) continue;
    const long long o = base + (long long)y * a.W + x;
    const int v = lv[i], r = lp[i];
    a.parent[o] = v == IGN ? -1 : (ty0 + (r >> 6)) * a.W + tx0 + (r & (TILE - 1));
    a.area[o] = 0;
    a.hit[o] = 0;
    a.val[o] = (unsigned char)v;
  }
}

// ---- border pass -----------------------------------------------------------------------------------------------------------------

// Every read of parent[] here is an agent-scope relaxed atomic load: a plain load may be served stale from this CU's L1 or another
// XCD's L2 while other workgroups link.  Termination: parent[x] <= x always, so x strictly decreases: at most N < cap steps.  The
// cap turns a defect into status[0]; an index outside the frame (a defect too) is never followed.
__device__ __forceinline__ int find_global(int* parent, int x, int N, int cap, int* status) {
  for (int n = 0; n < cap; ++n) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    if ((unsigned)p >= (unsigned)N) break;
    x = p;
  }
  atomicOr(status, 1);
  return -1;
}

// The lock-free union.  Termination: a failed atomicMin returns old < a, so the larger root strictly decreases from turn to turn:
// at most N < cap turns.  No thread waits for another: no flag, no spin, no ticket.
__device__ __forceinline__ void unite_global(int* parent, int a, int b, int N, int cap, int* status) {
  for (int n = 0; n < cap; ++n) {
    a = find_global(parent, a, N, cap, status);
    b = find_global(parent, b, N, cap, status);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, 1);
}

__global__ __launch_bounds__(BORDER_THREADS) void objects_border_kernel(ObjArgs a) {
  const int t = threadIdx.x;
  if (t >= 2 * TILE - 1) return;
  const int b2 = blockIdx.z;
  const int tx0 = ((int)blockIdx.x % a.tiles_x) * TILE, ty0 = ((int)blockIdx.x / a.tiles_x) * TILE;
  const bool top = t < TILE;                    // (t == 0: the corner, which is on both)
  const int x = top ? tx0 + t : tx0, y = top ? ty0 : ty0 + (t - TILE + 1);
  if (x >= a.W || y >= a.H) return;
  const bool left = !top || t == 0;
  const long long base = (long long)b2 * a.N;
  int* parent = a.parent + base;
  const unsigned char* val = a.val + base;
  const int W = a.W, i = y * W + x;
  const int v = val[i];
  if (v == IGN) return;
  if (top && y > 0) {  // the row above lies in other tiles
    if (val[i - W] == v) unite_global(parent, i, i - W, a.N, a.cap, a.status);
    if (a.conn8) {
      if (x > 0 && val[i - W - 1] == v) unite_global(parent, i, i - W - 1, a.N, a.cap, a.status);
      if (x + 1 < W && val[i - W + 1] == v) unite_global(parent, i, i - W + 1, a.N, a.cap, a.status);
    }
  }
  if (left && x > 0) {  // the column to the left lies in other tiles
    if (val[i - 1] == v) unite_global(parent, i, i - 1, a.N, a.cap, a.status);
    if (a.conn8) {
      if (!top && val[i - W - 1] == v) unite_global(parent, i, i - W - 1, a.N, a.cap, a.status);  // (y > ty0 >= 0; the corner's NW is above)
      if (y + 1 < a.H && val[i + W - 1] == v) unite_global(parent, i, i + W - 1, a.N, a.cap, a.status);
    }
  }
}

// ---- count pass ------------------------------------------------------------------------------------------------------------------

// The lanes with `flush` set hand {root, packed area << 16 | hit} over; those that hold the same root combine and one lane sends the
// atomics.  Called by whole waves.
__device__ __forceinline__ void wave_flush(bool flush, int root, unsigned packed, int* area, int* hit, int lane) {
  unsigned long long todo = __ballot(flush);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(root, lead);
    const bool in = flush && root == r0;
    const unsigned long long m = __ballot(in);
    unsigned s = in ? packed : 0u;
    if (m & (m - 1)) {  // (more than one lane holds it; the same in every lane)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    }
    if (lane == lead) {
      atomicAdd(area + r0, (int)(s >> 16));
      if (s & 0xffffu) atomicAdd(hit + r0, (int)(s & 0xffffu));
    }
    todo &= ~m;
  }
}

__global__ __launch_bounds__(THREADS) void objects_count_kernel(ObjArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int side = blockIdx.z & 1, b = blockIdx.z >> 1;
  const long long base = (long long)blockIdx.z * a.N;
  const int* parent = a.parent + base;  // plain loads: the border kernel has ended
  const unsigned char* vg = a.val + (long long)b * 2 * a.N;
  const unsigned char* vp = vg + a.N;
  int* area = a.area + base;
  int* hit = a.hit + base;
  int* root_out = side == 0 ? a.root_g : a.root_p;
  if (root_out) root_out += (long long)b * a.N;
  const long long i0 = ((long long)blockIdx.x * THREADS + tid) * RUN;

  int carry_root = -1, prev_parent = -2, prev_root = -1;
  unsigned carry = 0u;
#pragma unroll 1
  for (int j = 0; j < RUN; ++j) {
    const long long i = i0 + j;
    const bool inside = i < a.N;
    const int par = inside ? parent[i] : -1;
    int root = -1;
    if ((unsigned)par < (unsigned)a.N) {  // (IGN pixels hold -1)
      if (par == prev_parent) {
        root = prev_root;
      } else {
        // Termination: parent[x] <= x, so x strictly decreases: at most N < cap steps; the cap and the range test turn a defect
        // into status[0].
        int x = par;
        bool ended = false;
        for (int n = 0; n < a.cap; ++n) {
          const int p = parent[x];
          if (p == x) {
            ended = true;
            break;
          }
          if ((unsigned)p >= (unsigned)a.N) break;
          x = p;
        }
        if (ended)
          root = x;
        else
          atomicOr(a.status, 1);
        prev_parent = par, prev_root = root;
      }
    }
    if (inside && root_out) root_out[i] = root;
    const bool flush = carry_root >= 0 && root != carry_root;
    wave_flush(flush, carry_root, carry, area, hit, lane);
    if (root != carry_root) carry_root = root, carry = 0u;
    if (root >= 0) carry += 0x10000u | (vg[i] == vp[i] ? 1u : 0u);
  }
  wave_flush(carry_root >= 0, carry_root, carry, area, hit, lane);
}

// ---- tally pass ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void objects_tally_kernel(ObjArgs a) {
  __shared__ unsigned cnt[32 * MAXS * DEC];
  __shared__ unsigned long long ms[32 * MAXS * 2];
  const int tid = threadIdx.x;
  const int n_cnt = a.K * a.S * DEC, n_ms = a.K * a.S * 2;
  for (int i = tid; i < n_cnt; i += THREADS) cnt[i] = 0u;
  for (int i = tid; i < n_ms; i += THREADS) ms[i] = 0ull;
  __syncthreads();
  const long long base = (long long)blockIdx.z * a.N;
  const long long i0 = ((long long)blockIdx.x * THREADS + tid) * RUN;
#pragma unroll 1
  for (int j = 0; j < RUN; ++j) {
    const long long i = i0 + j;
    if (i >= a.N) break;
    if (a.parent[base + i] != (int)i) continue;  // (IGN pixels hold -1)
    const long long ar = a.area[base + i], h = a.hit[base + i];
    const int c = a.val[base + i];
    if (ar < 1 || h < 0 || h > ar || c >= a.K) {  // (cannot be: a root counts itself)
      atomicOr(a.status, 1);
      continue;
    }
    int s = 0;
    for (int k = 0; k < a.S - 1; ++k) s += ar >= a.edge[k] ? 1 : 0;
    const int dj = (int)((10 * h) / ar);
    const int cell = c * a.S + s;
    atomicAdd(&cnt[cell * DEC + dj], 1u);
    atomicAdd(&ms[cell * 2 + 0], (unsigned long long)ar);
    if (h) atomicAdd(&ms[cell * 2 + 1], (unsigned long long)h);
  }
  __syncthreads();
  unsigned long long* obj = a.obj + (long long)blockIdx.z * n_cnt;  // (B, 2, K, S, 11): z = 2 b + side
  unsigned long long* mass = a.mass + (long long)blockIdx.z * n_ms;
  for (int i = tid; i < n_cnt; i += THREADS)
    if (cnt[i]) atomicAdd(obj + i, (unsigned long long)cnt[i]);
  for (int i = tid; i < n_ms; i += THREADS)
    if (ms[i]) atomicAdd(mass + i, ms[i]);
}

bool extents_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= SEGMIF_OBJECTS_MAX_FRAMES && (long long)H * W < (1ll << 31);
}

bool desc_ok(const SegmifObjects* d) {
  if ((d->connectivity != 4 && d->connectivity != 8) || d->n_edges < 0 || d->n_edges > SEGMIF_OBJECTS_MAX_EDGES) return false;
  long long last = 0;
  for (int k = 0; k < d->n_edges; ++k) {
    if (d->edges[k] <= last) return false;  // (below 1, or not strictly ascending)
    last = d->edges[k];
  }
  return true;
}

}  // namespace

extern "C" int64_t segmif_object_workspace_bytes(int B, int H, int W) {
  if (!extents_ok(B, H, W)) return 0;
  const int64_t bytes = (int64_t)B * H * W * SEGMIF_OBJECTS_WORKSPACE_PER_PIXEL;
  return (bytes + 7) / 8 * 8;
}

extern "C" int segmif_object_stats_i32(const SegmifObjects* desc, const int32_t* pred, const int64_t* label, int64_t* obj, int64_t* mass,
                                       int32_t* status, void* workspace, int32_t* root_g_or_null, int32_t* root_p_or_null, int B, int H,
                                       int W, int K, void* stream) {
  if (!desc || !pred || !label || !obj || !mass || !status || !workspace) return SEGMIF_EINVAL;
  if (K < 1 || K > 32 || !desc_ok(desc) || !extents_ok(B, H, W)) return SEGMIF_EINVAL;
  ObjArgs a;
  const long long N = (long long)H * W, all = N * 2 * B;
  a.pred = pred, a.label = (const long long*)label, a.obj = (unsigned long long*)obj, a.mass = (unsigned long long*)mass;
  a.status = status;
  a.parent = (int*)workspace, a.area = a.parent + all, a.hit = a.area + all, a.val = (unsigned char*)(a.hit + all);
  a.root_g = root_g_or_null, a.root_p = root_p_or_null;
  a.B = B, a.H = H, a.W = W, a.K = K, a.N = (int)N, a.tiles_x = (W + TILE - 1) / TILE;
  a.conn8 = desc->connectivity == 8, a.S = desc->n_edges + 1;
  a.cap = (int)(N < 0x7fffffffll ? N + 1 : N);  // H * W + 1 (one less at the very limit of int)
  for (int k = 0; k < MAXS; ++k) a.edge[k] = k < desc->n_edges ? desc->edges[k] : INT64_MAX;
  const long long tiles = (long long)a.tiles_x * ((H + TILE - 1) / TILE);
  const long long chunks = (N + THREADS * RUN - 1) / (THREADS * RUN);
  hipStream_t s = (hipStream_t)stream;
  const unsigned z = 2u * (unsigned)B;
  hipLaunchKernelGGL(objects_local_kernel, dim3((unsigned)tiles, 1, z), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(objects_border_kernel, dim3((unsigned)tiles, 1, z), dim3(BORDER_THREADS), 0, s, a);
  hipLaunchKernelGGL(objects_count_kernel, dim3((unsigned)chunks, 1, z), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(objects_tally_kernel, dim3((unsigned)chunks, 1, z), dim3(THREADS), 0, s, a);
  return (int)hipGetLastError();
}
