// Contour statistics of two label maps (include/segmif_hip.h, segmif_boundary_stats_i32): per frame and class the sizes of
// the two boundary bands and of their intersection (Boundary IoU), of the two contours and of their matches within a
// tolerance (boundary F-score), and the confusion matrix restricted to the ground truth's band (trimap mIoU).  Exact
// integers, no floating point.
//
//   grid : one workgroup of 512 threads per 64 x 64 output tile of a frame; block = (frame, tile row, tile column).
//   LDS  : G and P, the two maps of the tile plus a halo of R = max(d, theta + 1), one byte per pixel: 0..31 a class, IGN,
//          OUT (outside the frame).  Bit 6 is set later where the pixel lies in its map's band, bit 7 where it is a contour
//          pixel.  The tile sits at (32, 32) of a 128 x 128 plane whatever R is; the row pitch is 132 bytes = 33 dwords,
//          so threads that walk one row each (the row pass) fall on different banks.
//   band : uniform_d is tested as run lengths.  Row pass: h(y, x) = m(y, x) if the run of equal values that ends at x + d is
//          at least 2 d + 1 long, else MIXED; one thread per (map, row, half row), 4 pixels per LDS read.  Column pass: the
//          same run test on h down a column, one thread per (map, column, 16 rows).  A window that leaves the frame meets an
//          OUT byte and is not uniform; nothing else is needed for the frame's border.
//   match: contour pixels are found with the 3 x 3 compare (OUT neighbours skipped), 4 pixels per item, flags held in a
//          register across a barrier and then written into bit 7.  One map's contour bits, 1 << class, are ORed along rows
//          over 2 theta + 1 positions into a plane of 32-bit words (it overlays the h planes); a contour pixel of the other
//          map then looks down its column for its own class's bit.  The plane is filled twice, once per direction.
//   count: a thread carries (table entry, count) over its 8 consecutive pixels and touches the workgroup's LDS table only
//          when the entry changes; every non-zero entry of the table then costs one 64-bit global atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int THREADS = 512;
constexpr int TILE = SEGMIF_BOUNDARY_TILE;
constexpr int MAXR = 32;                 // halo: max(d, theta + 1) <= 32
constexpr int EXT = TILE + 2 * MAXR;     // 128: side of the byte planes
constexpr int PITCH = EXT + 4;           // 33 dwords
constexpr int HP = TILE + 4;             // pitch of the h planes: 17 dwords
constexpr int MAXT = 31;                 // largest theta
constexpr int WROWS = TILE + 2 * MAXT;   // rows of the word plane
constexpr int MAXK = 32;
constexpr uint32_t IGN = 32, OUT = 33, MIXED = 34, VAL = 0x3f, BAND = 0x40, CONT = 0x80;

static_assert(TILE == 64 && THREADS == 8 * TILE, "the thread-to-pixel maps below are written for 64 x 64 tiles and 512 threads");
static_assert(2 * EXT * HP <= WROWS * TILE * 4, "the h planes overlay the word plane");
static_assert(WROWS * (EXT / 4) <= 8 * THREADS, "a thread keeps the contour flags of 8 items in one register");

struct alignas(16) Label2 { long long v[2]; };
struct alignas(16) Pred4 { int v[4]; };
struct alignas(16) Word4 { uint32_t v[4]; };

// (table entry, count) carried over a thread's consecutive pixels
struct Run {
  int key = -1;
  unsigned n = 0;
  __device__ __forceinline__ void add(unsigned* tab, int k) {
    if (k != key) {
      if (n) atomicAdd(tab + key, n);
      key = k;
      n = 0;
    }
    ++n;
  }
  __device__ __forceinline__ void flush(unsigned* tab) {
    if (n) atomicAdd(tab + key, n);
    n = 0;
  }
};

// bit e set iff pixel (ry, x0 + e) of M is a contour pixel and x0 + e lies in [xlo, xhi)
__device__ __forceinline__ uint32_t contour4(const uint8_t* M, int ry, int x0, int xlo, int xhi) {
  unsigned long long rows[3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const uint8_t* base = M + (ry + dy - 1) * PITCH;
    const unsigned long long mid = *reinterpret_cast<const uint32_t*>(base + x0);
    const unsigned long long l = x0 > 0 ? base[x0 - 1] : OUT;
    const unsigned long long r = x0 + 4 < EXT ? base[x0 + 4] : OUT;
    rows[dy] = (l | (mid << 8) | (r << 40)) & 0x3f3f3f3f3f3full;  // (the band bit may be set already)
  }
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t c = (uint32_t)(rows[1] >> (8 * (e + 1))) & 0xff;
    bool diff = false;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t nb = (uint32_t)(rows[dy] >> (8 * (e + k))) & 0xff;
        diff |= (nb != c) & (nb != OUT);
      }
    const int x = x0 + e;
    if (c < IGN && diff && x >= xlo && x < xhi) m |= 1u << e;
  }
  return m;
}

// Wd[r][j] = OR of 1 << class over the contour pixels of M in row 32 - theta + r, columns 32 + j - theta .. 32 + j + theta
__device__ __forceinline__ void row_or(const uint8_t* M, uint32_t* Wd, int theta, int tid) {
  const int ntask = (TILE + 2 * theta) * (TILE / 4);
  for (int t = tid; t < ntask; t += THREADS) {
    const int r = t >> 4, x0 = MAXR + 4 * (t & 15);
    const uint8_t* row = M + (MAXR - theta + r) * PITCH;
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    for (int x = (x0 - theta) & ~3; x <= x0 + 3 + theta; x += 4) {
      const uint32_t wv = *reinterpret_cast<const uint32_t*>(row + x);
      if (!(wv & 0x80808080u)) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t v = (wv >> (8 * e)) & 0xff;
        const uint32_t bit = (v & CONT) ? 1u << (v & 31) : 0u;
        const int rel = x + e - x0;
        if (rel >= -theta && rel <= theta) o0 |= bit;
        if (rel >= 1 - theta && rel <= 1 + theta) o1 |= bit;
        if (rel >= 2 - theta && rel <= 2 + theta) o2 |= bit;
        if (rel >= 3 - theta && rel <= 3 + theta) o3 |= bit;
      }
    }
    *reinterpret_cast<Word4*>(Wd + r * TILE + (x0 - MAXR)) = Word4{{o0, o1, o2, o3}};
  }
}

__global__ __launch_bounds__(THREADS) void boundary_stats_kernel(const int32_t* __restrict__ pred, const long long* __restrict__ label,
                                                                 int H, int W, int K, int d, int theta, int tiles_x, int tiles_y,
                                                                 unsigned long long* __restrict__ cls,
                                                                 unsigned long long* __restrict__ trimap) {
  __shared__ __align__(16) uint8_t G[EXT * PITCH];
  __shared__ __align__(16) uint8_t P[EXT * PITCH];
  __shared__ __align__(16) uint32_t Wd[WROWS * TILE];
  __shared__ unsigned tab[MAXK * 8 + MAXK * MAXK];
  uint8_t* hG = reinterpret_cast<uint8_t*>(Wd);
  uint8_t* hP = hG + EXT * HP;

  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int x0f = tx * TILE, y0f = ty * TILE;  // the tile's corner in the frame
  const int R = max(d, theta + 1);
  const int ncls = K * 8, nent = ncls + K * K;
  for (int i = tid; i < nent; i += THREADS) tab[i] = 0u;

  // ---- load: rows [32 - R, 96 + R), columns rounded out to dwords; labels narrowed after the 64-bit range test
  {
    const int c_lo = (MAXR - R) & ~3, c_hi = (MAXR + TILE + R + 3) & ~3;
    const int ngrp = (c_hi - c_lo) >> 2, nitem = (TILE + 2 * R) * ngrp;
    const long long fbase = (long long)b * H * W;
    for (int it = tid; it < nitem; it += THREADS) {
      const int r = it / ngrp, q = it - r * ngrp;
      const int ry = MAXR - R + r, cx = c_lo + 4 * q;
      const int gy = y0f + ry - MAXR, gx = x0f + cx - MAXR;
      uint32_t gw = OUT * 0x01010101u, pw = OUT * 0x01010101u;
      if (gy >= 0 && gy < H && gx + 3 >= 0 && gx < W) {
        long long l[4];
        int p[4];
        bool in[4];
        const long long idx = fbase + (long long)gy * W + gx;
        if (gx >= 0 && gx + 3 < W) {
          const long long* lp = label + idx;
          const int* pp = pred + idx;
          if ((reinterpret_cast<uintptr_t>(lp) & 15) == 0) {
            const Label2 a = *reinterpret_cast<const Label2*>(lp), c = *reinterpret_cast<const Label2*>(lp + 2);
            l[0] = a.v[0], l[1] = a.v[1], l[2] = c.v[0], l[3] = c.v[1];
          } else {
            const Label2 a = *reinterpret_cast<const Label2*>(lp + 1);
            l[0] = lp[0], l[1] = a.v[0], l[2] = a.v[1], l[3] = lp[3];
          }
          if ((reinterpret_cast<uintptr_t>(pp) & 15) == 0) {
            const Pred4 a = *reinterpret_cast<const Pred4*>(pp);
            p[0] = a.v[0], p[1] = a.v[1], p[2] = a.v[2], p[3] = a.v[3];
          } else {
            p[0] = pp[0], p[1] = pp[1], p[2] = pp[2], p[3] = pp[3];
          }
          in[0] = in[1] = in[2] = in[3] = true;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            in[e] = gx + e >= 0 && gx + e < W;
            l[e] = in[e] ? label[idx + e] : 0;
            p[e] = in[e] ? pred[idx + e] : 0;
          }
        }
        gw = pw = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool gok = l[e] >= 0 && l[e] < (long long)K;
          const uint32_t g = !in[e] ? OUT : gok ? (uint32_t)l[e] : IGN;
          const uint32_t pv = !in[e] ? OUT : (gok && p[e] >= 0 && p[e] < K) ? (uint32_t)p[e] : IGN;
          gw |= g << (8 * e);
          pw |= pv << (8 * e);
        }
      }
      *reinterpret_cast<uint32_t*>(G + ry * PITCH + cx) = gw;
      *reinterpret_cast<uint32_t*>(P + ry * PITCH + cx) = pw;
    }
  }
  __syncthreads();

  // ---- band, row pass: h rows 0 .. 63 + 2 d stand for plane rows 32 - d .. 95 + d; columns are the tile's
  {
    const int nh = TILE + 2 * d, need = 2 * d + 1;
    for (int t = tid; t < nh * 4; t += THREADS) {
      const int row = t % nh, q = t / nh, hf = q >> 1;
      const uint8_t* src = ((q & 1) ? P : G) + (MAXR - d + row) * PITCH;
      uint8_t* dst = ((q & 1) ? hP : hG) + row * HP;
      const int j0 = 32 * hf, xe = MAXR + j0 + 32 + d;
      uint32_t run = 0, prev = 0xffffffffu, acc = 0;
      for (int x = (MAXR + j0 - d) & ~3; x < xe; x += 4) {
        const uint32_t wv = *reinterpret_cast<const uint32_t*>(src + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t v = (wv >> (8 * e)) & 0xff;
          run = v == prev ? run + 1 : 1;
          prev = v;
          const int j = x + e - d - MAXR;
          if (j >= j0 && j < j0 + 32) {
            acc = (acc >> 8) | ((run >= (uint32_t)need ? v : MIXED) << 24);
            if ((j & 3) == 3) *reinterpret_cast<uint32_t*>(dst + j - 3) = acc;
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- band, column pass: bit 6 of a tile pixel with a class is set iff its window is not uniform
  {
    const int j = tid & 63, s = (tid >> 6) & 3, need = 2 * d + 1;
    const uint8_t* hp = ((tid >> 8) ? hP : hG) + j;
    uint8_t* m = ((tid >> 8) ? P : G) + MAXR + j;
    uint32_t run = 0, prev = 0xffffffffu;
    for (int hr = 16 * s; hr <= 16 * s + 15 + 2 * d; ++hr) {
      const uint32_t v = hp[hr * HP];
      run = v == prev ? run + 1 : 1;
      prev = v;
      const int yo = hr - 2 * d;
      if (yo >= 16 * s && !(run >= (uint32_t)need && v != MIXED)) {
        uint8_t* px = m + (MAXR + yo) * PITCH;
        const uint32_t c = *px;
        if (c < IGN) *px = (uint8_t)(c | BAND);
      }
    }
  }
  __syncthreads();  // (the h planes are dead from here on: Wd may be written)

  // this thread's 8 pixels of the tile in the counting passes
  const int prow = tid >> 3, pcol = (tid & 7) * 8;
  const uint8_t* gpx = G + (MAXR + prow) * PITCH + MAXR + pcol;
  const uint8_t* ppx = P + (MAXR + prow) * PITCH + MAXR + pcol;

  // ---- band counts; contour flags of [32 - theta, 96 + theta)^2 into registers (both only read the planes)
  {
    Run a, bb, c, t;
    const uint32_t g2[2] = {*reinterpret_cast<const uint32_t*>(gpx), *reinterpret_cast<const uint32_t*>(gpx + 4)};
    const uint32_t p2[2] = {*reinterpret_cast<const uint32_t*>(ppx), *reinterpret_cast<const uint32_t*>(ppx + 4)};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t g = (g2[e >> 2] >> (8 * (e & 3))) & 0xff, p = (p2[e >> 2] >> (8 * (e & 3))) & 0xff;
      const int gv = g & VAL, pv = p & VAL;
      if (g & BAND) a.add(tab, gv * 8 + 0);
      if (p & BAND) bb.add(tab, pv * 8 + 1);
      if ((g & p & BAND) && gv == pv) c.add(tab, gv * 8 + 2);
      if ((g & BAND) && pv < (int)IGN) t.add(tab, ncls + gv * K + pv);
    }
    a.flush(tab), bb.flush(tab), c.flush(tab), t.flush(tab);
  }
  const int clo = MAXR - theta, chi = MAXR + TILE + theta;
  const int g_lo = clo >> 2, ng = ((chi + 3) >> 2) - g_lo, ncont = (TILE + 2 * theta) * ng;
  uint32_t fg = 0, fp = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int t = tid + i * THREADS;
    if (t < ncont) {
      const int r = t / ng, q = t - r * ng;
      fg |= contour4(G, clo + r, 4 * (g_lo + q), clo, chi) << (4 * i);
      fp |= contour4(P, clo + r, 4 * (g_lo + q), clo, chi) << (4 * i);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int t = tid + i * THREADS;
    if (t < ncont && (((fg | fp) >> (4 * i)) & 15)) {
      const int r = t / ng, q = t - r * ng;
      uint8_t* gq = G + (clo + r) * PITCH + 4 * (g_lo + q);
      uint8_t* pq = P + (clo + r) * PITCH + 4 * (g_lo + q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((fg >> (4 * i + e)) & 1) gq[e] |= (uint8_t)CONT;
        if ((fp >> (4 * i + e)) & 1) pq[e] |= (uint8_t)CONT;
      }
    }
  }
  __syncthreads();

  // ---- contour counts and matches: the prediction's contour bits spread along rows, ground-truth pixels look down columns
  row_or(P, Wd, theta, tid);
  __syncthreads();
  {
    Run n, m, np;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t g = gpx[e], p = ppx[e];
      if (p & CONT) np.add(tab, (int)(p & VAL) * 8 + 4);
      if (g & CONT) {
        const int gv = g & VAL;
        n.add(tab, gv * 8 + 3);
        const uint32_t* w = Wd + prow * TILE + pcol + e;
        bool hit = false;
        for (int r = 0; r <= 2 * theta && !hit; ++r) hit = (w[r * TILE] >> gv) & 1u;
        if (hit) m.add(tab, gv * 8 + 5);
      }
    }
    n.flush(tab), m.flush(tab), np.flush(tab);
  }
  __syncthreads();
  row_or(G, Wd, theta, tid);
  __syncthreads();
  {
    Run m;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t p = ppx[e];
      if (p & CONT) {
        const int pv = p & VAL;
        const uint32_t* w = Wd + prow * TILE + pcol + e;
        bool hit = false;
        for (int r = 0; r <= 2 * theta && !hit; ++r) hit = (w[r * TILE] >> pv) & 1u;
        if (hit) m.add(tab, pv * 8 + 6);
      }
    }
    m.flush(tab);
  }
  __syncthreads();
  for (int i = tid; i < nent; i += THREADS) {
    const unsigned v = tab[i];
    if (v) atomicAdd(i < ncls ? cls + (long long)b * ncls + i : trimap + (long long)b * K * K + (i - ncls), (unsigned long long)v);
  }
}

}  // namespace

extern "C" int segmif_boundary_stats_i32(const int32_t* pred, const int64_t* label, int B, int H, int W, int K, int d, int theta,
                                         int64_t* cls, int64_t* trimap, void* stream) {
  if (!pred || !label || !cls || !trimap || B < 1 || H < 1 || W < 1) return SEGMIF_EINVAL;
  if (K < 1 || K > MAXK || d < 1 || d > MAXR || theta < 0 || theta > MAXT) return SEGMIF_EINVAL;
  if (reinterpret_cast<uintptr_t>(cls) % 8 || reinterpret_cast<uintptr_t>(trimap) % 8) return SEGMIF_EINVAL;
  if (reinterpret_cast<uintptr_t>(label) % 8 || reinterpret_cast<uintptr_t>(pred) % 4) return SEGMIF_EINVAL;
  const long long tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
  const long long blocks = tiles_x * tiles_y * B;
  if (blocks > 0x7fffffffll) return SEGMIF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(cls, 0, (size_t)B * K * 8 * sizeof(int64_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(trimap, 0, (size_t)B * K * K * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(boundary_stats_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, pred, reinterpret_cast<const long long*>(label),
                     H, W, K, d, theta, (int)tiles_x, (int)tiles_y, reinterpret_cast<unsigned long long*>(cls),
                     reinterpret_cast<unsigned long long*>(trimap));
  return (int)hipGetLastError();
}
