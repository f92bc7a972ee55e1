// Strong augmentation of the student's unlabelled batch in self-training (DAFormer's strong_transform: colour jitter, then a
// Gaussian blur), per sample from one 64-byte record.  The rule is stated in include/segmif_hip.h.  All float arithmetic is
// float32 without contraction (no fused multiply-add), so a product and a sum round as the rule writes them.
//
//   mean : grid (segmif_strong_augment_blocks(h, w), B) of 256 threads.  A block of a sample without jitter leaves at once (the
//          sample rides in blockIdx.y: the branch is uniform).  A thread walks groups of 4 pixels with a block-count stride, three
//          16-byte loads a group, brightness and luma pointwise, its sum in double; then a wave shuffle tree, the four wave sums
//          through LDS added in wave order, and one double per block.  No atomics: the same bits in every run.
//   apply: grid (tiles, B) of 256 threads, a tile of TILE_H x TILE_W outputs.  Every block adds the sample's partials in index order
//          (uniform addresses) to get m_b.  With an effective radius of 0 the tile is pointwise: 16-byte loads, the jitter (or,
//          for a copy sample, nothing: the bits pass through), 16-byte stores, no LDS and no barrier.  Otherwise the tile plus
//          `radius` rows above and below and HALO_X columns left and right (a fixed, 16-byte-aligned column halo; only the groups
//          a tap can reach are loaded) is staged into LDS, planar per channel, the jitter applied once per staged pixel, the
//          reflection resolved as the pixel is loaded.  Per channel the row pass writes a second LDS plane and the column pass
//          reads it with 16-byte LDS loads into registers and stores 16 bytes.  The radius loops are unrolled to MAX_RADIUS with
//          a uniform exit, so taps and sums stay in registers.
//   LDS  : 3 x 48 x 80 + 48 x 64 floats = 58,368 bytes: two workgroups fit a CU's 160 KiB at any radius.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_RADIUS = 8;
constexpr int TILE_H = SEGMIF_STRONG_TILE_H, TILE_W = SEGMIF_STRONG_TILE_W;
constexpr int HALO_X = 8;                      // columns staged left and right of a tile: >= MAX_RADIUS, a multiple of 4
constexpr int STAGE_H = TILE_H + 2 * MAX_RADIUS, STAGE_W = TILE_W + 2 * HALO_X;
constexpr int MAX_MEAN_BLOCKS = 32;            // partial sums per sample
constexpr int MEAN_GROUPS_PER_THREAD = 4;

typedef uint32_t Quad __attribute__((ext_vector_type(4)));  // four floats' bits
typedef float Float4 __attribute__((ext_vector_type(4)));

struct Rec {
  int jitter_on, radius;
  float fb, fc, fs, fh;
};

__device__ __forceinline__ Rec load_rec(const SegmifStrongAugRec* __restrict__ rec, int b, int h, int w) {
  const SegmifStrongAugRec* r = rec + b;
  Rec o;
  o.jitter_on = r->jitter_on;
  o.fb = r->fb, o.fc = r->fc, o.fs = r->fs, o.fh = r->fh;
  const int lim = min(MAX_RADIUS, min(h - 1, w - 1));
  const int rad = r->radius;
  o.radius = (rad < 0 || rad > lim) ? 0 : rad;  // never index by an unchecked radius
  return o;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float luma(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }
__device__ __forceinline__ float frac(float v) { return v - floorf(v); }

// brightness, contrast (k = (1 - fc) m_b), saturation, hue: the rule's steps 1-5 on one pixel
__device__ __forceinline__ void jitter(float& r, float& g, float& b, const Rec& p, float k, float one_minus_fs) {
  r = clamp01(p.fb * r), g = clamp01(p.fb * g), b = clamp01(p.fb * b);
  r = clamp01(p.fc * r + k), g = clamp01(p.fc * g + k), b = clamp01(p.fc * b + k);
  const float l = one_minus_fs * luma(r, g, b);
  r = clamp01(p.fs * r + l), g = clamp01(p.fs * g + l), b = clamp01(p.fs * b + l);
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const bool eq = mx == mn;
  const float cr = mx - mn;
  const float s = cr / (eq ? 1.0f : mx), d = eq ? 1.0f : cr;
  const float rc = (mx - r) / d, gc = (mx - g) / d, bc = (mx - b) / d;
  float hh = mx == r ? bc - gc : (mx == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
  hh = frac(hh / 6.0f + 1.0f);
  hh = frac(hh + p.fh);
  const float h6 = 6.0f * hh, fl = floorf(h6), f = h6 - fl;
  int i = (int)fl % 6;
  i = i < 0 ? i + 6 : i;
  const float V = mx;
  const float pp = clamp01(V * (1.0f - s)), q = clamp01(V * (1.0f - s * f)), t = clamp01(V * (1.0f - s * (1.0f - f)));
  r = i == 0 || i == 5 ? V : (i == 1 ? q : (i == 4 ? t : pp));
  g = i == 1 || i == 2 ? V : (i == 3 ? q : (i == 0 ? t : pp));
  b = i == 3 || i == 4 ? V : (i == 5 ? q : (i == 2 ? t : pp));
}

__global__ __launch_bounds__(THREADS) void strong_mean_kernel(const float* __restrict__ x, const SegmifStrongAugRec* __restrict__ rec,
                                                              double* __restrict__ partial, long long hw) {
  const int b = blockIdx.y;
  if (rec[b].jitter_on == 0) return;
  __shared__ double wave_sum[THREADS / 64];
  const float fb = rec[b].fb;
  const float* xr = x + (long long)b * 3 * hw;
  const long long groups = hw >> 2;
  double sum = 0.0;
  for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * THREADS) {
    const Float4 r = *reinterpret_cast<const Float4*>(xr + (g << 2));
    const Float4 gr = *reinterpret_cast<const Float4*>(xr + hw + (g << 2));
    const Float4 bl = *reinterpret_cast<const Float4*>(xr + 2 * hw + (g << 2));
#pragma unroll
    for (int t = 0; t < 4; ++t) sum += (double)luma(clamp01(fb * r[t]), clamp01(fb * gr[t]), clamp01(fb * bl[t]));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_down(sum, s, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = wave_sum[0];
#pragma unroll
    for (int i = 1; i < THREADS / 64; ++i) total += wave_sum[i];
    partial[(long long)b * gridDim.x + blockIdx.x] = total;
  }
}

// index -i -> i and n - 1 + i -> n - 1 - i; whatever lies further out (never needed by an output of the frame) is clamped
__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i > n - 1 ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(THREADS) void strong_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               const SegmifStrongAugRec* __restrict__ rec, const double* __restrict__ partial,
                                                               float* __restrict__ mean, int n_partial, int h, int w, int tiles_x) {
  __shared__ __attribute__((aligned(16))) float stage[3][STAGE_H][STAGE_W];
  __shared__ __attribute__((aligned(16))) float rows[STAGE_H][TILE_W];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Rec p = load_rec(rec, b, h, w);
  const long long hw = (long long)h * w;
  float m = 0.0f;
  if (p.jitter_on != 0) {
    double total = 0.0;
    for (int i = 0; i < n_partial; ++i) total += partial[(long long)b * n_partial + i];
    m = (float)(total / (double)hw);
  }
  if (blockIdx.x == 0 && tid == 0) mean[b] = m;
  const float k = (1.0f - p.fc) * m, one_minus_fs = 1.0f - p.fs;
  const int y0 = (int)(blockIdx.x / tiles_x) * TILE_H, x0 = (int)(blockIdx.x % tiles_x) * TILE_W;
  const float* xr = x + (long long)b * 3 * hw;
  float* yr = y + (long long)b * 3 * hw;
  const int R = p.radius;

  if (R == 0) {  // pointwise: no LDS, no barrier
    for (int q = tid; q < TILE_H * (TILE_W / 4); q += THREADS) {
      const int gy = y0 + q / (TILE_W / 4), gx = x0 + (q % (TILE_W / 4)) * 4;
      if (gy >= h || gx >= w) continue;
      const long long off = (long long)gy * w + gx;
      Quad c[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = *reinterpret_cast<const Quad*>(xr + ch * hw + off);
      if (p.jitter_on != 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float r = __uint_as_float(c[0][t]), g = __uint_as_float(c[1][t]), bl = __uint_as_float(c[2][t]);
          jitter(r, g, bl, p, k, one_minus_fs);
          c[0][t] = __float_as_uint(r), c[1][t] = __float_as_uint(g), c[2][t] = __float_as_uint(bl);
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<Quad*>(yr + ch * hw + off) = c[ch];
    }
    return;
  }

  float taps[MAX_RADIUS + 1];
#pragma unroll
  for (int i = 0; i <= MAX_RADIUS; ++i) taps[i] = rec[b].taps[i];

  // stage rows y0 - R .. y0 + TILE_H - 1 + R and the column groups a tap can reach, jittered, reflection resolved here
  const int stage_rows = TILE_H + 2 * R;
  const int q_lo = (HALO_X - R) >> 2, q_hi = (HALO_X + TILE_W + R + 3) >> 2, q_n = q_hi - q_lo;
  for (int q = tid; q < stage_rows * q_n; q += THREADS) {
    const int sy = q / q_n, sx = (q_lo + q % q_n) * 4;
    const int gy = reflect(y0 - R + sy, h), gx = x0 - HALO_X + sx;
    Float4 c[3];
    if (gx >= 0 && gx + 3 < w) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = *reinterpret_cast<const Float4*>(xr + ch * hw + (long long)gy * w + gx);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long off = (long long)gy * w + reflect(gx + t, w);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][t] = xr[ch * hw + off];
      }
    }
    if (p.jitter_on != 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float r = c[0][t], g = c[1][t], bl = c[2][t];
        jitter(r, g, bl, p, k, one_minus_fs);
        c[0][t] = r, c[1][t] = g, c[2][t] = bl;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<Float4*>(&stage[ch][sy][sx]) = c[ch];
  }
  __syncthreads();

  for (int ch = 0; ch < 3; ++ch) {
    // along the rows: staged row sy, output columns of the tile
    for (int q = tid; q < stage_rows * (TILE_W / 4); q += THREADS) {
      const int sy = q / (TILE_W / 4), ox = (q % (TILE_W / 4)) * 4;
      const float* s = &stage[ch][sy][HALO_X + ox];
      Float4 acc;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = taps[0] * s[t];
#pragma unroll
      for (int d = 1; d <= MAX_RADIUS; ++d) {
        if (d > R) break;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = acc[t] + taps[d] * (s[t - d] + s[t + d]);
      }
      *reinterpret_cast<Float4*>(&rows[sy][ox]) = acc;
    }
    __syncthreads();
    // along the columns, from LDS into registers, then 16-byte stores
    for (int q = tid; q < TILE_H * (TILE_W / 4); q += THREADS) {
      const int oy = q / (TILE_W / 4), ox = (q % (TILE_W / 4)) * 4;
      const int gy = y0 + oy, gx = x0 + ox;
      if (gy >= h || gx >= w) continue;
      const Float4 c = *reinterpret_cast<const Float4*>(&rows[oy + R][ox]);
      Float4 acc;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = taps[0] * c[t];
#pragma unroll
      for (int d = 1; d <= MAX_RADIUS; ++d) {
        if (d > R) break;
        const Float4 up = *reinterpret_cast<const Float4*>(&rows[oy + R - d][ox]);
        const Float4 dn = *reinterpret_cast<const Float4*>(&rows[oy + R + d][ox]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = acc[t] + taps[d] * (up[t] + dn[t]);
      }
      *reinterpret_cast<Float4*>(yr + ch * hw + (long long)gy * w + gx) = acc;
    }
    __syncthreads();  // `rows` is rewritten by the next channel
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

extern "C" int segmif_strong_augment_blocks(int h, int w) {
  if (h < 1 || w < 4 || w % 4) return SEGMIF_EINVAL;
  const long long groups = ((long long)h * w) >> 2, per_block = (long long)THREADS * MEAN_GROUPS_PER_THREAD;
  const long long blocks = (groups + per_block - 1) / per_block;
  return (int)(blocks > MAX_MEAN_BLOCKS ? MAX_MEAN_BLOCKS : blocks);
}

extern "C" int segmif_strong_augment_f32(const float* x, float* y, const SegmifStrongAugRec* rec, double* partial, float* mean, int B,
                                         int h, int w, void* stream) {
  if (!x || !y || !rec || !partial || !mean) return SEGMIF_EINVAL;
  if (B < 1 || B > 65535 || h < 1 || w < 4 || w % 4) return SEGMIF_EINVAL;  // (B is the grids' y extent)
  if (misaligned(x, 16) || misaligned(y, 16) || misaligned(partial, 8) || misaligned(rec, 4) || misaligned(mean, 4)) return SEGMIF_EINVAL;
  const int tiles_x = (w + TILE_W - 1) / TILE_W;
  const long long tiles = (long long)((h + TILE_H - 1) / TILE_H) * tiles_x;
  if (tiles > 0x7fffffffLL) return SEGMIF_EINVAL;
  const int n_partial = segmif_strong_augment_blocks(h, w);
  hipLaunchKernelGGL(strong_mean_kernel, dim3((unsigned)n_partial, (unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, x, rec, partial,
                     (long long)h * w);
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(strong_apply_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, x, y, rec, partial, mean,
                     n_partial, h, w, tiles_x);
  return (int)hipGetLastError();
}
