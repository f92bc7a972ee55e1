// The fusion objectives of core/loss.py (:386-397 new_loss_sobel, :423-457, :479-505, :518-603) as one table-driven kernel pair.
// Single-channel float32 planes (planes, H, W): gen, ir, vis (the Y plane) and mask ((planes, mask_planes, H, W)).  A descriptor
// holds up to 8 terms
//     s_k = sum over pixels of rho( w * (L(gen) - t) )
//   L    identity | Sobelxy = |gx| + |gy| (zero padding, the stencils of core/loss.py:634-650)
//   t    L(a_ir ir + a_vis vis + a_mask mask_0)  |  max(L(ir), L(vis))
//   w    1 | mask_c | |1 - mask_c|, summed over the term's mask_channels planes c (torch's broadcast of (B,3,H,W) * (B,1,H,W))
//   rho  |.| | (.)^2
// Forward: one launch forms all s_k - the four planes go through an LDS tile with a 1-pixel halo (zero at a plane's edge, never
// the neighbouring image), rows by 16-byte loads where the row start allows; per-wave width-64 shuffle reduction, per-block
// double partials, then one fixed-order sum.  No floating-point atomics.
// Backward: one launch forms grad = sum_k coef[k] ds_k/dgen, recomputed from the inputs (2-pixel halo): phase one leaves the two
// planes  sum coef rho' sign(gx), sum coef rho' sign(gy)  over the tile + 1 pixel in LDS, phase two applies the adjoint Sobel
// stencils and adds the identity terms.  sign(0) = 0.  ir, vis and mask are data.
// Sobelxy of a linear target is formed as the same linear combination of the planes' gx / gy (the stencils are linear).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int TH = 16, TW = 64;      // pixels of a tile: 256 threads x 4 consecutive pixels of one row
constexpr int PITCH = 72, XOFF = 4;  // LDS row: tile column c at XOFF + c (c = -2 .. TW + 1), so the interior is 16-byte aligned
constexpr int MAXT = SEGMIF_OBJ_MAX_TERMS;

// a term as the kernels carry it (four scalar registers): the enums and mask_channels of a checked SegmifObjTerm in one word
struct Term {
  int code;  // op | target << 1 | weight << 2 | rho << 4 | mask_channels << 5
  float a_ir, a_vis, a_mask;
  __device__ __forceinline__ int op() const { return code & 1; }
  __device__ __forceinline__ int target() const { return (code >> 1) & 1; }
  __device__ __forceinline__ int weight() const { return (code >> 2) & 3; }
  __device__ __forceinline__ int rho() const { return (code >> 4) & 1; }
  __device__ __forceinline__ int mask_channels() const { return code >> 5; }
};

struct ObjArgs {
  const float *gen, *ir, *vis, *mask;  // ir / vis / mask: NULL when no term reads them (their tile is zeros)
  int H, W, mask_planes, vec, n_terms;
  Term term[MAXT];
};

__device__ __forceinline__ float sgn(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

// rows y0 - HALO .. y0 + TH + HALO - 1, columns x0 - HALO .. x0 + TW + HALO - 1 of plane p (zero outside the plane) -> t
template <int HALO>
__device__ __forceinline__ void load_tile(float* __restrict__ t, const float* __restrict__ p, int H, int W, int y0, int x0, int vec) {
  constexpr int ROWS = TH + 2 * HALO;
  if (vec) {  // W % 4 == 0 and 16-byte aligned planes: a group of four columns is inside the row or outside it
    for (int i = threadIdx.x; i < ROWS * (TW / 4); i += 256) {
      const int r = i / (TW / 4), c = (i % (TW / 4)) * 4;
      const int y = y0 - HALO + r, x = x0 + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p && (unsigned)y < (unsigned)H && x < W) v = *reinterpret_cast<const float4*>(p + (long long)y * W + x);
      *reinterpret_cast<float4*>(t + r * PITCH + XOFF + c) = v;
    }
    for (int i = threadIdx.x; i < ROWS * 2 * HALO; i += 256) {
      const int r = i / (2 * HALO), h = i % (2 * HALO);
      const int c = h < HALO ? h - HALO : TW + h - HALO;
      const int y = y0 - HALO + r, x = x0 + c;
      t[r * PITCH + XOFF + c] = (p && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? p[(long long)y * W + x] : 0.f;
    }
  } else {
    constexpr int COLS = TW + 2 * HALO;
    for (int i = threadIdx.x; i < ROWS * COLS; i += 256) {
      const int r = i / COLS, c = i % COLS - HALO;
      const int y = y0 - HALO + r, x = x0 + c;
      t[r * PITCH + XOFF + c] = (p && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? p[(long long)y * W + x] : 0.f;
    }
  }
}

// kernelx = [[-1,0,1],[-2,0,2],[-1,0,1]], kernely = [[1,2,1],[0,0,0],[-1,-2,-1]] (cross-correlation) on a 3 x 3 window
__device__ __forceinline__ void stencil(float a, float b, float c, float d, float f, float g, float h, float k, float& gx, float& gy) {
  gx = (c + 2.f * f + k) - (a + 2.f * d + g);
  gy = (a + 2.f * b + c) - (g + 2.f * h + k);
}

// four consecutive pixels starting at the 16-byte aligned LDS address c: values, gx, gy
__device__ __forceinline__ void window4(const float* c, float (&v)[4], float (&gx)[4], float (&gy)[4]) {
  float w[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float* p = c + (r - 1) * PITCH;
    const float4 m = *reinterpret_cast<const float4*>(p);
    w[r][0] = p[-1], w[r][1] = m.x, w[r][2] = m.y, w[r][3] = m.z, w[r][4] = m.w, w[r][5] = p[4];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    stencil(w[0][j], w[0][j + 1], w[0][j + 2], w[1][j], w[1][j + 2], w[2][j], w[2][j + 1], w[2][j + 2], gx[j], gy[j]);
    v[j] = w[1][j + 1];
  }
}

__device__ __forceinline__ void window1(const float* c, float& v, float& gx, float& gy) {
  stencil(c[-PITCH - 1], c[-PITCH], c[-PITCH + 1], c[-1], c[1], c[PITCH - 1], c[PITCH], c[PITCH + 1], gx, gy);
  v = c[0];
}

struct Pixel {  // one pixel of the four planes: value, gx, gy
  float g, i, v, m, gxg, gyg, gxi, gyi, gxv, gyv, gxm, gym;
};

// L(gen) - t of one term
__device__ __forceinline__ float residual(const Term& T, const Pixel& p) {
  if (T.op() == SEGMIF_OBJ_IDENTITY) {
    const float t = T.target() == SEGMIF_OBJ_TARGET_MAX ? fmaxf(p.i, p.v) : T.a_ir * p.i + T.a_vis * p.v + T.a_mask * p.m;
    return p.g - t;
  }
  float t;
  if (T.target() == SEGMIF_OBJ_TARGET_MAX) {
    t = fmaxf(fabsf(p.gxi) + fabsf(p.gyi), fabsf(p.gxv) + fabsf(p.gyv));
  } else {
    t = fabsf(T.a_ir * p.gxi + T.a_vis * p.gxv + T.a_mask * p.gxm) + fabsf(T.a_ir * p.gyi + T.a_vis * p.gyv + T.a_mask * p.gym);
  }
  return (fabsf(p.gxg) + fabsf(p.gyg)) - t;
}

// mext: this pixel in mask plane 0 of its image (global memory; planes c >= 1 are read there, plane 0 is p.m), hw = H * W
__device__ __forceinline__ float mask_weight(const Term& T, const Pixel& p, const float* __restrict__ mext, long long hw, int c) {
  const float m = c == 0 ? p.m : mext[c * hw];
  return T.weight() == SEGMIF_OBJ_WEIGHT_MASK ? m : fabsf(1.f - m);
}

// rho(w e) summed over the term's weights
__device__ __forceinline__ float term_value(const Term& T, const Pixel& p, const float* __restrict__ mext, long long hw) {
  const float e = residual(T, p);
  if (T.weight() == SEGMIF_OBJ_WEIGHT_ONE) return T.rho() == SEGMIF_OBJ_RHO_ABS ? fabsf(e) : e * e;
  float s = 0.f;
  for (int c = 0; c < T.mask_channels(); ++c) {
    const float u = mask_weight(T, p, mext, hw, c) * e;
    s += T.rho() == SEGMIF_OBJ_RHO_ABS ? fabsf(u) : u * u;
  }
  return s;
}

// d/dL(gen) of the same:  |.|: sign(e) sum |w|;  (.)^2: 2 e sum w^2
__device__ __forceinline__ float term_slope(const Term& T, const Pixel& p, const float* __restrict__ mext, long long hw) {
  const float e = residual(T, p);
  float s = 1.f;
  if (T.weight() != SEGMIF_OBJ_WEIGHT_ONE) {
    s = 0.f;
    for (int c = 0; c < T.mask_channels(); ++c) {
      const float w = mask_weight(T, p, mext, hw, c);
      s += T.rho() == SEGMIF_OBJ_RHO_ABS ? fabsf(w) : w * w;
    }
  }
  return T.rho() == SEGMIF_OBJ_RHO_ABS ? sgn(e) * s : 2.f * e * s;
}

// partial[blk][k] = this tile's share of s_k
__global__ __launch_bounds__(256) void objective_fwd_kernel(ObjArgs a, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tile[4][(TH + 2) * PITCH];
  __shared__ double wsum[4][MAXT];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const long long hw = (long long)a.H * a.W, img = blockIdx.z;
  load_tile<1>(tile[0], a.gen + img * hw, a.H, a.W, y0, x0, a.vec);
  load_tile<1>(tile[1], a.ir ? a.ir + img * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  load_tile<1>(tile[2], a.vis ? a.vis + img * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  load_tile<1>(tile[3], a.mask ? a.mask + img * a.mask_planes * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = (threadIdx.x & 15) * 4;
  const int y = y0 + ty, x = x0 + tx;
  float v[4][4], gx[4][4], gy[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) window4(tile[q] + (ty + 1) * PITCH + XOFF + tx, v[q], gx[q], gy[q]);
  float acc[MAXT];
#pragma unroll
  for (int k = 0; k < MAXT; ++k) acc[k] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (y < a.H && x + j < a.W) {
      const Pixel p = {v[0][j], v[1][j], v[2][j], v[3][j], gx[0][j], gy[0][j], gx[1][j], gy[1][j], gx[2][j], gy[2][j], gx[3][j], gy[3][j]};
      const float* mext = a.mask ? a.mask + img * a.mask_planes * hw + (long long)y * a.W + (x + j) : nullptr;
#pragma unroll
      for (int k = 0; k < MAXT; ++k)
        if (k < a.n_terms) acc[k] += term_value(a.term[k], p, mext, hw);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MAXT; ++k) {
    double s = (double)acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) wsum[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < MAXT) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[blk * MAXT + threadIdx.x] = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
  }
}

// sums[k] = the partials of term k in a fixed order: 32 strided runs, then a width-32 shuffle tree
__global__ __launch_bounds__(256) void objective_sum_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ sums) {
  const int k = threadIdx.x >> 5, l = threadIdx.x & 31;
  double s = 0.0;
  for (int b = l; b < nblk; b += 32) s += partial[(long long)b * MAXT + k];
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) s += __shfl_down(s, off, 32);
  if (l == 0) sums[k] = s;
}

__global__ __launch_bounds__(256) void objective_bwd_kernel(ObjArgs a, const float* __restrict__ coef, float* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) float tile[4][(TH + 4) * PITCH];
  __shared__ __attribute__((aligned(16))) float pxy[2][(TH + 2) * PITCH];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const long long hw = (long long)a.H * a.W, img = blockIdx.z;
  load_tile<2>(tile[0], a.gen + img * hw, a.H, a.W, y0, x0, a.vec);
  load_tile<2>(tile[1], a.ir ? a.ir + img * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  load_tile<2>(tile[2], a.vis ? a.vis + img * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  load_tile<2>(tile[3], a.mask ? a.mask + img * a.mask_planes * hw : nullptr, a.H, a.W, y0, x0, a.vec);
  const float* mimg = a.mask ? a.mask + img * a.mask_planes * hw : nullptr;
  __syncthreads();
  // phase one: rows y0 - 1 .. y0 + TH, columns x0 - 1 .. x0 + TW of the two planes (zero outside the image: no Sobel output there)
  for (int i = threadIdx.x; i < (TH + 2) * (TW + 2); i += 256) {
    const int r = i / (TW + 2), c = i % (TW + 2) - 1;
    const int y = y0 - 1 + r, x = x0 + c;
    float px = 0.f, py = 0.f;
    if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
      const int o = (r + 1) * PITCH + XOFF + c;
      Pixel p;
      window1(tile[0] + o, p.g, p.gxg, p.gyg);
      window1(tile[1] + o, p.i, p.gxi, p.gyi);
      window1(tile[2] + o, p.v, p.gxv, p.gyv);
      window1(tile[3] + o, p.m, p.gxm, p.gym);
      const float* mext = mimg ? mimg + (long long)y * a.W + x : nullptr;
      float s = 0.f;
#pragma unroll 1  // (a rolled loop: unrolled, the decoded terms of all eight iterations are hoisted into scalar registers and spill)
      for (int k = 0; k < a.n_terms; ++k)
        if (a.term[k].op() == SEGMIF_OBJ_SOBEL) s += coef[k] * term_slope(a.term[k], p, mext, hw);
      px = s * sgn(p.gxg);
      py = s * sgn(p.gyg);
    }
    pxy[0][r * PITCH + XOFF + c] = px;
    pxy[1][r * PITCH + XOFF + c] = py;
  }
  __syncthreads();
  // phase two: in(y, x) receives k[dy][dx] p(y - dy, x - dx) (the adjoint of the two correlations), plus the identity terms
  const int ty = threadIdx.x >> 4, tx = (threadIdx.x & 15) * 4;
  const int y = y0 + ty, x = x0 + tx;
  if (y >= a.H || x >= a.W) return;
  float wx[3][6], wy[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float* p = pxy[0] + (ty + r) * PITCH + XOFF + tx;
    const float* q = pxy[1] + (ty + r) * PITCH + XOFF + tx;
    const float4 m = *reinterpret_cast<const float4*>(p), n = *reinterpret_cast<const float4*>(q);
    wx[r][0] = p[-1], wx[r][1] = m.x, wx[r][2] = m.y, wx[r][3] = m.z, wx[r][4] = m.w, wx[r][5] = p[4];
    wy[r][0] = q[-1], wy[r][1] = n.x, wy[r][2] = n.y, wy[r][3] = n.z, wy[r][4] = n.w, wy[r][5] = q[4];
  }
  float ctr[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 m = *reinterpret_cast<const float4*>(tile[q] + (ty + 2) * PITCH + XOFF + tx);
    ctr[q][0] = m.x, ctr[q][1] = m.y, ctr[q][2] = m.z, ctr[q][3] = m.w;
  }
  float out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // window rows 0 / 1 / 2 = y - 1 / y / y + 1, columns j / j + 1 / j + 2 = x - 1 / x / x + 1
    float g = (wx[2][j] - wx[2][j + 2]) + 2.f * (wx[1][j] - wx[1][j + 2]) + (wx[0][j] - wx[0][j + 2]);
    g += (wy[2][j] + 2.f * wy[2][j + 1] + wy[2][j + 2]) - (wy[0][j] + 2.f * wy[0][j + 1] + wy[0][j + 2]);
    if (x + j < a.W) {
      Pixel p = {};
      p.g = ctr[0][j], p.i = ctr[1][j], p.v = ctr[2][j], p.m = ctr[3][j];
      const float* mext = mimg ? mimg + (long long)y * a.W + (x + j) : nullptr;
#pragma unroll 1
      for (int k = 0; k < a.n_terms; ++k)
        if (a.term[k].op() == SEGMIF_OBJ_IDENTITY) g += coef[k] * term_slope(a.term[k], p, mext, hw);
    }
    out[j] = g;
  }
  float* gp = grad + img * hw + (long long)y * a.W + x;
  if (a.vec) {
    *reinterpret_cast<float4*>(gp) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < a.W) gp[j] = out[j];
  }
}

bool aligned16(const void* p) { return !((uintptr_t)p & 15); }

// fills the kernel arguments; false: the descriptor or the geometry is refused
bool make_args(const SegmifFusionObjective* d, const float* gen, const float* ir, const float* vis, const float* mask, int mask_planes,
               int planes, int H, int W, ObjArgs& a) {
  if (!d || !gen || planes <= 0 || H <= 0 || W <= 0 || planes > 65535 || (H + TH - 1) / TH > 65535) return false;
  if (d->n_terms < 1 || d->n_terms > MAXT) return false;
  bool use_ir = false, use_vis = false, use_mask = false;
  for (int k = 0; k < d->n_terms; ++k) {
    const SegmifObjTerm& T = d->term[k];
    if (T.op != SEGMIF_OBJ_IDENTITY && T.op != SEGMIF_OBJ_SOBEL) return false;
    if (T.target != SEGMIF_OBJ_TARGET_LINEAR && T.target != SEGMIF_OBJ_TARGET_MAX) return false;
    if (T.weight != SEGMIF_OBJ_WEIGHT_ONE && T.weight != SEGMIF_OBJ_WEIGHT_MASK && T.weight != SEGMIF_OBJ_WEIGHT_INV_MASK) return false;
    if (T.rho != SEGMIF_OBJ_RHO_ABS && T.rho != SEGMIF_OBJ_RHO_SQUARE) return false;
    if (T.mask_channels < 1 || T.mask_channels > 4) return false;
    if (T.target == SEGMIF_OBJ_TARGET_MAX) {
      use_ir = use_vis = true;
    } else {
      use_ir |= T.a_ir != 0.f;
      use_vis |= T.a_vis != 0.f;
      use_mask |= T.a_mask != 0.f;
    }
    if (T.weight != SEGMIF_OBJ_WEIGHT_ONE) {
      use_mask = true;
      if (T.mask_channels > mask_planes) return false;
    }
  }
  if ((use_ir && !ir) || (use_vis && !vis) || (use_mask && (!mask || mask_planes < 1 || mask_planes > 4))) return false;
  a.gen = gen;
  a.ir = use_ir ? ir : nullptr;
  a.vis = use_vis ? vis : nullptr;
  a.mask = use_mask ? mask : nullptr;
  a.H = H, a.W = W;
  a.mask_planes = use_mask ? mask_planes : 1;
  a.vec = !(W & 3) && aligned16(gen) && aligned16(a.ir) && aligned16(a.vis) && aligned16(a.mask);
  a.n_terms = d->n_terms;
  for (int k = 0; k < MAXT; ++k) {
    const SegmifObjTerm& T = d->term[k < d->n_terms ? k : 0];
    a.term[k] = Term{T.op | T.target << 1 | T.weight << 2 | T.rho << 4 | T.mask_channels << 5, T.a_ir, T.a_vis, T.a_mask};
  }
  return true;
}

dim3 tiles(int planes, int H, int W) { return dim3((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)planes); }

}  // namespace

extern "C" int segmif_fusion_objective_blocks(int planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0) return 0;
  const long long n = (long long)((W + TW - 1) / TW) * ((H + TH - 1) / TH) * planes;
  return n > 0x7fffffffLL ? 0 : (int)n;
}

extern "C" int segmif_fusion_objective_f32(const SegmifFusionObjective* desc, const float* gen, const float* ir, const float* vis,
                                           const float* mask, int mask_planes, double* partial, double* sums8, int planes, int H,
                                           int W, void* stream) {
  ObjArgs a;
  if (!partial || !sums8 || !make_args(desc, gen, ir, vis, mask, mask_planes, planes, H, W, a)) return SEGMIF_EINVAL;
  const int nblk = segmif_fusion_objective_blocks(planes, H, W);
  if (nblk <= 0) return SEGMIF_EINVAL;
  hipLaunchKernelGGL(objective_fwd_kernel, tiles(planes, H, W), dim3(256), 0, (hipStream_t)stream, a, partial);
  hipLaunchKernelGGL(objective_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblk, sums8);
  return (int)hipGetLastError();
}

extern "C" int segmif_fusion_objective_bwd_f32(const SegmifFusionObjective* desc, const float* gen, const float* ir, const float* vis,
                                               const float* mask, int mask_planes, const float* coef8, float* grad, int planes,
                                               int H, int W, void* stream) {
  ObjArgs a;
  if (!coef8 || !grad || !make_args(desc, gen, ir, vis, mask, mask_planes, planes, H, W, a)) return SEGMIF_EINVAL;
  if (segmif_fusion_objective_blocks(planes, H, W) <= 0) return SEGMIF_EINVAL;
  a.vec = a.vec && aligned16(grad);
  hipLaunchKernelGGL(objective_bwd_kernel, tiles(planes, H, W), dim3(256), 0, (hipStream_t)stream, a, coef8, grad);
  return (int)hipGetLastError();
}
