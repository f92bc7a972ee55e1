// Multi-scale + flip inference (the SegFormer evaluation protocol) combined on the device (gfx950, wave64):
//   tta_vote_kernel     labels = argmax_c mean_v softmax_c(flip_v?(bilinear(view_v -> OH x OW)))
//   resize_flip_kernel  a view's network input: flip?(bilinear(x -> OH x OW)) on NCHW planes, in one pass
// Both restate bilinear_kernel's coordinate arithmetic (csrc/rowops.hip: align_corners = False, scale = in / out in fp32,
// src = max(0, scale * (dst + 0.5) - 0.5)), as bilinear_argmax_kernel does.  A mirrored view is sampled at the mirrored
// column in its own frame - flip(interpolate(x))[ox] = interpolate(x)[OW - 1 - ox] - so no view is ever resized or flipped
// in memory: the V low-resolution logit maps are read with high locality and only the labels are written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int kMaxViews = 16;

struct TtaSrc {
  const float* x;
  int ih, iw, ldx, flip;
  float sy, sx;  // ih / OH, iw / OW (as segmif_bilinear_nhwc_f32 forms them)
};

// The whole table is a kernel argument (512 bytes of the kernarg segment): no device allocation and no copy per call, and the
// view loop reads it through scalar loads (v is wave-uniform).
struct TtaTable {
  TtaSrc v[kMaxViews];
};

// One thread per output pixel, 256 along x, one output row per block (bilinear_argmax_kernel's layout: the row terms are
// wave-uniform).  CMAX bounds C at compile time so that the per-class accumulators and the current view's resized logits are
// registers: every loop over classes is fully unrolled and guarded by the (uniform) c < C.  The views are summed in table order
// by the one thread that owns the pixel - no atomics, so the result is bitwise reproducible and does not depend on B.
template <int CMAX>
__global__ __launch_bounds__(256) void tta_vote_kernel(const TtaTable tab, int n_views, int32_t* __restrict__ labels,
                                                       float* __restrict__ probs, int OH, int OW, int C) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= OW) return;
  const int oy = blockIdx.y;
  const long long b = blockIdx.z;
  float acc[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
  for (int v = 0; v < n_views; ++v) {
    const TtaSrc s = tab.v[v];
    const int col = s.flip ? OW - 1 - ox : ox;
    const float fy = fmaxf(s.sy * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float fx = fmaxf(s.sx * ((float)col + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, s.ih - 1), x0 = min((int)fx, s.iw - 1);  // (the min never binds: fy < ih, fx < iw)
    const int y1 = min(y0 + 1, s.ih - 1), x1 = min(x0 + 1, s.iw - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* base = s.x + b * s.ih * s.iw * s.ldx;
    const float* p00 = base + ((long long)y0 * s.iw + x0) * s.ldx;
    const float* p01 = base + ((long long)y0 * s.iw + x1) * s.ldx;
    const float* p10 = base + ((long long)y1 * s.iw + x0) * s.ldx;
    const float* p11 = base + ((long long)y1 * s.iw + x1) * s.ldx;
    float r[CMAX];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        r[c] = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
        m = fmaxf(m, r[c]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        r[c] = expf(r[c] - m);
        sum += r[c];
      }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) acc[c] += r[c] / sum;
    }
  }
  const float nv = (float)n_views;
  const long long px = (b * OH + oy) * OW + ox;
  float best = acc[0] / nv;
  int bi = 0;
  if (probs) probs[px * C] = best;
#pragma unroll
  for (int c = 1; c < CMAX; ++c) {
    if (c < C) {
      const float p = acc[c] / nv;
      if (probs) probs[px * C + c] = p;
      if (p > best) {  // (ties -> lowest index, as argmax_kernel)
        best = p;
        bi = c;
      }
    }
  }
  labels[px] = bi;
}

__global__ __launch_bounds__(256) void resize_flip_kernel(const float* __restrict__ x, float* __restrict__ y, int IH, int IW, int OH,
                                                          int OW, int flip, float sy, float sx) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= OW) return;
  const int oy = blockIdx.y;
  const long long plane = blockIdx.z;
  const int col = flip ? OW - 1 - ox : ox;
  const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f);
  const float fx = fmaxf(sx * ((float)col + 0.5f) - 0.5f, 0.f);
  const int y0 = min((int)fy, IH - 1), x0 = min((int)fx, IW - 1);
  const int y1 = min(y0 + 1, IH - 1), x1 = min(x0 + 1, IW - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float* r0 = x + (plane * IH + y0) * IW;
  const float* r1 = x + (plane * IH + y1) * IW;
  y[(plane * OH + oy) * OW + ox] = hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]);
}

}  // namespace

extern "C" int segmif_tta_vote_f32(const SegmifTtaView* views, int n_views, int32_t* labels, float* probs_or_null, int B, int OH,
                                   int OW, int C, void* stream) {
  if (!views || !labels || n_views < 1 || n_views > kMaxViews || B <= 0 || OH <= 0 || OW <= 0 || C < 1 || C > 32) return SEGMIF_EINVAL;
  if (OH > 65535 || B > 65535) return SEGMIF_EINVAL;  // (grid y / z)
  TtaTable tab = {};
  for (int v = 0; v < n_views; ++v) {
    const SegmifTtaView& s = views[v];
    if (!s.x || s.ih <= 0 || s.iw <= 0 || s.ldx < C) return SEGMIF_EINVAL;
    tab.v[v] = TtaSrc{s.x, s.ih, s.iw, s.ldx, s.flip != 0, (float)s.ih / (float)OH, (float)s.iw / (float)OW};
  }
  const dim3 grid((unsigned)((OW + 255) / 256), (unsigned)OH, (unsigned)B);
  if (C <= 16)
    hipLaunchKernelGGL(tta_vote_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, tab, n_views, labels, probs_or_null, OH, OW, C);
  else
    hipLaunchKernelGGL(tta_vote_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, tab, n_views, labels, probs_or_null, OH, OW, C);
  return (int)hipGetLastError();
}

extern "C" int segmif_resize_flip_nchw_f32(const float* x, float* y, int planes, int IH, int IW, int OH, int OW, int flip,
                                           void* stream) {
  if (!x || !y || planes <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return SEGMIF_EINVAL;
  if (OH > 65535 || planes > 65535) return SEGMIF_EINVAL;  // (grid y / z)
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
  const dim3 grid((unsigned)((OW + 255) / 256), (unsigned)OH, (unsigned)planes);
  hipLaunchKernelGGL(resize_flip_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, IH, IW, OH, OW, flip != 0, sy, sx);
  return (int)hipGetLastError();
}
