// Pseudo-labels of self-training (the EMA teacher of DAFormer, Hoyer et al. 2022; Tarvainen & Valpola's mean teacher): the
// teacher's quarter-resolution NHWC logits -> full-resolution labels, their confidence and the per-sample count of confident
// pixels in ONE pass.  The rule is stated in include/segmif_hip.h.  The sibling of bilinear_argmax_kernel (csrc/rowops.hip):
// like it, the (B, OH, OW, C) resized logits never exist.
//
// One thread per output pixel, grid (blocks of 256 columns, output row, image).  Two loops over the channels: the first is
// bilinear_argmax_kernel's (same interpolation expression, same comparison), the second forms the interpolation once more - the
// four source pixels are cache hits shared by the 16 output pixels of a x4 resize - and sums exp(v_c - v_max).  Nothing is kept in
// an indexed register array, so nothing spills to scratch.  The confident pixels are counted in integers: a ballot and a popcount
// per wave, one partial per wave in LDS, one 64-bit integer atomic per block.  Integer sums do not depend on their order: the
// count is exact and the same in every run.  No float atomics, no host synchronisation.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void pseudo_label_kernel(const float* __restrict__ x, long long* __restrict__ labels,
                                                               float* __restrict__ conf, unsigned long long* __restrict__ count,
                                                               int IH, int IW, int OH, int OW, int C, int ldx, float sy, float sx,
                                                               float tau, int below_ignore, int ignore_index) {
  __shared__ unsigned partial[THREADS / 64];
  const int ox = blockIdx.x * THREADS + threadIdx.x;
  const int oy = blockIdx.y;
  const long long b = blockIdx.z;
  bool confident = false;
  if (ox < OW) {
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = min(y0 + 1, IH - 1), x1 = min(x0 + 1, IW - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* base = x + b * IH * IW * ldx;
    const float* p00 = base + ((long long)y0 * IW + x0) * ldx;
    const float* p01 = base + ((long long)y0 * IW + x1) * ldx;
    const float* p10 = base + ((long long)y1 * IW + x0) * ldx;
    const float* p11 = base + ((long long)y1 * IW + x1) * ldx;
    // Channel 0 is written with the fused multiply-adds that the compiler forms for the peeled first channel of
    // bilinear_argmax_kernel (the loop's channels it contracts as a packed pair, in both kernels alike): the labels are that
    // kernel's on every pixel, ties included.
    float best = fmaf(hy, fmaf(hx, p00[0], lx * p01[0]), ly * fmaf(hx, p10[0], lx * p11[0]));
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float v = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
      if (v > best) {
        best = v;
        bi = c;
      }
    }
    // the maximum's own term is exp(0) = 1 exactly (NaN when the maximum is not finite), whatever the compiler makes of the second
    // evaluation: sum >= 1 and p_max <= 1 always
    float sum = expf(best - best);
    for (int c = 0; c < C; ++c) {
      const float v = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
      if (c != bi) sum += expf(v - best);
    }
    const float p_max = 1.f / sum;
    confident = p_max > tau;  // (false for a NaN)
    const long long o = (b * OH + oy) * OW + ox;
    labels[o] = (below_ignore && !confident) ? (long long)ignore_index : (long long)bi;
    if (conf) conf[o] = p_max;
  }
  const unsigned long long votes = __ballot(confident);
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = (unsigned)__popcll(votes);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned n = (partial[0] + partial[1]) + (partial[2] + partial[3]);
    if (n) atomicAdd(count + b, (unsigned long long)n);
  }
}

}  // namespace

extern "C" int segmif_pseudo_label_f32(const float* x, int64_t* labels, float* conf_or_null, int64_t* count, int B, int IH, int IW,
                                       int OH, int OW, int C, int ldx, float tau, int below_ignore, int ignore_index, void* stream) {
  if (!x || !labels || !count || B < 1 || IH < 1 || IW < 1 || OH < 1 || OW < 1 || C < 1 || C > 32 || ldx < C) return SEGMIF_EINVAL;
  if (B > 65535 || OH > 65535) return SEGMIF_EINVAL;  // (grid dimensions)
  if (!(tau >= 0.f && tau <= 1.f)) return SEGMIF_EINVAL;  // (NaN fails both comparisons)
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(count, 0, (size_t)B * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;  // (as segmif_bilinear_argmax_i32 forms them)
  const dim3 grid((unsigned)((OW + THREADS - 1) / THREADS), (unsigned)OH, (unsigned)B);
  hipLaunchKernelGGL(pseudo_label_kernel, grid, dim3(THREADS), 0, s, x, (long long*)labels, conf_or_null, (unsigned long long*)count,
                     IH, IW, OH, OW, C, ldx, sy, sx, tau, below_ignore, ignore_index);
  return (int)hipGetLastError();
}
