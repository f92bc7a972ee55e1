// Private to segmif_amd/csrc: how the objectives over NHWC logits (seg_objective.hip, region_objective.hip) bring a block of 256
// rows (rows x C, C <= 32, pitch ld) through LDS, one row per thread, and take a block of gradient rows back out the same way.
// 16-byte accesses when the pitch equals C and the base is 16-byte aligned (a row of C = 9 is 36 bytes: per-thread row accesses
// would not coalesce), scalar ones otherwise.  Each .hip file that includes this gets functions of its own (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace segmif {
namespace {

constexpr int ROWS = 256;  // rows of a block: one per thread
constexpr int PITCH = 33;  // LDS row pitch in floats (odd: a wave's rows fall into distinct banks)

// the block's rows r0 .. r0 + nr - 1 -> tile[row * PITCH + c]
__device__ __forceinline__ void stage_rows(float* __restrict__ tile, const float* __restrict__ x, long long r0, int nr, int C, int ld,
                                           int vec) {
  const int n = nr * C;
  if (vec) {  // ld == C, 16-byte aligned base: the block's floats are one aligned run (r0 * C * 4 bytes is a multiple of 16)
    const float* base = x + r0 * C;
    for (int i = threadIdx.x; i < n / 4; i += ROWS) {
      const float4 v = reinterpret_cast<const float4*>(base)[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * i + j;
        tile[(f / C) * PITCH + f % C] = e[j];
      }
    }
    for (int f = (n / 4) * 4 + threadIdx.x; f < n; f += ROWS) tile[(f / C) * PITCH + f % C] = base[f];
  } else {
    for (int f = threadIdx.x; f < n; f += ROWS) {
      const int r = f / C, c = f % C;
      tile[r * PITCH + c] = x[(r0 + r) * ld + c];
    }
  }
}

// the same way back: tile -> g (pitch ldd)
__device__ __forceinline__ void unstage_rows(const float* __restrict__ tile, float* __restrict__ g, long long r0, int nr, int C, int ldd,
                                             int vec) {
  const int n = nr * C;
  if (vec) {
    float* base = g + r0 * C;
    for (int i = threadIdx.x; i < n / 4; i += ROWS) {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * i + j;
        e[j] = tile[(f / C) * PITCH + f % C];
      }
      reinterpret_cast<float4*>(base)[i] = make_float4(e[0], e[1], e[2], e[3]);
    }
    for (int f = (n / 4) * 4 + threadIdx.x; f < n; f += ROWS) base[f] = tile[(f / C) * PITCH + f % C];
  } else {
    for (int f = threadIdx.x; f < n; f += ROWS) {
      const int r = f / C, c = f % C;
      g[(r0 + r) * ldd + c] = tile[r * PITCH + c];
    }
  }
}

inline bool aligned16(const void* p) { return !((uintptr_t)p & 15); }

}  // namespace
}  // namespace segmif
