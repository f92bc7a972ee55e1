// Private to segmif_amd/csrc: the one packer behind every weight image of the split-operand kernels (conv3x3_split, conv3x3_planes,
// gemm_split, gemm_pairs, mixffn).  An image is the fp32 weight (N, K), rows of pitch ldw, split into the planes of an arithmetic
// and stored in the order the main kernel streams them; the f16x3 images carry one float per row as well, 2^-e(n), the factor
// that takes the row's scale out again in the epilogue.
//   arithmetic  Bf16x6: x = p0 + p1 + p2 (bf3::split3).  F16x3: the row times 2^e(n), planes W0 | W - W0 | 2^-11 W0 (p16::split3h).
//   layout      a struct next to the geometry constants of the kernel that reads the image:
//                 static constexpr int PLANES     planes stored per element (2: an image without the 2^-11 W0 plane)
//                 int npad() const                (host) rows of the image: N rounded up to the tile
//                 long long elements() const      (host) elements of the image, padding rows and columns included; one thread each
//                 PackSlot slot(long long i)      (device) element i: its source, where its planes go, the padding halfword it owns
// Each .hip file that includes this gets kernels of its own (anonymous namespace), as each had before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"
#include "split_ops.h"

namespace segmif {
namespace {

struct PackSlot {
  int n, k;         // source w[n][k]; n < 0: zero fill (a row past N or a column past K)
  long long at[3];  // halfword index of each plane (the first PLANES are used)
  long long pad;    // halfword index of a padding halfword this element zeroes, or -1
};

// where the row scales 2^-e(n) live: p[(n / group) * group_stride + n % group] with group = 2^group_log2, so that the pack kernel
// pays no division per element (group_log2 31: one group, a plain array)
struct RowScales {
  float* p;
  int group_log2;
  long long group_stride;
  __device__ float& at(int n) const { return p[(long long)(n >> group_log2) * group_stride + (n & ((1u << group_log2) - 1u))]; }
};

struct Bf16x6 {
  static constexpr bool SCALED = false;
  static __device__ __forceinline__ void split(float x, uint32_t* p) { bf3::split3(x, 0.f, p[0], p[1], p[2]); }
};
struct F16x3 {
  static constexpr bool SCALED = true;
  static __device__ __forceinline__ void split(float x, uint32_t* p) { p16::split3h(x, 0.f, p[0], p[1], p[2]); }
};

// one wave per padded output row: 2^-e(n) with 2^14 <= 2^e(n) max |w[n][.]| < 2^15; 1 for an all-zero, vanishing or non-finite
// row and for the padding rows n >= N
__global__ void weight_row_scale_kernel(const float* __restrict__ w, int N, int K, long long ldw, RowScales dst) {
  const int n = blockIdx.x;
  float mx = 0.f;
  if (n < N)
    for (int k = threadIdx.x; k < K; k += 64) mx = fmaxf(mx, fabsf(w[n * ldw + k]));
  mx = p16::wave_max(mx);
  if (threadIdx.x == 0) dst.at(n) = 1.f / p16::pow2_scale(mx);  // exact: a power of two
}

template <class Arith, class Layout>
__global__ void weight_pack_kernel(const float* __restrict__ w, long long ldw, RowScales scales, Layout lay, long long total,
                                   uint16_t* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const PackSlot e = lay.slot(idx);
  float x = 0.f;
  if (e.n >= 0) {
    x = w[e.n * ldw + e.k];
    if constexpr (Arith::SCALED) x *= 1.f / scales.at(e.n);  // exact: a power of two
  }
  uint32_t p[3];
  Arith::split(x, p);
#pragma unroll
  for (int i = 0; i < Layout::PLANES; ++i) out[e.at[i]] = (uint16_t)(p[i] & 0xffffu);
  if (e.pad >= 0) out[e.pad] = 0;
}

// the fp32 weight (N, K), rows of pitch ldw
struct WeightSrc {
  const float* w;
  int N, K;
  long long ldw;
};

// What a *_pack entry point does after it has named its layout.  bytes: the entry point's own *_weight_bytes (0: invalid
// dimensions).  The row scales of an f16x3 image are the last npad() floats of those bytes unless the image keeps them elsewhere
// (`scales`).
template <class Arith, class Layout>
int pack_weight(WeightSrc src, const Layout& lay, int64_t bytes, void* out, hipStream_t stream, unsigned align_mask = 0,
                RowScales scales = {}) {
  if (!src.w || !out || bytes <= 0 || src.ldw < src.K || ((uintptr_t)out & align_mask)) return SEGMIF_EINVAL;
  const int npad = lay.npad();
  if (!scales.p) scales = {reinterpret_cast<float*>((unsigned char*)out + bytes) - npad, 31, 0};  // (not touched by Bf16x6)
  if (Arith::SCALED) {
    hipLaunchKernelGGL(weight_row_scale_kernel, dim3((unsigned)npad), dim3(64), 0, stream, src.w, src.N, src.K, src.ldw, scales);
  }
  const long long total = lay.elements();
  hipLaunchKernelGGL((weight_pack_kernel<Arith, Layout>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src.w, src.ldw,
                     scales, lay, total, (uint16_t*)out);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace segmif
