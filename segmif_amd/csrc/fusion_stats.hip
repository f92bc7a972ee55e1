// Fusion-quality statistics of a fused uint8 image against its two sources, per image, and the palette rendering of a
// label map.  Every statistic is an integer (the luma is integer arithmetic), so the results do not depend on how the
// work is cut into workgroups or on what else is in the batch:
//
//   joint_fa[b][f][a], joint_fv[b][f][v]   256 x 256 joint histograms, f = L(fused), v = L(vis), a = ir
//   sums[b] = { sum a v, sum (f[y][x] - f[y][x-1])^2, sum (f[y][x] - f[y-1][x])^2, H W }
//   ag[b]   = sum_{y < H-1, x < W-1} sqrt((dx^2 + dy^2) / 2)
//
// Histogram: a 256 x 256 table of 32-bit counters is 256 KiB and the CU has 160 KiB of LDS, so a workgroup keeps HALF a
// table (the rows of one parity of f: 128 x 256 x 4 B = 128 KiB) and counts only the pixels that fall into it; four
// workgroups (2 tables x 2 parities) read the same tile.  Parity, not the upper bit, because a dark or a bright image puts
// every pixel into one half of the f range but into both parities.  32-bit LDS counters cannot wrap below 2^32 pixels per
// tile; the flush adds the non-empty bins to the int64 table with 64-bit integer atomics, lane i -> bin i, so a wave's adds
// are one contiguous 512-byte run.  A thread takes four consecutive pixels and merges equal neighbouring keys before the
// LDS atomic (smooth images repeat keys along a row).
//
// ag: every term sqrtf(k / 2), k = 1 .. 130 050, lies in [2^-1/2, 255], so it is a multiple of 2^-24 below 2^8: the terms
// are summed as 64-bit integers in units of 2^-24 (exact, < 2^58 for 2^26 pixels) with integer atomics and converted to
// fp64 once - bitwise reproducible and independent of the grid, with no ordered combine needed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_once.h"
#include "segmif_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int HIST_THREADS = 1024;
constexpr int HALF_BINS = 128 * 256;  // one parity of f
constexpr size_t HIST_LDS = (size_t)HALF_BINS * sizeof(unsigned int);
constexpr int MOM_THREADS = 256;

__device__ __forceinline__ int luma(int r, int g, int b) { return (299 * r + 587 * g + 114 * b + 500) / 1000; }

// luma of four consecutive RGB pixels held in three little-endian dwords
__device__ __forceinline__ void luma4(uint32_t w0, uint32_t w1, uint32_t w2, int* f) {
  f[0] = luma(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255);
  f[1] = luma(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
  f[2] = luma((w1 >> 16) & 255, w1 >> 24, w2 & 255);
  f[3] = luma((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
}

// luma of pixels p .. p+3 of one image (n valid ones); ALIGNED: p % 4 == 0, n == 4, 4-byte aligned image base
template <bool ALIGNED>
__device__ __forceinline__ void load_luma4(const uint8_t* __restrict__ rgb, long long p, int n, int* f) {
  if (ALIGNED) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(rgb + 3 * p);
    luma4(w[0], w[1], w[2], f);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* q = rgb + 3 * (p + (i < n ? i : 0));
      f[i] = luma(q[0], q[1], q[2]);
    }
  }
}

template <bool ALIGNED>
__device__ __forceinline__ void load_gray4(const uint8_t* __restrict__ g, long long p, int n, int* a) {
  if (ALIGNED) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(g + p);
    a[0] = w & 255; a[1] = (w >> 8) & 255; a[2] = (w >> 16) & 255; a[3] = w >> 24;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = g[p + (i < n ? i : 0)];
  }
}

// grid (tiles, 4, B): blockIdx.y = 2 * table + parity (table 0: fused x ir, 1: fused x luma(vis))
template <bool ALIGNED>
__global__ __launch_bounds__(HIST_THREADS) void joint_hist_kernel(const uint8_t* __restrict__ fused, const uint8_t* __restrict__ vis,
                                                                  const uint8_t* __restrict__ ir, u64* __restrict__ joint_fa,
                                                                  u64* __restrict__ joint_fv, long long HW) {
  extern __shared__ unsigned int hist[];
  const int table = blockIdx.y >> 1, parity = blockIdx.y & 1, b = blockIdx.z;
  for (int i = threadIdx.x; i < HALF_BINS; i += HIST_THREADS) hist[i] = 0u;
  __syncthreads();
  const uint8_t* fimg = fused + (long long)b * HW * 3;
  const uint8_t* vimg = vis + (long long)b * HW * 3;
  const uint8_t* aimg = ir + (long long)b * HW;
  const long long groups = (HW + 3) / 4;
  const long long per = (groups + gridDim.x - 1) / gridDim.x;
  const long long g0 = per * blockIdx.x, g1 = min(groups, g0 + per);
  for (long long g = g0 + threadIdx.x; g < g1; g += HIST_THREADS) {
    const long long p = 4 * g;
    const int n = (int)min((long long)4, HW - p);
    int f[4], o[4];
    load_luma4<ALIGNED>(fimg, p, n, f);
    if (table) load_luma4<ALIGNED>(vimg, p, n, o);
    else load_gray4<ALIGNED>(aimg, p, n, o);
    int key = -1;
    unsigned int run = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= n || (f[i] & 1) != parity) continue;
      const int k = ((f[i] >> 1) << 8) | o[i];
      if (k == key) {
        ++run;
      } else {
        if (run) atomicAdd(&hist[key], run);
        key = k;
        run = 1;
      }
    }
    if (run) atomicAdd(&hist[key], run);
  }
  __syncthreads();
  u64* out = (table ? joint_fv : joint_fa) + (long long)b * 65536;
  for (int i = threadIdx.x; i < HALF_BINS; i += HIST_THREADS) {
    const unsigned int c = hist[i];
    if (c) atomicAdd(out + ((((i >> 8) * 2 + parity) << 8) | (i & 255)), (u64)c);
  }
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (blocks, B): sum a v, the squared forward differences of f along x and along y, and ag in units of 2^-24
template <bool ALIGNED>
__global__ __launch_bounds__(MOM_THREADS) void moments_kernel(const uint8_t* __restrict__ fused, const uint8_t* __restrict__ vis,
                                                              const uint8_t* __restrict__ ir, u64* __restrict__ sums,
                                                              u64* __restrict__ ag_fixed, int H, int W) {
  const int b = blockIdx.y;
  const long long HW = (long long)H * W;
  const uint8_t* fimg = fused + (long long)b * HW * 3;
  const uint8_t* vimg = vis + (long long)b * HW * 3;
  const uint8_t* aimg = ir + (long long)b * HW;
  const long long groups = (HW + 3) / 4;
  u64 s_av = 0, s_dx = 0, s_dy = 0, s_ag = 0;
  for (long long g = (long long)blockIdx.x * MOM_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * MOM_THREADS) {
    const long long p = 4 * g;
    const int n = (int)min((long long)4, HW - p);
    int f[5], d[4] = {0, 0, 0, 0}, v[4], a[4];
    load_luma4<ALIGNED>(fimg, p, n, f);
    load_luma4<ALIGNED>(vimg, p, n, v);
    load_gray4<ALIGNED>(aimg, p, n, a);
    f[4] = 0;
    if (p + 4 < HW) {
      const uint8_t* q = fimg + 3 * (p + 4);
      f[4] = luma(q[0], q[1], q[2]);
    }
    const bool below = p + W < HW;  // (ALIGNED: W % 4 == 0, the four pixels share a row)
    if (ALIGNED) {
      if (below) load_luma4<true>(fimg, p + W, 4, d);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long q = p + i + W;
        const uint8_t* r = fimg + 3 * (q < HW ? q : p);
        d[i] = luma(r[0], r[1], r[2]);
      }
    }
    int x = (int)(p % W);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < n) {
        s_av += (unsigned int)(a[i] * v[i]);
        const bool has_x = x < W - 1, has_y = p + i + W < HW;
        const int dx = has_x ? f[i + 1] - f[i] : 0;
        const int dy = has_y ? d[i] - f[i] : 0;
        s_dx += (unsigned int)(dx * dx);
        s_dy += (unsigned int)(dy * dy);
        if (has_x && has_y) {
          const float t = __fsqrt_rn(0.5f * (float)(dx * dx + dy * dy));  // exact argument (<= 65 025), <= 1 ulp root
          s_ag += (u64)(t * 16777216.0f);                                   // a multiple of 2^-24 below 2^8: exact
        }
      }
      if (++x == W) x = 0;
    }
  }
  __shared__ u64 part[MOM_THREADS / 64][4];
  s_av = wave_sum(s_av); s_dx = wave_sum(s_dx); s_dy = wave_sum(s_dy); s_ag = wave_sum(s_ag);
  if ((threadIdx.x & 63) == 0) {
    u64* q = part[threadIdx.x >> 6];
    q[0] = s_av; q[1] = s_dx; q[2] = s_dy; q[3] = s_ag;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 t = 0;
    for (int w = 0; w < MOM_THREADS / 64; ++w) t += part[w][threadIdx.x];
    if (t) atomicAdd(threadIdx.x < 3 ? sums + 4 * b + threadIdx.x : ag_fixed + b, t);
  }
}

// after the two kernels above: the pixel count, and ag += (its integer sum) * 2^-24
__global__ void stats_finish_kernel(long long* __restrict__ sums, double* __restrict__ ag, const u64* __restrict__ ag_fixed, int B,
                                    long long HW) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  sums[4 * b + 3] += HW;
  ag[b] += (double)ag_fixed[b] * (1.0 / 16777216.0);
}

__global__ __launch_bounds__(256) void palette_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ palette,
                                                      uint8_t* __restrict__ out, long long n, int K) {
  __shared__ uint8_t pal[256 * 3];
  for (int i = threadIdx.x; i < 3 * K; i += 256) pal[i] = palette[i];
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int l = labels[i];
    const bool in = l >= 0 && l < K;
    const int k = in ? 3 * l : 0;
    out[3 * i + 0] = in ? pal[k + 0] : (uint8_t)0;
    out[3 * i + 1] = in ? pal[k + 1] : (uint8_t)0;
    out[3 * i + 2] = in ? pal[k + 2] : (uint8_t)0;
  }
}

bool stats_dims_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 2 && W >= 2 && (long long)H * W <= (1ll << 30); }

}  // namespace

extern "C" int64_t segmif_fusion_stats_workspace_bytes(int B, int H, int W) {
  return stats_dims_ok(B, H, W) ? (int64_t)B * 8 : 0;
}

extern "C" int segmif_fusion_stats_u8(const uint8_t* fused_rgb, const uint8_t* vis_rgb, const uint8_t* ir, int64_t* joint_fa,
                                      int64_t* joint_fv, int64_t* sums, double* ag, void* workspace, int B, int H, int W,
                                      int accumulate, void* stream) {
  if (!fused_rgb || !vis_rgb || !ir || !joint_fa || !joint_fv || !sums || !ag || !workspace || !stats_dims_ok(B, H, W))
    return SEGMIF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  static segmif::PerDeviceFlag raised_flag;
  bool& raised = raised_flag.here();
  if (!raised) {
    hipError_t e = hipFuncSetAttribute((const void*)joint_hist_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIST_LDS);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)joint_hist_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIST_LDS);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  const long long HW = (long long)H * W;
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)B * 8, s);
  if (!accumulate) {  // (memset nodes in a captured graph: the caller zeroes nothing)
    if (e == hipSuccess) e = hipMemsetAsync(joint_fa, 0, (size_t)B * 65536 * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(joint_fv, 0, (size_t)B * 65536 * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(sums, 0, (size_t)B * 32, s);
    if (e == hipSuccess) e = hipMemsetAsync(ag, 0, (size_t)B * 8, s);
  }
  if (e != hipSuccess) return (int)e;
  const bool aligned = W % 4 == 0 && (((uintptr_t)fused_rgb | (uintptr_t)vis_rgb | (uintptr_t)ir) & 3) == 0;
  const long long groups = (HW + 3) / 4;
  // tiles per image: about two workgroups per CU over the whole launch, and no tile below 4096 groups (the flush and the
  // clearing of 128 KiB are a fixed cost per workgroup).  The counts do not depend on this choice.
  long long tiles = (512 + 4ll * B - 1) / (4ll * B);
  tiles = tiles < 1 ? 1 : tiles;
  const long long most = (groups + 4095) / 4096;
  if (tiles > most) tiles = most;
  const dim3 hgrid((unsigned)tiles, 4, (unsigned)B);
  long long mblocks = (groups + MOM_THREADS - 1) / MOM_THREADS;
  const long long mcap = B >= 1024 ? 1 : 1024 / B;
  if (mblocks > mcap) mblocks = mcap;
  const dim3 mgrid((unsigned)mblocks, (unsigned)B);
  u64* jfa = reinterpret_cast<u64*>(joint_fa);
  u64* jfv = reinterpret_cast<u64*>(joint_fv);
  u64* usums = reinterpret_cast<u64*>(sums);
  u64* fixed = reinterpret_cast<u64*>(workspace);
  if (aligned) {
    hipLaunchKernelGGL(joint_hist_kernel<true>, hgrid, dim3(HIST_THREADS), HIST_LDS, s, fused_rgb, vis_rgb, ir, jfa, jfv, HW);
    hipLaunchKernelGGL(moments_kernel<true>, mgrid, dim3(MOM_THREADS), 0, s, fused_rgb, vis_rgb, ir, usums, fixed, H, W);
  } else {
    hipLaunchKernelGGL(joint_hist_kernel<false>, hgrid, dim3(HIST_THREADS), HIST_LDS, s, fused_rgb, vis_rgb, ir, jfa, jfv, HW);
    hipLaunchKernelGGL(moments_kernel<false>, mgrid, dim3(MOM_THREADS), 0, s, fused_rgb, vis_rgb, ir, usums, fixed, H, W);
  }
  hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (long long*)sums, ag, fixed, B, HW);
  return (int)hipGetLastError();
}

extern "C" int segmif_palette_u8(const int32_t* labels, const uint8_t* palette, uint8_t* out, int64_t n, int K, void* stream) {
  if (!labels || !palette || !out || n < 0 || K < 1 || K > 256) return SEGMIF_EINVAL;
  if (n == 0) return 0;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(palette_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, labels, palette, out, (long long)n, K);
  return (int)hipGetLastError();
}
