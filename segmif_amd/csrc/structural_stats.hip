// Local-window fusion scores of a fused uint8 image against its two sources, per image: the sums behind Qabf
// (Xydeas-Petrovic edge preservation), SSIM (11 x 11 Gaussian, sigma 1.5, zero padding) and the pixel-domain VIF (four
// scales, sigma_nsq = 2).  The planes are those of fusion_stats.hip: f = L(fused), v = L(vis), a = ir.
//
//   luma_planes_kernel   f and v as uint8 planes in the workspace, so that every later kernel reads three planar images
//   qabf_kernel          3 x 3 Sobel of the three planes (exact integers, zero padding), the two Q maps in fp64, and the
//                        sums  num = sum Q_AF gA + Q_VF gV,  den = sum gA + gV
//   moments_kernel       <N, T, MODE>: one 32 x 16 output tile per workgroup.  The (16 + N - 1) x (32 + N - 1) halo tile of
//                        the three planes is staged in LDS (float for uint8 planes: exact; double for the fp64 planes of
//                        scales 2-4); each of the eight maps f, a, v, f^2, a^2, v^2, fa, fv is filtered by the separable
//                        Gaussian in fp64 - row pass into an LDS buffer, column pass into registers - and a per-pixel
//                        epilogue turns the eight moments into the SSIM map values (MODE 0) or the VIF log terms (MODE 1)
//                        of both pairs.  `pad` places the window: 5 with N = 11 is the zero-padded "same" filter of SSIM,
//                        0 is the "valid" filter of VIF.
//   decimate_kernel      the next VIF scale's planes: "valid" N x N Gaussian, every second row and column, fp64
//   finish_kernel        one workgroup per output value adds that value's per-workgroup partials in a fixed order
//
// Sums: lanes by a shuffle butterfly, waves in wave order, workgroups by finish_kernel (thread t takes partials t, t + 256,
// ..., then a fixed tree) - no floating-point atomics.  The grid of an image depends on H and W alone, so a result is bitwise
// reproducible and does not depend on the rest of the batch.
//
// LDS: the row pass reads float / double at consecutive columns per lane and the column pass reads doubles at consecutive
// columns (32 lanes x 8 B = one 256-byte bank row per half wave): both are conflict-free.  The row-pass buffer is doubled,
// so one barrier per map suffices (a buffer is rewritten two barriers after its last read).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int TW = 32, TH = 16;  // output tile of moments_kernel (TW * TH = 2 * THREADS)
constexpr int MAXN = 17;
constexpr int VIF_N[5] = {0, 17, 9, 5, 3};  // window of scale s = 1 .. 4

struct Taps {
  double w[MAXN];
};

__device__ __forceinline__ int luma(int r, int g, int b) { return (299 * r + 587 * g + 114 * b + 500) / 1000; }

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// out[k] = sum over the workgroup of v[k], k < K: lanes by the butterfly, waves in wave order
template <int K>
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* __restrict__ out) {
  __shared__ double part[THREADS / 64][K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) t += part[w][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// grid (blocks, B): fv[b][0] = L(fused[b]), fv[b][1] = L(vis[b])
__global__ __launch_bounds__(THREADS) void luma_planes_kernel(const uint8_t* __restrict__ fused, const uint8_t* __restrict__ vis,
                                                              uint8_t* __restrict__ fv, long long HW) {
  const int b = blockIdx.y;
  const uint8_t* fimg = fused + (long long)b * HW * 3;
  const uint8_t* vimg = vis + (long long)b * HW * 3;
  uint8_t* fo = fv + (long long)b * HW * 2;
  uint8_t* vo = fo + HW;
  const long long stride = (long long)gridDim.x * THREADS;
  for (long long p = (long long)blockIdx.x * THREADS + threadIdx.x; p < HW; p += stride) {
    const uint8_t* q = fimg + 3 * p;
    const uint8_t* r = vimg + 3 * p;
    fo[p] = (uint8_t)luma(q[0], q[1], q[2]);
    vo[p] = (uint8_t)luma(r[0], r[1], r[2]);
  }
}

// sx = x * [[-1,0,1],[-2,0,2],[-1,0,1]], sy = x * [[1,2,1],[0,0,0],[-1,-2,-1]]: true convolutions (masks flipped), zero padding
__device__ __forceinline__ void sobel(const uint8_t* __restrict__ p, int y, int x, int H, int W, int& sx, int& sy) {
  int n[3][3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = y + dy - 1, xx = x + dx - 1;
      const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
      n[dy][dx] = in ? (int)p[(long long)(in ? yy : 0) * W + (in ? xx : 0)] : 0;
    }
  sx = (n[0][0] + 2 * n[1][0] + n[2][0]) - (n[0][2] + 2 * n[1][2] + n[2][2]);
  sy = (n[2][0] + 2 * n[2][1] + n[2][2]) - (n[0][0] + 2 * n[0][1] + n[0][2]);
}

__device__ __forceinline__ double edge_angle(int sx, int sy) { return sx == 0 ? M_PI_2 : atan((double)sy / (double)sx); }

// Q_SF of one pixel: m2 = sx^2 + sy^2 (the comparison is decided on the integers), g = sqrt(m2), al = the angle
__device__ __forceinline__ double q_sf(int m2s, int m2f, double gs, double gf, double als, double alf) {
  const double G = m2s > m2f ? gf / gs : (m2s == m2f ? gf : gs / gf);
  const double A = 1.0 - fabs(als - alf) / M_PI_2;
  return 0.9994 / (1.0 + exp(-15.0 * (G - 0.5))) * 0.9879 / (1.0 + exp(-22.0 * (A - 0.8)));
}

// grid (blocks, B), one pixel per thread: partial[b][block] = { num, den }
__global__ __launch_bounds__(THREADS) void qabf_kernel(const uint8_t* __restrict__ fv, const uint8_t* __restrict__ ir, int H, int W,
                                                       double* __restrict__ partial, long long per_image) {
  const int b = blockIdx.y;
  const long long HW = (long long)H * W;
  const uint8_t* pf = fv + (long long)b * HW * 2;
  const uint8_t* pv = pf + HW;
  const uint8_t* pa = ir + (long long)b * HW;
  const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (p < HW) {
    const int y = (int)(p / W), x = (int)(p % W);
    int fx, fy, ax, ay, vx, vy;
    sobel(pf, y, x, H, W, fx, fy);
    sobel(pa, y, x, H, W, ax, ay);
    sobel(pv, y, x, H, W, vx, vy);
    const int m2f = fx * fx + fy * fy, m2a = ax * ax + ay * ay, m2v = vx * vx + vy * vy;  // <= 2 * 1020^2
    const double gf = sqrt((double)m2f), ga = sqrt((double)m2a), gv = sqrt((double)m2v);
    const double alf = edge_angle(fx, fy), ala = edge_angle(ax, ay), alv = edge_angle(vx, vy);
    acc[0] = q_sf(m2a, m2f, ga, gf, ala, alf) * ga + q_sf(m2v, m2f, gv, gf, alv, alf) * gv;
    acc[1] = ga + gv;
  }
  block_sum_store<2>(acc, partial + (long long)b * per_image + 2ll * blockIdx.x);
}

template <typename T>
struct Staged {
  typedef double type;
};
template <>
struct Staged<uint8_t> {
  typedef float type;  // 0 .. 255: exact
};

// map M of the eight at one staged pixel: f, a, v, f^2, a^2, v^2, f a, f v
template <int M, typename S>
__device__ __forceinline__ double map_value(const S* __restrict__ f, const S* __restrict__ a, const S* __restrict__ v, int i) {
  if (M == 0) return (double)f[i];
  if (M == 1) return (double)a[i];
  if (M == 2) return (double)v[i];
  if (M == 3) return (double)f[i] * (double)f[i];
  if (M == 4) return (double)a[i] * (double)a[i];
  if (M == 5) return (double)v[i] * (double)v[i];
  if (M == 6) return (double)f[i] * (double)a[i];
  return (double)f[i] * (double)v[i];
}

// the pytorch_ssim map value of (x, y) from the moments of the 0 .. 255 planes: images are taken as x / 255
__device__ __forceinline__ double ssim_value(double m1, double m2, double e11, double e22, double e12) {
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double mu1 = m1 / 255.0, mu2 = m2 / 255.0;
  const double s1 = e11 / 65025.0 - mu1 * mu1, s2 = e22 / 65025.0 - mu2 * mu2, s12 = e12 / 65025.0 - mu1 * mu2;
  return ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
}

// the two log terms of vifp at one pixel: index 1 = the source (reference image), 2 = the fused image (distorted)
__device__ __forceinline__ void vif_terms(double mu1, double mu2, double e11, double e22, double e12, double& num, double& den) {
  double s1 = e11 - mu1 * mu1, s2 = e22 - mu2 * mu2;
  const double s12 = e12 - mu1 * mu2;
  s1 = s1 < 0.0 ? 0.0 : s1;
  s2 = s2 < 0.0 ? 0.0 : s2;
  double g = s12 / (s1 + 1e-10), sv = s2 - g * s12;
  if (s1 < 1e-10) { g = 0.0; sv = s2; s1 = 0.0; }
  if (s2 < 1e-10) { g = 0.0; sv = 0.0; }
  if (g < 0.0) { sv = s2; g = 0.0; }
  if (sv <= 1e-10) sv = 1e-10;
  num = log10(1.0 + g * g * s1 / (sv + 2.0));
  den = log10(1.0 + s1 / 2.0);
}

template <int M, int N, typename S>
__device__ __forceinline__ void filter_map(const S* __restrict__ sf, const S* __restrict__ sa, const S* __restrict__ sv,
                                           double* __restrict__ tmp, const Taps& taps, double (&acc)[8][2]) {
  constexpr int IH = TH + N - 1, IW = TW + N - 1;
  double* t = tmp + (M & 1) * (IH * TW);
#pragma unroll 1
  for (int i = threadIdx.x; i < IH * TW; i += THREADS) {  // row pass
    const int r = i / TW, c = i % TW;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) s += taps.w[k] * map_value<M>(sf, sa, sv, r * IW + c + k);
    t[i] = s;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // column pass: output pixel threadIdx.x + j * THREADS of the tile
    const int o = threadIdx.x + j * THREADS, r = o / TW, c = o % TW;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) s += taps.w[k] * t[(r + k) * TW + c];
    asm volatile("" : "+v"(s));  // the sum is formed here: left alone, the compiler keeps all 8 x 2 x N loaded values to the end
    acc[M][j] = s;
  }
}

// grid (tiles, B).  Planes pf, pa, pv of H x W with batch strides bf, ba, bv (elements); the window's top-left tap of output
// (oy, ox) is input (oy - pad, ox - pad), input outside the image is zero; outputs outside OH x OW are not counted.
// partial[b][tile] = MODE 0: { sum ssim(f, a), sum ssim(f, v) };  MODE 1: { num(a, f), den(a, f), num(v, f), den(v, f) }
template <int N, typename T, int MODE>
__global__ __launch_bounds__(THREADS) void moments_kernel(const T* __restrict__ pf, const T* __restrict__ pa, const T* __restrict__ pv,
                                                          long long bf, long long ba, long long bv, int H, int W, int pad, int OH,
                                                          int OW, int tiles_x, Taps taps, double* __restrict__ partial,
                                                          long long per_image) {
  typedef typename Staged<T>::type S;
  constexpr int IH = TH + N - 1, IW = TW + N - 1, K = MODE == 0 ? 2 : 4;
  __shared__ S stage[3][IH * IW];
  __shared__ double tmp[2 * IH * TW];
  const int b = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int oy0 = ty * TH, ox0 = tx * TW;
  const T* f = pf + (long long)b * bf;
  const T* a = pa + (long long)b * ba;
  const T* v = pv + (long long)b * bv;
  for (int i = threadIdx.x; i < IH * IW; i += THREADS) {
    const int y = oy0 - pad + i / IW, x = ox0 - pad + i % IW;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    const long long q = in ? (long long)y * W + x : 0;
    stage[0][i] = in ? (S)f[q] : (S)0;
    stage[1][i] = in ? (S)a[q] : (S)0;
    stage[2][i] = in ? (S)v[q] : (S)0;
  }
  __syncthreads();
  double acc[8][2];
  filter_map<0, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<1, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<2, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<3, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<4, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<5, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<6, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  filter_map<7, N>(stage[0], stage[1], stage[2], tmp, taps, acc);
  double sum[K];
#pragma unroll
  for (int k = 0; k < K; ++k) sum[k] = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = threadIdx.x + j * THREADS;
    if (oy0 + o / TW >= OH || ox0 + o % TW >= OW) continue;
    if (MODE == 0) {
      sum[0] += ssim_value(acc[0][j], acc[1][j], acc[3][j], acc[4][j], acc[6][j]);
      sum[1] += ssim_value(acc[0][j], acc[2][j], acc[3][j], acc[5][j], acc[7][j]);
    } else {
      double num, den;
      vif_terms(acc[1][j], acc[0][j], acc[4][j], acc[3][j], acc[6][j], num, den);
      sum[0] += num;
      sum[1] += den;
      vif_terms(acc[2][j], acc[0][j], acc[5][j], acc[3][j], acc[7][j], num, den);
      sum[2] += num;
      sum[3] += den;
    }
  }
  block_sum_store<K>(sum, partial + (long long)b * per_image + (long long)K * blockIdx.x);
}

// grid (blocks, 3, B): out[b][plane][y][x] = sum_ij w[i] w[j] in[2 y + i][2 x + j], y < OH = ceil((H - N + 1) / 2), x alike
template <int N, typename T>
__global__ __launch_bounds__(THREADS) void decimate_kernel(const T* __restrict__ pf, const T* __restrict__ pa, const T* __restrict__ pv,
                                                           long long bf, long long ba, long long bv, int W, double* __restrict__ out,
                                                           long long bo, int OH, int OW, Taps taps) {
  const int plane = blockIdx.y, b = blockIdx.z;
  const T* in = plane == 0 ? pf + (long long)b * bf : (plane == 1 ? pa + (long long)b * ba : pv + (long long)b * bv);
  const long long P = (long long)OH * OW;
  const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (p >= P) return;
  const int y = (int)(p / OW), x = (int)(p % OW);
  const T* q = in + (long long)(2 * y) * W + 2 * x;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) r += taps.w[j] * (double)q[(long long)i * W + j];
    s += taps.w[i] * r;
  }
  out[(long long)b * bo + plane * P + p] = s;
}

struct Segments {      // of one image's partials: 0 qabf, 1 ssim, 2 .. 5 vif scale 1 .. 4
  long long off[6];    // first double
  long long count[6];  // workgroups
};

// grid (20, B): slot 0, 1 -> qabf[b][0 .. 1]; 2, 3 -> ssim[b][0 .. 1]; 4 + 8 src + 2 scale + t -> vif[b][src][scale][t]
__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ partial, long long per_image, Segments seg,
                                                         double* __restrict__ qabf, double* __restrict__ ssim, double* __restrict__ vif) {
  __shared__ double tree[THREADS];
  const int slot = blockIdx.x, b = blockIdx.y;
  int s, K, k;
  double* out;
  if (slot < 4) {
    s = slot >> 1; K = 2; k = slot & 1;
    out = (slot < 2 ? qabf : ssim) + 2ll * b + k;
  } else {
    const int i = slot - 4, src = i >> 3, scale = (i >> 1) & 3, t = i & 1;
    s = 2 + scale; K = 4; k = 2 * src + t;
    out = vif + 16ll * b + i;
  }
  const double* p = partial + (long long)b * per_image + seg.off[s] + k;
  double acc = 0.0;
  for (long long i = threadIdx.x; i < seg.count[s]; i += THREADS) acc += p[i * K];
  tree[threadIdx.x] = acc;
  __syncthreads();
  for (int h = THREADS / 2; h; h >>= 1) {
    if ((int)threadIdx.x < h) tree[threadIdx.x] += tree[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = tree[0];
}

struct Layout {
  int h[5], w[5];            // planes of scale 1 .. 4
  int oh[5], ow[5];          // their moment maps ("valid")
  long long tiles[5];        // workgroups of moments_kernel per image
  long long plane_off[5];    // scale 2 .. 4: first double of the image's three planes
  long long planes;          // doubles per image
  long long nq, ns;          // workgroups per image of qabf_kernel and of the SSIM launch
  Segments seg;
  long long per_image;       // partial doubles per image
  long long u8_bytes, planes_bytes, partial_bytes;
};

long long tiles_of(int oh, int ow) { return (long long)((oh + TH - 1) / TH) * ((ow + TW - 1) / TW); }

bool structural_dims_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 41 && W >= 41 && (long long)H * W <= (1ll << 30);
}

Layout layout_of(int B, int H, int W) {
  Layout L;
  L.h[1] = H; L.w[1] = W;
  L.planes = 0;
  for (int s = 1; s <= 4; ++s) {
    const int n = VIF_N[s];
    if (s > 1) {
      L.h[s] = (L.h[s - 1] - n + 2) / 2;
      L.w[s] = (L.w[s - 1] - n + 2) / 2;
      L.plane_off[s] = L.planes;
      L.planes += 3ll * L.h[s] * L.w[s];
    }
    L.oh[s] = L.h[s] - n + 1;
    L.ow[s] = L.w[s] - n + 1;
    L.tiles[s] = tiles_of(L.oh[s], L.ow[s]);
  }
  const long long HW = (long long)H * W;
  L.nq = (HW + THREADS - 1) / THREADS;
  L.ns = tiles_of(H, W);
  long long off = 0;
  L.seg.off[0] = off; L.seg.count[0] = L.nq; off += 2 * L.nq;
  L.seg.off[1] = off; L.seg.count[1] = L.ns; off += 2 * L.ns;
  for (int s = 1; s <= 4; ++s) {
    L.seg.off[1 + s] = off; L.seg.count[1 + s] = L.tiles[s]; off += 4 * L.tiles[s];
  }
  L.per_image = off;
  L.u8_bytes = ((long long)B * 2 * HW + 7) / 8 * 8;
  L.planes_bytes = (long long)B * L.planes * 8;
  L.partial_bytes = (long long)B * L.per_image * 8;
  return L;
}

// normalised 1-D Gaussian of n taps; the n x n window of the definitions is its outer product
Taps gaussian(int n, double sd) {
  Taps t;
  double sum = 0.0;
  for (int i = 0; i < MAXN; ++i) t.w[i] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = i - (n - 1) / 2.0;
    t.w[i] = exp(-d * d / (2.0 * sd * sd));
    sum += t.w[i];
  }
  for (int i = 0; i < n; ++i) t.w[i] /= sum;
  return t;
}

template <int N, typename T>
void launch_vif_scale(const Layout& L, int s, const T* pf, const T* pa, const T* pv, long long bf, long long ba, long long bv, int B,
                      double* partial, hipStream_t st) {
  const int tiles_x = (L.ow[s] + TW - 1) / TW;
  hipLaunchKernelGGL((moments_kernel<N, T, 1>), dim3((unsigned)L.tiles[s], (unsigned)B), dim3(THREADS), 0, st, pf, pa, pv, bf, ba, bv,
                     L.h[s], L.w[s], 0, L.oh[s], L.ow[s], tiles_x, gaussian(N, N / 5.0), partial + L.seg.off[1 + s], L.per_image);
}

template <int N, typename T>
void launch_decimate(const Layout& L, int s, const T* pf, const T* pa, const T* pv, long long bf, long long ba, long long bv, int B,
                     double* planes, hipStream_t st) {  // scale s - 1 -> s
  const long long P = (long long)L.h[s] * L.w[s];
  hipLaunchKernelGGL((decimate_kernel<N, T>), dim3((unsigned)((P + THREADS - 1) / THREADS), 3, (unsigned)B), dim3(THREADS), 0, st, pf,
                     pa, pv, bf, ba, bv, L.w[s - 1], planes + L.plane_off[s], L.planes, L.h[s], L.w[s], gaussian(N, N / 5.0));
}

}  // namespace

extern "C" int64_t segmif_structural_stats_workspace_bytes(int B, int H, int W) {
  if (!structural_dims_ok(B, H, W)) return 0;
  const Layout L = layout_of(B, H, W);
  return (int64_t)(L.u8_bytes + L.planes_bytes + L.partial_bytes);
}

extern "C" int segmif_structural_stats_u8(const uint8_t* fused_rgb, const uint8_t* vis_rgb, const uint8_t* ir, double* qabf,
                                          double* ssim, double* vif, void* workspace, int B, int H, int W, void* stream) {
  if (!fused_rgb || !vis_rgb || !ir || !qabf || !ssim || !vif || !workspace || !structural_dims_ok(B, H, W)) return SEGMIF_EINVAL;
  if ((uintptr_t)workspace & 7) return SEGMIF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout_of(B, H, W);
  const long long HW = (long long)H * W;
  uint8_t* fv = reinterpret_cast<uint8_t*>(workspace);
  double* planes = reinterpret_cast<double*>(fv + L.u8_bytes);
  double* partial = planes + (long long)B * L.planes;
  const uint8_t* pf = fv;
  const uint8_t* pv = fv + HW;

  long long lblocks = (HW + THREADS - 1) / THREADS;
  if (lblocks > 4096) lblocks = 4096;
  hipLaunchKernelGGL(luma_planes_kernel, dim3((unsigned)lblocks, (unsigned)B), dim3(THREADS), 0, st, fused_rgb, vis_rgb, fv, HW);
  hipLaunchKernelGGL(qabf_kernel, dim3((unsigned)L.nq, (unsigned)B), dim3(THREADS), 0, st, (const uint8_t*)fv, ir, H, W,
                     partial + L.seg.off[0], L.per_image);
  hipLaunchKernelGGL((moments_kernel<11, uint8_t, 0>), dim3((unsigned)L.ns, (unsigned)B), dim3(THREADS), 0, st, pf, ir, pv, 2 * HW, HW,
                     2 * HW, H, W, 5, H, W, (W + TW - 1) / TW, gaussian(11, 1.5), partial + L.seg.off[1], L.per_image);
  launch_vif_scale<17, uint8_t>(L, 1, pf, ir, pv, 2 * HW, HW, 2 * HW, B, partial, st);
  launch_decimate<9, uint8_t>(L, 2, pf, ir, pv, 2 * HW, HW, 2 * HW, B, planes, st);
  for (int s = 2; s <= 4; ++s) {
    const long long P = (long long)L.h[s] * L.w[s];
    const double* qf = planes + L.plane_off[s];
    if (s == 2) {
      launch_vif_scale<9, double>(L, s, qf, qf + P, qf + 2 * P, L.planes, L.planes, L.planes, B, partial, st);
      launch_decimate<5, double>(L, 3, qf, qf + P, qf + 2 * P, L.planes, L.planes, L.planes, B, planes, st);
    } else if (s == 3) {
      launch_vif_scale<5, double>(L, s, qf, qf + P, qf + 2 * P, L.planes, L.planes, L.planes, B, partial, st);
      launch_decimate<3, double>(L, 4, qf, qf + P, qf + 2 * P, L.planes, L.planes, L.planes, B, planes, st);
    } else {
      launch_vif_scale<3, double>(L, s, qf, qf + P, qf + 2 * P, L.planes, L.planes, L.planes, B, partial, st);
    }
  }
  hipLaunchKernelGGL(finish_kernel, dim3(20, (unsigned)B), dim3(THREADS), 0, st, (const double*)partial, L.per_image, L.seg, qabf, ssim,
                     vif);
  return (int)hipGetLastError();
}
