// The segmentation objectives of core/loss.py (:342-383 OhemCELoss, SoftmaxFocalLoss, NormalLoss) and torch's weighted / smoothed
// cross entropy as one descriptor-driven kernel pair over NHWC logits (rows x C, pitch ld >= C, C <= 32) and int64 labels.
// Per pixel, with e_c = exp(x_c - max x), p = e / sum e, y the label, w the class weights (1 when NULL), q = sum_{c != y} e_c / sum e
// (never 1 - p_y, which cancels as p_y -> 1):
//   gamma == 0   l = (1 - eps) (-w_y log p_y) + (eps / C) sum_c (-w_c log p_c)                    (torch's cross entropy)
//                dl/dx_c = (1 - eps) w_y (p_c - d_cy) + (eps / C) (p_c sum_k w_k - w_c),          p_y - 1 taken as -q
//   gamma > 0    l = -w_y q^gamma log p_y                                                        (SoftmaxFocalLoss; eps == 0)
//                dl/dx_c = w_y (d_cy - p_c) q^gamma (gamma p_y r - 1),  r = log(p_y) / q = log1p(-q) / q, -1 at q = 0; for
//                q >= 1/2 the quotient is formed from log p_y itself (log1p(-q) loses 1 - q there).  Finite for gamma < 1.
// A pixel whose label is ignore_index or outside [0, C) is ignored: l = 0, gradient 0.
// Reductions: MEAN_VALID sum l / sum_valid w_y (NaN when nothing is valid, as torch); MEAN_ALL sum l / rows; OHEM(t, n_min): the
// mean of {l > t} when that set has at least n_min members, else the mean of the n_min largest l over ALL rows (ignored zeros
// included, as the reference sorts the whole view(-1)): with kappa the n_min-th largest, sum_{l > kappa} l + (n_min - #{l > kappa})
// kappa.  kappa comes from an exact 4 x 8-bit radix select over the order-preserving integer image of the floats (any finite
// value, either sign; -0 is stored as +0): the forward builds the first digit's histogram, then histogram / one-block scan
// launches alternate.  Pixels with l == kappa share the n_min - #{l > kappa} remaining slots equally (the record's tie weight; 1
// when the value is unique) - the VALUE is the reference's exactly, the GRADIENT differs from its arbitrary sort order only when
// two valid pixels have bit-equal losses.  Every launch is issued whichever branch the data takes; the branch is decided on the
// device.  Integer atomics only (histograms); every floating-point sum has a fixed order: bit-identical from run to run, no host
// synchronisation, capturable in a hipGraph.
// Forward: one launch over blocks of 256 rows - the block's logits go through LDS (16-byte loads when ld == C and the base is
// 16-byte aligned: a row of C = 9 is 36 bytes, per-thread row reads would not coalesce), each thread holds its row in registers.
// Backward: one launch; recomputes the softmax, reads the saved l (OHEM), the record and the upstream gradient from device memory
// and writes dlogits already scaled.
// The weighted entry points (self-training: a confidence weight per pixel and / or per sample) instantiate the SAME two kernels
// with WEIGHTED = true: the forward sums u_i l_i, the backward scales the pixel's share by u_i, u_i = pixel_weight[i] *
// sample_weight[i / rows_per_sample] (either NULL: 1).  The denominators do not contain u.  WEIGHTED = false is the code as it was.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "seg_rows.h"
#include "segmif_hip.h"

using namespace segmif;

namespace {

constexpr int HEADER = 4352;     // bytes: 4 x 256 histogram counters, then the select state (4 counters), padded
constexpr int NPART = 5;         // doubles of a block's partial: sum l, denominator, #{l > t}, sum_{l > t} l, sum_{l > kappa} l

struct SegArgs {
  const float* x;
  const long long* labels;
  const float* w;  // NULL: all 1
  long long rows;
  int C, ld, vec, ignore_index, reduction;
  float gamma, eps, t;
  const float* pixel_weight;   // WEIGHTED only; NULL: all 1
  const float* sample_weight;  // WEIGHTED only; NULL: all 1
  long long rows_per_sample;
};

struct Workspace {
  unsigned* hist;   // [4][256]
  unsigned* state;  // prefix, remaining k, #{l == kappa}
  double* partial;  // [nblk][NPART]
  float* l;         // [rows] (OHEM)
};

__host__ __device__ inline long long num_blocks(long long rows) { return (rows + ROWS - 1) / ROWS; }

__host__ __device__ inline Workspace carve(void* ws, long long rows) {
  char* p = (char*)ws;
  Workspace w;
  w.hist = (unsigned*)p;
  w.state = (unsigned*)(p + 4096);
  w.partial = (double*)(p + HEADER);
  w.l = (float*)(p + HEADER + num_blocks(rows) * NPART * sizeof(double));
  return w;
}

// larger float <=> larger key, for every finite value
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// one row's softmax in registers: p[c] (0 for c >= C), and what the loss and its gradient need of it
struct Row {
  float p[32];
  float logp_y, p_y, q, w_y, wsum, wlogp;  // wsum = sum_c w_c, wlogp = sum_c w_c log p_c
};

__device__ __forceinline__ void row_softmax(const float* __restrict__ t, const float* __restrict__ w, int C, int y, bool smooth, Row& R) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    R.p[c] = c < C ? t[c] : -INFINITY;
    mx = fmaxf(mx, R.p[c]);
  }
  float sum = 0.f, rest = 0.f, xy = 0.f, ey = 0.f;
  R.w_y = w ? w[y] : 1.f;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if (c < C) {
      const float x = R.p[c], e = expf(x - mx);
      R.p[c] = e;
      sum += e;
      if (c == y) {
        xy = x, ey = e;
      } else {
        rest += e;
      }
    } else {
      R.p[c] = 0.f;
    }
  }
  const float inv = 1.f / sum, logsum = logf(sum);
  R.logp_y = (xy - mx) - logsum;  // (exact difference when y holds the maximum)
  R.p_y = ey * inv;
  R.q = rest * inv;
  R.wsum = 0.f, R.wlogp = 0.f;
  if (smooth) {  // log p_c = (x_c - max) - log sum e: the logits once more
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      if (c < C) {
        const float wc = w ? w[c] : 1.f;
        R.wsum += wc;
        R.wlogp += wc * ((t[c] - mx) - logsum);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) R.p[c] *= inv;
}

__device__ __forceinline__ float pixel_loss(const SegArgs& a, const Row& R) {
  float l;
  if (a.gamma > 0.f) {
    l = -R.w_y * powf(R.q, a.gamma) * R.logp_y;
  } else {
    l = -R.w_y * R.logp_y;
    if (a.eps > 0.f) l = (1.f - a.eps) * l - (a.eps / (float)a.C) * R.wlogp;
  }
  return l == 0.f ? 0.f : l;  // (-0 -> +0: one key per value)
}

__device__ __forceinline__ bool is_valid(const SegArgs& a, long long lab) { return lab != a.ignore_index && lab >= 0 && lab < a.C; }

// u_i of row r (weights are data: read as given, no gradient)
__device__ __forceinline__ float row_weight(const SegArgs& a, long long r) {
  const float pw = a.pixel_weight ? a.pixel_weight[r] : 1.f;
  const float sw = a.sample_weight ? a.sample_weight[r / a.rows_per_sample] : 1.f;
  return pw * sw;
}

// block-wide fixed-order sums of NV doubles per thread -> out[0 .. NV) by thread 0
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], double (*red)[NPART], double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

template <bool WEIGHTED>
__global__ __launch_bounds__(ROWS) void seg_objective_fwd_kernel(SegArgs a, void* ws) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  __shared__ unsigned hist[256];
  __shared__ double red[4][NPART];
  const Workspace W = carve(ws, a.rows);
  const long long r0 = (long long)blockIdx.x * ROWS;
  const int nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  const bool ohem = a.reduction == SEGMIF_SEG_OHEM;
  hist[threadIdx.x] = 0;
  stage_rows(tile, a.x, r0, nr, a.C, a.ld, a.vec);
  __syncthreads();
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if ((int)threadIdx.x < nr) {
    const long long lab = a.labels[r0 + threadIdx.x];
    float l = 0.f;
    if (is_valid(a, lab)) {
      Row R;
      row_softmax(tile + threadIdx.x * PITCH, a.w, a.C, (int)lab, a.eps > 0.f, R);
      l = pixel_loss(a, R);
      if constexpr (WEIGHTED) l *= row_weight(a, r0 + threadIdx.x);  // (the denominator below stays w_y)
      v[0] = (double)l;
      v[1] = (double)R.w_y;
    }
    if (ohem) {
      W.l[r0 + threadIdx.x] = l;
      atomicAdd(&hist[order_key(l) >> 24], 1u);
      if (l > a.t) v[2] = 1.0, v[3] = (double)l;
    }
  }
  block_sums<4>(v, red, W.partial + (long long)blockIdx.x * NPART);  // (its barrier also completes the LDS histogram)
  if (ohem && hist[threadIdx.x]) atomicAdd(&W.hist[threadIdx.x], hist[threadIdx.x]);
}

// digit `pass` (1..3) of the keys that carry the prefix chosen so far
__global__ __launch_bounds__(ROWS) void seg_objective_hist_kernel(void* ws, long long rows, int pass) {
  __shared__ unsigned hist[256];
  const Workspace W = carve(ws, rows);
  hist[threadIdx.x] = 0;
  __syncthreads();
  const long long r = (long long)blockIdx.x * ROWS + threadIdx.x;
  const unsigned prefix = W.state[0];
  if (r < rows) {
    const unsigned k = order_key(W.l[r]);
    if ((k >> (32 - 8 * pass)) == prefix) atomicAdd(&hist[(k >> (24 - 8 * pass)) & 255u], 1u);
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&W.hist[pass * 256 + threadIdx.x], hist[threadIdx.x]);
}

// one block: the digit of pass `pass` that holds the k-th largest key; k becomes the rank inside that digit
__global__ __launch_bounds__(256) void seg_objective_scan_kernel(void* ws, long long rows, int pass, unsigned n_min) {
  __shared__ unsigned h[256];
  const Workspace W = carve(ws, rows);
  h[threadIdx.x] = W.hist[pass * 256 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned k = pass == 0 ? n_min : W.state[1];
    const unsigned prefix = pass == 0 ? 0u : W.state[0];
    int d = 255;
    for (; d > 0 && h[d] < k; --d) k -= h[d];  // (the keys under the prefix number at least k: the loop ends inside the table)
    W.state[0] = (prefix << 8) | (unsigned)d;
    W.state[1] = k;
    W.state[2] = h[d];
  }
}

// per-block sum of the l above kappa
__global__ __launch_bounds__(ROWS) void seg_objective_above_kernel(void* ws, long long rows) {
  __shared__ double red[4][NPART];
  const Workspace W = carve(ws, rows);
  const long long r = (long long)blockIdx.x * ROWS + threadIdx.x;
  const unsigned kappa = W.state[0];
  double v[1] = {0.0};
  if (r < rows) {
    const float l = W.l[r];
    if (order_key(l) > kappa) v[0] = (double)l;
  }
  block_sums<1>(v, red, W.partial + (long long)blockIdx.x * NPART + 4);
}

// one block: the partials in a fixed order (256 strided runs, then a tree), then the record {loss, 1 / denominator, kappa, tie weight}
__global__ __launch_bounds__(256) void seg_objective_final_kernel(void* ws, long long rows, int reduction, float t, unsigned n_min,
                                                                  float* __restrict__ record) {
  __shared__ double red[NPART][256];
  const Workspace W = carve(ws, rows);
  const long long nblk = num_blocks(rows);
  const int nv = reduction == SEGMIF_SEG_OHEM ? NPART : 2;
  for (int k = 0; k < nv; ++k) {
    double s = 0.0;
    for (long long b = threadIdx.x; b < nblk; b += 256) s += W.partial[b * NPART + k];
    red[k][threadIdx.x] = s;
  }
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int k = 0; k < nv; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = red[0][0], den = red[1][0];
    float loss, coef, kappa = -INFINITY, tie = 1.f;
    if (reduction == SEGMIF_SEG_MEAN_VALID) {
      loss = (float)(sum / den), coef = (float)(1.0 / den);
    } else if (reduction == SEGMIF_SEG_MEAN_ALL) {
      loss = (float)(sum / (double)rows), coef = (float)(1.0 / (double)rows);
    } else {
      const double n_gt = red[2][0];
      if (n_gt >= (double)n_min) {  // the n_min-th largest is above t: the mean of everything above t
        loss = (float)(red[3][0] / n_gt), coef = (float)(1.0 / n_gt), kappa = t, tie = 0.f;
      } else {
        const unsigned rank = W.state[1], equal = W.state[2];  // the n_min-th largest is the rank-th of `equal` copies of kappa
        kappa = key_value(W.state[0]);
        loss = (float)((red[4][0] + (double)rank * (double)kappa) / (double)n_min);
        coef = (float)(1.0 / (double)n_min);
        tie = (float)((double)rank / (double)equal);
      }
    }
    record[0] = loss, record[1] = coef, record[2] = kappa, record[3] = tie;
  }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(ROWS) void seg_objective_bwd_kernel(SegArgs a, const void* ws, const float* __restrict__ record,
                                                                 const float* __restrict__ upstream, float* __restrict__ g, int ldd,
                                                                 int vec_out) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  const long long r0 = (long long)blockIdx.x * ROWS;
  const int nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  stage_rows(tile, a.x, r0, nr, a.C, a.ld, a.vec);
  __syncthreads();
  if ((int)threadIdx.x < nr) {
    float* t = tile + threadIdx.x * PITCH;
    const long long lab = a.labels[r0 + threadIdx.x];
    float s = 0.f;  // this pixel's share of the mean, times the upstream gradient
    if (is_valid(a, lab)) {
      s = upstream[0] * record[1];
      if (a.reduction == SEGMIF_SEG_OHEM) {
        const float l = carve(const_cast<void*>(ws), a.rows).l[r0 + threadIdx.x], kappa = record[2];
        s = l > kappa ? s : (l == kappa ? s * record[3] : 0.f);
      }
      if constexpr (WEIGHTED) s *= row_weight(a, r0 + threadIdx.x);
    }
    if (s != 0.f) {  // (an ignored or unselected pixel gets exact zeros, whatever the coefficient)
      Row R;
      const int y = (int)lab;
      row_softmax(t, a.w, a.C, y, false, R);
      if (a.gamma > 0.f) {
        const float ratio = R.q < 0.5f ? (R.q > 0.f ? log1pf(-R.q) / R.q : -1.f) : R.logp_y / R.q;
        const float f = s * R.w_y * powf(R.q, a.gamma) * (a.gamma * R.p_y * ratio - 1.f);
#pragma unroll
        for (int c = 0; c < 32; ++c)
          if (c < a.C) t[c] = f * (c == y ? R.q : -R.p[c]);
      } else {
        float wsum = 0.f;
        if (a.eps > 0.f)
          for (int c = 0; c < a.C; ++c) wsum += a.w ? a.w[c] : 1.f;
        const float hard = s * (1.f - a.eps) * R.w_y, soft = s * a.eps / (float)a.C;
#pragma unroll
        for (int c = 0; c < 32; ++c) {
          if (c < a.C) {
            float d = hard * (c == y ? -R.q : R.p[c]);
            if (a.eps > 0.f) d += soft * (wsum * R.p[c] - (a.w ? a.w[c] : 1.f));
            t[c] = d;
          }
        }
      }
    } else {
      for (int c = 0; c < a.C; ++c) t[c] = 0.f;
    }
  }
  __syncthreads();
  unstage_rows(tile, g, r0, nr, a.C, ldd, vec_out);
}

bool known_reduction(int r) { return r == SEGMIF_SEG_MEAN_VALID || r == SEGMIF_SEG_MEAN_ALL || r == SEGMIF_SEG_OHEM; }

// fills the kernel arguments; false: the descriptor or the geometry is refused
bool make_args(const SegmifSegObjective* d, const float* logits, const int64_t* labels, const float* w, int64_t rows, int C, int ld,
               SegArgs& a) {
  if (!d || !logits || !labels || rows < 1 || rows > 0x7fffffffLL * ROWS || C < 1 || C > 32 || ld < C) return false;
  if (!(d->gamma >= 0.f) || !(d->label_smoothing >= 0.f && d->label_smoothing < 1.f) || !std::isfinite(d->gamma)) return false;
  if (d->gamma > 0.f && d->label_smoothing > 0.f) return false;
  if (!known_reduction(d->reduction)) return false;
  if (d->reduction == SEGMIF_SEG_OHEM && (d->ohem_n_min < 1 || d->ohem_n_min > rows || rows > 0xffffffffLL || !std::isfinite(d->ohem_t)))
    return false;
  a.x = logits, a.labels = (const long long*)labels, a.w = w;
  a.rows = rows, a.C = C, a.ld = ld;
  a.vec = ld == C && aligned16(logits);
  a.ignore_index = d->ignore_index, a.reduction = d->reduction;
  a.gamma = d->gamma, a.eps = d->label_smoothing, a.t = d->ohem_t;
  a.pixel_weight = a.sample_weight = nullptr, a.rows_per_sample = 1;
  return true;
}

// the weighted entries' extra arguments; false: refused.  Both NULL leaves `a` what make_args made: the unweighted kernels run.
bool add_weights(SegArgs& a, const float* pixel_weight, const float* sample_weight, int64_t rows_per_sample) {
  if (!pixel_weight && !sample_weight) return true;
  if (a.reduction == SEGMIF_SEG_OHEM) return false;
  if (sample_weight && (rows_per_sample < 1 || a.rows % rows_per_sample != 0)) return false;
  a.pixel_weight = pixel_weight, a.sample_weight = sample_weight;
  a.rows_per_sample = sample_weight ? rows_per_sample : 1;
  return true;
}

int launch_forward(const SegArgs& a, unsigned n_min, void* workspace, float* record4, hipStream_t s) {
  const long long rows = a.rows;
  const dim3 grid((unsigned)num_blocks(rows)), block(ROWS);
  if (a.reduction == SEGMIF_SEG_OHEM) {
    const hipError_t e = hipMemsetAsync(workspace, 0, HEADER, s);
    if (e != hipSuccess) return (int)e;
  }
  if (a.pixel_weight || a.sample_weight)
    hipLaunchKernelGGL(seg_objective_fwd_kernel<true>, grid, block, 0, s, a, workspace);
  else
    hipLaunchKernelGGL(seg_objective_fwd_kernel<false>, grid, block, 0, s, a, workspace);
  if (a.reduction == SEGMIF_SEG_OHEM) {
    for (int pass = 0; pass < 4; ++pass) {
      if (pass) hipLaunchKernelGGL(seg_objective_hist_kernel, grid, block, 0, s, workspace, rows, pass);
      hipLaunchKernelGGL(seg_objective_scan_kernel, dim3(1), dim3(256), 0, s, workspace, rows, pass, n_min);
    }
    hipLaunchKernelGGL(seg_objective_above_kernel, grid, block, 0, s, workspace, rows);
  }
  hipLaunchKernelGGL(seg_objective_final_kernel, dim3(1), dim3(256), 0, s, workspace, rows, a.reduction, a.t, n_min, record4);
  return (int)hipGetLastError();
}

int launch_backward(const SegArgs& a, const void* workspace, const float* record4, const float* upstream, float* dlogits, int ldd,
                    hipStream_t s) {
  const int vec_out = ldd == a.C && aligned16(dlogits);
  const dim3 grid((unsigned)num_blocks(a.rows)), block(ROWS);
  if (a.pixel_weight || a.sample_weight)
    hipLaunchKernelGGL(seg_objective_bwd_kernel<true>, grid, block, 0, s, a, workspace, record4, upstream, dlogits, ldd, vec_out);
  else
    hipLaunchKernelGGL(seg_objective_bwd_kernel<false>, grid, block, 0, s, a, workspace, record4, upstream, dlogits, ldd, vec_out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t segmif_seg_objective_workspace_bytes(int64_t rows, int reduction) {
  if (rows < 1 || !known_reduction(reduction)) return 0;
  return HEADER + num_blocks(rows) * NPART * (int64_t)sizeof(double) + (reduction == SEGMIF_SEG_OHEM ? rows * (int64_t)sizeof(float) : 0);
}

extern "C" int segmif_seg_objective_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                        const float* class_weight, void* workspace, float* record4, int64_t rows, int C, int ld,
                                        void* stream) {
  SegArgs a;
  if (!workspace || !record4 || !make_args(desc, logits, labels, class_weight, rows, C, ld, a)) return SEGMIF_EINVAL;
  return launch_forward(a, (unsigned)desc->ohem_n_min, workspace, record4, (hipStream_t)stream);
}

extern "C" int segmif_seg_objective_bwd_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                            const float* class_weight, const void* workspace, const float* record4,
                                            const float* upstream, float* dlogits, int64_t rows, int C, int ld, int ldd, void* stream) {
  SegArgs a;
  if (!record4 || !upstream || !dlogits || ldd < C || !make_args(desc, logits, labels, class_weight, rows, C, ld, a)) return SEGMIF_EINVAL;
  if (a.reduction == SEGMIF_SEG_OHEM && !workspace) return SEGMIF_EINVAL;
  return launch_backward(a, workspace, record4, upstream, dlogits, ldd, (hipStream_t)stream);
}

extern "C" int segmif_seg_objective_weighted_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                                 const float* class_weight, const float* pixel_weight, const float* sample_weight,
                                                 int64_t rows_per_sample, void* workspace, float* record4, int64_t rows, int C, int ld,
                                                 void* stream) {
  SegArgs a;
  if (!workspace || !record4 || !make_args(desc, logits, labels, class_weight, rows, C, ld, a)) return SEGMIF_EINVAL;
  if (!add_weights(a, pixel_weight, sample_weight, rows_per_sample)) return SEGMIF_EINVAL;
  return launch_forward(a, (unsigned)desc->ohem_n_min, workspace, record4, (hipStream_t)stream);
}

extern "C" int segmif_seg_objective_weighted_bwd_f32(const SegmifSegObjective* desc, const float* logits, const int64_t* labels,
                                                     const float* class_weight, const float* pixel_weight, const float* sample_weight,
                                                     int64_t rows_per_sample, const void* workspace, const float* record4,
                                                     const float* upstream, float* dlogits, int64_t rows, int C, int ld, int ldd,
                                                     void* stream) {
  SegArgs a;
  if (!record4 || !upstream || !dlogits || ldd < C || !make_args(desc, logits, labels, class_weight, rows, C, ld, a)) return SEGMIF_EINVAL;
  if (!add_weights(a, pixel_weight, sample_weight, rows_per_sample)) return SEGMIF_EINVAL;
  if (a.reduction == SEGMIF_SEG_OHEM && !workspace) return SEGMIF_EINVAL;
  return launch_backward(a, workspace, record4, upstream, dlogits, ldd, (hipStream_t)stream);
}
