// Confidence calibration statistics of the segmentation net's softmax (include/segmif_calib.h has the rule): reliability tables
// {n, correct, sum of conf} per temperature and confidence bin, the counts above confidence thresholds, the sums of NLL and Brier
// score, in ONE gather pass over the quarter-resolution NHWC logits.  This project's addition, NOT the reference's evaluation.  A
// sibling of pseudo_label_kernel (csrc/pseudo_label.hip): like it, the (B, OH, OW, C) resized logits and their softmax never exist.
//
// One thread per output pixel, a block takes 256 columns of 4 rows, grid (column blocks, row blocks, image).  A thread interpolates
// its pixel's C logits ONCE into registers (fully unrolled arrays of 12 or 32, every index a compile-time constant: no scratch),
// finds the argmax, then walks the temperatures: C - 1 exponentials each, kept in registers for the Brier term.  The bin is a loop
// over at most 31 wave-uniform edges.  A wave combines its lanes before it touches LDS: for each bin that occurs in the wave, two
// ballots give n and correct, a fixed xor-shuffle tree gives the sum of conf * 2^32 (exact integers), and one lane adds the three
// to the block's LDS tables with integer atomics; the thresholds are two ballots each.  At the end a block sends one 64-bit
// integer atomic per non-zero counter.  NLL and Brier are summed in double: per wave in a fixed shuffle tree, each wave into its
// own LDS slot row after row, per block in wave order into the workspace; calibration_final_kernel sums the blocks in a fixed
// order and adds the total to the running value with one add.  No float atomics, no host synchronisation, bit-identical runs.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "segmif_calib.h"
#include "segmif_hip.h"

namespace {

constexpr int THREADS = SEGMIF_CALIB_BLOCK_COLUMNS;
constexpr int WAVES = THREADS / 64;
constexpr int ROWS_PB = SEGMIF_CALIB_BLOCK_ROWS;
constexpr int MAXT = SEGMIF_CALIB_MAX_TEMPERATURES;
constexpr int MAXM = SEGMIF_CALIB_MAX_EDGES + 1;
constexpr int MAXK = SEGMIF_CALIB_MAX_THRESHOLDS;

struct CalArgs {
  const float* x;
  const long long* label;
  unsigned long long* counts;
  unsigned long long* above;
  unsigned long long* totals;
  double* partial;
  float* conf;
  int* pred;
  int B, IH, IW, OH, OW, C, ldx, NT, NE, NK;
  float sy, sx;
  float r[MAXT];  // 1 / T_t, formed on the host in float32
  float edge[MAXM];
  float tau[MAXK];
};

constexpr float FLT_MAX_F = 3.402823466e+38f;

__device__ __forceinline__ unsigned popc64(unsigned long long m) { return (unsigned)__popcll(m); }

template <int CMAX>
__global__ __launch_bounds__(THREADS) void calibration_kernel(CalArgs a) {
  __shared__ unsigned long long h_q[MAXT * MAXM];
  __shared__ double red[MAXT * 2 * WAVES];
  __shared__ unsigned h_n[MAXT * MAXM], h_c[MAXT * MAXM], a_n[MAXT * MAXK], a_c[MAXT * MAXK], tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.NE + 1, C = a.C;
  constexpr bool REG = CMAX > 0;  // the logits and exponentials of a pixel in registers, or (CMAX == 0) in the block's dynamic LDS
  extern __shared__ float planes[];
  float* const vs = planes + tid;
  float* const es = planes + C * THREADS + tid;
  for (int i = tid; i < a.NT * M; i += THREADS) h_n[i] = 0u, h_c[i] = 0u, h_q[i] = 0ull;
  for (int i = tid; i < a.NT * a.NK; i += THREADS) a_n[i] = 0u, a_c[i] = 0u;
  for (int i = tid; i < a.NT * 2 * WAVES; i += THREADS) red[i] = 0.0;
  if (tid < 4) tot[tid] = 0u;
  __syncthreads();

  const int ox = blockIdx.x * THREADS + tid;
  const long long b = blockIdx.z;
  const bool inside = ox < a.OW;
  const float fx = fmaxf(a.sx * ((float)ox + 0.5f) - 0.5f, 0.f);
  const int x0 = min((int)fx, a.IW - 1), x1 = min(x0 + 1, a.IW - 1);
  const float lx = fx - (float)x0, hx = 1.f - lx;
  const float* base = a.x + b * a.IH * a.IW * a.ldx;

#pragma unroll 1
  for (int ry = 0; ry < ROWS_PB; ++ry) {
    const int oy = blockIdx.y * ROWS_PB + ry;
    if (oy >= a.OH) break;  // (the same in every thread of the block)
    const long long o = (b * a.OH + oy) * a.OW + ox;
    const long long y = inside ? a.label[o] : -1ll;
    const bool labelled = inside && (unsigned long long)y < (unsigned long long)C;  // the full 64 bits
    const int yi = labelled ? (int)y : -1;
    const float fy = fmaxf(a.sy * ((float)oy + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, a.IH - 1), y1 = min(y0 + 1, a.IH - 1);
    const float ly = fy - (float)y0, hy = 1.f - ly;
    const float* p00 = base + ((long long)y0 * a.IW + x0) * a.ldx;
    const float* p01 = base + ((long long)y0 * a.IW + x1) * a.ldx;
    const float* p10 = base + ((long long)y1 * a.IW + x0) * a.ldx;
    const float* p11 = base + ((long long)y1 * a.IW + x1) * a.ldx;
    float v[REG ? CMAX : 1];
    float best = 0.f, vy = 0.f;
    int bi = 0;
    bool bad = false;
    if constexpr (REG) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c) v[c] = 0.f;
      if (labelled) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) v[c] = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
      }
      best = v[0], vy = v[0];
      bad = !(fabsf(v[0]) <= FLT_MAX_F);
#pragma unroll
      for (int c = 1; c < CMAX; ++c) {
        if (c < C) {
          bad |= !(fabsf(v[c]) <= FLT_MAX_F);
          if (v[c] > best) best = v[c], bi = c;
          if (c == yi) vy = v[c];
        }
      }
    } else {  // a thread's own column of the block's LDS planes: vs[c * THREADS], es[c * THREADS]
      best = -INFINITY;
      for (int c = 0; c < C; ++c) {
        const float x = labelled ? hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]) : 0.f;
        vs[c * THREADS] = x;
        bad |= !(fabsf(x) <= FLT_MAX_F);
        if (x > best || c == 0) best = x, bi = c;  // (c == 0: a NaN or -inf first channel is still the start)
        if (c == yi) vy = x;
      }
    }
    const bool valid = labelled && !bad;
    const bool correct = valid && bi == yi;
    if (inside && a.pred) a.pred[o] = valid ? bi : -1;
    {
      const unsigned long long mv = __ballot(valid), mi = __ballot(inside && !labelled), mn = __ballot(labelled && bad);
      if (lane == 0) {
        if (mv) atomicAdd(&tot[0], popc64(mv));
        if (mi) atomicAdd(&tot[1], popc64(mi));
        if (mn) atomicAdd(&tot[2], popc64(mn));
      }
    }
    if (!__syncthreads_or((int)valid) && !a.conf) continue;  // a row block without a valid pixel (the same in every thread)

#pragma unroll 1
    for (int t = 0; t < a.NT; ++t) {
      const float r = a.r[t];
      float e[REG ? CMAX : 1];
      float s = 0.f, brier = 0.f;
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          e[c] = 0.f;
          if (c < C) {
            e[c] = c == bi ? 1.f : expf((v[c] - best) * r);
            s += e[c];
          }
        }
      } else {
        for (int c = 0; c < C; ++c) {
          const float ec = c == bi ? 1.f : expf((vs[c * THREADS] - best) * r);
          es[c * THREADS] = ec;
          s += ec;
        }
      }
      const float conf = 1.f / s;
      const float nll = logf(s) - (vy - best) * r;
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          if (c < C) {
            const float d = e[c] * conf - (c == yi ? 1.f : 0.f);
            brier += d * d;
          }
        }
      } else {
        for (int c = 0; c < C; ++c) {
          const float d = es[c * THREADS] * conf - (c == yi ? 1.f : 0.f);
          brier += d * d;
        }
      }
      int bin = 0;
      for (int k = 0; k < a.NE; ++k) bin += conf >= a.edge[k] ? 1 : 0;
      if (inside && a.conf) a.conf[(((long long)t * a.B + b) * a.OH + oy) * a.OW + ox] = valid ? conf : NAN;
      const unsigned long long q = (unsigned long long)(conf * 4294967296.f);  // exact: conf >= 1 / 32 up to rounding

      // the reliability table: once per bin that occurs in this wave
      unsigned long long todo = __ballot(valid);
      while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int b0 = __shfl(bin, lead);
        const bool in = valid && bin == b0;
        const unsigned long long m = __ballot(in), mc = __ballot(in && correct);
        unsigned long long qs = in ? q : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) qs += __shfl_xor(qs, off);
        if (lane == lead) {
          const int i = t * M + b0;
          atomicAdd(&h_n[i], popc64(m));
          if (mc) atomicAdd(&h_c[i], popc64(mc));
          atomicAdd(&h_q[i], qs);
        }
        todo &= ~m;
      }
      for (int k = 0; k < a.NK; ++k) {
        const bool over = valid && conf > a.tau[k];  // strict, as pseudo_label's
        const unsigned long long m = __ballot(over), mc = __ballot(over && correct);
        if (lane == 0 && m) {
          atomicAdd(&a_n[t * a.NK + k], popc64(m));
          if (mc) atomicAdd(&a_c[t * a.NK + k], popc64(mc));
        }
      }
      double sn = valid ? (double)nll : 0.0, sb = valid ? (double)brier : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sn += __shfl_xor(sn, off);
        sb += __shfl_xor(sb, off);
      }
      if (lane == 0) {  // this wave's own slots, row after row
        red[(t * 2 + 0) * WAVES + wave] += sn;
        red[(t * 2 + 1) * WAVES + wave] += sb;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < a.NT * M; i += THREADS) {
    unsigned long long* out = a.counts + (long long)i * 3;
    if (h_n[i]) atomicAdd(out + 0, (unsigned long long)h_n[i]);
    if (h_c[i]) atomicAdd(out + 1, (unsigned long long)h_c[i]);
    if (h_q[i]) atomicAdd(out + 2, h_q[i]);
  }
  for (int i = tid; i < a.NT * a.NK; i += THREADS) {
    if (a_n[i]) atomicAdd(a.above + (long long)i * 2 + 0, (unsigned long long)a_n[i]);
    if (a_c[i]) atomicAdd(a.above + (long long)i * 2 + 1, (unsigned long long)a_c[i]);
  }
  if (tid < 3 && tot[tid]) atomicAdd(a.totals + tid, (unsigned long long)tot[tid]);
  if (tid < a.NT * 2) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double* w = red + tid * WAVES;
    a.partial[blk * (a.NT * 2) + tid] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

// block `out` of NT * 2: the blocks' partials of one sum, strided per thread, then a tree - a fixed order - and ONE add to the
// running value
__global__ __launch_bounds__(THREADS) void calibration_final_kernel(const double* __restrict__ partial, long long nblk, int n_out,
                                                                    double* __restrict__ sums) {
  __shared__ double red[THREADS];
  const int out = blockIdx.x;
  double acc = 0.0;
  for (long long i = threadIdx.x; i < nblk; i += THREADS) acc += partial[i * n_out + out];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[out] = sums[out] + red[0];
}

bool extents_ok(int B, int OH, int OW, int NT) {
  return B >= 1 && OH >= 1 && OW >= 1 && NT >= 1 && NT <= MAXT && B <= SEGMIF_CALIB_MAX_GRID && OH <= SEGMIF_CALIB_MAX_GRID;
}

long long num_blocks(int B, int OH, int OW) {
  return (long long)((OW + THREADS - 1) / THREADS) * ((OH + ROWS_PB - 1) / ROWS_PB) * B;
}

bool desc_ok(const SegmifCalib* d) {
  if (d->n_temperatures < 1 || d->n_temperatures > MAXT || d->n_edges < 0 || d->n_edges > SEGMIF_CALIB_MAX_EDGES ||
      d->n_thresholds < 0 || d->n_thresholds > MAXK)
    return false;
  for (int t = 0; t < d->n_temperatures; ++t)
    if (!std::isfinite(d->temperatures[t]) || !(d->temperatures[t] > 0.f)) return false;
  float last = 0.f;
  for (int k = 0; k < d->n_edges; ++k) {  // (a NaN fails both comparisons)
    if (!(d->edges[k] > last && d->edges[k] < 1.f)) return false;
    last = d->edges[k];
  }
  for (int k = 0; k < d->n_thresholds; ++k)
    if (!(d->thresholds[k] >= 0.f && d->thresholds[k] <= 1.f)) return false;
  return true;
}

}  // namespace

extern "C" int64_t segmif_calibration_workspace_bytes(int B, int OH, int OW, int NT) {
  if (!extents_ok(B, OH, OW, NT)) return 0;
  return num_blocks(B, OH, OW) * NT * 2 * (int64_t)sizeof(double);
}

extern "C" int segmif_calibration_stats_f32(const SegmifCalib* desc, const float* x, const int64_t* label, int64_t* counts,
                                            int64_t* above, int64_t* totals, double* sums, void* workspace, float* conf_or_null,
                                            int32_t* pred_or_null, int B, int IH, int IW, int OH, int OW, int C, int ldx, void* stream) {
  if (!desc || !x || !label || !counts || !totals || !sums || !workspace) return SEGMIF_EINVAL;
  if (!desc_ok(desc) || (desc->n_thresholds > 0 && !above)) return SEGMIF_EINVAL;
  if (C < 1 || C > 32 || ldx < C || IH < 1 || IW < 1 || !extents_ok(B, OH, OW, desc->n_temperatures)) return SEGMIF_EINVAL;
  CalArgs a;
  a.x = x, a.label = (const long long*)label, a.counts = (unsigned long long*)counts, a.above = (unsigned long long*)above;
  a.totals = (unsigned long long*)totals, a.partial = (double*)workspace, a.conf = conf_or_null, a.pred = pred_or_null;
  a.B = B, a.IH = IH, a.IW = IW, a.OH = OH, a.OW = OW, a.C = C, a.ldx = ldx;
  a.NT = desc->n_temperatures, a.NE = desc->n_edges, a.NK = desc->n_thresholds;
  a.sy = (float)IH / (float)OH, a.sx = (float)IW / (float)OW;  // (as segmif_pseudo_label_f32 forms them)
  for (int t = 0; t < MAXT; ++t) a.r[t] = t < a.NT ? 1.f / desc->temperatures[t] : 1.f;
  for (int k = 0; k < MAXM; ++k) a.edge[k] = k < a.NE ? desc->edges[k] : 2.f;
  for (int k = 0; k < MAXK; ++k) a.tau[k] = k < a.NK ? desc->thresholds[k] : 2.f;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((OW + THREADS - 1) / THREADS), (unsigned)((OH + ROWS_PB - 1) / ROWS_PB), (unsigned)B);
  if (C <= 12)
    hipLaunchKernelGGL(calibration_kernel<12>, grid, dim3(THREADS), 0, s, a);
  else  // two planes of C x 256 floats in LDS: at most 64 KiB beside the 10.3 KiB of tables
    hipLaunchKernelGGL(calibration_kernel<0>, grid, dim3(THREADS), (size_t)2 * C * THREADS * sizeof(float), s, a);
  hipLaunchKernelGGL(calibration_final_kernel, dim3((unsigned)(a.NT * 2)), dim3(THREADS), 0, s, (const double*)workspace,
                     num_blocks(B, OH, OW), a.NT * 2, sums);
  return (int)hipGetLastError();
}
