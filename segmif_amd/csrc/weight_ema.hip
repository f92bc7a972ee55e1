// Exponential moving average of the parameters (gfx950, wave64), one launch after the optimizer's update over the SAME multi-tensor
// table (param, grad, m, v, numel, lr, wd) and chunk_entry / chunk_off arrays that utils/optimizer.FusedAdamW uploads per step.
//   weight_ema_kernel   one block per 65 536-element chunk: (hi, lo) <- (hi, lo) + (1 - d_t) * (p - (hi, lo))
// The average is a PAIR of floats, hi + lo, updated in double: at decay 0.9999 and learning rates of 1e-4 and below the increment
// (1 - d) * (p - ema) lies at or under half an ulp of a float32 average, which then rounds it away and stops averaging.  The pair
// carries 48 bits; hi alone is the float32 rounding of the average and is what a model loads.
// Purely element-wise: no atomics, no reductions, so the result is bitwise reproducible.  Non-finite values are not special-cased:
// a p that is inf or NaN makes its average NaN.  The kernel reads p, hi, lo (12 bytes) and writes hi, lo (8 bytes) per element; the
// double arithmetic (two conversions, one fma, one subtraction per element) sits under that traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

struct EmaEntry {  // = backward.hip's AdamEntry (segmif_adamw_entry_bytes()); only p and n are read here
  float* p;
  float* g;
  float* m;
  float* v;
  long long n;
  float lr, wd;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ void ema_one(float p, float& hi, float& lo, double a) {
  double e = (double)hi + (double)lo;
  e += a * ((double)p - e);
  hi = (float)e;
  lo = (float)(e - (double)hi);
}

// `step` counts the group's attempts (the host's state["step"]); with the guard's per-parameter counts the applied count is
// t = step - skipped steps of the parameter, exactly what adamw_guarded_kernel's bias correction uses.  Thread 0 forms
// a = 1 - d_t in double once and hands it over in LDS.
__global__ __launch_bounds__(256) void weight_ema_kernel(const EmaEntry* __restrict__ table, float* const* __restrict__ ema,
                                                         const int* __restrict__ chunk_entry, const long long* __restrict__ chunk_off,
                                                         int chunk_elems, double decay, int warmup, int step,
                                                         const SegmifGradGuardRecord* __restrict__ rec,
                                                         const int* __restrict__ entry_slot,
                                                         const SegmifGradParamCount* __restrict__ param_count) {
  __shared__ double a_sh;
  if (rec && rec->skip_now) return;  // (uniform: before hi or lo is touched)
  const int ent = chunk_entry[blockIdx.x];
  const EmaEntry e = table[ent];
  const long long base = chunk_off[blockIdx.x];
  if (!e.p || base >= e.n) return;
  if (threadIdx.x == 0) {
    long long t = (long long)step;
    if (entry_slot && param_count) t -= (long long)param_count[entry_slot[ent]].skipped;
    if (t < 1) t = 1;
    double d = decay;
    if (warmup) {
      const double w = (1.0 + (double)t) / (10.0 + (double)t);
      d = w < d ? w : d;
    }
    a_sh = 1.0 - d;
  }
  __syncthreads();
  const double a = a_sh;
  const long long left = e.n - base;
  const int count = left < (long long)chunk_elems ? (int)left : chunk_elems;
  const float* p = e.p + base;
  float* hi = ema[2 * ent] + base;
  float* lo = ema[2 * ent + 1] + base;
  const int nvec = (aligned16(p) && aligned16(hi) && aligned16(lo)) ? (count & ~3) : 0;
  for (int i = threadIdx.x * 4; i < nvec; i += 1024) {
    const f32x4 pq = *reinterpret_cast<const f32x4*>(p + i);
    f32x4 hq = *reinterpret_cast<const f32x4*>(hi + i), lq = *reinterpret_cast<const f32x4*>(lo + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float hk = hq[k], lk = lq[k];
      ema_one(pq[k], hk, lk, a);
      hq[k] = hk, lq[k] = lk;
    }
    *reinterpret_cast<f32x4*>(hi + i) = hq;
    *reinterpret_cast<f32x4*>(lo + i) = lq;
  }
  for (int i = nvec + threadIdx.x; i < count; i += 256) {
    float hk = hi[i], lk = lo[i];
    ema_one(p[i], hk, lk, a);
    hi[i] = hk, lo[i] = lk;
  }
}

}  // namespace

extern "C" int segmif_weight_ema_f32(const void* table, float* const* ema, const int32_t* chunk_entry, const int64_t* chunk_off,
                                     int nchunks, int chunk_elems, double decay, int warmup, int step,
                                     const SegmifGradGuardRecord* record, const int32_t* entry_slot,
                                     const SegmifGradParamCount* param_count, void* stream) {
  if (!table || !ema || !chunk_entry || !chunk_off || nchunks <= 0 || chunk_elems <= 0 || (chunk_elems & 3) ||
      segmif_adamw_entry_bytes() != (int)sizeof(EmaEntry) || !(decay > 0.0 && decay < 1.0) || step < 1 ||
      (entry_slot == nullptr) != (param_count == nullptr))
    return SEGMIF_EINVAL;
  hipLaunchKernelGGL(weight_ema_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const EmaEntry*)table, ema,
                     (const int*)chunk_entry, (const long long*)chunk_off, chunk_elems, decay, warmup, step, record,
                     (const int*)entry_slot, param_count);
  return (int)hipGetLastError();
}
