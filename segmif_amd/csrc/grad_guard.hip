// The guarded optimizer step (gfx950, wave64): global gradient norm, clipping and skip-on-non-finite, all decided on the device.
//   grad_sumsq_kernel     one block per 65 536-element chunk of the multi-tensor table: sum of squares in double + non-finite count
//   grad_finalize_kernel  one block: chunks -> entries -> total in a fixed order; norm, clip coefficient, skip flag, counters
//   adamw_guarded_kernel  adamw_kernel's arithmetic (csrc/backward.hip) on g * coef; returns untouched when the step is skipped
//   grad_scale_kernel     g *= coef in place (the stand-alone clip_grad_norm_)
// Every kernel walks the table (param, grad, m, v, numel, lr, wd) and the chunk_entry / chunk_off arrays that
// utils/optimizer.FusedAdamW uploads once per step.  No float atomics: every sum has one fixed order, so the record is bitwise
// reproducible.  The host never reads anything back inside a step; the decision travels from kernel to kernel in the record.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

struct GuardEntry {  // = backward.hip's AdamEntry (segmif_adamw_entry_bytes())
  float* p;
  float* g;
  float* m;
  float* v;
  long long n;
  float lr, wd;
};

struct ChunkPartial {
  double sumsq;
  uint32_t nonfinite, pad;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Thread t owns the float4 groups t, t + 256, .. of its chunk, and lane k of every group feeds accumulator k: the same
// assignment on the vector path (16-byte aligned gradient) and on the scalar one, so the sum does not depend on alignment.
// A float squared is exact in double (48 bits of product); only the additions round.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const GuardEntry* __restrict__ table, const int* __restrict__ chunk_entry,
                                                         const long long* __restrict__ chunk_off, int chunk_elems,
                                                         ChunkPartial* __restrict__ partial) {
  __shared__ double wsum[4];
  __shared__ uint32_t wbad[4];
  const GuardEntry e = table[chunk_entry[blockIdx.x]];
  const long long base = chunk_off[blockIdx.x];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t bad = 0;
  if (e.g && base < e.n) {
    const long long left = e.n - base;
    const int count = left < (long long)chunk_elems ? (int)left : chunk_elems;
    const float* g = e.g + base;
    const bool vec = aligned16(g);
    for (int i = threadIdx.x * 4; i < count; i += 1024) {
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec && i + 4 <= count) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(g + i);
        x[0] = q[0], x[1] = q[1], x[2] = q[2], x[3] = q[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i + k < count) x[k] = g[i + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (isfinite(x[k]))
          acc[k] += (double)x[k] * (double)x[k];
        else
          ++bad;
      }
    }
  }
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    bad += __shfl_down(bad, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wsum[wave] = s, wbad[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    ChunkPartial out;
    out.sumsq = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    out.nonfinite = wbad[0] + wbad[1] + wbad[2] + wbad[3];
    out.pad = 0;
    partial[blockIdx.x] = out;
  }
}

// One block.  The chunks of an entry are neighbours in the chunk arrays; the thread that meets an entry's first chunk adds that
// entry's partials in chunk order.  Then the entries are added in table order, 256 at a time through LDS, by thread 0.
__global__ __launch_bounds__(256) void grad_finalize_kernel(const GuardEntry* __restrict__ table, int nentries,
                                                            const int* __restrict__ chunk_entry, int nchunks,
                                                            const ChunkPartial* __restrict__ partial,
                                                            SegmifGradEntryStat* __restrict__ per_entry,
                                                            SegmifGradGuardRecord* __restrict__ rec, const int* __restrict__ entry_slot,
                                                            SegmifGradParamCount* __restrict__ param_count, float max_norm,
                                                            int skip_nonfinite) {
  __shared__ double tile_sum[256];
  __shared__ uint32_t tile_bad[256];
  __shared__ uint32_t skip_sh;
  for (int i = threadIdx.x; i < nentries; i += 256) {  // (an entry of zero elements owns no chunk)
    SegmifGradEntryStat z;
    z.sumsq = 0.0, z.nonfinite = 0, z.reserved = 0;
    per_entry[i] = z;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nchunks; c += 256) {
    const int ent = chunk_entry[c];
    if (ent < 0 || ent >= nentries || (c > 0 && chunk_entry[c - 1] == ent)) continue;
    double s = 0.0;
    uint32_t bad = 0;
    for (int k = c; k < nchunks && chunk_entry[k] == ent; ++k) s += partial[k].sumsq, bad += partial[k].nonfinite;
    SegmifGradEntryStat o;
    o.sumsq = s, o.nonfinite = bad, o.reserved = 0;
    per_entry[ent] = o;
  }
  __syncthreads();
  double total = 0.0;
  uint32_t total_bad = 0;
  for (int t0 = 0; t0 < nentries; t0 += 256) {
    const int i = t0 + threadIdx.x;
    tile_sum[threadIdx.x] = i < nentries ? per_entry[i].sumsq : 0.0;
    tile_bad[threadIdx.x] = i < nentries ? per_entry[i].nonfinite : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = nentries - t0 < 256 ? nentries - t0 : 256;
      for (int k = 0; k < m; ++k) total += tile_sum[k], total_bad += tile_bad[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    const float coef = fminf(1.0f, max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_; max_norm = +inf gives 1
    const uint32_t skip = (total_bad != 0 && skip_nonfinite) ? 1u : 0u;
    rec->sumsq = total;
    rec->norm = norm;
    rec->coef = coef;
    rec->nonfinite = total_bad;
    rec->skip_now = skip;
    rec->attempts += 1;
    if (skip) {
      rec->skipped += 1;
      rec->consecutive_skips += 1;
    } else {
      rec->applied += 1;
      rec->consecutive_skips = 0;
      if (coef < 1.0f) rec->clipped += 1;
    }
    skip_sh = skip;
  }
  __syncthreads();
  if (entry_slot && param_count) {  // per parameter: skipped steps it took part in (bias correction), steps it offended in
    const bool skip = skip_sh != 0;
    for (int i = threadIdx.x; i < nentries; i += 256) {
      if (!table[i].g) continue;
      const int slot = entry_slot[i];
      if (skip) param_count[slot].skipped += 1;
      if (per_entry[i].nonfinite) param_count[slot].offended += 1;
    }
  }
}

__device__ __forceinline__ float adamw_one(float p, float g, float& m, float& v, float b1, float b2, float eps, float step,
                                           float decay, float bc2_sqrt) {
  m = b1 * m + (1.0f - b1) * g;
  v = b2 * v + (1.0f - b2) * g * g;
  return p * decay - step * m / (sqrtf(v) / bc2_sqrt + eps);
}

// `step` counts this group's attempts (the host's state["step"]); the applied count t = step - skipped steps of the parameter.
// Thread 0 forms the bias corrections from t in double, as torch.optim.AdamW does on the host, and hands them over in LDS.
__global__ __launch_bounds__(256) void adamw_guarded_kernel(const GuardEntry* __restrict__ table, const int* __restrict__ chunk_entry,
                                                            const long long* __restrict__ chunk_off, double beta1, double beta2,
                                                            float eps, int step, int chunk_elems,
                                                            const SegmifGradGuardRecord* __restrict__ rec,
                                                            const int* __restrict__ entry_slot,
                                                            const SegmifGradParamCount* __restrict__ param_count) {
  __shared__ float bc[2];
  if (rec->skip_now) return;  // (uniform: before p, m or v is touched)
  const int ent = chunk_entry[blockIdx.x];
  const GuardEntry e = table[ent];
  const long long base = chunk_off[blockIdx.x];
  if (!e.g || base >= e.n) return;
  if (threadIdx.x == 0) {
    long long t = (long long)step - (long long)param_count[entry_slot[ent]].skipped;
    if (t < 1) t = 1;
    bc[0] = (float)(1.0 - pow(beta1, (double)t));
    bc[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
  }
  __syncthreads();
  const float coef = rec->coef;  // 1.0f exactly when nothing is clipped: g * coef == g
  const float b1 = (float)beta1, b2 = (float)beta2;
  const float lr_t = e.lr / bc[0], decay = 1.0f - e.lr * e.wd, bc2_sqrt = bc[1];
  const long long left = e.n - base;
  const int count = left < (long long)chunk_elems ? (int)left : chunk_elems;
  float* p = e.p + base;
  const float* g = e.g + base;
  float* m = e.m + base;
  float* v = e.v + base;
  const int nvec = (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) ? (count & ~3) : 0;
  for (int i = threadIdx.x * 4; i < nvec; i += 1024) {
    f32x4 pq = *reinterpret_cast<const f32x4*>(p + i), mq = *reinterpret_cast<const f32x4*>(m + i);
    f32x4 vq = *reinterpret_cast<const f32x4*>(v + i);
    const f32x4 gq = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float mk = mq[k], vk = vq[k];
      pq[k] = adamw_one(pq[k], gq[k] * coef, mk, vk, b1, b2, eps, lr_t, decay, bc2_sqrt);
      mq[k] = mk, vq[k] = vk;
    }
    *reinterpret_cast<f32x4*>(m + i) = mq;
    *reinterpret_cast<f32x4*>(v + i) = vq;
    *reinterpret_cast<f32x4*>(p + i) = pq;
  }
  for (int i = nvec + threadIdx.x; i < count; i += 256) {
    float mk = m[i], vk = v[i];
    p[i] = adamw_one(p[i], g[i] * coef, mk, vk, b1, b2, eps, lr_t, decay, bc2_sqrt);
    m[i] = mk, v[i] = vk;
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const GuardEntry* __restrict__ table, const int* __restrict__ chunk_entry,
                                                         const long long* __restrict__ chunk_off, int chunk_elems,
                                                         const SegmifGradGuardRecord* __restrict__ rec) {
  if (rec->skip_now) return;
  const float coef = rec->coef;
  if (coef == 1.0f) return;  // g * 1 is g: nothing to write
  const GuardEntry e = table[chunk_entry[blockIdx.x]];
  const long long base = chunk_off[blockIdx.x];
  if (!e.g || base >= e.n) return;
  const long long left = e.n - base;
  const int count = left < (long long)chunk_elems ? (int)left : chunk_elems;
  float* g = e.g + base;
  const int nvec = aligned16(g) ? (count & ~3) : 0;
  for (int i = threadIdx.x * 4; i < nvec; i += 1024) {
    f32x4 q = *reinterpret_cast<const f32x4*>(g + i);
    q *= coef;
    *reinterpret_cast<f32x4*>(g + i) = q;
  }
  for (int i = nvec + threadIdx.x; i < count; i += 256) g[i] *= coef;
}

bool bad_table(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks, int chunk_elems) {
  return !table || !chunk_entry || !chunk_off || nchunks <= 0 || chunk_elems <= 0 || (chunk_elems & 3) ||
         segmif_adamw_entry_bytes() != (int)sizeof(GuardEntry);
}

}  // namespace

static_assert(sizeof(SegmifGradGuardRecord) == 48, "SegmifGradGuardRecord layout");
static_assert(sizeof(SegmifGradEntryStat) == 16 && sizeof(SegmifGradParamCount) == 8, "per-entry / per-parameter layout");

extern "C" int segmif_grad_guard_record_bytes(void) { return (int)sizeof(SegmifGradGuardRecord); }
extern "C" int segmif_grad_entry_stat_bytes(void) { return (int)sizeof(SegmifGradEntryStat); }
extern "C" int segmif_grad_param_count_bytes(void) { return (int)sizeof(SegmifGradParamCount); }

extern "C" int64_t segmif_grad_norm_workspace_bytes(int nchunks) {
  return nchunks > 0 ? (int64_t)nchunks * (int64_t)sizeof(ChunkPartial) : 0;
}

extern "C" int segmif_grad_norm_f32(const void* table, int nentries, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks,
                                    int chunk_elems, void* workspace, SegmifGradEntryStat* per_entry, SegmifGradGuardRecord* record,
                                    const int32_t* entry_slot, SegmifGradParamCount* param_count, float max_norm, int skip_nonfinite,
                                    void* stream) {
  if (bad_table(table, chunk_entry, chunk_off, nchunks, chunk_elems) || nentries <= 0 || !workspace || !per_entry || !record ||
      !(max_norm > 0.f) || (entry_slot == nullptr) != (param_count == nullptr))
    return SEGMIF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, (const GuardEntry*)table, (const int*)chunk_entry,
                     (const long long*)chunk_off, chunk_elems, (ChunkPartial*)workspace);
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, s, (const GuardEntry*)table, nentries, (const int*)chunk_entry, nchunks,
                     (const ChunkPartial*)workspace, per_entry, record, (const int*)entry_slot, param_count, max_norm, skip_nonfinite);
  return (int)hipGetLastError();
}

extern "C" int segmif_adamw_guarded_f32(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks,
                                        int chunk_elems, double beta1, double beta2, float eps, int step,
                                        const SegmifGradGuardRecord* record, const int32_t* entry_slot,
                                        const SegmifGradParamCount* param_count, void* stream) {
  if (bad_table(table, chunk_entry, chunk_off, nchunks, chunk_elems) || !record || !entry_slot || !param_count || step < 1 ||
      !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return SEGMIF_EINVAL;
  hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const GuardEntry*)table,
                     (const int*)chunk_entry, (const long long*)chunk_off, beta1, beta2, eps, step, chunk_elems, record,
                     (const int*)entry_slot, param_count);
  return (int)hipGetLastError();
}

extern "C" int segmif_grad_scale_f32(const void* table, const int32_t* chunk_entry, const int64_t* chunk_off, int nchunks, int chunk_elems,
                                     const SegmifGradGuardRecord* record, void* stream) {
  if (bad_table(table, chunk_entry, chunk_off, nchunks, chunk_elems) || !record) return SEGMIF_EINVAL;
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const GuardEntry*)table,
                     (const int*)chunk_entry, (const long long*)chunk_off, chunk_elems, record);
  return (int)hipGetLastError();
}
