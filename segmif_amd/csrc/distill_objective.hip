// Knowledge distillation on the nets' NHWC logits (include/segmif_distill.h): per-pixel KD (Hinton et al. 2015) and channel-wise
// distillation (CWD, Shu et al., ICCV 2021), forward and backward.  This project's addition, NOT the reference's training.
// Student s and teacher t: rows x C float32 (C <= 32), pitches lds / ldt, rows = B * P; z = x / T.
//   PIXEL    softmax over a row's classes:       k_i  = sum_c p_ic ((zt - lse_t,i) - (zs - lse_s,i)),   loss = T^2 sum k_i / rows,
//            dloss/ds_ic = (T / rows) (q_ic - p_ic)
//   CHANNEL  softmax over a sample's positions:  k_bc = sum_j p_bcj ((zt - lse_t,bc) - (zs - lse_s,bc)), loss = T^2 sum k_bc / (B C),
//            dloss/ds_bjc = (T / (B C)) (q_bcj - p_bcj)
// with p = softmax(zt), q = softmax(zs).  A probability is exp(z - max) / sum; the KL term is formed from (z - max) - log sum, never
// from log(p): a teacher probability that underflows to 0 contributes 0.  NaN / inf propagate as through torch's softmax.
// Every kernel that forms probabilities brings a block of ROWS rows through LDS with seg_rows.h (a 36-byte row does not coalesce
// per thread): first the teacher's, which the thread that owns a row turns into registers {p, z - lse}, then the student's into
// the same tile.
// Pixel forward: one launch (a double per block) + the one-block fixed-order sum.  Channel forward: a statistics launch on a grid
// (blocks per sample, B) - column threads (class c, group g) read a tile's rows g, g + G, ... from memory - whose blocks leave
// (max, sum exp) per class and tensor; one small block per sample that combines those in block order into the table {max, sum,
// log sum} the loss pass and the backward read; a loss launch on the statistics' grid that forms p (lt - ls) per row in registers,
// hands the products back through the tile and sums them per column in double; the same final sum.  Backward, both modes: one
// launch, the softmaxes recomputed, dstudent written through the tile already multiplied by upstream[0] and record[1].  No atomics,
// fixed-order sums, launch counts from the shapes.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "seg_rows.h"
#include "segmif_distill.h"
#include "segmif_hip.h"

using namespace segmif;

namespace {

static_assert(ROWS == SEGMIF_DISTILL_BLOCK_ROWS, "the header states the tile's rows");
constexpr int MAXBLK = SEGMIF_DISTILL_MAX_BLOCKS_PER_SAMPLE;
constexpr int TABLE = 6 * 32;  // floats of a sample's table: {max, sum, log sum} x {student, teacher} x 32 classes
constexpr int STAT = 4 * 32;   // floats of a block's statistics: {max, sum} x {student, teacher} x 32 classes

struct DistArgs {
  const float* s;
  const float* t;
  long long rows, P;
  int B, C, lds, ldt, vs, vt, mode, nbs;  // nbs: blocks per sample (channel)
  float T;
};

__host__ __device__ inline long long num_tiles(long long n) { return (n + ROWS - 1) / ROWS; }

// channel workspace: [B][TABLE] floats | [B][nbs] doubles (loss partials) | [B][nbs][STAT] floats (statistics partials)
struct ChannelWs {
  float* table;
  double* partial;
  float* stat;
};

__host__ __device__ inline ChannelWs carve(void* ws, int B, int nbs) {
  char* p = (char*)ws;
  ChannelWs w;
  w.table = (float*)p;
  w.partial = (double*)(p + (long long)B * TABLE * sizeof(float));
  w.stat = (float*)(p + (long long)B * TABLE * sizeof(float) + (long long)B * nbs * sizeof(double));
  return w;
}

// the weight of a partial (max m, sum S) under the common maximum M; a partial that saw nothing but -inf weighs 0
__device__ __forceinline__ float weight_of(float m, float M) { return m == -INFINITY ? 0.f : expf(m - M); }

// one row's softmax over its classes in registers: p[c] and lp[c] = z_c - lse (both 0 for c >= C)
template <int CMAX>
__device__ __forceinline__ void row_softmax(const float* __restrict__ x, int C, float T, float (&p)[CMAX], float (&lp)[CMAX]) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    lp[c] = c < C ? x[c] / T : -INFINITY;
    mx = fmaxf(mx, lp[c]);
  }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (c < C) {
      lp[c] -= mx;
      p[c] = expf(lp[c]);
      sum += p[c];
    } else {
      lp[c] = 0.f, p[c] = 0.f;
    }
  }
  const float logsum = logf(sum);
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (c < C) {
      p[c] = p[c] / sum;
      lp[c] -= logsum;
    }
  }
}

// one row's share of the softmaxes over positions, from a sample's table {max, sum, log sum}[32] in LDS
template <int CMAX>
__device__ __forceinline__ void row_from_table(const float* __restrict__ x, const float* __restrict__ tab, int C, float T,
                                               float (&p)[CMAX], float (&lp)[CMAX]) {
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (c < C) {
      const float d = x[c] / T - tab[c];
      p[c] = expf(d) / tab[32 + c];
      lp[c] = d - tab[64 + c];
    } else {
      p[c] = 0.f, lp[c] = 0.f;
    }
  }
}

// block-wide sum of one double per thread in a fixed order (a tree over red[ROWS]); every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = ROWS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

template <int CMAX>
__global__ __launch_bounds__(ROWS) void distill_pixel_fwd_kernel(DistArgs a, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  __shared__ double red[ROWS];
  const long long r0 = (long long)blockIdx.x * ROWS;
  const int nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  const bool mine = (int)threadIdx.x < nr;
  float p[CMAX], lt[CMAX];
  stage_rows(tile, a.t, r0, nr, a.C, a.ldt, a.vt);
  __syncthreads();
  if (mine) row_softmax<CMAX>(tile + threadIdx.x * PITCH, a.C, a.T, p, lt);
  __syncthreads();
  stage_rows(tile, a.s, r0, nr, a.C, a.lds, a.vs);
  __syncthreads();
  double v = 0.0;
  if (mine) {
    float q[CMAX], ls[CMAX];
    row_softmax<CMAX>(tile + threadIdx.x * PITCH, a.C, a.T, q, ls);
    float k = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < a.C) k += p[c] * (lt[c] - ls[c]);
    v = (double)k;
  }
  const double total = block_sum(v, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// (max, sum exp) of this block's tiles of sample blockIdx.y, per class, for the student and for the teacher.  No LDS staging here:
// thread (c, g) = g * C + c reads its column's rows g, g + G, ... straight from memory - with a dense pitch the G * C threads read
// G * C consecutive floats per step - twice (the tile's maximum, then sum exp(z - max): the second read finds the tile in cache).
__global__ __launch_bounds__(ROWS) void distill_channel_stats_kernel(DistArgs a, void* ws) {
  __shared__ float redm[2][ROWS], reds[2][ROWS];
  const ChannelWs W = carve(ws, a.B, a.nbs);
  const int b = blockIdx.y, C = a.C, G = ROWS / C;  // G groups of column threads
  const int c = threadIdx.x % C, g = threadIdx.x / C;
  const long long ntiles = num_tiles(a.P);
  float ms = -INFINITY, Ss = 0.f, mt = -INFINITY, St = 0.f;
  if (g < G) {
    for (long long tl = blockIdx.x; tl < ntiles; tl += a.nbs) {
      const long long p0 = tl * ROWS, r0 = (long long)b * a.P + p0;
      const int nr = (int)(a.P - p0 < ROWS ? a.P - p0 : ROWS);
      if (g >= nr) continue;
      const float* __restrict__ xs = a.s + r0 * a.lds + c;
      const float* __restrict__ xt = a.t + r0 * a.ldt + c;
      float tms = -INFINITY, tmt = -INFINITY;
      for (int r = g; r < nr; r += G) {
        tms = fmaxf(tms, xs[(long long)r * a.lds] / a.T);
        tmt = fmaxf(tmt, xt[(long long)r * a.ldt] / a.T);
      }
      float tss = 0.f, tst = 0.f;
      for (int r = g; r < nr; r += G) {
        const float zs = xs[(long long)r * a.lds] / a.T, zt = xt[(long long)r * a.ldt] / a.T;
        tss += zs == -INFINITY ? 0.f : expf(zs - tms);
        tst += zt == -INFINITY ? 0.f : expf(zt - tmt);
      }
      const float Ms = fmaxf(ms, tms), Mt = fmaxf(mt, tmt);
      Ss = Ss * weight_of(ms, Ms) + tss * weight_of(tms, Ms);
      St = St * weight_of(mt, Mt) + tst * weight_of(tmt, Mt);
      ms = Ms, mt = Mt;
    }
  }
  redm[0][threadIdx.x] = ms, reds[0][threadIdx.x] = Ss;
  redm[1][threadIdx.x] = mt, reds[1][threadIdx.x] = St;
  __syncthreads();
  if ((int)threadIdx.x < 2 * C) {  // per tensor and class, the groups in order
    const int which = (int)threadIdx.x / C, k0 = (int)threadIdx.x % C;
    float M = -INFINITY;
    for (int k = 0; k < G; ++k) M = fmaxf(M, redm[which][k * C + k0]);
    float sum = 0.f;
    for (int k = 0; k < G; ++k) sum += reds[which][k * C + k0] * weight_of(redm[which][k * C + k0], M);
    float* out = W.stat + ((long long)b * a.nbs + blockIdx.x) * STAT;
    out[(2 * which) * 32 + k0] = M;
    out[(2 * which + 1) * 32 + k0] = sum;
  }
}

// one block of 64 threads per sample: its table from its blocks' statistics, in block order -> the head of the workspace,
// [6][32] floats: student {max, sum, log sum}, teacher the same.  The loss pass and the backward read it from there.
__global__ __launch_bounds__(64) void distill_channel_table_kernel(DistArgs a, void* ws) {
  const ChannelWs W = carve(ws, a.B, a.nbs);
  const int b = blockIdx.x, which = threadIdx.x >> 5, c = threadIdx.x & 31;
  float* tab = W.table + (long long)b * TABLE + which * 96;
  if (c < a.C) {
    const float* st = W.stat + (long long)b * a.nbs * STAT + 2 * which * 32 + c;
    float M = -INFINITY;
    for (int k = 0; k < a.nbs; ++k) M = fmaxf(M, st[(long long)k * STAT]);
    float sum = 0.f;
    for (int k = 0; k < a.nbs; ++k) sum += st[(long long)k * STAT + 32] * weight_of(st[(long long)k * STAT], M);
    tab[c] = M, tab[32 + c] = sum, tab[64 + c] = logf(sum);
  } else {
    tab[c] = 0.f, tab[32 + c] = 1.f, tab[64 + c] = 0.f;
  }
}

template <int CMAX>
__global__ __launch_bounds__(ROWS) void distill_channel_loss_kernel(DistArgs a, void* ws) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  __shared__ float tab[TABLE];
  __shared__ double red[ROWS];
  const ChannelWs W = carve(ws, a.B, a.nbs);
  const int b = blockIdx.y, C = a.C, G = ROWS / C;
  const int c = threadIdx.x % C, g = threadIdx.x / C;
  const bool column = g < G;
  if (threadIdx.x < TABLE) tab[threadIdx.x] = W.table[(long long)b * TABLE + threadIdx.x];
  __syncthreads();
  const long long ntiles = num_tiles(a.P);
  double acc = 0.0;
  for (long long tl = blockIdx.x; tl < ntiles; tl += a.nbs) {
    const long long p0 = tl * ROWS, r0 = (long long)b * a.P + p0;
    const int nr = (int)(a.P - p0 < ROWS ? a.P - p0 : ROWS);
    const bool mine = (int)threadIdx.x < nr;
    float* row = tile + threadIdx.x * PITCH;
    float p[CMAX], lt[CMAX];
    stage_rows(tile, a.t, r0, nr, C, a.ldt, a.vt);
    __syncthreads();
    if (mine) row_from_table<CMAX>(row, tab + 96, C, a.T, p, lt);
    __syncthreads();
    stage_rows(tile, a.s, r0, nr, C, a.lds, a.vs);
    __syncthreads();
    if (mine) {
      float q[CMAX], ls[CMAX];
      row_from_table<CMAX>(row, tab, C, a.T, q, ls);
#pragma unroll
      for (int k = 0; k < CMAX; ++k)
        if (k < C) row[k] = p[k] * (lt[k] - ls[k]);
    }
    __syncthreads();
    if (column)
      for (int r = g; r < nr; r += G) acc += (double)tile[r * PITCH + c];
    __syncthreads();
  }
  const double total = block_sum(acc, red);
  if (threadIdx.x == 0) W.partial[(long long)b * a.nbs + blockIdx.x] = total;
}

// one block: n doubles in a fixed order (256 strided runs, then a tree) -> record {loss, gradient scale, T, loss / T^2}
__global__ __launch_bounds__(ROWS) void distill_final_kernel(const double* __restrict__ partial, long long n, double den, float T,
                                                            float* __restrict__ record) {
  __shared__ double red[ROWS];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += ROWS) s += partial[i];
  const double total = block_sum(s, red);
  if (threadIdx.x == 0) {
    const double mean = total / den;
    record[0] = (float)((double)T * (double)T * mean);
    record[1] = (float)((double)T / den);
    record[2] = T;
    record[3] = (float)mean;
  }
}

template <int CMAX>
__global__ __launch_bounds__(ROWS) void distill_bwd_kernel(DistArgs a, const void* ws, const float* __restrict__ record,
                                                          const float* __restrict__ upstream, float* __restrict__ g, int ldd,
                                                          int vec_out) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  __shared__ float tab[TABLE];
  const bool channel = a.mode == SEGMIF_DISTILL_CHANNEL;
  long long r0;
  int nr;
  if (channel) {
    const long long p0 = (long long)blockIdx.x * ROWS;
    r0 = (long long)blockIdx.y * a.P + p0;
    nr = (int)(a.P - p0 < ROWS ? a.P - p0 : ROWS);
    if (threadIdx.x < TABLE) tab[threadIdx.x] = ((const float*)ws)[(long long)blockIdx.y * TABLE + threadIdx.x];
  } else {
    r0 = (long long)blockIdx.x * ROWS;
    nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  }
  const bool mine = (int)threadIdx.x < nr;
  float* row = tile + threadIdx.x * PITCH;
  float p[CMAX], lp[CMAX];
  stage_rows(tile, a.t, r0, nr, a.C, a.ldt, a.vt);
  __syncthreads();
  if (mine) {
    if (channel)
      row_from_table<CMAX>(row, tab + 96, a.C, a.T, p, lp);
    else
      row_softmax<CMAX>(row, a.C, a.T, p, lp);
  }
  __syncthreads();
  stage_rows(tile, a.s, r0, nr, a.C, a.lds, a.vs);
  __syncthreads();
  if (mine) {
    float q[CMAX];
    if (channel)
      row_from_table<CMAX>(row, tab, a.C, a.T, q, lp);
    else
      row_softmax<CMAX>(row, a.C, a.T, q, lp);
    const float coef = upstream[0] * record[1];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < a.C) row[c] = coef * (q[c] - p[c]);
  }
  __syncthreads();
  unstage_rows(tile, g, r0, nr, a.C, ldd, vec_out);
}

bool known_mode(int mode) { return mode == SEGMIF_DISTILL_PIXEL || mode == SEGMIF_DISTILL_CHANNEL; }

// the geometry alone; false: refused
bool geometry_ok(int64_t rows, int64_t P, int C, int mode) {
  if (rows < 1 || P < 1 || rows % P != 0 || C < 1 || C > 32 || !known_mode(mode)) return false;
  if (mode == SEGMIF_DISTILL_CHANNEL) return rows / P <= SEGMIF_DISTILL_MAX_BATCH && num_tiles(P) <= 0x7fffffffLL;
  return num_tiles(rows) <= 0x7fffffffLL;
}

int blocks_per_sample(int64_t P) { return (int)(num_tiles(P) < MAXBLK ? num_tiles(P) : MAXBLK); }

// fills the kernel arguments; false: the descriptor or the geometry is refused
bool make_args(const SegmifDistill* d, const float* s, const float* t, int64_t rows, int64_t P, int C, int lds, int ldt, DistArgs& a) {
  if (!d || !s || !t || !geometry_ok(rows, P, C, d->mode) || lds < C || ldt < C) return false;
  if (!std::isfinite(d->temperature) || !(d->temperature > 0.f)) return false;
  a.s = s, a.t = t, a.rows = rows, a.P = P, a.B = (int)(rows / P), a.C = C, a.lds = lds, a.ldt = ldt;
  a.mode = d->mode, a.T = d->temperature;
  // a sample's first row must be 16-byte aligned too, where samples are walked one by one
  const bool starts = d->mode == SEGMIF_DISTILL_PIXEL || (P * C) % 4 == 0;
  a.vs = lds == C && aligned16(s) && starts;
  a.vt = ldt == C && aligned16(t) && starts;
  a.nbs = d->mode == SEGMIF_DISTILL_CHANNEL ? blocks_per_sample(P) : 0;
  return true;
}

}  // namespace

extern "C" int64_t segmif_distill_workspace_bytes(int64_t rows, int64_t rows_per_sample, int C, int mode) {
  if (!geometry_ok(rows, rows_per_sample, C, mode)) return 0;
  if (mode == SEGMIF_DISTILL_PIXEL) return num_tiles(rows) * (int64_t)sizeof(double);
  const int64_t B = rows / rows_per_sample, nbs = blocks_per_sample(rows_per_sample);
  return B * TABLE * (int64_t)sizeof(float) + B * nbs * (int64_t)sizeof(double) + B * nbs * STAT * (int64_t)sizeof(float);
}

extern "C" int segmif_distill_objective_f32(const SegmifDistill* desc, const float* student, const float* teacher, void* workspace,
                                            float* record4, int64_t rows, int64_t rows_per_sample, int C, int lds, int ldt,
                                            void* stream) {
  DistArgs a;
  if (!workspace || !record4 || !make_args(desc, student, teacher, rows, rows_per_sample, C, lds, ldt, a)) return SEGMIF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(ROWS);
  if (a.mode == SEGMIF_DISTILL_PIXEL) {
    const long long nblk = num_tiles(rows);
    if (C <= 12)
      hipLaunchKernelGGL(distill_pixel_fwd_kernel<12>, dim3((unsigned)nblk), block, 0, s, a, (double*)workspace);
    else
      hipLaunchKernelGGL(distill_pixel_fwd_kernel<32>, dim3((unsigned)nblk), block, 0, s, a, (double*)workspace);
    hipLaunchKernelGGL(distill_final_kernel, dim3(1), block, 0, s, (const double*)workspace, nblk, (double)rows, a.T, record4);
  } else {
    const dim3 grid((unsigned)a.nbs, (unsigned)a.B);
    hipLaunchKernelGGL(distill_channel_stats_kernel, grid, block, 0, s, a, workspace);
    hipLaunchKernelGGL(distill_channel_table_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a, workspace);
    if (C <= 12)
      hipLaunchKernelGGL(distill_channel_loss_kernel<12>, grid, block, 0, s, a, workspace);
    else
      hipLaunchKernelGGL(distill_channel_loss_kernel<32>, grid, block, 0, s, a, workspace);
    hipLaunchKernelGGL(distill_final_kernel, dim3(1), block, 0, s, (const double*)carve(workspace, a.B, a.nbs).partial,
                       (long long)a.B * a.nbs, (double)a.B * (double)C, a.T, record4);
  }
  return (int)hipGetLastError();
}

extern "C" int segmif_distill_objective_bwd_f32(const SegmifDistill* desc, const float* student, const float* teacher,
                                                const void* workspace, const float* record4, const float* upstream, float* dstudent,
                                                int64_t rows, int64_t rows_per_sample, int C, int lds, int ldt, int ldd, void* stream) {
  DistArgs a;
  if (!workspace || !record4 || !upstream || !dstudent || ldd < C ||
      !make_args(desc, student, teacher, rows, rows_per_sample, C, lds, ldt, a))
    return SEGMIF_EINVAL;
  const bool starts = a.mode == SEGMIF_DISTILL_PIXEL || (rows_per_sample * C) % 4 == 0;
  const int vec_out = ldd == C && aligned16(dstudent) && starts;
  const dim3 grid = a.mode == SEGMIF_DISTILL_PIXEL ? dim3((unsigned)num_tiles(rows))
                                                   : dim3((unsigned)num_tiles(rows_per_sample), (unsigned)a.B);
  if (C <= 12)
    hipLaunchKernelGGL(distill_bwd_kernel<12>, grid, dim3(ROWS), 0, (hipStream_t)stream, a, workspace, record4, upstream, dstudent,
                       ldd, vec_out);
  else
    hipLaunchKernelGGL(distill_bwd_kernel<32>, grid, dim3(ROWS), 0, (hipStream_t)stream, a, workspace, record4, upstream, dstudent,
                       ldd, vec_out);
  return (int)hipGetLastError();
}
