// The region objectives added to the per-pixel ones of seg_objective.hip: Lovasz-Softmax (Berman et al. 2018, the batch as one set)
// and soft Dice, over NHWC logits (rows x C, pitch ld >= C, C <= 32) and int64 labels.  Neither is the reference's.  A row is valid
// when its label lies in [0, C) and is not ignore_index; p = softmax(x), fg_ic = [y_i == c], sums over the P valid rows:
//   Lovasz  e_ic = |fg_ic - p_ic|, for the labelled class formed as q = sum_{k != y} e_k / sum e_k (never 1 - p_y).  Per class the
//           errors are sorted in descending order, bit-equal float32 errors by ASCENDING ROW INDEX; with G = sum fg and F_k the
//           foreground rows among the first k:  J_k = 1 - (G - F_k) / (G + k - F_k), J_0 = 0, g_k = J_k - J_{k-1},
//           loss_c = sum_k e_(k) g_k.  An absent class (G = 0) gives g = (1, 0, 0, ...): loss_c = max_i p_ic.
//           Gradient: g taken as constant, d loss_c / d e_i = g_rank(i), through sign(p_ic - fg_ic) and the softmax.
//   Dice    I_c = sum p_ic fg_ic, S_c = sum p_ic, G_c = sum fg_ic, D_c = 1 - (2 I_c + s) / (S_c + G_c + s).
// The result is the mean over the classes with G > 0 (PRESENT) or over all C (ALL); with no valid row it is 0 with gradient 0.
//
// Lovasz, forward: the row pass writes, per class, a (key, value) pair per row: key = bits(1.0f) - bits(e) - the errors lie in
// [0, 1], so their raw bits are ordered and an ASCENDING sort of the key is the descending sort of e; an invalid row gets
// bits(1.0f) + 1 and lands behind every valid one - and value = row << 1 | fg.  A stable LSD radix sort follows, four 8-bit digits,
// every class in one grid (blockIdx.y), three launches per digit:
//   histogram  per tile of 2048 pairs, written digit-major: hist[class][digit][tile]           (LDS integer atomics: counts only)
//   scan       one block per class, exclusive, over the 256 x tiles counters in that order
//   scatter    a pair's place = scanned counter of (digit, tile) + pairs of that digit before it in the tile, and that rank is
//              ballots and prefix sums, never an atomic: 64 pairs per wave and round in index order, the lanes with the same digit
//              found by eight ballots, the waves' and rounds' counts added in order.  The order of ties is therefore the row order.
// Then the foreground flags of the sorted pairs are counted per tile and scanned (integers), and one pass forms g_k in double from
// the integers (k, F_k, G), accumulates e g in a fixed order and scatters g back to row order (into the second sort buffer, free
// by then) for the backward.  A one-block finish writes the record and the per-class weights.  Dice: the row pass writes per-block
// double partials of I, S, G; the finish forms D_c and the two coefficients of d D_c / d p_ic.
// Backward: one launch; recomputes the softmax, reads a_c = d loss / d p_c (Lovasz: -+ g / n; Dice: (b_c - a_c fg) / n), the record's
// 1 / n and the upstream gradient on the device and writes dx_j = p_j (a_j - sum_c a_c p_c), the labelled logit's through q.
// Hand-over between workgroups only across launches; the launch sequence does not depend on the data; integer atomics only in
// LDS histograms; every floating-point sum in a fixed order: bit-identical from run to run, no host synchronisation, capturable.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "seg_rows.h"
#include "segmif_hip.h"

using namespace segmif;

namespace {

constexpr int ITEMS = 8;              // rounds of a sort tile
constexpr int TILE = ROWS * ITEMS;    // pairs of a sort tile
constexpr int SCAN_THREADS = 1024;
constexpr unsigned KEY_ONE = 0x3f800000u, KEY_INVALID = KEY_ONE + 1u;  // keys of e = 0 (the last valid one) and of an invalid row
constexpr int HEADER = 512;           // bytes: float weight[32] (1 for an averaged class, else 0), a[32], b[32]; unsigned G[32]

struct RegArgs {
  const float* x;
  const long long* labels;
  long long rows;
  int C, ld, vec, ignore_index, kind;
};

struct Workspace {
  float *weight, *a, *b;  // per class
  unsigned* G;            // per class: foreground rows (Lovasz)
  double* partial;        // Lovasz [C][tiles]; Dice [row blocks][C][3]
  unsigned* hist;         // [C][256][tiles]
  unsigned* tilefg;       // [C][tiles]
  uint2 *buf0, *buf1;     // [C][rows] pairs; buf1 holds g [C][rows] floats after the sort
};

__host__ __device__ inline long long row_blocks(long long rows) { return (rows + ROWS - 1) / ROWS; }
__host__ __device__ inline long long sort_tiles(long long rows) { return (rows + TILE - 1) / TILE; }
__host__ __device__ inline long long pad16(long long bytes) { return (bytes + 15) & ~15LL; }

// byte offsets of the parts behind the header, each on a 16-byte boundary, and the size of the whole
struct Layout {
  long long hist, tilefg, buf0, buf1, bytes;
};

__host__ __device__ inline Layout layout(long long rows, int C, int kind) {
  Layout l = {0, 0, 0, 0, 0};
  if (kind == SEGMIF_REGION_DICE) {
    l.bytes = HEADER + row_blocks(rows) * C * 3 * (long long)sizeof(double);
    return l;
  }
  const long long nt = sort_tiles(rows);
  l.hist = HEADER + pad16(C * nt * (long long)sizeof(double));
  l.tilefg = l.hist + C * 256 * nt * (long long)sizeof(unsigned);
  l.buf0 = l.tilefg + pad16(C * nt * (long long)sizeof(unsigned));
  l.buf1 = l.buf0 + pad16(C * rows * (long long)sizeof(uint2));
  l.bytes = l.buf1 + C * rows * (long long)sizeof(uint2);
  return l;
}

__host__ __device__ inline void carve(void* ws, long long rows, int C, int kind, Workspace& w) {
  char* p = (char*)ws;
  const Layout l = layout(rows, C, kind);
  w.weight = (float*)p, w.a = w.weight + 32, w.b = w.weight + 64, w.G = (unsigned*)(w.weight + 96);
  w.partial = (double*)(p + HEADER);
  w.hist = (unsigned*)(p + l.hist), w.tilefg = (unsigned*)(p + l.tilefg);  // (Lovasz only)
  w.buf0 = (uint2*)(p + l.buf0), w.buf1 = (uint2*)(p + l.buf1);
}

__device__ __forceinline__ bool is_valid(const RegArgs& a, long long lab) { return lab != a.ignore_index && lab >= 0 && lab < a.C; }

// one row's softmax in registers: p[c] (0 for c >= C), q = 1 - p_y without the cancellation; all of them in [0, 1]
__device__ __forceinline__ void row_softmax(const float* __restrict__ t, int C, int y, float (&p)[32], float& q) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    p[c] = c < C ? t[c] : -INFINITY;
    mx = fmaxf(mx, p[c]);
  }
  float sum = 0.f, rest = 0.f;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if (c < C) {
      const float e = expf(p[c] - mx);
      p[c] = e;
      sum += e;
      if (c != y) rest += e;
    } else {
      p[c] = 0.f;
    }
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < 32; ++c) p[c] = fminf(p[c] * inv, 1.f);
  q = fminf(rest * inv, 1.f);
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// Lovasz: the pairs of every class; Dice: the block's partials of I, S, G
__global__ __launch_bounds__(ROWS) void region_fwd_kernel(RegArgs a, void* ws) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  __shared__ double red[4][32][3];
  Workspace W;
  carve(ws, a.rows, a.C, a.kind, W);
  const long long r0 = (long long)blockIdx.x * ROWS, row = r0 + threadIdx.x;
  const int nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  stage_rows(tile, a.x, r0, nr, a.C, a.ld, a.vec);
  __syncthreads();
  const bool live = (int)threadIdx.x < nr;
  const long long lab = live ? a.labels[row] : -1;
  const bool valid = live && is_valid(a, lab);
  const int y = valid ? (int)lab : -1;
  float p[32], q = 0.f;
  if (valid) {
    row_softmax(tile + threadIdx.x * PITCH, a.C, y, p, q);
  } else {
#pragma unroll
    for (int c = 0; c < 32; ++c) p[c] = 0.f;
  }
  if (a.kind == SEGMIF_REGION_LOVASZ) {
    if (live) {
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        if (c < a.C) {
          const unsigned key = valid ? KEY_ONE - __float_as_uint(c == y ? q : p[c]) : KEY_INVALID;
          W.buf0[(long long)c * a.rows + row] = make_uint2(key, ((unsigned)row << 1) | (c == y ? 1u : 0u));
        }
      }
    }
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if (c < a.C) {  // (uniform)
      const double s = wave_sum((double)p[c]), i = wave_sum(c == y ? (double)p[c] : 0.0), g = wave_sum(c == y ? 1.0 : 0.0);
      if (lane == 0) red[wave][c][0] = i, red[wave][c][1] = s, red[wave][c][2] = g;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < a.C * 3) {
    const int c = threadIdx.x / 3, k = threadIdx.x % 3;
    W.partial[(long long)blockIdx.x * a.C * 3 + threadIdx.x] = ((red[0][c][k] + red[1][c][k]) + red[2][c][k]) + red[3][c][k];
  }
}

// digit `shift / 8` of the tile's keys -> hist[class][digit][tile]
__global__ __launch_bounds__(ROWS) void region_hist_kernel(const uint2* __restrict__ src, unsigned* __restrict__ hist, long long rows,
                                                           long long tiles, int shift) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long cb = (long long)blockIdx.y * rows, i0 = (long long)blockIdx.x * TILE;
  for (int it = 0; it < ITEMS; ++it) {
    const long long i = i0 + it * ROWS + threadIdx.x;
    if (i < rows) atomicAdd(&h[(src[cb + i].x >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[((long long)blockIdx.y * 256 + threadIdx.x) * tiles + blockIdx.x] = h[threadIdx.x];
}

// one block per class: data[class][0 .. n) -> its exclusive prefix sums in place; total[class] (when given) = the sum
__global__ __launch_bounds__(SCAN_THREADS) void region_scan_kernel(unsigned* __restrict__ data, long long n, unsigned* __restrict__ total) {
  __shared__ unsigned wsum[SCAN_THREADS / 64];
  unsigned* d = data + (long long)blockIdx.x * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;
  for (long long i0 = 0; i0 < n; i0 += 4 * SCAN_THREADS) {
    const long long i = i0 + 4 * threadIdx.x;
    unsigned v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? d[i + j] : 0u;
    const unsigned s = (v[0] + v[1]) + (v[2] + v[3]);
    unsigned inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      if (w < wave) before += wsum[w];
      all += wsum[w];
    }
    __syncthreads();
    unsigned ex = carry + before + (inc - s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < n) d[i + j] = ex;
      ex += v[j];
    }
    carry += all;
  }
  if (total && threadIdx.x == 0) total[blockIdx.x] = carry;
}

// the lanes of the wave that hold the same digit as this one (among the active lanes)
__device__ __forceinline__ unsigned long long same_digit(unsigned digit, bool active) {
  unsigned long long mask = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bal = __ballot(active && bit);
    mask &= bit ? bal : ~bal;
  }
  return mask;
}

__global__ __launch_bounds__(ROWS) void region_scatter_kernel(const uint2* __restrict__ src, uint2* __restrict__ dst,
                                                              const unsigned* __restrict__ hist, long long rows, long long tiles,
                                                              int shift) {
  __shared__ unsigned base[256];      // where the tile's next pair of a digit goes (within the class)
  __shared__ unsigned count[4][256];  // pairs of a digit in each wave's 64 of this round
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cb = (long long)blockIdx.y * rows, i0 = (long long)blockIdx.x * TILE;
  base[threadIdx.x] = hist[((long long)blockIdx.y * 256 + threadIdx.x) * tiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) count[w][threadIdx.x] = 0;
  __syncthreads();
  for (int it = 0; it < ITEMS; ++it) {
    if (i0 + it * ROWS >= rows) break;  // (uniform)
    const long long i = i0 + it * ROWS + threadIdx.x;
    const bool active = i < rows;
    const uint2 kv = active ? src[cb + i] : make_uint2(0u, 0u);
    const unsigned digit = (kv.x >> shift) & 255u;
    const unsigned long long mask = same_digit(digit, active);
    const unsigned rank = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (active && rank == 0) count[wave][digit] = (unsigned)__popcll(mask);
    __syncthreads();
    if (active) {
      unsigned pos = base[digit] + rank;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (w < wave) pos += count[w][digit];
      if (pos < rows) dst[cb + pos] = kv;  // (always: the counters were made from these very keys)
    }
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += count[w][threadIdx.x], count[w][threadIdx.x] = 0;
    base[threadIdx.x] += s;
    __syncthreads();
  }
}

// foreground rows of each tile of the sorted pairs
__global__ __launch_bounds__(ROWS) void region_fgcount_kernel(const uint2* __restrict__ sorted, unsigned* __restrict__ tilefg,
                                                              long long rows, long long tiles) {
  __shared__ unsigned wc[4];
  const long long cb = (long long)blockIdx.y * rows, i0 = (long long)blockIdx.x * TILE;
  unsigned n = 0;
  for (int it = 0; it < ITEMS; ++it) {
    const long long i = i0 + it * ROWS + threadIdx.x;
    if (i < rows) {
      const uint2 kv = sorted[cb + i];
      n += kv.x <= KEY_ONE ? (kv.y & 1u) : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) tilefg[(long long)blockIdx.y * tiles + blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
}

__device__ __forceinline__ double jaccard(double G, double k, double F) { return 1.0 - (G - F) / (G + k - F); }

// g_k of the tile's sorted pairs from (k, F_k, G); sum e g -> partial[class][tile]; g -> gout[class][row]
__global__ __launch_bounds__(ROWS) void region_lovasz_kernel(const uint2* __restrict__ sorted, const unsigned* __restrict__ tilefg,
                                                             const unsigned* __restrict__ Gs, float* __restrict__ gout,
                                                             double* __restrict__ partial, long long rows, long long tiles) {
  __shared__ unsigned wc[4];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cb = (long long)blockIdx.y * rows, i0 = (long long)blockIdx.x * TILE;
  const double G = (double)Gs[blockIdx.y];
  unsigned running = tilefg[(long long)blockIdx.y * tiles + blockIdx.x];  // foreground rows before this tile
  double acc = 0.0;
  for (int it = 0; it < ITEMS; ++it) {
    if (i0 + it * ROWS >= rows) break;  // (uniform)
    const long long i = i0 + it * ROWS + threadIdx.x;
    const uint2 kv = i < rows ? sorted[cb + i] : make_uint2(KEY_INVALID, 0u);
    const bool valid = kv.x <= KEY_ONE, fg = valid && (kv.y & 1u);
    const unsigned long long bal = __ballot(fg);
    if (lane == 0) wc[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = running + (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += wc[w];
      all += wc[w];
    }
    if (valid) {  // the valid rows are the first P of the order: this one is the k-th, k = i + 1
      const double k = (double)(i + 1), F0 = (double)before, F1 = F0 + (fg ? 1.0 : 0.0);
      const double g = jaccard(G, k, F1) - (i == 0 ? 0.0 : jaccard(G, k - 1.0, F0));
      acc += (double)__uint_as_float(KEY_ONE - kv.x) * g;
      const long long row = (long long)(kv.y >> 1);
      if (row < rows) gout[cb + row] = (float)g;
    }
    __syncthreads();
    running += all;
  }
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * tiles + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one block: the partials in a fixed order (256 strided runs, then a tree), then the record {loss, 1 / n, n, P} (n classes
// averaged, P valid rows), the classes' weights (1 for an averaged class, else 0) and, for Dice, the coefficients of
// d D_c / d p_ic = b_c - a_c fg_ic
__global__ __launch_bounds__(256) void region_final_kernel(void* ws, long long rows, int C, int kind, int classes, float smooth,
                                                           float* __restrict__ record) {
  __shared__ double red[256];
  __shared__ double sums[32][3];
  Workspace W;
  carve(ws, rows, C, kind, W);
  const bool dice = kind == SEGMIF_REGION_DICE;
  const long long n = dice ? row_blocks(rows) : sort_tiles(rows);
  for (int c = 0; c < C; ++c) {
    for (int k = 0; k < (dice ? 3 : 1); ++k) {
      double s = 0.0;
      for (long long b = threadIdx.x; b < n; b += 256) s += dice ? W.partial[(b * C + c) * 3 + k] : W.partial[(long long)c * n + b];
      red[threadIdx.x] = s;
      __syncthreads();
      for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
      }
      if (threadIdx.x == 0) sums[c][k] = red[0];
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    double total = 0.0, P = 0.0;
    int averaged = 0;
    for (int c = 0; c < C; ++c) P += dice ? sums[c][2] : (double)W.G[c];
    for (int c = 0; c < C; ++c) {
      const double G = dice ? sums[c][2] : (double)W.G[c];
      const bool in = P > 0.0 && (classes == SEGMIF_REGION_ALL || G > 0.0);
      double a = 0.0, b = 0.0, l = sums[c][0];
      if (dice) {
        const double I = sums[c][0], den = sums[c][1] + G + (double)smooth;
        l = 1.0 - (2.0 * I + (double)smooth) / den;
        a = 2.0 / den, b = (2.0 * I + (double)smooth) / (den * den);
      }
      if (in) total += l, ++averaged;
      W.a[c] = in ? (float)a : 0.f, W.b[c] = in ? (float)b : 0.f;
      W.weight[c] = in ? 1.f : 0.f;
    }
    const double inv = averaged ? 1.0 / (double)averaged : 0.0;
    record[0] = averaged ? (float)(total * inv) : 0.f, record[1] = (float)inv, record[2] = (float)averaged, record[3] = (float)P;
  }
}

__global__ __launch_bounds__(ROWS) void region_bwd_kernel(RegArgs a, const void* ws, const float* __restrict__ record,
                                                          const float* __restrict__ upstream, float* __restrict__ g, int ldd,
                                                          int vec_out) {
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  Workspace W;
  carve(const_cast<void*>(ws), a.rows, a.C, a.kind, W);
  const long long r0 = (long long)blockIdx.x * ROWS, row = r0 + threadIdx.x;
  const int nr = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  stage_rows(tile, a.x, r0, nr, a.C, a.ld, a.vec);
  __syncthreads();
  if ((int)threadIdx.x < nr) {
    float* t = tile + threadIdx.x * PITCH;
    const long long lab = a.labels[row];
    if (is_valid(a, lab)) {
      const int y = (int)lab;
      const float up = upstream[0] * record[1];  // an averaged class's share of the mean, times the upstream gradient
      const float* coef = reinterpret_cast<const float*>(W.buf1);  // Lovasz: g [C][rows]
      float p[32], q, ay = 0.f, py = 0.f, rest = 0.f;                         // a_c = d loss / d p_c; rest = sum_{c != y} a_c p_c
      row_softmax(t, a.C, y, p, q);
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        if (c < a.C) {
          const float w = up * W.weight[c];
          float ac;
          if (a.kind == SEGMIF_REGION_LOVASZ) {
            ac = w * coef[(long long)c * a.rows + row];
            if (c == y) ac = -ac;  // e = 1 - p_y there, p_c elsewhere
          } else {
            ac = w * (W.b[c] - (c == y ? W.a[c] : 0.f));
          }
          if (c == y) {
            ay = ac, py = p[c];
          } else {
            rest += ac * p[c];
          }
          t[c] = ac;
        }
      }
      const float s = ay * py + rest;
#pragma unroll
      for (int c = 0; c < 32; ++c)
        if (c < a.C) t[c] = c == y ? p[c] * (ay * q - rest) : p[c] * (t[c] - s);
    } else {
      for (int c = 0; c < a.C; ++c) t[c] = 0.f;
    }
  }
  __syncthreads();
  unstage_rows(tile, g, r0, nr, a.C, ldd, vec_out);
}

bool known_kind(int k) { return k == SEGMIF_REGION_LOVASZ || k == SEGMIF_REGION_DICE; }

// rows x C within a 32-bit signed index (the sort counts pairs in 32 bits and a pair carries its row in 31)
bool geometry_ok(int64_t rows, int C) { return rows >= 1 && C >= 1 && C <= 32 && rows <= 0x7fffffffLL / C; }

// fills the kernel arguments; false: the descriptor or the geometry is refused
bool make_args(const SegmifRegionObjective* d, const float* logits, const int64_t* labels, int64_t rows, int C, int ld, RegArgs& a) {
  if (!d || !logits || !labels || !geometry_ok(rows, C) || ld < C) return false;
  if (!known_kind(d->kind) || (d->classes != SEGMIF_REGION_PRESENT && d->classes != SEGMIF_REGION_ALL)) return false;
  if (!(d->smooth >= 0.f) || !std::isfinite(d->smooth)) return false;
  a.x = logits, a.labels = (const long long*)labels;
  a.rows = rows, a.C = C, a.ld = ld;
  a.vec = ld == C && aligned16(logits);
  a.ignore_index = d->ignore_index, a.kind = d->kind;
  return true;
}

}  // namespace

extern "C" int64_t segmif_region_objective_workspace_bytes(int64_t rows, int C, int kind) {
  if (!geometry_ok(rows, C) || !known_kind(kind)) return 0;
  return layout(rows, C, kind).bytes;
}

extern "C" int segmif_region_objective_f32(const SegmifRegionObjective* desc, const float* logits, const int64_t* labels, void* workspace,
                                           float* record4, int64_t rows, int C, int ld, void* stream) {
  RegArgs a;
  if (!workspace || !aligned16(workspace) || !record4 || !make_args(desc, logits, labels, rows, C, ld, a)) return SEGMIF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(region_fwd_kernel, dim3((unsigned)row_blocks(rows)), dim3(ROWS), 0, s, a, workspace);
  if (a.kind == SEGMIF_REGION_LOVASZ) {
    Workspace W;
    carve(workspace, rows, C, a.kind, W);
    const long long tiles = sort_tiles(rows);
    const dim3 grid((unsigned)tiles, (unsigned)C);
    uint2 *src = W.buf0, *dst = W.buf1;
    for (int shift = 0; shift < 32; shift += 8) {  // (an even number of passes: the sorted pairs end in buf0)
      hipLaunchKernelGGL(region_hist_kernel, grid, dim3(ROWS), 0, s, src, W.hist, (long long)rows, tiles, shift);
      hipLaunchKernelGGL(region_scan_kernel, dim3((unsigned)C), dim3(SCAN_THREADS), 0, s, W.hist, 256 * tiles, (unsigned*)nullptr);
      hipLaunchKernelGGL(region_scatter_kernel, grid, dim3(ROWS), 0, s, src, dst, W.hist, (long long)rows, tiles, shift);
      uint2* t = src;
      src = dst, dst = t;
    }
    hipLaunchKernelGGL(region_fgcount_kernel, grid, dim3(ROWS), 0, s, W.buf0, W.tilefg, (long long)rows, tiles);
    hipLaunchKernelGGL(region_scan_kernel, dim3((unsigned)C), dim3(SCAN_THREADS), 0, s, W.tilefg, tiles, W.G);
    hipLaunchKernelGGL(region_lovasz_kernel, grid, dim3(ROWS), 0, s, W.buf0, W.tilefg, W.G, (float*)W.buf1, W.partial, (long long)rows,
                       tiles);
  }
  hipLaunchKernelGGL(region_final_kernel, dim3(1), dim3(256), 0, s, workspace, (long long)rows, C, a.kind, (int)desc->classes,
                     desc->smooth, record4);
  return (int)hipGetLastError();
}

extern "C" int segmif_region_objective_bwd_f32(const SegmifRegionObjective* desc, const float* logits, const int64_t* labels,
                                               const void* workspace, const float* record4, const float* upstream, float* dlogits,
                                               int64_t rows, int C, int ld, int ldd, void* stream) {
  RegArgs a;
  if (!workspace || !aligned16(workspace) || !record4 || !upstream || !dlogits || ldd < C || !make_args(desc, logits, labels, rows, C, ld, a))
    return SEGMIF_EINVAL;
  const int vec_out = ldd == C && aligned16(dlogits);
  hipLaunchKernelGGL(region_bwd_kernel, dim3((unsigned)row_blocks(rows)), dim3(ROWS), 0, (hipStream_t)stream, a, workspace, record4,
                     upstream, dlogits, ldd, vec_out);
  return (int)hipGetLastError();
}
