// ClassMix (Olsson et al. 2021; the mixing step of DAFormer): classes of one crop of an augmented batch pasted into another.
// The rule is stated in include/segmif_hip.h.  Everything here moves integers or copies float bits: no float arithmetic.
//
//   select: one 64-thread block per receiver.  The donor's row of the (B, 257) class counts (segmif_label_stats_i64 over the
//           crop labels) gives the present classes by ballot, 64 classes a round; k comes from the popcount, a class's rank
//           among the present keys from a loop over the classes; the selection leaves as 8 words of bits, `pasted` as the sum
//           of the selected counts; the tally takes integer global atomics.
//   apply : grid (blocks, B) of 256 threads, a thread per group of 4 consecutive pixels of a row (w % 4 == 0), the block
//           count capped and the rest strided.  Per group two 16-byte loads of the donor's labels, a 4-bit mask, then per
//           plane one 16-byte load from the donor (mask 15), from the receiver (mask 0) or from both, and a 16-byte store.
//           A sample that does not mix is a straight copy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;  // over the whole grid: 256 CUs x 8 blocks, the rest is strided
constexpr int SEL_WORDS = 8;
constexpr int BINS = 257;

typedef uint32_t Quad __attribute__((ext_vector_type(4)));            // four floats' bits
typedef unsigned long long Pair __attribute__((ext_vector_type(2)));  // two labels

// Makes all four words of a loaded line live, so that the compiler neither narrows a 16-byte load to the words a blend happens
// to use nor sinks it into the branches.  Placed after a batch of loads has been issued, it costs nothing.
__device__ __forceinline__ void keep_whole(Quad& q) { asm volatile("" : "+v"(q)); }

// donor of receiver b, or b itself for a sample that does not mix (donor == b, or a value outside 0..B-1)
__device__ __forceinline__ int donor_of(const int32_t* __restrict__ row, int b, int B) {
  const int d = row[0];
  return (d < 0 || d >= B) ? b : d;
}

__global__ __launch_bounds__(64) void class_mix_select_kernel(const long long* __restrict__ counts, const int32_t* __restrict__ table,
                                                              int B, int n_class, long long min_pixels, uint32_t* __restrict__ sel,
                                                              long long* __restrict__ pasted, unsigned long long* __restrict__ tally) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t* row = table + (long long)b * (2 + n_class);
  const int32_t* key = row + 2;
  const int d = donor_of(row, b, B), force = row[1];
  uint32_t* out = sel + (long long)b * SEL_WORDS;
  if (d == b) {
    if (lane < SEL_WORDS) out[lane] = 0u;
    if (lane == 0) pasted[b] = 0;
    return;
  }
  const long long* cnt = counts + (long long)d * BINS;
  long long n[4];
  unsigned long long present[4];
  int total = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = r * 64 + lane;
    n[r] = c < n_class ? cnt[c] : 0;
    present[r] = __ballot(c < n_class && n[r] > min_pixels);
    total += __popcll(present[r]);
  }
  const int k = (total + (total & 1)) >> 1;
  long long sum = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = r * 64 + lane;
    const bool mine = (present[r] >> lane) & 1ull;
    bool chosen = false;
    if (force >= 0) {
      chosen = mine && c == force;
    } else if (mine) {
      const int my = key[c];
      int rank = 0;
#pragma unroll
      for (int ro = 0; ro < 4; ++ro) {  // at most 255 iterations in all; equal keys (the wrapper refuses them) rank by class
        for (int o = ro * 64; o < min(ro * 64 + 64, n_class); ++o) {
          const int ko = key[o];
          rank += ((present[ro] >> (o & 63)) & 1ull) && (ko < my || (ko == my && o < c));
        }
      }
      chosen = rank < k;
    }
    const unsigned long long bits = __ballot(chosen);
    if (lane == 0) {
      out[2 * r] = (uint32_t)bits;
      out[2 * r + 1] = (uint32_t)(bits >> 32);
    }
    if (chosen) {
      sum += n[r];
      if (tally) {
        atomicAdd(&tally[2 * c], 1ull);
        atomicAdd(&tally[2 * c + 1], (unsigned long long)n[r]);
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_down(sum, s, 64);
  if (lane == 0) pasted[b] = sum;
}

__device__ __forceinline__ Quad blend(Quad recv, Quad don, unsigned int mask) {
  Quad o;
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = (mask >> t) & 1u ? don[t] : recv[t];
  return o;
}

__global__ __launch_bounds__(THREADS) void class_mix_apply_kernel(const float* __restrict__ ir3, const float* __restrict__ vis3,
                                                                  const float* __restrict__ mask3, const long long* __restrict__ label,
                                                                  const int32_t* __restrict__ table, const uint32_t* __restrict__ sel,
                                                                  int B, long long hw, int n_class, float* __restrict__ ir3_out,
                                                                  float* __restrict__ vis3_out, float* __restrict__ mask3_out,
                                                                  long long* __restrict__ label_out) {
  const int b = blockIdx.y;
  const int d = donor_of(table + (long long)b * (2 + n_class), b, B);
  const bool mixing = d != b;
  uint32_t s[SEL_WORDS];
#pragma unroll
  for (int i = 0; i < SEL_WORDS; ++i) s[i] = mixing ? sel[(long long)b * SEL_WORDS + i] : 0u;
  const float* in[3] = {ir3, vis3, mask3};
  float* out[3] = {ir3_out, vis3_out, mask3_out};
  const long long groups = hw >> 2;
  const long long lab_r = (long long)b * hw, lab_d = (long long)d * hw;
  for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * THREADS) {
    const long long p = g << 2;
    unsigned int m = 0;
    Pair dl[2] = {Pair{0, 0}, Pair{0, 0}};
    if (mixing) {
      Quad d0 = *reinterpret_cast<const Quad*>(label + lab_d + p), d1 = *reinterpret_cast<const Quad*>(label + lab_d + p + 2);
      keep_whole(d0);
      keep_whole(d1);
      dl[0] = __builtin_bit_cast(Pair, d0);
      dl[1] = __builtin_bit_cast(Pair, d1);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned long long v = dl[t >> 1][t & 1];  // the full 64-bit value, not its low byte
        if (v < (unsigned long long)n_class) {
          uint32_t word = 0;
#pragma unroll
          for (int i = 0; i < SEL_WORDS; ++i) word = ((unsigned int)v >> 5) == (unsigned int)i ? s[i] : word;
          m |= ((word >> ((unsigned int)v & 31u)) & 1u) << t;
        }
      }
    }
    // A group takes its planes from one place (the donor when all four pixels are pasted, else the receiver) and, when it is
    // split, from the donor as well.  The loads of a tensor's three planes are issued together, then kept whole, then blended.
    const bool all = m == 15u, split = m != 0u && !all;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      Quad one[3], two[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const long long r_off = ((long long)b * 3 + ch) * hw + p, d_off = ((long long)d * 3 + ch) * hw + p;
        one[ch] = *reinterpret_cast<const Quad*>(in[q] + (all ? d_off : r_off));
        two[ch] = one[ch];
        if (split) two[ch] = *reinterpret_cast<const Quad*>(in[q] + d_off);
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        keep_whole(one[ch]);
        keep_whole(two[ch]);
        *reinterpret_cast<Quad*>(out[q] + ((long long)b * 3 + ch) * hw + p) = blend(one[ch], two[ch], split ? m : 0u);
      }
    }
    Pair l0 = dl[0], l1 = dl[1];
    if (!all) {
      Quad r0 = *reinterpret_cast<const Quad*>(label + lab_r + p), r1 = *reinterpret_cast<const Quad*>(label + lab_r + p + 2);
      keep_whole(r0);
      keep_whole(r1);
      const Pair k0 = __builtin_bit_cast(Pair, r0), k1 = __builtin_bit_cast(Pair, r1);
      l0[0] = m & 1u ? dl[0][0] : k0[0];
      l0[1] = m & 2u ? dl[0][1] : k0[1];
      l1[0] = m & 4u ? dl[1][0] : k1[0];
      l1[1] = m & 8u ? dl[1][1] : k1[1];
    }
    *reinterpret_cast<Pair*>(label_out + lab_r + p) = l0;
    *reinterpret_cast<Pair*>(label_out + lab_r + p + 2) = l1;
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

extern "C" int segmif_class_mix_select(const int64_t* counts, const int32_t* table, int B, int n_class, int64_t min_pixels,
                                       int32_t* sel, int64_t* pasted, int64_t* tally, void* stream) {
  if (!counts || !table || !sel || !pasted) return SEGMIF_EINVAL;
  if (B < 1 || n_class < 1 || n_class > 255 || min_pixels < 0) return SEGMIF_EINVAL;
  if (misaligned(counts, 8) || misaligned(table, 4) || misaligned(sel, 8) || misaligned(pasted, 8) || misaligned(tally, 8)) return SEGMIF_EINVAL;
  hipLaunchKernelGGL(class_mix_select_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(counts), table, B, n_class, (long long)min_pixels,
                     reinterpret_cast<uint32_t*>(sel), reinterpret_cast<long long*>(pasted), reinterpret_cast<unsigned long long*>(tally));
  return (int)hipGetLastError();
}

extern "C" int segmif_class_mix_apply_f32(const float* ir3, const float* vis3, const float* mask3, const int64_t* label,
                                          const int32_t* table, const int32_t* sel, int B, int h, int w, int n_class, float* ir3_out,
                                          float* vis3_out, float* mask3_out, int64_t* label_out, void* stream) {
  if (!ir3 || !vis3 || !mask3 || !label || !table || !sel || !ir3_out || !vis3_out || !mask3_out || !label_out) return SEGMIF_EINVAL;
  if (B < 1 || B > 65535 || n_class < 1 || n_class > 255 || h < 1 || w < 1 || w % 4) return SEGMIF_EINVAL;  // (B is the grid's y extent)
  if (misaligned(ir3, 16) || misaligned(vis3, 16) || misaligned(mask3, 16) || misaligned(label, 16) || misaligned(ir3_out, 16) ||
      misaligned(vis3_out, 16) || misaligned(mask3_out, 16) || misaligned(label_out, 16) || misaligned(table, 4) || misaligned(sel, 8))
    return SEGMIF_EINVAL;
  const long long hw = (long long)h * w, groups = hw >> 2;
  long long blocks = (groups + THREADS - 1) / THREADS;
  const long long cap = MAX_BLOCKS / B > 0 ? MAX_BLOCKS / B : 1;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(class_mix_apply_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, ir3, vis3, mask3,
                     reinterpret_cast<const long long*>(label), table, reinterpret_cast<const uint32_t*>(sel), B, hw, n_class, ir3_out,
                     vis3_out, mask3_out, reinterpret_cast<long long*>(label_out));
  return (int)hipGetLastError();
}
