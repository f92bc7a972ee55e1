// Private to segmif_amd/csrc: the device helpers of the split operand formats and of the LDS-DMA that stages them.
//   bf16x6 (namespace bf3): x = p0 + p1 + p2, three bf16 rounded to nearest at each step (exact residuals); a product of two
//     such operands is six v_mfma_f32_32x32x16_bf16, least significant first (conv3x3_planes.hip holds the description).
//   f16x3 (namespace p16): an activation is a pair of halves, x = hi + 2^-11 lo with hi = RN16(x), lo = RN16(2^11 (x - hi)); a
//     weight row, scaled by a power of two, is three half planes W0 | W - W0 | 2^-11 W0; three v_mfma_f32_32x32x16_f16 per
//     product.  Every producer of such planes folds max |x| into a guard slot so that the host can tell whether the tensor
//     stayed inside the half's exponent range (ops.Planes16Guard).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace segmif {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int v = 0; v < 16; ++v) z[v] = 0.f;
  return z;
}

__device__ __forceinline__ f32x16 mfma16(const u32x4& a, const u32x4& b, const f32x16& c) {  // f16 operands held as dwords
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float gelu_exact(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// GELU(x) = x Phi(x) on ~16 vector-ALU operations (the libm erff of gelu_exact costs ~60), for kernels bound by their vector ALU
// phase.  Phi through erfc(z), z = |x| / sqrt 2, in the rational-times-Gaussian form of Abramowitz & Stegun 7.1.26 (|error of
// erf| <= 1.5e-7, i.e. <= 7.5e-8 |x| on GELU: about one fp32 ulp of x):
//     erfc(z) ~ (a1 t + .. + a5 t^5) exp(-z^2),  t = 1 / (1 + p z);   Phi = x >= 0 ? 1 - erfc / 2 : erfc / 2.
// (r6) The fused Mix-FFN of stages 1-2 (mixffn.hip) and the PAIRS dwconv producer of stages 3-4 (rowops.hip) both use it: the
// same function on both halves of the encoder, inside the same guarded inference scope; the fp32 kernels (training, and the path
// a tripped pair is repeated on) keep gelu_exact.
__device__ __forceinline__ float gelu_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(ax, 0.3275911f * 0.70710678118654752440f, 1.0f));
  float q = fmaf(t, 0.5f * 1.061405429f, 0.5f * -1.453152027f);  // (coefficients carry the 1/2 of erfc / 2)
  q = fmaf(q, t, 0.5f * 1.421413741f);
  q = fmaf(q, t, 0.5f * -0.284496736f);
  q = fmaf(q, t, 0.5f * 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(x * x * -0.72134752044448170368f);  // exp(-x^2 / 2)
  const float half_erfc = q * t * e;
  const float phi = x >= 0.f ? 1.0f - half_erfc : half_erfc;
  return x * phi;
}

// ---- LDS-DMA: global_load_lds_dwordx4, 16 bytes per lane, a wave's 1 KB lands lane-linearly at lds_wave_base ---------------
__device__ __forceinline__ void dma16(const unsigned char* src, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// the LDS byte address of a pointer into shared memory: what dma16s takes as its M0 value
__device__ __forceinline__ uint32_t lds_addr(unsigned char* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)p;
}
// (r6) The same instruction in its SADDR form: a wave-uniform 64-bit base in SGPRs + a 32-bit per-lane offset.  From the builtin
// hipcc makes, per DMA instruction, a v_lshl_add_u64 into ONE shared 64-bit address register pair and the load from it - the next
// instruction's address write has to wait until the load in front has read that pair (a write-after-read interlock on a
// vector-memory operand: tens to hundreds of cycles beside the other team's MFMA stream), and every address costs two VGPR reads.
// Here the offsets sit in their own registers for the kernel's life and a DMA instruction is an s_mov of M0 and the load.
// m0 = lds_addr(lds_wave_base), wave-uniform.  The call site decides how it reaches an SGPR (plainly, or through
// __builtin_amdgcn_readfirstlane): the two forms compile to different code around the DMA.
__device__ __forceinline__ void dma16s(const unsigned char* sbase, uint32_t voff, uint32_t m0) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(m0) : "memory", "m0");
}

// ---- bf16x6 --------------------------------------------------------------------------------------------------------------
namespace bf3 {

constexpr int PX6[6] = {2, 1, 0, 1, 0, 0};  // six products, least significant first: plane of the first operand ...
constexpr int PY6[6] = {0, 1, 2, 0, 1, 0};  // ... and of the second

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {  // v_cvt_pk_bf16_f32: a -> low half
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// (x0, x1) -> three dwords, each (bf16 of x0 in the low half, of x1 in the high half); x = p0 + p1 + p2 to 24 bits
__device__ __forceinline__ void split3(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = pk_bf16(x0, x1);
  float r0 = x0 - __uint_as_float(p0 << 16), r1 = x1 - __uint_as_float(p0 & 0xffff0000u);
  p1 = pk_bf16(r0, r1);
  r0 -= __uint_as_float(p1 << 16);
  r1 -= __uint_as_float(p1 & 0xffff0000u);
  p2 = pk_bf16(r0, r1);
}

// 8 fp32 values (positions 8h .. 8h+7 of a chunk) -> one 16-byte piece per plane
__device__ __forceinline__ void split8(const float* y, u32x4& p0, u32x4& p1, u32x4& p2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t a, b, c;
    split3(y[2 * e], y[2 * e + 1], a, b, c);
    p0[e] = a;
    p1[e] = b;
    p2[e] = c;
  }
}

// 8 consecutive K-slots of a lane -> one MFMA operand per plane
struct Op3 {
  u32x4 p[3];
};
__device__ __forceinline__ Op3 split8(const f32x4 lo, const f32x4 hi) {
  Op3 o;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    uint32_t a, b, c;
    split3(lo[2 * e], lo[2 * e + 1], a, b, c);
    o.p[0][e] = a; o.p[1][e] = b; o.p[2][e] = c;
    split3(hi[2 * e], hi[2 * e + 1], a, b, c);
    o.p[0][2 + e] = a; o.p[1][2 + e] = b; o.p[2][2 + e] = c;
  }
  return o;
}
__device__ __forceinline__ Op3 split8(const f32x16 t, int s) {  // accumulator registers 8s .. 8s+7
  return split8(f32x4{t[8 * s], t[8 * s + 1], t[8 * s + 2], t[8 * s + 3]},
                f32x4{t[8 * s + 4], t[8 * s + 5], t[8 * s + 6], t[8 * s + 7]});
}
__device__ __forceinline__ bf16x8 op(const u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// six-product fp32-class accumulate: acc += A B with A's planes `a` (first MFMA operand: rows) and B's planes `b`
__device__ __forceinline__ f32x16 mma6(const u32x4* a, const u32x4* b, f32x16 acc) {
#pragma unroll
  for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(op(a[PX6[t]]), op(b[PY6[t]]), acc, 0, 0, 0);
  return acc;
}

}  // namespace bf3

// ---- f16x3 ---------------------------------------------------------------------------------------------------------------
namespace p16 {

constexpr int PIXEL_BYTES = 64;     // per 16-channel chunk: 2 planes x 16 halves
constexpr float LSCALE = 2048.f;    // the low half carries 2^11 x the residual

__device__ __forceinline__ void split2(float x0, float x1, uint32_t& hi, uint32_t& lo) {
  const f32x2 v = {x0, x1};
  const f16x2 a = __builtin_convertvector(v, f16x2);  // v_cvt_pk_f16_f32, round to nearest even
  hi = __builtin_bit_cast(uint32_t, a);
  // (r6) 2^11 (x - hi) as ONE v_fma_mix_f32 per value - hi read in place as a half, times -2^11, plus 2^11 x: the same real number as
  // (x - float(hi)) * 2^11 (every step of either form is exact), without the two v_cvt_f32_f16 and the subtraction
  const f32x2 xs = v * LSCALE;
  f32x2 res;
  const float m = -LSCALE;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(res[0]) : "v"(hi), "v"(m), "v"(xs[0]));
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(res[1]) : "v"(hi), "v"(m), "v"(xs[1]));
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(res, f16x2));
}

// 8 values (positions 8h .. 8h+7 of a chunk) -> one 16-byte piece per plane
__device__ __forceinline__ void split8(const float* y, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t a, b;
    split2(y[2 * e], y[2 * e + 1], a, b);
    hi[e] = a;
    lo[e] = b;
  }
}

// PAIRS rows (gemm_pairs.hip): a 16-channel group is 64 bytes, [16 hi | 16 lo].  Four consecutive lanes that hold 4 consecutive
// channels each (split into ha, hb / la, lb by split2) own one group; storing 8 bytes per lane and plane would be 32-byte
// partial writes with 32-byte holes - measured 10x slower than the fp32 store on the LayerNorm (profiles/r05_pairs_producers_log.txt).
// Instead the quad trades dwords (DPP quad_perm, no LDS) so that lane q stores the 16-byte piece q of the group: one fully
// coalesced dwordx4 store per lane.  -> the piece of lane (threadIdx.x & 3); all four lanes of the quad must be active.
__device__ __forceinline__ u32x4 quad_piece(uint32_t ha, uint32_t hb, uint32_t la, uint32_t lb) {
  // source lanes 2 (q & 1) and 2 (q & 1) + 1 of the quad: quad_perm [0, 2, 0, 2] = 0x88 and [1, 3, 1, 3] = 0xdd
  const uint32_t h0a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ha, 0x88, 0xf, 0xf, false);
  const uint32_t h0b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hb, 0x88, 0xf, 0xf, false);
  const uint32_t h1a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ha, 0xdd, 0xf, 0xf, false);
  const uint32_t h1b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hb, 0xdd, 0xf, 0xf, false);
  const uint32_t l0a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)la, 0x88, 0xf, 0xf, false);
  const uint32_t l0b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lb, 0x88, 0xf, 0xf, false);
  const uint32_t l1a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)la, 0xdd, 0xf, 0xf, false);
  const uint32_t l1b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lb, 0xdd, 0xf, 0xf, false);
  const bool low = (threadIdx.x & 2) != 0;  // lanes 2, 3 of the quad store the lo plane's pieces
  return u32x4{low ? l0a : h0a, low ? l0b : h0b, low ? l1a : h1a, low ? l1b : h1b};
}

// ---- range bookkeeping -----------------------------------------------------------------------------------------------
// A producer tracks the largest magnitude it wrote on the HIGH halves' bit patterns (|half| as a 15-bit unsigned integer is
// monotone in magnitude; +inf = 0x7c00, every NaN lies above it), two halves per operation (v_and_b32 + v_pk_max_u16 - the
// same count as one v_max_f32 per value, and unlike v_max_f32 an integer maximum cannot drop a NaN).  Values beyond the
// half's range have already become inf in the conversion, so the pattern carries exactly what the guard asks about.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t absmax_pk(uint32_t m, uint32_t halves) {
  const us2 a = __builtin_bit_cast(us2, m), b = __builtin_bit_cast(us2, halves & 0x7fff7fffu);
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(a, b));
}

// (r6) The same with the STICKY bit of the low halves: a value whose high half rounded to zero (|x| < 2^-25) while its low half did
// not is carried by the low half alone - fewer than 23 bits - yet read 0 on the high halves' patterns, like an exact zero, and
// passed the guard (the one hole of the range contract).  Such a value now counts as the smallest subnormal
// (pattern 1 = 2^-24): a tensor whose LARGEST magnitude is that small reports a maximum below the guard's lower bound and is
// repeated on bf16 triples; a healthy tensor's maximum is unaffected (its patterns are far above 1).  v_and + v_pk_min_u16 +
// v_pk_max_u16 per pair of values, in epilogues only.
// (r6, later) min(|lo|, 1) is written as v_pk_min_u16 by hand: from __builtin_elementwise_min against the constant {1, 1} hipcc makes
// "lo != 0 ? 1 : 0" per half - v_bfe, two v_cmp_ne_u16 + s_nop + v_cndmask, v_perm: 12 instructions and 4 wait states per pair of values,
// ~800 per 16 x 32 patch of the dominant conv's epilogue (found in the ISA behind profiles/r06_tail_epilogue_timeline.txt).
__device__ __forceinline__ uint32_t sticky_pk(uint32_t lo_abs) {  // per half: 1 where the (sign-stripped) half is non-zero
  uint32_t s;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(s) : "v"(lo_abs), "v"(0x00010001u));
  return s;
}
__device__ __forceinline__ uint32_t absmax_pk(uint32_t m, uint32_t hi, uint32_t lo) {
  const uint32_t s = sticky_pk(lo & 0x7fff7fffu);
  return absmax_pk(__builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, m), __builtin_bit_cast(us2, s))), hi);
}

// four dwords of each plane at once: the sticky bits of the four low dwords are OR-ed first (a half of the OR is non-zero exactly when
// one of its four halves is: the same maximum as four absmax_pk calls, 14 instructions instead of 20)
__device__ __forceinline__ uint32_t absmax_pk4(uint32_t m, const u32x4& hi, const u32x4& lo) {
  const uint32_t s = sticky_pk((lo[0] | lo[1] | lo[2] | lo[3]) & 0x7fff7fffu);
  m = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, m), __builtin_bit_cast(us2, s)));
  return absmax_pk(absmax_pk(absmax_pk(absmax_pk(m, hi[0]), hi[1]), hi[2]), hi[3]);
}

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = v > w ? v : w;
  }
  return v;
}

__device__ __forceinline__ float wave_max(float v) {  // (weights' row scales: finite by construction)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// The look before the atomic: an atomic load (hipcc emits it with the cache-bypassing sc0 sc1 bits, so it sees other CUs'
// atomics; a plain load would keep hitting a stale line in the CU's L1 and every wave would go on to the atomic).  It has a
// price: its LATENCY (several microseconds under load) is what the reporting wave ends on, and atomics on one cache line queue
// (~10 ns each; the slot words of 16 neighbouring images share a line).  Fine for kernels whose waves live for tens of
// microseconds - the convs, attention, the CrossPath tail: one look per wave or per persistent workgroup.  NOT for row
// kernels whose waves live for a microsecond: the first LayerNorm that wrote half pairs spent 330 us instead of 22 this way
// (profiles/r05_pairs_producers_log.txt) - those use fold_pat_block / fold_pat_async below.
__device__ __forceinline__ uint32_t slot_peek(const uint32_t* slot) {
  return __atomic_load_n(slot, __ATOMIC_RELAXED);
}

// Fold this wave's running maximum (absmax_pk patterns) into the range slots of images b_lo .. b_hi (a wave whose rows
// straddle an image boundary reports to both: conservative).  A slot holds the IEEE bit pattern of a non-negative float
// (or NaN: it compares above inf).  The plain load first: a tensor has a few hundred thousand waves and all but a handful
// carry a value below the running maximum - one atomic per wave on a single address serialises in the L2 (measured 10x
// on segmif_planes16_from_f32).
__device__ __forceinline__ void fold_pat(uint32_t* slots, int b_lo, int b_hi, uint32_t pat) {
  uint32_t v = (pat & 0xffffu) > (pat >> 16) ? (pat & 0xffffu) : (pat >> 16);
  v = wave_umax(v);
  if ((threadIdx.x & 63) == 0 && v) {
    const uint32_t bits = __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)v));  // exact; NaN stays NaN
    for (int b = b_lo; b <= b_hi; ++b)
      if (bits > slot_peek(slots + b)) atomicMax(slots + b, bits);
  }
}

// fold_pat without the look: the atomic is issued unconditionally and its result is not used, so the wave does not wait for it
// (a no-return global_atomic_umax leaves like a store).  For kernels whose waves live for a microsecond - the LayerNorm that
// writes half pairs - the look's LATENCY (a cache-bypassing load: several microseconds under load) is what costs: every wave
// ends on it and holds its slot meanwhile (measured: 20 us -> 190 us).  Such a kernel spreads its reports over several rows of
// slots instead, so that the atomics do not queue on one address.
__device__ __forceinline__ void fold_pat_async(uint32_t* slots, int b_lo, int b_hi, uint32_t pat) {
  uint32_t v = (pat & 0xffffu) > (pat >> 16) ? (pat & 0xffffu) : (pat >> 16);
  v = wave_umax(v);
  if ((threadIdx.x & 63) == 0 && v) {
    const uint32_t bits = __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)v));
    for (int b = b_lo; b <= b_hi; ++b) (void)__hip_atomic_fetch_max(slots + b, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The same for a whole workgroup of up to 16 waves reporting to ONE image: the waves' maxima meet in LDS and one lane makes the
// slot access (row kernels whose waves are short: see slot_peek).  Must be reached by every wave of the workgroup that is
// still alive, partial waves included (lanes that left a wave early count as zero).
__device__ __forceinline__ void fold_pat_block(uint32_t* slots, int b, uint32_t pat) {
  __shared__ uint32_t red_pat[16];
  uint32_t v = (pat & 0xffffu) > (pat >> 16) ? (pat & 0xffffu) : (pat >> 16);
  v = wave_umax(v);
  const int nw = (int)((blockDim.x * blockDim.y * blockDim.z + 63) >> 6);
  if (threadIdx.x < 16) red_pat[threadIdx.x] = 0u;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_pat[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nw && w < 16; ++w) v = red_pat[w] > v ? red_pat[w] : v;
    if (v) {  // (no look: the workgroup would sit on the load's latency; one fire-and-forget atomic per workgroup)
      const uint32_t bits = __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)v));
      (void)__hip_atomic_fetch_max(slots + b, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The same bookkeeping on fp32 values a kernel is ABOUT to split (when touching the split halves again would cost registers):
// running maximum of |x| as an IEEE bit pattern - an integer maximum, so a NaN (any sign) is kept, not dropped.
__device__ __forceinline__ uint32_t absmax_bits(uint32_t m, float a, float b) {
  const uint32_t x = __float_as_uint(a) & 0x7fffffffu, y = __float_as_uint(b) & 0x7fffffffu;
  const uint32_t t = x > y ? x : y;
  return m > t ? m : t;  // (v_max3_u32)
}
__device__ __forceinline__ void fold_bits(uint32_t* slots, int b_lo, int b_hi, uint32_t bits) {
  bits = wave_umax(bits);
  if ((threadIdx.x & 63) == 0 && bits) {
    for (int b = b_lo; b <= b_hi; ++b)
      if (bits > slot_peek(slots + b)) atomicMax(slots + b, bits);
  }
}

// The power of two that puts the largest magnitude recorded in n range slots (IEEE bit patterns) into [2^13, 2^14): what the
// training kernels multiply their staged operands by before splitting them into halves (exact, taken out again afterwards).
// All-zero slots: 1.  An inf / NaN maximum: NaN - the consumer's whole output turns NaN instead of quietly wrong.
// (n <= 64 words, read one per lane and reduced across the wave: a scalar loop over 48 words was a chain of 48 dependent
// loads at the head of every workgroup - a third of a 30 us workgroup in the training step's convs.)
__device__ __forceinline__ float scale_of(uint32_t mx) {  // mx: IEEE bit pattern of a maximum of magnitudes
  if (mx >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
  if (!mx) return 1.f;
  int eb = 13 - ((int)(mx >> 23) - 127) + 127;
  eb = eb < 1 ? 1 : (eb > 254 ? 254 : eb);
  return __uint_as_float((uint32_t)eb << 23);
}
__device__ __forceinline__ float range_scale(const uint32_t* slots, int n) {
  const int lane = threadIdx.x & 63;
  return scale_of(wave_umax(lane < n ? slots[lane] : 0u));
}

// ---- f16x3 MFMA operands: an activation operand is a half pair (hi, lo = 2^11 residual), split in registers; a weight operand
// is the three planes W0 | W - W0 | 2^-11 W0; products least significant first: lo W0s, hi Wl, hi W0
struct Op2 {
  u32x4 hi, lo;
};
__device__ __forceinline__ Op2 split8h(const f32x4 a, const f32x4 b) {
  const float y[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  Op2 o;
  split8(y, o.hi, o.lo);
  return o;
}
__device__ __forceinline__ Op2 split8h(const f32x16 t, int s) {  // accumulator registers 8s .. 8s+7
  return split8h(f32x4{t[8 * s], t[8 * s + 1], t[8 * s + 2], t[8 * s + 3]},
                 f32x4{t[8 * s + 4], t[8 * s + 5], t[8 * s + 6], t[8 * s + 7]});
}
__device__ __forceinline__ f16x8 oph(const u32x4 v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ u32x4 times_2m11(const u32x4 v) {  // 8 halves x 2^-11 (v_pk_mul_f16; exact up to the half's own rounding)
  const f16x8 s = {(_Float16)0x1p-11f, (_Float16)0x1p-11f, (_Float16)0x1p-11f, (_Float16)0x1p-11f,
                   (_Float16)0x1p-11f, (_Float16)0x1p-11f, (_Float16)0x1p-11f, (_Float16)0x1p-11f};
  return __builtin_bit_cast(u32x4, oph(v) * s);
}
// acc += W X with the weight planes `w` as the MFMA's first operand (rows) and the half pair `x` as its second
__device__ __forceinline__ f32x16 mma3(const u32x4* w, const Op2& x, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(oph(w[2]), oph(x.lo), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(oph(w[1]), oph(x.hi), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(oph(w[0]), oph(x.hi), acc, 0, 0, 0);
  return acc;
}
// three half planes W0 | W - W0 | 2^-11 W0 of two adjacent scaled values -> one dword per plane
__device__ __forceinline__ void split3h(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  const f16x2 w0 = {(_Float16)x0, (_Float16)x1};
  const f16x2 wl = {(_Float16)(x0 - (float)w0[0]), (_Float16)(x1 - (float)w0[1])};
  const f16x2 ws = {(_Float16)((float)w0[0] * (1.f / LSCALE)), (_Float16)((float)w0[1] * (1.f / LSCALE))};
  p0 = __builtin_bit_cast(uint32_t, w0);
  p1 = __builtin_bit_cast(uint32_t, wl);
  p2 = __builtin_bit_cast(uint32_t, ws);
}
// the power of two that brings mx into [2^14, 2^15) (1 for zero / non-finite input): a weight row's (or tile's) scale
__device__ __forceinline__ float pow2_scale(float mx) {
  int e = 0;
  if (mx >= 1e-30f && mx <= 3e38f) e = 14 - (int)((__float_as_uint(mx) >> 23) - 127);
  return ldexpf(1.f, e);
}

}  // namespace p16
}  // namespace segmif
