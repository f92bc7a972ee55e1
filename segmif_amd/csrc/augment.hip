// The training loader's augmentation on resident uint8 frames (datasets/voc_fusion3.py:169-216 with datasets/imutils.py:
// random_scaling2 -> random_fliplr2 -> PhotoMetricDistortion (brightness, contrast) -> random_crop2 -> / 255 -> CHW), bit for
// bit.  The host draws the random parameters and builds Pillow's resize tables (fixed-point bilinear coefficients, nearest
// indices); the kernels read every geometry value from a per-sample record in device memory, so a batch is two launches and
// no host sync.  Integer arithmetic only, apart from the photometric step (float32, as numpy's) and the final division.
//
//   pick  : grid (10 candidates, B).  Class counts of the candidate's crop window over the VIRTUAL label (nearest-resized
//           through the index tables, flipped, padded with 255), LDS histograms; the last block of a sample to finish keeps
//           the first accepted candidate (imutils.py:225-238) and writes its origin into the record.
//           pick_class is the same kernel with a second rule per sample: more than t pixels of a wanted class in the window.
//   apply : grid (crop_w / 64, crop_h / 16, B).  Horizontal pass of the rows the tile needs into LDS as uint8 (Pillow rounds
//           between its passes), vertical pass from LDS, then flip / photometric / pad / crop / 255 and 16-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int TW = 64;         // output tile: 64 x 16 pixels, 256 threads, 4 pixels of one row per thread
constexpr int TH = 16;
constexpr int MAX_ROWS = 96;   // horizontal-pass rows a tile may need: 16 * (in / out) + taps, in / out <= 4
constexpr int LDW = 17;        // dwords per LDS row: 64 bytes + 1 dword, so that the 4 output rows of a wave, whose first
                               // source rows lie in/out apart, fall on different banks
constexpr int NCH = 5;         // ir, mask, R, G, B
constexpr int MAX_TAPS = 16;
constexpr int PREC = 22;       // Pillow's PRECISION_BITS for 8-bit channels
constexpr int NCAND = 10;

struct Geo {
  int src, h, w, nw, nh, flip, pad_h, pad_w, taps_x, taps_y;
  const int32_t *tx, *ty, *nx, *ny;
  bool ok;
};

// Everything a kernel dereferences is checked here against the sizes the caller passed: a record that does not fit them
// makes its blocks return without touching memory.
__device__ __forceinline__ Geo load_geo(const SegmifAugmentRec* __restrict__ r, const int32_t* __restrict__ tab, long long tab_words,
                                        int N, int h, int w) {
  Geo g;
  g.src = r->src; g.h = r->h; g.w = r->w; g.nw = r->nw; g.nh = r->nh; g.flip = r->flip;
  g.pad_h = r->pad_h; g.pad_w = r->pad_w; g.taps_x = r->taps_x; g.taps_y = r->taps_y;
  const long long ox = r->tab_x, oy = r->tab_y, onx = r->near_x, ony = r->near_y;
  // (w <= 4 nw, h <= 4 nh: MAX_ROWS holds a tile's horizontal-pass rows only up to a shrink by 4)
  g.ok = g.src >= 0 && g.src < N && g.h == h && g.w == w && g.nw > 0 && g.nh > 0 && g.nw <= 4 * SEGMIF_AUGMENT_MAX_SIDE &&
         (long long)w <= 4ll * g.nw && (long long)h <= 4ll * g.nh &&
         g.nh <= 4 * SEGMIF_AUGMENT_MAX_SIDE && g.taps_x >= 1 && g.taps_x <= MAX_TAPS && g.taps_y >= 1 && g.taps_y <= MAX_TAPS &&
         ox >= 0 && oy >= 0 && onx >= 0 && ony >= 0 && ox + (long long)g.nw * (2 + g.taps_x) <= tab_words &&
         oy + (long long)g.nh * (2 + g.taps_y) <= tab_words && onx + g.nw <= tab_words && ony + g.nh <= tab_words;
  g.tx = tab + ox; g.ty = tab + oy; g.nx = tab + onx; g.ny = tab + ony;
  return g;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// label of pixel (fy, fx) of the resized, flipped image (both inside it)
__device__ __forceinline__ int virtual_label(const Geo& g, const uint8_t* __restrict__ lab, int fy, int fx) {
  const int rx = g.flip ? g.nw - 1 - fx : fx;
  const int sy = clampi(g.ny[fy], 0, g.h - 1), sx = clampi(g.nx[rx], 0, g.w - 1);
  return lab[(long long)sy * g.w + sx];
}

// CLASS: the second acceptance rule (segmif_augment_pick_class_u8).  A sample with want = (c, t), 0 <= c <= 254, accepts the
// candidates whose window holds MORE than t pixels of class c and keeps the first of them, else the candidate with the most
// such pixels (lowest index on ties); any other sample goes through the reference's rule below, word for word.  Each block
// folds (accepted, index, n) into one 64-bit key whose maximum is the kept candidate, in the record's reserved words.
template <bool CLASS>
__global__ __launch_bounds__(1024) void pick_kernel(const uint8_t* __restrict__ label, int N, int h, int w, SegmifAugmentRec* __restrict__ rec,
                                                    const int32_t* __restrict__ tab, long long tab_words, int crop_h, int crop_w,
                                                    const int32_t* __restrict__ want, int32_t* __restrict__ got,
                                                    unsigned long long* __restrict__ tally, int n_class_tally) {
  __shared__ unsigned int hist[16][256];
  __shared__ unsigned int tot[256];
  SegmifAugmentRec* r = rec + blockIdx.y;
  const Geo g = load_geo(r, tab, tab_words, N, h, w);
  if (!g.ok) return;
  const int c = blockIdx.x;
  const int hs = r->cand[2 * c], ws = r->cand[2 * c + 1];
  const uint8_t* lab = label + (long long)g.src * h * w;
  unsigned int* mine = hist[threadIdx.x >> 6];
  for (int i = threadIdx.x; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0u;
  __syncthreads();
  // 16 consecutive pixels of a row per thread and step; equal neighbours are counted as one run (label maps are blocky, a
  // histogram atomic per pixel would serialise on one bin)
  const int chunks = (crop_w + 15) >> 4;
  const int total = crop_h * chunks;
  for (int i = threadIdx.x; i < total; i += 1024) {
    const int oy = i / chunks, ox0 = (i - oy * chunks) << 4;
    const int fy = hs + oy - g.pad_h;
    if (fy < 0 || fy >= g.nh) continue;  // a row of padding: ignore label only
    int cur = 255, run = 0;
    const int ox1 = min(ox0 + 16, crop_w);
    for (int ox = ox0; ox < ox1; ++ox) {
      const int fx = ws + ox - g.pad_w;
      const int v = (fx >= 0 && fx < g.nw) ? virtual_label(g, lab, fy, fx) : 255;
      if (v != cur) {
        if (run && cur != 255) atomicAdd(&mine[cur], (unsigned)run);
        cur = v;
        run = 0;
      }
      ++run;
    }
    if (run && cur != 255) atomicAdd(&mine[cur], (unsigned)run);
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    unsigned int s = 0;
    for (int k = 0; k < 16; ++k) s += hist[k][threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if constexpr (CLASS) {
      const int wc = want[2 * blockIdx.y], wt = want[2 * blockIdx.y + 1];
      if (wc >= 0 && wc <= 254 && wt >= 0) {  // (the wrapper refuses anything else that is not negative; here it falls through)
        const unsigned int n = tot[wc];
        const bool ok = n > (unsigned)wt;
        // accepted candidates beat rejected ones and the lower index wins among them; rejected ones compare by n, then index
        const unsigned long long key = ok ? (1ull << 62) | ((unsigned long long)(15 - c) << 32) | n
                                          : ((unsigned long long)n << 4) | (unsigned long long)(15 - c);
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(&r->reserved[0]);
        atomicMax(slot, key);
        if (ok) atomicOr(reinterpret_cast<unsigned int*>(&r->accept_mask), 1u << c);
        __threadfence();
        const unsigned int ticket = atomicAdd(reinterpret_cast<unsigned int*>(&r->ticket), 1u);
        if (ticket == NCAND - 1) {
          __threadfence();
          const unsigned int mask = atomicExch(reinterpret_cast<unsigned int*>(&r->accept_mask), 0u);
          const unsigned long long best = atomicExch(slot, 0ull);
          const bool hit = (best >> 62) != 0;
          const int chosen = hit ? 15 - (int)((best >> 32) & 15u) : 15 - (int)(best & 15u);
          const unsigned int n_chosen = hit ? (unsigned int)best : (unsigned int)(best >> 4);
          r->accepted = (int32_t)mask;
          r->chosen = chosen;
          r->box_h = r->cand[2 * chosen];
          r->box_w = r->cand[2 * chosen + 1];
          got[blockIdx.y] = (int32_t)n_chosen;
          if (tally && wc < n_class_tally) {
            atomicAdd(&tally[2 * wc], 1ull);
            if (hit) atomicAdd(&tally[2 * wc + 1], 1ull);
          }
          atomicExch(reinterpret_cast<unsigned int*>(&r->ticket), 0u);
        }
        return;
      }
    }
    unsigned long long sum = 0, mx = 0;
    for (int k = 0; k < 255; ++k) {  // bin 255 is the ignore label
      sum += tot[k];
      mx = tot[k] > mx ? tot[k] : mx;
    }
    // imutils.py:235: len(cnt > 1) is len(cnt), i.e. any non-ignore pixel; max / sum < 0.75 as 4 max < 3 sum
    const unsigned int ok = (sum > 0 && 4ull * mx < 3ull * sum) ? 1u : 0u;
    if (ok) atomicOr(reinterpret_cast<unsigned int*>(&r->accept_mask), 1u << c);
    __threadfence();
    const unsigned int ticket = atomicAdd(reinterpret_cast<unsigned int*>(&r->ticket), 1u);
    if (ticket == NCAND - 1) {  // every candidate of this sample is counted
      __threadfence();
      const unsigned int mask = atomicExch(reinterpret_cast<unsigned int*>(&r->accept_mask), 0u);
      int chosen = NCAND - 1;  // none accepted: the loop's last draw stays
      for (int k = NCAND - 1; k >= 0; --k)
        if (mask & (1u << k)) chosen = k;
      r->accepted = (int32_t)mask;
      r->chosen = chosen;
      r->box_h = r->cand[2 * chosen];
      r->box_w = r->cand[2 * chosen + 1];
      if constexpr (CLASS) got[blockIdx.y] = -1;
      atomicExch(reinterpret_cast<unsigned int*>(&r->ticket), 0u);
    }
  }
}

__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> PREC, 0, 255); }

// PhotoMetricDistortion.convert on one value: uint8(clip(float32(v) * alpha + beta, 0, 255)), two rounded float32 operations
__device__ __forceinline__ int convert(int v, float alpha, float beta) {
  float f = __fadd_rn(__fmul_rn((float)v, alpha), beta);
  f = fminf(fmaxf(f, 0.0f), 255.0f);
  return (int)f;
}

struct alignas(16) F4 { float v[4]; };
struct alignas(16) L2 { long long v[2]; };

__global__ __launch_bounds__(256) void apply_kernel(const uint8_t* __restrict__ ir, const uint8_t* __restrict__ vis,
                                                    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ label, int N, int h,
                                                    int w, const SegmifAugmentRec* __restrict__ rec, const int32_t* __restrict__ tab,
                                                    long long tab_words, int crop_h, int crop_w, float* __restrict__ ir3,
                                                    float* __restrict__ vis3, float* __restrict__ mask3, long long* __restrict__ label_out) {
  __shared__ uint32_t hp[NCH][MAX_ROWS][LDW];
  const int b = blockIdx.z;
  const SegmifAugmentRec* r = rec + b;
  const Geo g = load_geo(r, tab, tab_words, N, h, w);
  if (!g.ok) return;
  const int box_h = r->box_h, box_w = r->box_w;
  const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
  const int fx0 = box_w + ox0 - g.pad_w;        // column c of the tile is column fx0 + c of the resized, flipped image
  const int fy0 = box_h + oy0 - g.pad_h;
  const int rows_out = min(TH, crop_h - oy0), cols_out = min(TW, crop_w - ox0);
  const int fyA = max(fy0, 0), fyB = min(fy0 + rows_out, g.nh);
  const int sx = 2 + g.taps_x, sy = 2 + g.taps_y;
  const long long plane = (long long)h * w;
  const uint8_t* irs = ir + g.src * plane;
  const uint8_t* mks = mask + g.src * plane;
  const uint8_t* vs = vis + g.src * plane * 3;
  int y_first = 0, nrows = 0;
  if (fyA < fyB) {
    y_first = clampi(g.ty[(long long)fyA * sy], 0, g.h - 1);
    const int last = clampi(g.ty[(long long)(fyB - 1) * sy], 0, g.h - 1);
    const int y_end = min(last + clampi(g.ty[(long long)(fyB - 1) * sy + 1], 1, g.taps_y), g.h);
    nrows = clampi(y_end - y_first, 0, MAX_ROWS);
  }
  // horizontal pass: source rows y_first .. y_first + nrows - 1 at the tile's columns, stored by OUTPUT column (the flip is here)
  uint8_t* hpb = reinterpret_cast<uint8_t*>(&hp[0][0][0]);
  for (int i = threadIdx.x; i < nrows * TW; i += 256) {
    const int row = i >> 6, c = i & 63;
    const int fx = fx0 + c;
    if (c >= cols_out || fx < 0 || fx >= g.nw) continue;
    const int rx = g.flip ? g.nw - 1 - fx : fx;
    const int32_t* e = g.tx + (long long)rx * sx;
    const int xmin = clampi(e[0], 0, g.w - 1);
    const int n = min(clampi(e[1], 1, g.taps_x), g.w - xmin);
    const long long base = (long long)(y_first + row) * g.w + xmin;
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0, a3 = a0, a4 = a0;
    for (int t = 0; t < n; ++t) {
      const int k = e[2 + t];
      a0 += k * irs[base + t];
      a1 += k * mks[base + t];
      const uint8_t* p = vs + (base + t) * 3;
      a2 += k * p[0];
      a3 += k * p[1];
      a4 += k * p[2];
    }
    const int o = row * (LDW * 4) + c;
    hpb[0 * MAX_ROWS * LDW * 4 + o] = (uint8_t)clip8(a0);
    hpb[1 * MAX_ROWS * LDW * 4 + o] = (uint8_t)clip8(a1);
    hpb[2 * MAX_ROWS * LDW * 4 + o] = (uint8_t)clip8(a2);
    hpb[3 * MAX_ROWS * LDW * 4 + o] = (uint8_t)clip8(a3);
    hpb[4 * MAX_ROWS * LDW * 4 + o] = (uint8_t)clip8(a4);
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx4 = threadIdx.x & 15;
  const int oy = oy0 + ty, ox = ox0 + 4 * tx4;
  if (oy >= crop_h || ox >= crop_w) return;  // (crop_w is a multiple of 4: a thread's 4 pixels are inside together)
  const int fy = fy0 + ty;
  const bool row_in = fy >= 0 && fy < g.nh;
  int acc[NCH][4];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[ch][j] = 1 << (PREC - 1);
  if (row_in) {
    const int32_t* e = g.ty + (long long)fy * sy;
    const int r0 = clampi(e[0], 0, g.h - 1) - y_first;
    const int n = clampi(e[1], 1, g.taps_y);
    for (int t = 0; t < n; ++t) {
      const int k = e[2 + t];
      const int row = clampi(r0 + t, 0, MAX_ROWS - 1);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const uint32_t word = hp[ch][row][tx4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ch][j] += k * (int)((word >> (8 * j)) & 255u);
      }
    }
  }
  const int bright = r->bright_on, contrast = r->contrast_on;
  const float beta = r->beta, alpha = r->alpha;
  // imutils.py:205-210: the padding is float32(mean_rgb[c]) in EVERY image, the grey ones included
  const float padv[3] = {__fdiv_rn(123.675f, 255.0f), __fdiv_rn(116.28f, 255.0f), __fdiv_rn(103.53f, 255.0f)};
  F4 o_ir[3], o_vis[3], o_mask[3];
  L2 o_lab[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int fx = fx0 + 4 * tx4 + j;
    const bool in = row_in && fx >= 0 && fx < g.nw;
    if (in) {
      const float vi = __fdiv_rn((float)clip8(acc[0][j]), 255.0f), vm = __fdiv_rn((float)clip8(acc[1][j]), 255.0f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int v = clip8(acc[2 + c][j]);
        if (bright) v = convert(v, 1.0f, beta);
        if (contrast) v = convert(v, alpha, 0.0f);
        o_vis[c].v[j] = __fdiv_rn((float)v, 255.0f);
        o_ir[c].v[j] = vi;
        o_mask[c].v[j] = vm;
      }
      o_lab[j >> 1].v[j & 1] = virtual_label(g, label + g.src * plane, fy, fx);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) o_ir[c].v[j] = o_vis[c].v[j] = o_mask[c].v[j] = padv[c];
      o_lab[j >> 1].v[j & 1] = 255;
    }
  }
  const long long cp = (long long)crop_h * crop_w;
  const long long pix = (long long)oy * crop_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long o = ((long long)b * 3 + c) * cp + pix;
    *reinterpret_cast<F4*>(ir3 + o) = o_ir[c];
    *reinterpret_cast<F4*>(vis3 + o) = o_vis[c];
    *reinterpret_cast<F4*>(mask3 + o) = o_mask[c];
  }
  L2* lo = reinterpret_cast<L2*>(label_out + (long long)b * cp + pix);
  lo[0] = o_lab[0];
  lo[1] = o_lab[1];
}

bool sizes_ok(int N, int h, int w, int B, int crop_h, int crop_w) {
  return N > 0 && h > 0 && w > 0 && h <= SEGMIF_AUGMENT_MAX_SIDE && w <= SEGMIF_AUGMENT_MAX_SIDE && B > 0 && B <= 65535 && crop_h > 0 &&
         crop_w > 0 && crop_h <= 4 * SEGMIF_AUGMENT_MAX_SIDE && crop_w <= 4 * SEGMIF_AUGMENT_MAX_SIDE;
}

}  // namespace

extern "C" int segmif_augment_record_bytes(void) { return (int)sizeof(SegmifAugmentRec); }

extern "C" int segmif_augment_pick_u8(const uint8_t* label, int N, int h, int w, SegmifAugmentRec* rec, const int32_t* tab,
                                      int64_t tab_words, int B, int crop_h, int crop_w, void* stream) {
  if (!label || !rec || !tab || tab_words <= 0 || !sizes_ok(N, h, w, B, crop_h, crop_w)) return SEGMIF_EINVAL;
  hipLaunchKernelGGL(pick_kernel<false>, dim3(NCAND, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, label, N, h, w, rec, tab,
                     (long long)tab_words, crop_h, crop_w, (const int32_t*)nullptr, (int32_t*)nullptr, (unsigned long long*)nullptr, 0);
  return (int)hipGetLastError();
}

extern "C" int segmif_augment_pick_class_u8(const uint8_t* label, int N, int h, int w, SegmifAugmentRec* rec, const int32_t* tab,
                                            int64_t tab_words, int B, int crop_h, int crop_w, const int32_t* want, int32_t* got,
                                            int64_t* tally, int n_class_tally, void* stream) {
  if (!label || !rec || !tab || tab_words <= 0 || !want || !got || !sizes_ok(N, h, w, B, crop_h, crop_w)) return SEGMIF_EINVAL;
  if ((uintptr_t)rec & 7 || (uintptr_t)tally & 7 || (tally && n_class_tally < 1) || n_class_tally < 0) return SEGMIF_EINVAL;  // 64-bit atomics
  hipLaunchKernelGGL(pick_kernel<true>, dim3(NCAND, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, label, N, h, w, rec, tab,
                     (long long)tab_words, crop_h, crop_w, want, got, reinterpret_cast<unsigned long long*>(tally), n_class_tally);
  return (int)hipGetLastError();
}

extern "C" int segmif_augment_apply_u8(const uint8_t* ir, const uint8_t* vis, const uint8_t* mask, const uint8_t* label, int N, int h, int w,
                                       const SegmifAugmentRec* rec, const int32_t* tab, int64_t tab_words, int B, int crop_h, int crop_w,
                                       float* ir3, float* vis3, float* mask3, int64_t* label_out, void* stream) {
  if (!ir || !vis || !mask || !label || !rec || !tab || tab_words <= 0 || !ir3 || !vis3 || !mask3 || !label_out ||
      !sizes_ok(N, h, w, B, crop_h, crop_w) || (crop_w & 3))
    return SEGMIF_EINVAL;
  for (const void* p : {(const void*)ir3, (const void*)vis3, (const void*)mask3, (const void*)label_out})
    if ((uintptr_t)p & 15) return SEGMIF_EINVAL;  // 16-byte stores
  const dim3 grid((unsigned)((crop_w + TW - 1) / TW), (unsigned)((crop_h + TH - 1) / TH), (unsigned)B);
  hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, ir, vis, mask, label, N, h, w, rec, tab,
                     (long long)tab_words, crop_h, crop_w, ir3, vis3, mask3, (long long*)label_out);
  return (int)hipGetLastError();
}
