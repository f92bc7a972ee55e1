// Class statistics of label maps: counts[n][v] = pixels of frame n equal to v (v in 0..255), column 256 = values outside
// 0..255 (the int64 entry only).  Exact integers: LDS histograms per wave, one 64-bit global atomic per non-empty bin and
// block.  The resident uint8 label set (segmif_amd.data.DeviceDataset.label) is counted in one launch; the int64 entry counts
// the labels of produced batches.
//
//   grid : blocks_per_frame * N blocks of 256 threads, a frame's 16-byte chunks dealt round robin to its blocks' threads.
//   chunk: the elements whose ADDRESSES lie in one aligned 16-byte line, so a full chunk is one aligned 16-byte load whatever
//          the alignment of the frame (a slice of a larger tensor may start at any byte); the first and the last chunk of a
//          frame may be partial and are read element by element.
//   runs : label maps are blocky.  A thread carries (value, count) across ALL its chunks and touches the histogram only when
//          the value changes, so a constant frame costs one LDS atomic per thread instead of one per pixel on one bin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "segmif_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int BINS = 257;
constexpr long long CHUNKS_PER_BLOCK = 4096;  // 16 chunks a thread: 64 KiB of uint8 labels a block

struct alignas(16) Line { uint32_t w[4]; };

__device__ __forceinline__ int bin_of(uint8_t v) { return v; }
__device__ __forceinline__ int bin_of(long long v) { return (v >= 0 && v <= 255) ? (int)v : 256; }

template <typename T>
__global__ __launch_bounds__(THREADS) void label_stats_kernel(const T* __restrict__ label, long long pixels, long long per_block,
                                                              long long blocks_per_frame, unsigned long long* __restrict__ counts) {
  constexpr int E = 16 / (int)sizeof(T);  // elements of a full chunk
  __shared__ unsigned int hist[WAVES][BINS];
  const long long n = blockIdx.x / blocks_per_frame, j = blockIdx.x - n * blocks_per_frame;
  const T* frame = label + n * pixels;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(frame);
  const long long head = (long long)(addr & 15) / (long long)sizeof(T);  // elements of the first line that precede the frame
  const T* line0 = frame - head;                                        // (never dereferenced below `frame`)
  const long long chunks = (head + pixels + E - 1) / E;
  for (int i = threadIdx.x; i < WAVES * BINS; i += THREADS) (&hist[0][0])[i] = 0u;
  __syncthreads();
  unsigned int* mine = hist[threadIdx.x >> 6];
  int cur = -1;
  unsigned int run = 0;
  const long long k0 = j * per_block, k1 = min(k0 + per_block, chunks);
  for (long long k = k0 + threadIdx.x; k < k1; k += THREADS) {
    const long long e0 = k * E - head;  // first element of the chunk, relative to the frame
    if (e0 >= 0 && e0 + E <= pixels) {
      const Line l = *reinterpret_cast<const Line*>(line0 + k * E);
      T v[E];
      __builtin_memcpy(v, &l, 16);
#pragma unroll
      for (int t = 0; t < E; ++t) {
        const int b = bin_of(v[t]);
        if (b != cur) {
          if (run) atomicAdd(&mine[cur], run);
          cur = b;
          run = 0;
        }
        ++run;
      }
    } else {
      const long long a = max(e0, 0ll), z = min(e0 + E, pixels);
      for (long long e = a; e < z; ++e) {
        const int b = bin_of(frame[e]);
        if (b != cur) {
          if (run) atomicAdd(&mine[cur], run);
          cur = b;
          run = 0;
        }
        ++run;
      }
    }
  }
  if (run) atomicAdd(&mine[cur], run);
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += THREADS) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += hist[w][b];
    if (s) atomicAdd(&counts[n * BINS + b], s);
  }
}

template <typename T>
int launch(const T* label, int N, int64_t pixels, int64_t* counts, void* stream) {
  if (!label || !counts || N < 1 || pixels < 1) return SEGMIF_EINVAL;
  if (reinterpret_cast<uintptr_t>(label) % sizeof(T) || reinterpret_cast<uintptr_t>(counts) % 8) return SEGMIF_EINVAL;
  constexpr long long E = 16 / (long long)sizeof(T);
  const long long chunks = (pixels + E - 1) / E + 1;  // (+ 1: a frame that starts inside a line spills into one more)
  long long per_block = CHUNKS_PER_BLOCK, bpf = (chunks + per_block - 1) / per_block;
  while ((long long)N * bpf > (1ll << 22)) {  // the grid stays below 2^22 blocks (2^30 threads): blocks take more chunks instead
    per_block *= 2;
    bpf = (chunks + per_block - 1) / per_block;
  }
  if (per_block * E >= (1ll << 32)) return SEGMIF_EINVAL;  // a block's 32-bit LDS counters would wrap: N * pixels >= 2^54
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * BINS * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(label_stats_kernel<T>, dim3((unsigned)((long long)N * bpf)), dim3(THREADS), 0, s, label, (long long)pixels, per_block,
                     bpf, reinterpret_cast<unsigned long long*>(counts));
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int segmif_label_stats_u8(const uint8_t* label, int N, int64_t pixels, int64_t* counts, void* stream) {
  return launch<uint8_t>(label, N, pixels, counts, stream);
}

extern "C" int segmif_label_stats_i64(const int64_t* label, int N, int64_t pixels, int64_t* counts, void* stream) {
  return launch<long long>(reinterpret_cast<const long long*>(label), N, pixels, counts, stream);
}
