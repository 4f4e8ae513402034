// Device side of the COCO run-length encoding of bit-packed masks: the positions at which the column-major bit stream of a
// mask changes value (host_results.rle_transitions_host states the rule; the kernels equal it exactly). The host then only
// turns those positions into the delta-coded counts string (cgg_rle_strings_from_transitions, rle.hip): per mask it
// receives a few hundred 4-byte positions instead of a 128 KB plane.
//
//   count   one wave per (mask, 64-column strip), walking down the block-rows: lane r loads the 8 bytes of row r, 64 ballots
//           hand lane c the word of column c (bit r = row r), which is stored to the column-major planes `cols`; the
//           transition word is w ^ ((w << 1) | prev), prev = the pixel above (bit 63 of the block-row above; for row 0 the
//           bottom pixel of the column to the left, read from the input; 0 for column 0). Uniform blocks (all 0 / all 1: most
//           of an object mask) skip the ballots. The strip's transition count goes to `counts`.
//   scan    one block: exclusive scan of the n * strips counts -> the strips' first output index (int64) and offsets[0..n]
//   emit    one wave per (mask, strip): lane c recomputes its column's transition words from `cols`, a wave scan of the column
//           counts places the lanes, each lane peels its words with count-trailing-zeros and writes x * H + row. A mask is
//           written iff all of it fits below `capacity` (offsets[i + 1] <= capacity).
//
// No host read, no allocation, no atomics: three launches that a stream capture can hold.
#include "cgg_common.h"

namespace {

constexpr int RT_WAVES = 4;                 // waves per block of the count / emit kernels (each wave works alone)
constexpr int RT_SCAN_THREADS = 1024;

struct RtLayout {
  int64_t counts_off;   // bytes
  int64_t bases_off;
  int64_t total;
};

inline RtLayout rt_layout(int64_t n, int H, int W) {
  const int64_t S = (W + 63) / 64, HB = (H + 63) / 64;
  RtLayout l;
  l.counts_off = n * S * 64 * HB * 8;
  l.bases_off = l.counts_off + ((n * S * 4 + 7) & ~(int64_t)7);
  l.total = l.bases_off + n * S * 8;
  return l;
}

__device__ __forceinline__ uint64_t rt_low_bits(int k) {      // k in 1..64
  return ~0ull >> (64 - k);
}

// lane r holds row r of a 64 x 64 bit block (bit c = column c) -> lane c holds column c (bit r = row r)
__device__ __forceinline__ uint64_t rt_transpose_wave(uint64_t w) {
  const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
  const int lane = threadIdx.x & 63;
  uint64_t t = 0;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const uint64_t b = __ballot((lo >> c) & 1u);
    if (lane == c) t = b;
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const uint64_t b = __ballot((hi >> c) & 1u);
    if (lane == 32 + c) t = b;
  }
  return t;
}

__global__ __launch_bounds__(RT_WAVES * 64) void cgg_rt_count_kernel(const uint8_t* __restrict__ bits, int64_t nstrips, int S,
                                                                     int H, int W, int HB, int64_t mask_stride, int row_bytes,
                                                                     uint64_t* __restrict__ cols, uint32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
  if (idx >= nstrips) return;                       // whole waves leave: the ballots below see full waves only
  const int64_t i = idx / S;
  const int x0 = (int)(idx - i * S) * 64;
  const int ncols = W - x0 < 64 ? W - x0 : 64;
  const int nb = (ncols + 7) >> 3;                  // bytes of this strip present in a row
  const uint64_t cmask = rt_low_bits(ncols);
  const uint8_t* plane = bits + i * mask_stride;
  const bool col_valid = lane < ncols;
  // the pixel before the top of column x0 + lane in the stream: the bottom pixel of the column to its left
  uint64_t prev = 0;
  {
    const int xl = x0 + lane - 1;
    if (col_valid && xl >= 0) prev = (plane[(int64_t)(H - 1) * row_bytes + (xl >> 3)] >> (xl & 7)) & 1u;
  }
  uint64_t* dst = cols + ((i * S * 64 + x0 + lane) * HB);
  uint32_t cnt = 0;
  for (int by = 0; by < HB; ++by) {
    const int rows = H - by * 64 < 64 ? H - by * 64 : 64;
    uint64_t w = 0;
    if (lane < rows) {
      const uint8_t* p = plane + (int64_t)(by * 64 + lane) * row_bytes + (x0 >> 3);
      if (nb == 8 && (((uintptr_t)p) & 7u) == 0) {
        w = *(const uint64_t*)p;
      } else {
        for (int b = 0; b < nb; ++b) w |= (uint64_t)p[b] << (8 * b);
      }
      w &= cmask;                                   // pad bits may hold anything
    }
    uint64_t t;
    if (__ballot(w != 0) == 0) {
      t = 0;
    } else if (rows == 64 && __ballot(w != cmask) == 0) {
      t = col_valid ? ~0ull : 0;
    } else {
      t = rt_transpose_wave(w);
    }
    dst[by] = t;
    const uint64_t tw = col_valid ? ((t ^ ((t << 1) | prev)) & rt_low_bits(rows)) : 0;
    cnt += (uint32_t)__popcll(tw);
    prev = t >> 63;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  if (lane == 0) counts[idx] = cnt;
}

// exclusive scan of counts[0 .. nstrips) -> bases (int64); offsets[i] = bases[i * S], offsets[n] = total
__global__ __launch_bounds__(RT_SCAN_THREADS) void cgg_rt_scan_kernel(const uint32_t* __restrict__ counts, int64_t nstrips, int S,
                                                                      int n, int64_t* __restrict__ bases,
                                                                      int64_t* __restrict__ offsets) {
  __shared__ int64_t wave_sum[RT_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < nstrips; c0 += RT_SCAN_THREADS) {
    const int64_t idx = c0 + tid;
    const int64_t v = idx < nstrips ? (int64_t)counts[idx] : 0;
    int64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int k = 0; k < RT_SCAN_THREADS / 64; ++k) {
      const int64_t s = wave_sum[k];
      if (k < wv) before += s;
      all += s;
    }
    const int64_t excl = carry + before + inc - v;
    if (idx < nstrips) {
      bases[idx] = excl;
      if (idx % S == 0) offsets[idx / S] = excl;
    }
    carry += all;
    __syncthreads();
  }
  if (tid == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(RT_WAVES * 64) void cgg_rt_emit_kernel(const uint64_t* __restrict__ cols,
                                                                    const uint32_t* __restrict__ counts,
                                                                    const int64_t* __restrict__ bases,
                                                                    const int64_t* __restrict__ offsets, int64_t nstrips, int S, int H,
                                                                    int W, int HB, uint32_t* __restrict__ positions, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
  if (idx >= nstrips) return;
  if (counts[idx] == 0) return;
  const int64_t i = idx / S;
  if (offsets[i + 1] > capacity) return;            // the mask does not fit: the host encodes it from its `cols` planes
  const int x = (int)(idx - i * S) * 64 + lane;
  const bool col_valid = x < W;
  const uint64_t* src = cols + ((i * S * 64 + x) * HB);
  uint64_t prev0 = 0;
  if (col_valid && x > 0) prev0 = (src[-1] >> ((H - 1) & 63)) & 1u;      // last word of column x - 1, bit of row H - 1
  uint32_t mine = 0;
  if (col_valid) {
    uint64_t prev = prev0;
    for (int by = 0; by < HB; ++by) {
      const int rows = H - by * 64 < 64 ? H - by * 64 : 64;
      const uint64_t t = src[by];
      mine += (uint32_t)__popcll((t ^ ((t << 1) | prev)) & rt_low_bits(rows));
      prev = t >> 63;
    }
  }
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (mine == 0) return;
  uint32_t* out = positions + bases[idx] + (inc - mine);     // ends at most at offsets[i + 1] <= capacity
  const uint32_t p0 = (uint32_t)x * (uint32_t)H;
  uint64_t prev = prev0;
  for (int by = 0; by < HB; ++by) {
    const int rows = H - by * 64 < 64 ? H - by * 64 : 64;
    const uint64_t t = src[by];
    uint64_t tw = (t ^ ((t << 1) | prev)) & rt_low_bits(rows);
    prev = t >> 63;
    while (tw) {
      *out++ = p0 + (uint32_t)(by * 64 + __builtin_ctzll(tw));
      tw &= tw - 1;
    }
  }
}

}  // namespace

extern "C" int64_t cgg_rle_transitions_workspace_bytes(int n, int H, int W) {
  if (n < 0 || H <= 0 || W <= 0) return 0;
  return rt_layout(n, H, W).total;
}

extern "C" int cgg_rle_transitions(const uint8_t* bits, int n, int H, int W, int64_t mask_stride_bytes, int row_bytes, void* ws,
                                   uint32_t* positions, int64_t capacity, int64_t* offsets, cgg_stream_t stream) {
  CGG_REQUIRE(n >= 0 && H > 0 && W > 0 && row_bytes > 0 && (int64_t)row_bytes * 8 >= W &&
                  mask_stride_bytes >= (int64_t)H * row_bytes && capacity >= 0,
              CGG_EINVAL, "cgg_rle_transitions: bad sizes (n=%d H=%d W=%d row_bytes=%d mask_stride_bytes=%lld capacity=%lld)", n, H,
              W, row_bytes, (long long)mask_stride_bytes, (long long)capacity);
  CGG_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CGG_EINVAL, "cgg_rle_transitions: H * W = %lld does not fit 31 bits",
              (long long)H * W);
  CGG_REQUIRE(offsets && (n == 0 || (bits && ws)) && (capacity == 0 || positions), CGG_EINVAL,
              "cgg_rle_transitions: null pointer");
  CGG_REQUIRE((((uintptr_t)ws) & 7u) == 0 && (((uintptr_t)offsets) & 7u) == 0 && (((uintptr_t)positions) & 3u) == 0, CGG_EINVAL,
              "cgg_rle_transitions: ws / offsets must be 8-byte and positions 4-byte aligned");
  const int S = (W + 63) / 64, HB = (H + 63) / 64;
  const int64_t nstrips = (int64_t)n * S;
  CGG_REQUIRE(nstrips <= (int64_t)0x7fffffff, CGG_EINVAL, "cgg_rle_transitions: n * ceil(W / 64) = %lld strips",
              (long long)nstrips);
  hipStream_t s = (hipStream_t)stream;
  const RtLayout l = rt_layout(n, H, W);
  uint64_t* cols = (uint64_t*)ws;
  uint32_t* counts = (uint32_t*)((char*)ws + l.counts_off);
  int64_t* bases = (int64_t*)((char*)ws + l.bases_off);
  const unsigned blocks = (unsigned)((nstrips + RT_WAVES - 1) / RT_WAVES);
  if (n > 0) {
    hipLaunchKernelGGL(cgg_rt_count_kernel, dim3(blocks), dim3(RT_WAVES * 64), 0, s, bits, nstrips, S, H, W, HB, mask_stride_bytes,
                       row_bytes, cols, counts);
    CGG_CHECK_LAUNCH("cgg_rle_transitions(count)");
  }
  hipLaunchKernelGGL(cgg_rt_scan_kernel, dim3(1), dim3(RT_SCAN_THREADS), 0, s, counts, nstrips, S, n, bases, offsets);
  CGG_CHECK_LAUNCH("cgg_rle_transitions(scan)");
  if (n > 0 && capacity > 0) {
    hipLaunchKernelGGL(cgg_rt_emit_kernel, dim3(blocks), dim3(RT_WAVES * 64), 0, s, cols, counts, bases, offsets, nstrips, S, H, W,
                       HB, positions, capacity);
    CGG_CHECK_LAUNCH("cgg_rle_transitions(emit)");
  }
  return CGG_OK;
}
