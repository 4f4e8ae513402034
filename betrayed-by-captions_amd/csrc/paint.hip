// build-flags: -ffp-contract=off
// Drawing a result over its image on the device (paint.py states the rules in numpy; the kernels equal them bit for bit).
//
//   cgg_paint_instances_u8   one launch: a thread owns 8 horizontally adjacent pixels (one byte of every bit-packed mask) with the
//                            24 running channel values in registers, walks the n masks in order (a mask that is not kept is
//                            skipped by the whole wave: `keep[i]` is uniform), then blends the edge pixels with white once and
//                            the box frames in order. A mask byte of 0 costs its one load; a non-zero byte also loads the bytes
//                            above, below, left and right for the edge test. A block is 4 rows x 64 bytes: the neighbour rows
//                            INSIDE the tile are lines the tile's own waves fetch for their fills (vector cache / L2); the
//                            rows across a tile border belong to another workgroup, possibly on another XCD with its own L2,
//                            and may be fetched twice. Not measured; the kernel's time at the measured shape is VALU work.
//   cgg_label_components_i32 union-find over the id map, label = smallest linear index: init (the start of the pixel's run within its
//                            64-pixel row segment, one ballot), merge (atomicMin unions with the left segment and the row above),
//                            flatten + integer atomic sums at the root, compact (roots append their record). Every loop is bounded
//                            by H * W steps and sets status[1] when it hits the bound; no loop waits for another workgroup.
//   cgg_paint_panoptic_u8    one launch: sorted id table + colours in LDS, binary search per pixel, fill once, edge once.
//
// The blend is the reference's numpy line evaluated in float64: v * (1 - alpha) + c * alpha, two rounded products and one rounded
// sum (contraction off for this file, and __dmul_rn / __dadd_rn besides), truncated to uint8.
#include "cgg_common.h"

namespace {

constexpr int PI_THREADS = 256;          // 4 rows x 64 mask bytes
constexpr int PI_MAX_N = CGG_PAINT_MAX_MASKS;
constexpr int PP_MAX_IDS = CGG_PAINT_MAX_IDS;
constexpr int CC_THREADS = 256;

__device__ __forceinline__ uint8_t paint_blend(uint8_t v, double ca, double oma) {
  // ca = colour * alpha (one rounded product, as numpy forms it before the sum)
  return (uint8_t)(int)__dadd_rn(__dmul_rn((double)v, oma), ca);
}

__global__ __launch_bounds__(PI_THREADS) void cgg_paint_instances_kernel(
    const uint8_t* img, uint8_t* out, int H, int W, const uint8_t* __restrict__ bits, int n,      // out may be img: no __restrict__
    int64_t mask_stride, int row_bytes, const uint8_t* __restrict__ keep, const uint8_t* __restrict__ colors,
    const int32_t* __restrict__ boxes, const uint8_t* __restrict__ box_colors, double alpha, double oma, double ealpha, double eoma,
    int thickness, int edges, int gx) {
  const int RB = (W + 7) >> 3;                       // bytes of a row that hold pixels
  const int tile_y = (int)(blockIdx.x / (unsigned)gx);
  const int bx = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)gx) * 64 + (threadIdx.x & 63);
  const int y = tile_y * 4 + (threadIdx.x >> 6);
  if (bx >= RB || y >= H) return;
  const int x0 = bx * 8;
  const int npx = W - x0 < 8 ? W - x0 : 8;
  const uint32_t valid = 0xffu >> (8 - npx);         // pad bits may hold anything
  const uint32_t last_valid = 0xffu >> (8 - (W - (RB - 1) * 8));
  uint8_t v[24];
  const int64_t pix = ((int64_t)y * W + x0) * 3;
#pragma unroll
  for (int k = 0; k < 24; ++k) v[k] = k < npx * 3 ? img[pix + k] : (uint8_t)0;
  uint32_t edge = 0;
  const int64_t row_off = (int64_t)y * row_bytes + bx;
  for (int i = 0; i < n; ++i) {
    if (!keep[i]) continue;                          // uniform
    const uint8_t* p = bits + (int64_t)i * mask_stride + row_off;
    const uint32_t b = (uint32_t)p[0] & valid;
    if (b == 0) continue;
    const double c0 = __dmul_rn((double)colors[i * 3 + 0], alpha);
    const double c1 = __dmul_rn((double)colors[i * 3 + 1], alpha);
    const double c2 = __dmul_rn((double)colors[i * 3 + 2], alpha);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if ((b >> k) & 1u) {
        v[k * 3 + 0] = paint_blend(v[k * 3 + 0], c0, oma);
        v[k * 3 + 1] = paint_blend(v[k * 3 + 1], c1, oma);
        v[k * 3 + 2] = paint_blend(v[k * 3 + 2], c2, oma);
      }
    }
    if (edges) {
      const uint32_t up = y > 0 ? (uint32_t)p[-row_bytes] : 0u;
      const uint32_t dn = y + 1 < H ? (uint32_t)p[row_bytes] : 0u;
      const uint32_t lf = bx > 0 ? ((uint32_t)p[-1] >> 7) : 0u;
      uint32_t rt = 0;
      if (bx + 1 < RB) rt = ((uint32_t)p[1] & (bx + 2 == RB ? last_valid : 0xffu)) & 1u;
      const uint32_t inner = up & dn & ((b << 1) | lf) & ((b >> 1) | (rt << 7));
      edge |= b & ~inner;
    }
  }
  if (edge) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if ((edge >> k) & 1u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k * 3 + c] = paint_blend(v[k * 3 + c], __dmul_rn(255.0, ealpha), eoma);
      }
    }
  }
  if (boxes) {
    for (int i = 0; i < n; ++i) {
      if (!keep[i]) continue;
      const int bx0 = boxes[i * 4 + 0], by0 = boxes[i * 4 + 1], bx1 = boxes[i * 4 + 2], by1 = boxes[i * 4 + 3];
      if (y < by0 || y > by1 || x0 > bx1 || x0 + npx - 1 < bx0) continue;
      const bool yband = (int64_t)y - by0 < thickness || (int64_t)by1 - y < thickness;
      const double c0 = __dmul_rn((double)box_colors[i * 3 + 0], ealpha);
      const double c1 = __dmul_rn((double)box_colors[i * 3 + 1], ealpha);
      const double c2 = __dmul_rn((double)box_colors[i * 3 + 2], ealpha);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int x = x0 + k;
        if (x < bx0 || x > bx1) continue;
        if (yband || (int64_t)x - bx0 < thickness || (int64_t)bx1 - x < thickness) {
          v[k * 3 + 0] = paint_blend(v[k * 3 + 0], c0, eoma);
          v[k * 3 + 1] = paint_blend(v[k * 3 + 1], c1, eoma);
          v[k * 3 + 2] = paint_blend(v[k * 3 + 2], c2, eoma);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 24; ++k)
    if (k < npx * 3) out[pix + k] = v[k];
}

// bool planes (one byte per pixel, non-zero = set) -> the bit-packed rows the paint kernel reads; a thread writes one byte
__global__ __launch_bounds__(256) void cgg_pack_bool_rows_kernel(const uint8_t* __restrict__ m, int64_t rows, int W, int row_bytes,
                                                                 uint8_t* __restrict__ bits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * row_bytes) return;
  const int64_t r = t / row_bytes;
  const int x0 = (int)(t - r * row_bytes) * 8;
  const uint8_t* src = m + r * W + x0;
  uint32_t b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (x0 + k < W && src[k]) b |= 1u << k;
  bits[t] = (uint8_t)b;
}

// ---- connected components ----------------------------------------------------------------------------------------------------

__device__ __forceinline__ int cc_find(const int32_t* L, int x, int64_t bound, int32_t* status) {
  int64_t steps = 0;
  int p = L[x];
  while (p != x) {
    if (++steps > bound) {
      atomicOr(status + 1, 1);
      break;
    }
    x = p;
    p = L[x];
  }
  return x;
}

// unite the sets of a and b: the larger root is linked under the smaller, so a set's root is its smallest linear index
__device__ __forceinline__ void cc_union(int32_t* L, int a, int b, int64_t bound, int32_t* status) {
  int64_t steps = 0;
  a = cc_find(L, a, bound, status);
  b = cc_find(L, b, bound, status);
  while (a != b) {
    if (++steps > bound) {
      atomicOr(status + 1, 1);
      return;
    }
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }                                               // a > b
    const int old = atomicMin(L + a, b);
    if (old == a) return;                           // a was a root and now hangs under b
    a = old;                                        // a had a parent already: go on uniting that parent with b
  }
}

// one wave per 64-pixel row segment: label = first pixel of the run (equal id) within the segment; void / negative ids = -1
__global__ __launch_bounds__(CC_THREADS) void cgg_cc_init_kernel(const int32_t* __restrict__ pan, int H, int W, int S, int void_id,
                                                                 int32_t* __restrict__ L, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
  if (seg >= (int64_t)H * S) return;                // whole waves leave
  const int y = (int)(seg / S);
  const int x = (int)(seg - (int64_t)y * S) * 64 + lane;
  const bool in = x < W;
  const int64_t p = (int64_t)y * W + x;
  const int id = in ? pan[p] : -1;
  const int left = (in && lane > 0) ? pan[p - 1] : -1;
  const uint64_t starts = __ballot(lane == 0 || id != left);
  if (!in) return;
  if (id < 0) atomicOr(status + 1, 2);
  const uint64_t below = starts & (~0ull >> (63 - lane));
  const int first = 63 - __builtin_clzll(below);    // bit 0 is always set
  L[p] = (id < 0 || id == void_id) ? -1 : (int32_t)(p - lane + first);
}

__global__ __launch_bounds__(CC_THREADS) void cgg_cc_merge_kernel(const int32_t* __restrict__ pan, int H, int W, int void_id,
                                                                  int32_t* __restrict__ L, int32_t* __restrict__ status) {
  const int64_t HW = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= HW) return;
  if (L[p] < 0) return;
  const int id = pan[p];
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const bool w = x > 0 && pan[p - 1] == id;
  if (w && (x & 63) == 0) cc_union(L, (int)p, (int)p - 1, HW, status);         // runs are joined inside a segment already
  if (y == 0) return;
  const bool nn = pan[p - W] == id;
  const bool nw = x > 0 && pan[p - W - 1] == id;
  const bool ne = x + 1 < W && pan[p - W + 1] == id;
  if (nn) {
    if (!(w && nw)) cc_union(L, (int)p, (int)(p - W), HW, status);             // else p ~ W ~ NW ~ N already
  } else {
    if (nw && !w) cc_union(L, (int)p, (int)(p - W - 1), HW, status);           // with w: W's own N is NW
    if (ne) cc_union(L, (int)p, (int)(p - W + 1), HW, status);
  }
}

// root of every pixel, and the integer sums of the component at its root. One wave per row segment: the first pixel of a run adds
// the whole run (its length, the sum of its x, y times its length) with one atomic per word.
__global__ __launch_bounds__(CC_THREADS) void cgg_cc_flatten_kernel(int H, int W, int S, int32_t* __restrict__ L,
                                                                    int32_t* __restrict__ area, unsigned long long* __restrict__ sx,
                                                                    unsigned long long* __restrict__ sy, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
  if (seg >= (int64_t)H * S) return;
  const int y = (int)(seg / S);
  const int x = (int)(seg - (int64_t)y * S) * 64 + lane;
  const bool in = x < W;
  const int64_t p = (int64_t)y * W + x;
  int root = -1;
  if (in && L[p] >= 0) root = cc_find(L, (int)p, (int64_t)H * W, status);
  const int left = __shfl_up(root, 1);
  const uint64_t starts = __ballot(lane == 0 || root != left);
  if (root < 0) return;
  L[p] = root;
  if (!((starts >> lane) & 1ull)) return;
  const uint64_t after = lane == 63 ? 0ull : (starts >> (lane + 1));
  int len = after ? __builtin_ctzll(after) + 1 : 64 - lane;
  if (x + len > W) len = W - x;
  atomicAdd(area + root, len);
  atomicAdd(sx + root, (unsigned long long)len * (unsigned long long)x + (unsigned long long)len * (len - 1) / 2);
  atomicAdd(sy + root, (unsigned long long)len * (unsigned long long)y);
}

__global__ __launch_bounds__(CC_THREADS) void cgg_cc_compact_kernel(const int32_t* __restrict__ pan, int64_t HW,
                                                                    const int32_t* __restrict__ L, const int32_t* __restrict__ area,
                                                                    const unsigned long long* __restrict__ sx,
                                                                    const unsigned long long* __restrict__ sy,
                                                                    int64_t* __restrict__ records, int capacity,
                                                                    int32_t* __restrict__ status) {
  const int64_t p = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= HW) return;
  if (L[p] != (int32_t)p) return;
  const int slot = atomicAdd(status, 1);
  if (slot >= capacity) return;
  int64_t* r = records + (int64_t)slot * 5;
  r[0] = p;
  r[1] = pan[p];
  r[2] = area[p];
  r[3] = (int64_t)sx[p];
  r[4] = (int64_t)sy[p];
}

// ---- panoptic paint -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void cgg_paint_panoptic_kernel(const uint8_t* img, uint8_t* out,       /* out may be img */
                                                                 const int32_t* __restrict__ pan, int H, int W,
                                                                 const int32_t* __restrict__ ids, const uint8_t* __restrict__ colors,
                                                                 int nids, double alpha, double oma, double ealpha, double eoma,
                                                                 int edges) {
  __shared__ int32_t s_ids[PP_MAX_IDS];
  __shared__ uint8_t s_col[PP_MAX_IDS * 3];
  for (int k = threadIdx.x; k < nids; k += blockDim.x) s_ids[k] = ids[k];
  for (int k = threadIdx.x; k < nids * 3; k += blockDim.x) s_col[k] = colors[k];
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int id = pan[p];
  int lo = 0, hi = nids;                            // first table entry >= id
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  uint8_t v0 = img[p * 3 + 0], v1 = img[p * 3 + 1], v2 = img[p * 3 + 2];
  if (lo < nids && s_ids[lo] == id) {
    v0 = paint_blend(v0, __dmul_rn((double)s_col[lo * 3 + 0], alpha), oma);
    v1 = paint_blend(v1, __dmul_rn((double)s_col[lo * 3 + 1], alpha), oma);
    v2 = paint_blend(v2, __dmul_rn((double)s_col[lo * 3 + 2], alpha), oma);
    if (edges) {
      const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
      const bool e = x == 0 || x == W - 1 || y == 0 || y == H - 1 || pan[p - 1] != id || pan[p + 1] != id || pan[p - W] != id ||
                     pan[p + W] != id;
      if (e) {
        const double w = __dmul_rn(255.0, ealpha);
        v0 = paint_blend(v0, w, eoma);
        v1 = paint_blend(v1, w, eoma);
        v2 = paint_blend(v2, w, eoma);
      }
    }
  }
  out[p * 3 + 0] = v0;
  out[p * 3 + 1] = v1;
  out[p * 3 + 2] = v2;
}

inline bool paint_alpha_ok(double alpha, double oma) { return alpha >= 0.0 && alpha <= 1.0 && oma >= 0.0 && oma <= 1.0; }

}  // namespace

extern "C" int cgg_paint_instances_u8(const uint8_t* img, uint8_t* out, int H, int W, const uint8_t* bits, int n,
                                      int64_t mask_stride_bytes, int row_bytes, const uint8_t* keep, const uint8_t* colors,
                                      const int32_t* boxes, const uint8_t* box_colors, double alpha, double one_minus_alpha,
                                      int thickness, int edges, cgg_stream_t stream) {
  CGG_REQUIRE(H > 0 && W > 0 && n >= 0 && thickness >= 0, CGG_EINVAL, "cgg_paint_instances_u8: bad sizes (H=%d W=%d n=%d thickness=%d)",
              H, W, n, thickness);
  CGG_REQUIRE(img && out, CGG_EINVAL, "cgg_paint_instances_u8: null image pointer");
  CGG_REQUIRE(n == 0 || (bits && keep && colors), CGG_EINVAL, "cgg_paint_instances_u8: null pointer (bits / keep / colors)");
  CGG_REQUIRE(!boxes || box_colors || n == 0, CGG_EINVAL, "cgg_paint_instances_u8: null pointer (box_colors beside boxes)");
  CGG_REQUIRE(n == 0 || (row_bytes > 0 && (int64_t)row_bytes * 8 >= W && mask_stride_bytes >= (int64_t)H * row_bytes), CGG_EINVAL,
              "cgg_paint_instances_u8: bad mask layout (W=%d row_bytes=%d mask_stride_bytes=%lld)", W, row_bytes,
              (long long)mask_stride_bytes);
  CGG_REQUIRE(paint_alpha_ok(alpha, one_minus_alpha), CGG_EINVAL, "cgg_paint_instances_u8: alpha and 1 - alpha must lie in [0, 1]");
  CGG_REQUIRE(n <= PI_MAX_N, CGG_EUNSUPPORTED, "cgg_paint_instances_u8: n = %d masks (at most %d)", n, PI_MAX_N);
  CGG_REQUIRE((int64_t)H * W * 3 <= ((int64_t)1 << 31), CGG_EUNSUPPORTED, "cgg_paint_instances_u8: image of %lld bytes (at most 2^31)",
              (long long)H * W * 3);
  const int RB = (W + 7) / 8;
  const int gx = (RB + 63) / 64;
  const dim3 grid((unsigned)((int64_t)gx * ((H + 3) / 4)));         // <= 2^31 / 3 / 8 / 4 + H / 4 blocks: fits one dimension
  const double ea = 0.8, eo = 1 - 0.8;              // edges and boxes: white / the box colour at alpha 0.8, as the fills at 0.8
  hipLaunchKernelGGL(cgg_paint_instances_kernel, grid, dim3(PI_THREADS), 0, (hipStream_t)stream, img, out, H, W, bits, n,
                     mask_stride_bytes, row_bytes, keep, colors, n > 0 ? boxes : nullptr, box_colors, alpha, one_minus_alpha, ea, eo,
                     thickness, edges, gx);
  CGG_CHECK_LAUNCH("cgg_paint_instances_u8");
  return CGG_OK;
}

extern "C" int cgg_pack_bool_rows_u8(const uint8_t* masks, int64_t rows, int W, int row_bytes, uint8_t* bits, cgg_stream_t stream) {
  CGG_REQUIRE(rows >= 0 && W > 0 && row_bytes > 0 && (int64_t)row_bytes * 8 >= W, CGG_EINVAL,
              "cgg_pack_bool_rows_u8: bad sizes (rows=%lld W=%d row_bytes=%d)", (long long)rows, W, row_bytes);
  CGG_REQUIRE(rows == 0 || (masks && bits), CGG_EINVAL, "cgg_pack_bool_rows_u8: null pointer");
  CGG_REQUIRE(rows * row_bytes < ((int64_t)1 << 38), CGG_EUNSUPPORTED, "cgg_pack_bool_rows_u8: %lld output bytes",
              (long long)(rows * row_bytes));
  if (rows == 0) return CGG_OK;
  hipLaunchKernelGGL(cgg_pack_bool_rows_kernel, dim3((unsigned)((rows * row_bytes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     masks, rows, W, row_bytes, bits);
  CGG_CHECK_LAUNCH("cgg_pack_bool_rows_u8");
  return CGG_OK;
}

extern "C" int64_t cgg_label_components_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
  return (int64_t)H * W * 24;                       // labels + areas (int32), x sums + y sums (uint64)
}

extern "C" int cgg_label_components_i32(const int32_t* pan, int H, int W, int void_id, void* ws, int64_t* records, int capacity,
                                        int32_t* status, cgg_stream_t stream) {
  CGG_REQUIRE(H > 0 && W > 0 && capacity >= 0, CGG_EINVAL, "cgg_label_components_i32: bad sizes (H=%d W=%d capacity=%d)", H, W, capacity);
  CGG_REQUIRE(pan && ws && status && (capacity == 0 || records), CGG_EINVAL, "cgg_label_components_i32: null pointer");
  CGG_REQUIRE((((uintptr_t)ws) & 7u) == 0 && (((uintptr_t)records) & 7u) == 0 && (((uintptr_t)status) & 3u) == 0, CGG_EINVAL,
              "cgg_label_components_i32: ws / records must be 8-byte and status 4-byte aligned");
  const int64_t HW = (int64_t)H * W;
  CGG_REQUIRE(HW < ((int64_t)1 << 31), CGG_EUNSUPPORTED, "cgg_label_components_i32: H * W = %lld does not fit 31 bits", (long long)HW);
  hipStream_t s = (hipStream_t)stream;
  // layout: the 64-bit sums first (8-byte aligned), then the 32-bit words
  unsigned long long* sx = (unsigned long long*)ws;
  unsigned long long* sy = sx + HW;
  int32_t* L = (int32_t*)(sy + HW);
  int32_t* area = L + HW;
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)HW * 16, s);
  if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)HW * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, 8, s);
  CGG_REQUIRE(e == hipSuccess, (int)e, "cgg_label_components_i32: memset failed: %s", hipGetErrorString(e));
  const int S = (W + 63) / 64;
  const unsigned seg_blocks = (unsigned)(((int64_t)H * S + CC_THREADS / 64 - 1) / (CC_THREADS / 64));
  const unsigned pix_blocks = (unsigned)((HW + CC_THREADS - 1) / CC_THREADS);
  hipLaunchKernelGGL(cgg_cc_init_kernel, dim3(seg_blocks), dim3(CC_THREADS), 0, s, pan, H, W, S, void_id, L, status);
  CGG_CHECK_LAUNCH("cgg_label_components_i32(init)");
  hipLaunchKernelGGL(cgg_cc_merge_kernel, dim3(pix_blocks), dim3(CC_THREADS), 0, s, pan, H, W, void_id, L, status);
  CGG_CHECK_LAUNCH("cgg_label_components_i32(merge)");
  hipLaunchKernelGGL(cgg_cc_flatten_kernel, dim3(seg_blocks), dim3(CC_THREADS), 0, s, H, W, S, L, area, sx, sy, status);
  CGG_CHECK_LAUNCH("cgg_label_components_i32(flatten)");
  hipLaunchKernelGGL(cgg_cc_compact_kernel, dim3(pix_blocks), dim3(CC_THREADS), 0, s, pan, HW, L, area, sx, sy, records, capacity,
                     status);
  CGG_CHECK_LAUNCH("cgg_label_components_i32(compact)");
  return CGG_OK;
}

extern "C" int cgg_paint_panoptic_u8(const uint8_t* img, uint8_t* out, const int32_t* pan, int H, int W, const int32_t* ids,
                                     const uint8_t* colors, int nids, double alpha, double one_minus_alpha, int edges,
                                     cgg_stream_t stream) {
  CGG_REQUIRE(H > 0 && W > 0 && nids >= 0, CGG_EINVAL, "cgg_paint_panoptic_u8: bad sizes (H=%d W=%d nids=%d)", H, W, nids);
  CGG_REQUIRE(img && out && pan && (nids == 0 || (ids && colors)), CGG_EINVAL, "cgg_paint_panoptic_u8: null pointer");
  CGG_REQUIRE(paint_alpha_ok(alpha, one_minus_alpha), CGG_EINVAL, "cgg_paint_panoptic_u8: alpha and 1 - alpha must lie in [0, 1]");
  CGG_REQUIRE(nids <= PP_MAX_IDS, CGG_EUNSUPPORTED, "cgg_paint_panoptic_u8: table of %d ids (at most %d)", nids, PP_MAX_IDS);
  const int64_t HW = (int64_t)H * W;
  CGG_REQUIRE(HW * 3 <= ((int64_t)1 << 31), CGG_EUNSUPPORTED, "cgg_paint_panoptic_u8: image of %lld bytes (at most 2^31)",
              (long long)HW * 3);
  const double ea = 0.8, eo = 1 - 0.8;
  hipLaunchKernelGGL(cgg_paint_panoptic_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, out, pan, H,
                     W, ids, colors, nids, alpha, one_minus_alpha, ea, eo, edges);
  CGG_CHECK_LAUNCH("cgg_paint_panoptic_u8");
  return CGG_OK;
}
