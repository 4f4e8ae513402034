// The reference's training pipeline (large-scale jitter) on the device, two launches per batch: raw HWC uint8 images, instance masks
// and semantic maps -> the (B, 3, H, W) float32 batch, the (N, H, W) uint8 masks, the (B, 1, H, W) semantic maps and the per-instance
// area / box the annotation filter needs. Replaces, per sample, [3P] mmdet RandomFlip -> Resize(ratio_range, keep_ratio) ->
// RandomCrop(absolute) -> FilterAnnotations(by_mask) -> Pad(size) -> Normalize(to_rgb), which the reference runs on the CPU: at ratio 2
// it resizes a float image and every mask to 2048^2 and throws three quarters away. Flip, resize and crop compose into index
// arithmetic, so every output pixel of the window is ONE gather from the raw sample: 4 source pixels (image) or 1 (masks, semantic map).
// The random decisions (flip, resized size, window corner) arrive in the descriptor rows. The arithmetic is the rule written down in
// train_prep.py (`prepare_train_host`), bit for bit:
//   window    output (y, x) is resized pixel (Y, X) = (y + oy, x + ox); inside the image iff y < min(nh - oy, ch), x < min(nw - ox, cw)
//   taps      scale = 1 / (d / s) in double; fx = float((k + 0.5) * scale - 0.5), two separately rounded double operations;
//             i = floor(fx), fx -= i, clamped at both ends; a0 = 1 - fx, a1 = fx (float32: the image is float from the loader on)
//   pixel     R = float(float(p[i0] a0) + float(p[i1] a1)) per source row; v = float(float(R0 b0) + float(R1 b1));
//             value = float(float(v - mean) * (1 / std)); under flip source column c is read at w - 1 - c
//   nearest   row min(floor(Y * scale), h - 1) in double, columns likewise and mirrored under flip; a mask pixel is set where the
//             source byte is non-zero, the semantic map copies the byte
//   outside   the image planes hold one constant per plane, masks 0, the semantic map seg_pad
// The rounding of (k + 0.5) * scale - 0.5 decides which source pixel a tap lands on and every product and sum above is rounded on its
// own, so nothing here may be contracted into a fused multiply-add: the file is built with contraction off (the flag below, and the
// pragma for a build that ignores the flag line).
//
// Image kernel: the tile geometry of image_prep.hip -- a workgroup of 4 wavefronts owns a 16 x 256 tile of one image's output planes,
// a lane 4 consecutive columns, non-temporal float4 stores when W % 4 == 0. Only the window is computed. The source bytes a tile needs
// are staged into LDS (u8_resize.h) when they fit U8_LDS_BYTES (always when upsampling, where up to 4 output pixels share a source
// pixel at ratio 2); a tile that downsamples by more than ~1.5 x reads its taps from global memory. The workgroup of an image's
// first tile also initialises the statistics rows of the image's instances, so the caller clears nothing.
//
// Plane kernel: one 16 x 256 tile of one instance mask or one semantic map per workgroup, one byte gathered per pixel, 4 pixels packed
// into one dword store when W % 4 == 0. A mask tile reduces its area, and the smallest / largest set column and row, inside the
// wavefront from the ballots of the 4 pixel columns (population count; first and last set lane = the cross-lane minimum and maximum),
// combines the 4 wavefronts through LDS and leaves with one atomicAdd / atomicMin / atomicMax each on the instance's int32
// statistics row -- issued by one lane, and only by tiles that hold a set pixel.
//
// Panoptic samples (cgg_train_prep_panoptic_u8): the image kernel, then ONE kernel that gathers one id of the panoptic id map per output
// pixel and derives every thing mask, the semantic plane and the statistics from it (stated at the kernel).
//
// Polygon samples (cgg_train_prep_polygons_u8): the image kernel, then a fill kernel that rasterises every instance's COCO polygons
// into a column-major bit plane at source resolution (rule 6 of train_prep.py, stated at the kernel), then the plane kernel's body
// over those bits instead of staged bytes.
//
// build-flags: -ffp-contract=off
#include "cgg_common.h"

// the tap rule, the tile's LDS image and the address of a tap in it, the three-plane store, PrepConst
#include "u8_resize.h"

#pragma clang fp contract(off)

#define TP_TW 256
#define TP_TH 16
#define TP_IMG_COLS CGG_TRAIN_PREP_IMG_COLS
#define TP_INST_COLS CGG_TRAIN_PREP_INST_COLS

// rule 2 for one resized index k of an axis with source length s: taps i0 / i1 and their float32 weights
__device__ __forceinline__ void tp_coef(int k, int s, double scale, int& i0, int& i1, float& a0, float& a1) {
  const U8Tap t = u8_tap(k, s, scale);
  a0 = 1.f - t.fx;
  a1 = t.fx;
  i0 = t.i0;
  i1 = t.i1;
}

// rule 3: the source index of resized index k
__device__ __forceinline__ int tp_nearest(int k, int s, double scale) { return min((int)floor((double)k * scale), s - 1); }

__device__ __forceinline__ float tp_pixel(int p00, int p01, int p10, int p11, float a0, float a1, float b0, float b1) {
  const float r0 = (float)p00 * a0 + (float)p01 * a1, r1 = (float)p10 * a0 + (float)p11 * a1;
  return r0 * b0 + r1 * b1;
}

__global__ __launch_bounds__(256) void cgg_train_prep_image_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                                                    PrepConst cst, float* __restrict__ out, int32_t* __restrict__ stats,
                                                                    int H, int W, int ch, int cw) {
  __shared__ uint32_t lds[U8_LDS_BYTES / 4];
  const int b = blockIdx.z;
  const int32_t* d = table + TP_IMG_COLS * b;
  const int off = d[0], h = d[1], w = d[2], pitch = d[3], nh = d[4], nw = d[5], oy = d[6], ox = d[7], flip = d[8];
  const int eh = min(nh - oy, ch), ew = min(nw - ox, cw);     // the image's extent inside the plane (>= 1: oy <= max(nh - ch, 0))
  const int x0 = blockIdx.x * TP_TW, y0 = blockIdx.y * TP_TH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double sx = 1.0 / ((double)nw / (double)w), sy = 1.0 / ((double)nh / (double)h);

  if (blockIdx.x == 0 && blockIdx.y == 0) {                    // the statistics rows of this image's instances: 0, +max, +max, -1, -1
    const int first = d[9], n = d[10];
    for (int t = threadIdx.x; t < 5 * n; t += 256) {
      const int j = t % 5;
      stats[(size_t)5 * first + t] = j == 0 ? 0 : (j <= 2 ? INT32_MAX : -1);
    }
  }

  // ---- the tile's source span (workgroup-uniform) and its LDS image -----------------------------------------------------------
  const bool inside = x0 < ew && y0 < eh;
  const U8Tile tile = u8_tile_stage(lds, src, inside, off, h, w, pitch, y0 + oy, min(y0 + TP_TH, eh) - 1 + oy, x0 + ox,
                                     min(x0 + TP_TW, ew) - 1 + ox, sy, sx, flip != 0);
  if (tile.use_lds) __syncthreads();               // uniform: every wavefront of the workgroup takes the same side

  // ---- this lane's 4 columns ----------------------------------------------------------------------------------------------------
  const int xl = x0 + 4 * lane;
  int xi0[4], xi1[4];
  float xa0[4], xa1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    xi0[c] = xi1[c] = 0;
    xa0[c] = xa1[c] = 0.f;
    if (inside && xl + c < ew) {
      tp_coef(xl + c + ox, w, sx, xi0[c], xi1[c], xa0[c], xa1[c]);
      xi0[c] = 3 * (flip ? w - 1 - xi0[c] : xi0[c]);
      xi1[c] = 3 * (flip ? w - 1 - xi1[c] : xi1[c]);
    }
  }
  const size_t plane = (size_t)H * W;

#pragma unroll 1
  for (int r = 0; r < TP_TH / 4; ++r) {
    const int y = y0 + 4 * wv + r;
    if (y >= H || xl >= W) break;
    float v[3][4];
    const bool yin = y < eh;
    int j0 = 0, j1 = 0;
    float b0 = 0.f, b1 = 0.f;
    if (inside && yin) tp_coef(y + oy, h, sy, j0, j1, b0, b1);
    const int base0 = u8_tile_row(tile, off, pitch, j0), base1 = u8_tile_row(tile, off, pitch, j1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int x = xl + c;
      if (inside && yin && x < ew) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int chn = cst.to_rgb ? 2 - q : q;
          const int p00 = tile.mem[base0 + xi0[c] + chn], p01 = tile.mem[base0 + xi1[c] + chn];
          const int p10 = tile.mem[base1 + xi0[c] + chn], p11 = tile.mem[base1 + xi1[c] + chn];
          const float o = tp_pixel(p00, p01, p10, p11, xa0[c], xa1[c], b0, b1);
          v[q][c] = (o - cst.mean[q]) * cst.rstd[q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q][c] = cst.pad[q];
      }
    }
    u8_store_planes(out + (size_t)b * 3 * plane + (size_t)y * W + xl, plane, v, xl, W);
  }
}

// The plane kernel's body, over the reader of an instance's source pixels: BITS false = the staged row-major bytes (non-zero = set),
// BITS true = the column-major bit plane the polygon fill kernel left in the workspace (plane z at word z * pw; pixel (r, c) of an
// h x w source is bit c * h + r). Rule 3 and the statistics are this one piece of code for both.
template <bool BITS>
__device__ __forceinline__ void tp_plane_body(int (*red)[5], const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                              const int32_t* __restrict__ itable, const uint32_t* __restrict__ bits, int pw,
                                              uint8_t* __restrict__ masks, uint8_t* __restrict__ seg, int32_t* __restrict__ stats,
                                              int N, int H, int W, int ch, int cw, int seg_pad) {
  const int z = blockIdx.z;
  const bool is_seg = !BITS && z >= N;                         // workgroup-uniform: planes N .. N + B - 1 are the semantic maps
  int b, moff = -1, mpitch = 0;
  if (is_seg) {
    b = z - N;
  } else {
    b = itable[TP_INST_COLS * z];
    moff = BITS ? 0 : itable[TP_INST_COLS * z + 1];            // a polygon instance row: image index, first part, parts
    mpitch = BITS ? 0 : itable[TP_INST_COLS * z + 2];
  }
  const uint32_t* ib = BITS ? bits + (size_t)z * pw : nullptr;
  const int32_t* d = table + TP_IMG_COLS * b;
  const int h = d[1], w = d[2], nh = d[4], nw = d[5], oy = d[6], ox = d[7], flip = d[8];
  if (is_seg) {
    moff = d[11];
    mpitch = w;
  }
  uint8_t* dst = is_seg ? seg + (size_t)b * H * W : masks + (size_t)z * H * W;
  const int fill = is_seg ? seg_pad : 0;
  const bool have = moff >= 0;                                 // a sample without a semantic map: the whole plane is seg_pad
  const int eh = have ? min(nh - oy, ch) : 0, ew = have ? min(nw - ox, cw) : 0;
  const int x0 = blockIdx.x * TP_TW, y0 = blockIdx.y * TP_TH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double sx = 1.0 / ((double)nw / (double)w), sy = 1.0 / ((double)nh / (double)h);

  const int xl = x0 + 4 * lane;
  int rx[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    rx[c] = 0;
    if (xl + c < ew) {
      const int i = tp_nearest(xl + c + ox, w, sx);
      rx[c] = flip ? w - 1 - i : i;
    }
  }
  const bool vec = (W & 3) == 0;
  int area = 0, ymin = INT32_MAX, ymax = -1;                   // wavefront-uniform: they are built from ballots
  unsigned long long cols[4] = {0, 0, 0, 0};

#pragma unroll 1
  for (int r = 0; r < TP_TH / 4; ++r) {
    const int y = y0 + 4 * wv + r;                             // wavefront-uniform
    if (y >= H) break;
    const bool yin = y < eh;
    const int rowbase = yin ? (BITS ? tp_nearest(y + oy, h, sy) : moff + tp_nearest(y + oy, h, sy) * mpitch) : 0;
    int v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = fill;
      if (yin && xl + c < ew) {
        if (BITS) {
          const uint32_t q = (uint32_t)rx[c] * (uint32_t)h + (uint32_t)rowbase;   // < h * w <= 2^31 - 32
          v[c] = (int)((ib[q >> 5] >> (q & 31)) & 1u);
        } else {
          const int p = src[rowbase + rx[c]];
          v[c] = is_seg ? p : (p != 0);
        }
      }
    }
    if (!is_seg) {
      unsigned long long row = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long m = __ballot(v[c] != 0);      // pixels outside the extent or the plane are 0 here
        area += __popcll(m);
        cols[c] |= m;
        row |= m;
      }
      if (row) {
        ymin = min(ymin, y);
        ymax = max(ymax, y);
      }
    }
    if (xl < W) {
      uint8_t* o = dst + (size_t)y * W + xl;
      if (vec) {                                               // W % 4 == 0 and xl % 4 == 0: a whole, aligned dword
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (xl + c < W) o[c] = (uint8_t)v[c];
      }
    }
  }

  if (!is_seg) {                                               // workgroup-uniform
    int xmin = INT32_MAX, xmax = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (cols[c]) {                                           // first / last lane with a set pixel in column c of its four
        xmin = min(xmin, x0 + 4 * (int)__builtin_ctzll(cols[c]) + c);
        xmax = max(xmax, x0 + 4 * (63 - (int)__builtin_clzll(cols[c])) + c);
      }
    if (lane == 0) {
      red[wv][0] = area;
      red[wv][1] = xmin;
      red[wv][2] = ymin;
      red[wv][3] = xmax;
      red[wv][4] = ymax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int a = 0, x_lo = INT32_MAX, y_lo = INT32_MAX, x_hi = -1, y_hi = -1;
      for (int k = 0; k < 4; ++k) {
        a += red[k][0];
        x_lo = min(x_lo, red[k][1]);
        y_lo = min(y_lo, red[k][2]);
        x_hi = max(x_hi, red[k][3]);
        y_hi = max(y_hi, red[k][4]);
      }
      if (a > 0) {
        int32_t* s = stats + (size_t)5 * z;
        atomicAdd(s, a);
        atomicMin(s + 1, x_lo);
        atomicMin(s + 2, y_lo);
        atomicMax(s + 3, x_hi);
        atomicMax(s + 4, y_hi);
      }
    }
  }
}

__global__ __launch_bounds__(256) void cgg_train_prep_plane_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                                                    const int32_t* __restrict__ itable, uint8_t* __restrict__ masks,
                                                                    uint8_t* __restrict__ seg, int32_t* __restrict__ stats, int N,
                                                                    int H, int W, int ch, int cw, int seg_pad) {
  __shared__ int red[4][5];
  tp_plane_body<false>(red, src, table, itable, nullptr, 0, masks, seg, stats, N, H, W, ch, cw, seg_pad);
}

// the same planes from the polygon fill kernel's bit planes (no semantic plane: polygon samples carry none)
__global__ __launch_bounds__(256) void cgg_train_prep_plane_bits_kernel(const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ itable,
                                                                         const uint32_t* __restrict__ bits, int pw,
                                                                         uint8_t* __restrict__ masks, int32_t* __restrict__ stats, int N,
                                                                         int H, int W, int ch, int cw) {
  __shared__ int red[4][5];
  tp_plane_body<true>(red, nullptr, table, itable, bits, pw, masks, nullptr, stats, N, H, W, ch, cw, 0);
}

// ---- panoptic samples: every plane from ONE gather of the id map -------------------------------------------------------------------
#define TP_PAN_COLS CGG_TRAIN_PREP_PAN_COLS
#define TP_SEG_COLS CGG_TRAIN_PREP_SEG_COLS
#define TP_MAX_SEG CGG_TRAIN_PREP_MAX_SEGMENTS

// the packed (slot, category) of `id` among the n rows sorted by id (lower bound, then equality); an id no row lists: no slot, 255
__device__ __forceinline__ int tp_find(const int32_t* ids, const int32_t* pks, int n, int id) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    if (ids[lo + half] < id) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  int r = 255;
  if (lo < n && ids[lo] == id) r = pks[lo];
  return r;
}

// Panoptic kernel: one 16 x 256 tile of ALL of one image's mask planes and of its semantic plane per workgroup (the tile geometry of
// the plane kernel: a lane owns 4 consecutive columns, a wavefront 4 rows). The image's segment rows sit in LDS (<= 256 rows, 2 KB);
// each pixel inside the extent gathers one id (rule 3), finds it by binary search and keeps (slot << 8) | category in a register --
// 16 per lane. The semantic byte is the low byte; plane `first + t` is slot == t + 1. Nearest gathers commute with "compare the id",
// so this is the plane kernel's output for the bitmaps pan == id. A bit set in LDS records which slots the tile holds: an absent
// slot's tile is zeros without any reduction; a present one reduces exactly as the plane kernel does (ballots, LDS across the four
// wavefronts -- two buffers in turn, so one barrier per slot -- then one atomic of each kind from one lane).
__global__ __launch_bounds__(256) void cgg_train_prep_panoptic_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                                                       const int32_t* __restrict__ ptable,
                                                                       const int32_t* __restrict__ stable, uint8_t* __restrict__ masks,
                                                                       uint8_t* __restrict__ seg, int32_t* __restrict__ stats, int H,
                                                                       int W, int ch, int cw, int seg_pad) {
  __shared__ int32_t s_id[TP_MAX_SEG], s_pk[TP_MAX_SEG];
  __shared__ uint32_t s_present[TP_MAX_SEG / 32 + 1];          // bit s: slot field s (1 .. 256) occurs in this tile
  __shared__ int red[2][4][5];
  const int b = blockIdx.z;
  const int32_t* d = table + TP_IMG_COLS * b;
  const int h = d[1], w = d[2], nh = d[4], nw = d[5], oy = d[6], ox = d[7], flip = d[8], first = d[9], things = d[10];
  const int32_t* pd = ptable + TP_PAN_COLS * b;
  const int moff = pd[0], mpitch = pd[1], rgb = pd[2], sfirst = pd[3], ns = pd[4];
  if ((int)threadIdx.x < ns) {                                 // ns <= 256: one row per thread
    s_id[threadIdx.x] = stable[TP_SEG_COLS * (sfirst + (int)threadIdx.x)];
    s_pk[threadIdx.x] = stable[TP_SEG_COLS * (sfirst + (int)threadIdx.x) + 1];
  }
  if (threadIdx.x < TP_MAX_SEG / 32 + 1) s_present[threadIdx.x] = 0;
  __syncthreads();

  const int eh = min(nh - oy, ch), ew = min(nw - ox, cw);
  const int x0 = blockIdx.x * TP_TW, y0 = blockIdx.y * TP_TH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double sx = 1.0 / ((double)nw / (double)w), sy = 1.0 / ((double)nh / (double)h);
  const int xl = x0 + 4 * lane;
  const int bpp = rgb ? 3 : 4;
  int rx[4];                                                   // byte offset of the source pixel inside its row
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    rx[c] = 0;
    if (xl + c < ew) {
      const int i = tp_nearest(xl + c + ox, w, sx);
      rx[c] = bpp * (flip ? w - 1 - i : i);
    }
  }

  // ---- one id per pixel -> (slot << 8) | category; outside the extent: no slot, seg_pad
  int pk[4][4];
  bool have_last = false;
  int last_id = 0, last_pk = 0, last_slot = 0;
#pragma unroll
  for (int r = 0; r < TP_TH / 4; ++r) {
    const int y = y0 + 4 * wv + r;
    const bool yin = y < eh;                                   // eh <= ch <= H
    const int rowbase = yin ? moff + tp_nearest(y + oy, h, sy) * mpitch : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int v = seg_pad;
      if (yin && xl + c < ew) {
        const int a = rowbase + rx[c];
        int id;
        if (rgb)
          id = (int)src[a] | ((int)src[a + 1] << 8) | ((int)src[a + 2] << 16);
        else
          id = *reinterpret_cast<const int32_t*>(src + a);    // moff, mpitch and the base are multiples of 4
        if (!have_last || id != last_id) {                     // neighbours mostly share their segment
          last_pk = tp_find(s_id, s_pk, ns, id);
          last_id = id;
          have_last = true;
        }
        v = last_pk;
        const int slot = v >> 8;
        if (slot != last_slot) {
          if (slot) atomicOr(&s_present[slot >> 5], 1u << (slot & 31));
          last_slot = slot;
        }
      }
      pk[r][c] = v;
    }
  }
  __syncthreads();

  const bool vec = (W & 3) == 0;
  const size_t plane = (size_t)H * W;
  if (seg != nullptr && xl < W) {
    uint8_t* dst = seg + (size_t)b * plane;
#pragma unroll
    for (int r = 0; r < TP_TH / 4; ++r) {
      const int y = y0 + 4 * wv + r;
      if (y < H) {
        uint8_t* o = dst + (size_t)y * W + xl;
        if (vec) {                                             // W % 4 == 0 and xl % 4 == 0: a whole, aligned dword
          *reinterpret_cast<uint32_t*>(o) = (uint32_t)(pk[r][0] & 255) | ((uint32_t)(pk[r][1] & 255) << 8) |
                                            ((uint32_t)(pk[r][2] & 255) << 16) | ((uint32_t)(pk[r][3] & 255) << 24);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (xl + c < W) o[c] = (uint8_t)(pk[r][c] & 255);
        }
      }
    }
  }

  int par = 0;
#pragma unroll 1
  for (int t = 1; t <= things; ++t) {                          // slot field t = plane first + t - 1
    uint8_t* dst = masks + (size_t)(first + t - 1) * plane;
    const bool present = (s_present[t >> 5] >> (t & 31)) & 1u; // workgroup-uniform
    int area = 0, ymin = INT32_MAX, ymax = -1;
    unsigned long long cols[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < TP_TH / 4; ++r) {
      const int y = y0 + 4 * wv + r;                           // wavefront-uniform
      if (y < H) {
        int v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (pk[r][c] >> 8) == t;   // all 0 where the slot is absent, and outside the extent
        if (present) {
          unsigned long long row = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const unsigned long long m = __ballot(v[c] != 0);
            area += __popcll(m);
            cols[c] |= m;
            row |= m;
          }
          if (row) {
            ymin = min(ymin, y);
            ymax = max(ymax, y);
          }
        }
        if (xl < W) {
          uint8_t* o = dst + (size_t)y * W + xl;
          if (vec) {
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (xl + c < W) o[c] = (uint8_t)v[c];
          }
        }
      }
    }
    if (present) {                                             // workgroup-uniform: the barrier is reached by all or none
      int xmin = INT32_MAX, xmax = -1;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (cols[c]) {
          xmin = min(xmin, x0 + 4 * (int)__builtin_ctzll(cols[c]) + c);
          xmax = max(xmax, x0 + 4 * (63 - (int)__builtin_clzll(cols[c])) + c);
        }
      if (lane == 0) {
        red[par][wv][0] = area;
        red[par][wv][1] = xmin;
        red[par][wv][2] = ymin;
        red[par][wv][3] = xmax;
        red[par][wv][4] = ymax;
      }
      __syncthreads();
      // the other buffer is written next: a wavefront reaches that write only after the NEXT barrier, which thread 0 reaches
      // after it has read this one
      if (threadIdx.x == 0) {
        int a = 0, x_lo = INT32_MAX, y_lo = INT32_MAX, x_hi = -1, y_hi = -1;
        for (int k = 0; k < 4; ++k) {
          a += red[par][k][0];
          x_lo = min(x_lo, red[par][k][1]);
          y_lo = min(y_lo, red[par][k][2]);
          x_hi = max(x_hi, red[par][k][3]);
          y_hi = max(y_hi, red[par][k][4]);
        }
        if (a > 0) {
          int32_t* s = stats + (size_t)5 * (first + t - 1);
          atomicAdd(s, a);
          atomicMin(s + 1, x_lo);
          atomicMin(s + 2, y_lo);
          atomicMax(s + 3, x_hi);
          atomicMax(s + 4, y_hi);
        }
      }
      par ^= 1;
    }
  }
}

// The images own consecutive ranges of the N instances, in order: image b's part of that rule. `next` carries the walk from row to
// row (0 before the first); after the last row the ranges must have tiled 0 .. N.
static int tp_instance_range(const char* me, int b, int B, int64_t first, int64_t n, int64_t* next, int N) {
  CGG_REQUIRE(n >= 0 && first == *next && first + n <= N, CGG_EINVAL,
              "%s: image %d: instances %lld .. %lld must follow the previous image's (%lld) and stay below N = %d", me, b,
              (long long)first, (long long)(first + n), (long long)*next, N);
  *next = first + n;
  CGG_REQUIRE(b < B - 1 || *next == N, CGG_EINVAL, "%s: the images own %lld instances, N = %d", me, (long long)*next, N);
  return CGG_OK;
}

// Everything both entry points check about the scalar arguments, the outputs and the image rows, before any launch. `panoptic`: there
// is no instance table (the things are found in the id map) and no staged semantic map (column 11 must be -1).
static int tp_validate(const char* me, bool panoptic, const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset,
                       int64_t inst_table_offset, const int32_t* img_table_host, const int32_t* inst_table_host, int B, int N,
                       const float* mean, const float* std_, const float* pad_val, int seg_pad, int crop_h, int crop_w, float* img,
                       uint8_t* masks, uint8_t* seg, int32_t* stats, int H, int W) {
  CGG_REQUIRE(staged && img_table_host && mean && std_ && pad_val && img, CGG_EINVAL, "%s: null pointer", me);
  CGG_REQUIRE(N >= 0 && (N == 0 || ((panoptic || inst_table_host) && masks && stats)), CGG_EINVAL,
              "%s: N = %d instances need %smasks and stats", me, N, panoptic ? "" : "inst_table_host, ");
  CGG_REQUIRE(B >= 1 && H >= 1 && W >= 1, CGG_EINVAL, "%s: B, H, W must be >= 1 (got %d, %d, %d)", me, B, H, W);
  CGG_REQUIRE(crop_h >= 1 && crop_w >= 1 && crop_h <= H && crop_w <= W, CGG_EINVAL,
              "%s: the crop window %d x %d must be >= 1 and fit the %d x %d plane", me, crop_h, crop_w, H, W);
  CGG_REQUIRE(seg_pad >= 0 && seg_pad <= 255, CGG_EINVAL, "%s: seg_pad must be a byte (got %d)", me, seg_pad);
  CGG_REQUIRE(B <= CGG_IMAGE_PREP_MAX_DIM && H <= CGG_IMAGE_PREP_MAX_DIM && W <= CGG_IMAGE_PREP_MAX_DIM &&
                  (int64_t)N + B <= CGG_IMAGE_PREP_MAX_DIM,
              CGG_EUNSUPPORTED, "%s: B + N, H, W must be <= %d (got %d + %d, %d, %d)", me, CGG_IMAGE_PREP_MAX_DIM, B, N, H, W);
  U8_TRY(u8_check_staged_bytes(me, staged_bytes));
  U8_TRY(u8_check_table(me, "image", img_table_offset, B, TP_IMG_COLS, staged_bytes));
  if (!panoptic) U8_TRY(u8_check_table(me, "instance", inst_table_offset, N, TP_INST_COLS, staged_bytes));
  CGG_REQUIRE((((uintptr_t)staged) & 3u) == 0 && (((uintptr_t)stats) & 3u) == 0, CGG_EALIGN, "%s: staged and stats must be 4-byte aligned",
              me);
  CGG_REQUIRE((W & 3) != 0 || (cgg_aligned16(img) && (((uintptr_t)masks) & 3u) == 0 && (((uintptr_t)seg) & 3u) == 0), CGG_EALIGN,
              "%s: when W %% 4 == 0, img must be 16-byte and masks / seg 4-byte aligned", me);
  U8_TRY(u8_check_norm3(me, mean, std_, pad_val));
  int64_t next = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* d = img_table_host + TP_IMG_COLS * b;
    const int64_t off = d[0], h = d[1], w = d[2], pitch = d[3], nh = d[4], nw = d[5], oy = d[6], ox = d[7], flip = d[8], first = d[9],
                  n = d[10], soff = d[11];
    U8_TRY(u8_check_sizes(me, b, h, w, nh, nw));
    CGG_REQUIRE(oy >= 0 && ox >= 0 && oy <= (nh > crop_h ? nh - crop_h : 0) && ox <= (nw > crop_w ? nw - crop_w : 0), CGG_EINVAL,
                "%s: image %d: the window at (%lld, %lld) lies outside the %lld x %lld resized image (crop %d x %d)", me, b,
                (long long)oy, (long long)ox, (long long)nh, (long long)nw, crop_h, crop_w);
    CGG_REQUIRE(flip == 0 || flip == 1, CGG_EINVAL, "%s: image %d: flip must be 0 or 1 (got %lld)", me, b, (long long)flip);
    U8_TRY(u8_check_bytes(me, b, off, h, w, pitch, staged_bytes));
    U8_TRY(tp_instance_range(me, b, B, first, n, &next, N));
    CGG_REQUIRE(!panoptic || soff == -1, CGG_EINVAL,
                "%s: image %d: the semantic-map offset must be -1 (got %lld): no semantic map is staged", me, b,
                (long long)soff);
    CGG_REQUIRE(!seg || soff == -1 || (soff >= 0 && soff + h * w <= staged_bytes), CGG_EINVAL,
                "%s: image %d: the semantic map at byte %lld extends past the %lld staged bytes", me, b, (long long)soff,
                (long long)staged_bytes);
    for (int64_t i = first; i < (panoptic ? first : first + n); ++i) {
      const int32_t* t = inst_table_host + TP_INST_COLS * i;
      const int64_t ib = t[0], ioff = t[1], ipitch = t[2];
      CGG_REQUIRE(ib >= 0 && ib < B, CGG_EINVAL, "%s: instance %lld: image index %lld out of range (B = %d)", me, (long long)i,
                  (long long)ib, B);
      CGG_REQUIRE(ib == b, CGG_EINVAL, "%s: instance %lld belongs to image %lld but lies in image %d's range", me, (long long)i,
                  (long long)ib, b);
      CGG_REQUIRE(ipitch >= w, CGG_EINVAL, "%s: instance %lld: row pitch %lld < w = %lld", me, (long long)i, (long long)ipitch,
                  (long long)w);
      CGG_REQUIRE(ioff >= 0 && ioff + h * ipitch <= staged_bytes, CGG_EINVAL,
                  "%s: instance %lld (bytes %lld .. %lld) extends past the %lld staged bytes", me, (long long)i, (long long)ioff,
                  (long long)(ioff + h * ipitch), (long long)staged_bytes);
    }
  }
  return CGG_OK;
}

// the first launch of both entry points: the image planes, and the statistics rows initialised
static int tp_launch_image(const char* me, const uint8_t* staged, const int32_t* table, int B, const float* mean, const float* std_,
                           const float* pad_val, int to_rgb, int crop_h, int crop_w, float* img, int32_t* stats, int H, int W,
                           cgg_stream_t stream) {
  const PrepConst cst = u8_prep_const(mean, std_, pad_val, to_rgb, 1);   // Pad runs ahead of Normalize
  const unsigned gx = (unsigned)((W + TP_TW - 1) / TP_TW), gy = (unsigned)((H + TP_TH - 1) / TP_TH);
  hipLaunchKernelGGL(cgg_train_prep_image_kernel, dim3(gx, gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream, staged, table, cst, img,
                     stats, H, W, crop_h, crop_w);
  CGG_CHECK_LAUNCH(me);
  return CGG_OK;
}

extern "C" int cgg_train_prep_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                                 const int32_t* img_table_host, const int32_t* inst_table_host, int B, int N, const float* mean,
                                 const float* std_, const float* pad_val, int to_rgb, int seg_pad, int crop_h, int crop_w, float* img,
                                 uint8_t* masks, uint8_t* seg, int32_t* stats, int H, int W, cgg_stream_t stream) {
  const char* me = "cgg_train_prep_u8";
  int rc = tp_validate(me, false, staged, staged_bytes, img_table_offset, inst_table_offset, img_table_host, inst_table_host, B, N, mean,
                       std_, pad_val, seg_pad, crop_h, crop_w, img, masks, seg, stats, H, W);
  if (rc != CGG_OK) return rc;
  const int32_t* table = reinterpret_cast<const int32_t*>(staged + img_table_offset);
  rc = tp_launch_image(me, staged, table, B, mean, std_, pad_val, to_rgb, crop_h, crop_w, img, stats, H, W, stream);
  if (rc != CGG_OK) return rc;
  const unsigned gx = (unsigned)((W + TP_TW - 1) / TP_TW), gy = (unsigned)((H + TP_TH - 1) / TP_TH);
  const int planes = N + (seg ? B : 0);
  if (planes > 0) {
    hipLaunchKernelGGL(cgg_train_prep_plane_kernel, dim3(gx, gy, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, staged, table,
                       reinterpret_cast<const int32_t*>(staged + inst_table_offset), masks, seg, stats, N, H, W, crop_h, crop_w, seg_pad);
    CGG_CHECK_LAUNCH(me);
  }
  return CGG_OK;
}

extern "C" int cgg_train_prep_panoptic_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset,
                                          int64_t pan_table_offset, int64_t seg_table_offset, const int32_t* img_table_host,
                                          const int32_t* pan_table_host, const int32_t* seg_table_host, int B, int N, int S,
                                          const float* mean, const float* std_, const float* pad_val, int to_rgb, int seg_pad,
                                          int crop_h, int crop_w, float* img, uint8_t* masks, uint8_t* seg, int32_t* stats, int H, int W,
                                          cgg_stream_t stream) {
  const char* me = "cgg_train_prep_panoptic_u8";
  CGG_REQUIRE(pan_table_host && S >= 0 && (S == 0 || seg_table_host), CGG_EINVAL,
              "%s: null pointer (pan_table_host, or seg_table_host with S = %d segment rows)", me, S);
  int rc = tp_validate(me, true, staged, staged_bytes, img_table_offset, 0, img_table_host, nullptr, B, N, mean, std_, pad_val, seg_pad,
                       crop_h, crop_w, img, masks, seg, stats, H, W);
  if (rc != CGG_OK) return rc;
  U8_TRY(u8_check_table(me, "panoptic", pan_table_offset, B, TP_PAN_COLS, staged_bytes));
  U8_TRY(u8_check_table(me, "segment", seg_table_offset, S, TP_SEG_COLS, staged_bytes));
  int64_t next = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* d = img_table_host + TP_IMG_COLS * b;
    const int32_t* p = pan_table_host + TP_PAN_COLS * b;
    const int64_t h = d[1], w = d[2], things = d[10], off = p[0], pitch = p[1], fmt = p[2], first = p[3], n = p[4];
    CGG_REQUIRE(fmt == 0 || fmt == 1, CGG_EINVAL, "%s: image %d: id-map format must be 0 (int32) or 1 (RGB bytes) (got %lld)", me, b,
                (long long)fmt);
    CGG_REQUIRE(pitch >= (fmt ? 3 : 4) * w, CGG_EINVAL, "%s: image %d: id-map row pitch %lld < %d * w = %lld", me, b, (long long)pitch,
                fmt ? 3 : 4, (long long)((fmt ? 3 : 4) * w));
    CGG_REQUIRE(fmt == 1 || ((off & 3) == 0 && (pitch & 3) == 0), CGG_EINVAL,
                "%s: image %d: an int32 id map needs a byte offset (%lld) and a row pitch (%lld) that are multiples of 4", me, b,
                (long long)off, (long long)pitch);
    CGG_REQUIRE(off >= 0 && off + h * pitch <= staged_bytes, CGG_EINVAL,
                "%s: image %d: the id map (bytes %lld .. %lld) extends past the %lld staged bytes", me, b, (long long)off,
                (long long)(off + h * pitch), (long long)staged_bytes);
    CGG_REQUIRE(n >= 0 && first == next && first + n <= S, CGG_EINVAL,
                "%s: image %d: segment rows %lld .. %lld must follow the previous image's (%lld) and stay below S = %d", me, b,
                (long long)first, (long long)(first + n), (long long)next, S);
    CGG_REQUIRE(n <= TP_MAX_SEG, CGG_EUNSUPPORTED, "%s: image %d has %lld segment rows, more than %d", me, b, (long long)n, TP_MAX_SEG);
    bool seen[TP_MAX_SEG + 1] = {false};
    int64_t slots = 0;
    for (int64_t i = first; i < first + n; ++i) {
      const int32_t* t = seg_table_host + TP_SEG_COLS * i;
      const int64_t id = t[0], slot = (int64_t)t[1] >> 8, cat = t[1] & 255;
      CGG_REQUIRE(i == first || id > t[-TP_SEG_COLS], CGG_EINVAL,
                  "%s: image %d: segment row %lld: ids must ascend strictly (%lld after %lld)", me, b, (long long)i, (long long)id,
                  (long long)(i == first ? 0 : t[-TP_SEG_COLS]));
      CGG_REQUIRE(cat <= 254, CGG_EINVAL, "%s: image %d: segment row %lld: category %lld > 254", me, b, (long long)i, (long long)cat);
      CGG_REQUIRE(slot >= 0 && slot <= things && slot <= TP_MAX_SEG && (slot == 0 || !seen[slot]), CGG_EINVAL,
                  "%s: image %d: segment row %lld: slot %lld -- the non-zero slots must be a permutation of 1 .. %lld", me, b,
                  (long long)i, (long long)slot, (long long)things);
      if (slot) {
        seen[slot] = true;
        ++slots;
      }
    }
    CGG_REQUIRE(slots == things, CGG_EINVAL, "%s: image %d: %lld thing slots in the segment rows, %lld instances in the image row", me,
                b, (long long)slots, (long long)things);
    next = first + n;
  }
  CGG_REQUIRE(next == S, CGG_EINVAL, "%s: the images own %lld segment rows, S = %d", me, (long long)next, S);
  const int32_t* table = reinterpret_cast<const int32_t*>(staged + img_table_offset);
  rc = tp_launch_image(me, staged, table, B, mean, std_, pad_val, to_rgb, crop_h, crop_w, img, stats, H, W, stream);
  if (rc != CGG_OK) return rc;
  if (N > 0 || seg) {
    const unsigned gx = (unsigned)((W + TP_TW - 1) / TP_TW), gy = (unsigned)((H + TP_TH - 1) / TP_TH);
    hipLaunchKernelGGL(cgg_train_prep_panoptic_kernel, dim3(gx, gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream, staged, table,
                       reinterpret_cast<const int32_t*>(staged + pan_table_offset),
                       reinterpret_cast<const int32_t*>(staged + seg_table_offset), masks, seg, stats, H, W, crop_h, crop_w, seg_pad);
    CGG_CHECK_LAUNCH(me);
  }
  return CGG_OK;
}

// ---- polygon samples: the masks rasterised on the device (rule 6 of train_prep.py) ------------------------------------------------
#define TP_POLY_INST_COLS CGG_TRAIN_PREP_POLY_INST_COLS
#define TP_POLY_PART_COLS CGG_TRAIN_PREP_POLY_PART_COLS
#define PF_LDS_WORDS (CGG_POLY_LDS_BITS / 32)
#define PF_SCAN_WORDS (CGG_POLY_SCAN_BITS / 32)
static_assert(PF_SCAN_WORDS == 256, "one word per thread of the fill kernel's workgroup");

// one edge of a part as rleFrPoly walks it: the start after the optional swap, the number of steps m = max(dx, dy), the slope
struct PfEdge {
  int xs, ys, m, flip, steep;
  double s;
};

__device__ __forceinline__ int pf_vertex(double c) { return (int)(5.0 * c + 0.5); }   // product and sum rounded on their own

__device__ __forceinline__ PfEdge pf_edge(const double* __restrict__ xy, int k, int j) {
  const int j1 = j + 1 == k ? 0 : j + 1;
  int xs = pf_vertex(xy[2 * j]), ys = pf_vertex(xy[2 * j + 1]), xe = pf_vertex(xy[2 * j1]), ye = pf_vertex(xy[2 * j1 + 1]);
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  PfEdge e;
  e.steep = dx < dy;
  e.flip = e.steep ? ys > ye : xs > xe;
  if (e.flip) {
    int t = xs;
    xs = xe;
    xe = t;
    t = ys;
    ys = ye;
    ye = t;
  }
  e.xs = xs;
  e.ys = ys;
  e.m = max(dx, dy);
  e.s = e.m == 0 ? 0.0 : (e.steep ? (double)(xe - xs) / (double)dy : (double)(ye - ys) / (double)dx);
  return e;
}

// point d (0 .. m) of an edge; an edge of one point (dx == dy == 0) is its vertex
__device__ __forceinline__ void pf_point(const PfEdge& e, int d, int& u, int& v) {
  const int t = e.flip ? e.m - d : d;
  if (e.m == 0) {
    u = e.xs;
    v = e.ys;
  } else if (!e.steep) {
    u = t + e.xs;
    v = (int)(((double)e.ys + e.s * (double)t) + 0.5);
  } else {
    v = t + e.ys;
    u = (int)(((double)e.xs + e.s * (double)t) + 0.5);
  }
}

// Fill kernel: one workgroup of 4 wavefronts per instance, the instance's parts in turn. Per part: (1) crossings -- wavefront wv
// takes edges wv, wv + 4, ..., its lanes stride over the edge's points d; a point and its predecessor (d - 1, or the previous edge's
// last point) are closed-form, and a change of column toggles bit a = xd * h + yd of the toggle plane (atomic XOR: LDS, or the
// workspace for a plane of more than CGG_POLY_LDS_BITS pixels); (2) fill -- pixel p is set iff the number of crossings <= p is odd:
// blocks of 256 words, one per thread; an inclusive prefix XOR inside the word by shift-XOR, the parity of the words before it in
// the wavefront from one ballot, the wavefronts before it and the blocks before it through LDS; a set carry inverts the word. The
// part's plane is OR-ed into the instance's (the first part stores: nothing is read that this workgroup did not write). Reading a
// toggle word clears it for the next part. Every word of the bit plane is written, an instance without parts as zeros.
__global__ __launch_bounds__(256) void cgg_poly_fill_kernel(const uint8_t* __restrict__ staged, const int32_t* __restrict__ table,
                                                             const int32_t* __restrict__ itable, const int32_t* __restrict__ ptable,
                                                             uint32_t* __restrict__ ws, int pw, int N, int force_ws) {
  __shared__ uint32_t s_tog[PF_LDS_WORDS];
  __shared__ int s_par[2][4];
  const int z = blockIdx.x;
  const int b = itable[TP_POLY_INST_COLS * z], p0 = itable[TP_POLY_INST_COLS * z + 1], parts = itable[TP_POLY_INST_COLS * z + 2];
  const int h = table[TP_IMG_COLS * b + 1], w = table[TP_IMG_COLS * b + 2];
  const int hw = h * w, nwords = (hw + 31) >> 5;               // hw <= 2^31 - 32, nwords <= pw
  const bool glob = force_ws || hw > CGG_POLY_LDS_BITS;        // workgroup-uniform
  uint32_t* out = ws + (size_t)z * pw;
  uint32_t* gt = ws + ((size_t)N + z) * pw;                    // this instance's toggle plane on the workspace route
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  for (int i = tid; i < nwords; i += 256) {
    if (glob)
      atomicExch(gt + i, 0u);
    else
      s_tog[i] = 0u;
    if (parts == 0) out[i] = 0u;
  }
  __threadfence();
  __syncthreads();

#pragma unroll 1
  for (int part = 0; part < parts; ++part) {
    const int32_t* row = ptable + TP_POLY_PART_COLS * (p0 + part);
    const double* xy = reinterpret_cast<const double*>(staged + row[0]);
    const int k = row[1];
    // ---- (1) crossings
#pragma unroll 1
    for (int j = wv; j < k; j += 4) {
      const PfEdge e = pf_edge(xy, k, j);
#pragma unroll 1
      for (int d = lane; d <= e.m; d += 64) {
        if (j == 0 && d == 0) continue;                        // the sequence's first point has no predecessor
        int u0, v0, u1, v1;
        pf_point(e, d, u1, v1);
        if (d > 0) {
          pf_point(e, d - 1, u0, v0);
        } else {
          const PfEdge q = pf_edge(xy, k, j - 1);
          pf_point(q, q.m, u0, v0);
        }
        if (u1 == u0) continue;
        const double xd = ((double)(u1 < u0 ? u1 : u1 - 1) + 0.5) / 5.0 - 0.5;
        if (floor(xd) != xd || xd < 0.0 || xd > (double)(w - 1)) continue;
        double yd = ((double)min(v0, v1) + 0.5) / 5.0 - 0.5;
        yd = yd < 0.0 ? 0.0 : (yd > (double)h ? (double)h : yd);
        const int a = (int)xd * h + (int)ceil(yd);             // <= h * w; a == h * w lies past the last pixel
        if (a < hw) {
          if (glob)
            atomicXor(gt + (a >> 5), 1u << (a & 31));
          else
            atomicXor(&s_tog[a >> 5], 1u << (a & 31));
        }
      }
    }
    __threadfence();
    __syncthreads();
    // ---- (2) fill
    int carry = 0, par = 0;                                    // workgroup-uniform
#pragma unroll 1
    for (int base = 0; base < nwords; base += PF_SCAN_WORDS) {
      const int i = base + tid;
      uint32_t x = 0u;
      if (i < nwords) {
        if (glob) {
          x = atomicExch(gt + i, 0u);
        } else {
          x = s_tog[i];
          s_tog[i] = 0u;
        }
      }
      x ^= x << 1;
      x ^= x << 2;
      x ^= x << 4;
      x ^= x << 8;
      x ^= x << 16;
      const unsigned long long m = __ballot((x >> 31) != 0u);  // bit 31 of the inclusive scan = the word's parity
      if (lane == 0) s_par[par][wv] = __popcll(m) & 1;
      __syncthreads();
      // s_par[par] is written again two blocks on: a wavefront gets there only after the next barrier, which every wavefront
      // reaches after it has read this one
      int before = (__popcll(m & ((1ull << lane) - 1ull)) & 1) ^ carry;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = s_par[par][q];
        if (q < wv) before ^= t;
        carry ^= t;
      }
      if (before) x = ~x;
      if (i < nwords) {
        if (i == nwords - 1 && (hw & 31)) x &= (1u << (hw & 31)) - 1u;
        out[i] = part ? (out[i] | x) : x;                      // word i is this thread's in every part
      }
      par ^= 1;
    }
    __threadfence();
    __syncthreads();
  }
}

// h, w, first instance, instances of the image rows, as the polygon entry points need them: sizes, and ranges that tile 0 .. N
// (ranges_checked: tp_validate has walked them already)
static int pf_validate_images(const char* me, const int32_t* img_table_host, int B, int N, int force_ws, bool ranges_checked,
                              int64_t* pw, int* any_ws) {
  CGG_REQUIRE(img_table_host, CGG_EINVAL, "%s: null pointer (img_table_host)", me);
  CGG_REQUIRE(B >= 1 && N >= 0, CGG_EINVAL, "%s: B must be >= 1 and N >= 0 (got %d, %d)", me, B, N);
  CGG_REQUIRE(B <= CGG_IMAGE_PREP_MAX_DIM && (int64_t)N + B <= CGG_IMAGE_PREP_MAX_DIM, CGG_EUNSUPPORTED,
              "%s: B + N must be <= %d (got %d + %d)", me, CGG_IMAGE_PREP_MAX_DIM, B, N);
  int64_t next = 0, words = 0;
  int ws = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* d = img_table_host + TP_IMG_COLS * b;
    const int64_t h = d[1], w = d[2], first = d[9], n = d[10];
    CGG_REQUIRE(h >= 1 && w >= 1, CGG_EINVAL, "%s: image %d is zero-sized (%lld x %lld)", me, b, (long long)h, (long long)w);
    CGG_REQUIRE(h <= CGG_IMAGE_PREP_MAX_DIM && w <= CGG_IMAGE_PREP_MAX_DIM && h * w <= (int64_t)INT32_MAX - 31, CGG_EUNSUPPORTED,
                "%s: image %d is %lld x %lld: larger than %d on a side, or more than 2^31 - 32 pixels", me, b, (long long)h,
                (long long)w, CGG_IMAGE_PREP_MAX_DIM);
    if (!ranges_checked) U8_TRY(tp_instance_range(me, b, B, first, n, &next, N));
    if (n > 0) {
      words = words > (h * w + 31) / 32 ? words : (h * w + 31) / 32;
      if (h * w > CGG_POLY_LDS_BITS) ws = 1;
    }
  }
  *pw = words;
  *any_ws = (ws || force_ws) && N > 0;
  return CGG_OK;
}

extern "C" int64_t cgg_train_prep_polygons_workspace_bytes(const int32_t* img_table_host, int B, int N, int force_workspace) {
  int64_t pw = 0;
  int any_ws = 0;
  const int rc = pf_validate_images("cgg_train_prep_polygons_workspace_bytes", img_table_host, B, N, force_workspace, false, &pw, &any_ws);
  if (rc != CGG_OK) return rc;
  return (int64_t)N * pw * 4 * (any_ws ? 2 : 1);
}

// everything the fill kernel relies on, checked on the host: the tables, the coordinates, the workspace
static int pf_validate(const char* me, const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                       int64_t part_table_offset, const int32_t* img_table_host, const int32_t* inst_table_host,
                       const int32_t* part_table_host, const uint8_t* staged_host, int B, int N, int P, const uint32_t* workspace,
                       int64_t workspace_bytes, int force_ws, bool ranges_checked, int64_t* pw_out) {
  CGG_REQUIRE(staged && img_table_host && P >= 0 && (N <= 0 || (inst_table_host && workspace)) &&
                  (P == 0 || (part_table_host && staged_host)),
              CGG_EINVAL, "%s: null pointer (staged, img_table_host; inst_table_host, workspace with N = %d; part_table_host, "
              "staged_host with P = %d)", me, N, P);
  U8_TRY(u8_check_staged_bytes(me, staged_bytes));
  int64_t pw = 0;
  int any_ws = 0;
  U8_TRY(pf_validate_images(me, img_table_host, B, N, force_ws, ranges_checked, &pw, &any_ws));
  U8_TRY(u8_check_table(me, "image", img_table_offset, B, TP_IMG_COLS, staged_bytes));
  U8_TRY(u8_check_table(me, "instance", inst_table_offset, N, TP_POLY_INST_COLS, staged_bytes));
  U8_TRY(u8_check_table(me, "part", part_table_offset, P, TP_POLY_PART_COLS, staged_bytes));
  CGG_REQUIRE((((uintptr_t)staged) & 7u) == 0 && (((uintptr_t)workspace) & 3u) == 0, CGG_EALIGN,
              "%s: staged must be 8-byte and workspace 4-byte aligned", me);
  int64_t next = 0;
  for (int b = 0; b < B; ++b) {                                // every instance inside its image's range names that image
    const int32_t* d = img_table_host + TP_IMG_COLS * b;
    for (int64_t i = d[9]; i < (int64_t)d[9] + d[10]; ++i) {
      const int32_t* t = inst_table_host + TP_POLY_INST_COLS * i;
      const int64_t ib = t[0], first = t[1], n = t[2];
      CGG_REQUIRE(ib == b, CGG_EINVAL, "%s: instance %lld belongs to image %lld but lies in image %d's range", me, (long long)i,
                  (long long)ib, b);
      CGG_REQUIRE(n >= 0 && first == next && first + n <= P, CGG_EINVAL,
                  "%s: instance %lld: parts %lld .. %lld must follow the previous instance's (%lld) and stay below P = %d", me,
                  (long long)i, (long long)first, (long long)(first + n), (long long)next, P);
      next = first + n;
    }
  }
  CGG_REQUIRE(next == P, CGG_EINVAL, "%s: the instances own %lld parts, P = %d", me, (long long)next, P);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t off = part_table_host[TP_POLY_PART_COLS * p], k = part_table_host[TP_POLY_PART_COLS * p + 1];
    CGG_REQUIRE(k >= 1, CGG_EINVAL, "%s: part %lld has %lld vertices (one or more expected)", me, (long long)p, (long long)k);
    CGG_REQUIRE(off >= 0 && (off & 7) == 0, CGG_EINVAL, "%s: part %lld: byte offset %lld must be a non-negative multiple of 8", me,
                (long long)p, (long long)off);
    CGG_REQUIRE(off + 16 * k <= staged_bytes, CGG_EINVAL, "%s: part %lld (bytes %lld .. %lld) extends past the %lld staged bytes", me,
                (long long)p, (long long)off, (long long)(off + 16 * k), (long long)staged_bytes);
    for (int64_t c = 0; c < 2 * k; ++c) {
      double v;
      __builtin_memcpy(&v, staged_host + off + 8 * c, 8);
      CGG_REQUIRE(v - v == 0.0, CGG_EINVAL, "%s: part %lld: coordinate %lld is not finite", me, (long long)p, (long long)c);
      CGG_REQUIRE(fabs(v) <= (double)CGG_IMAGE_PREP_MAX_DIM, CGG_EUNSUPPORTED,
                  "%s: part %lld: coordinate %lld is %g, beyond +-%d (the bound of the edge walk)", me, (long long)p, (long long)c, v,
                  CGG_IMAGE_PREP_MAX_DIM);
    }
  }
  const int64_t need = (int64_t)N * pw * 4 * (any_ws ? 2 : 1);
  CGG_REQUIRE(workspace_bytes >= need, CGG_EUNSUPPORTED, "%s: the workspace holds %lld bytes, %lld are needed", me,
              (long long)workspace_bytes, (long long)need);
  *pw_out = pw;
  return CGG_OK;
}

static int pf_launch(const char* me, const uint8_t* staged, int64_t img_table_offset, int64_t inst_table_offset, int64_t part_table_offset,
                     int N, uint32_t* workspace, int pw, int force_ws, cgg_stream_t stream) {
  if (N > 0) {
    hipLaunchKernelGGL(cgg_poly_fill_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, staged,
                       reinterpret_cast<const int32_t*>(staged + img_table_offset),
                       reinterpret_cast<const int32_t*>(staged + inst_table_offset),
                       reinterpret_cast<const int32_t*>(staged + part_table_offset), workspace, pw, N, force_ws ? 1 : 0);
    CGG_CHECK_LAUNCH(me);
  }
  return CGG_OK;
}

extern "C" int cgg_polygon_fill_bits(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                                     int64_t part_table_offset, const int32_t* img_table_host, const int32_t* inst_table_host,
                                     const int32_t* part_table_host, const uint8_t* staged_host, int B, int N, int P,
                                     uint32_t* workspace, int64_t workspace_bytes, int force_workspace, cgg_stream_t stream) {
  const char* me = "cgg_polygon_fill_bits";
  int64_t pw = 0;
  const int rc = pf_validate(me, staged, staged_bytes, img_table_offset, inst_table_offset, part_table_offset, img_table_host,
                             inst_table_host, part_table_host, staged_host, B, N, P, workspace, workspace_bytes, force_workspace, false,
                             &pw);
  if (rc != CGG_OK) return rc;
  return pf_launch(me, staged, img_table_offset, inst_table_offset, part_table_offset, N, workspace, (int)pw, force_workspace, stream);
}

extern "C" int cgg_train_prep_polygons_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset,
                                          int64_t inst_table_offset, int64_t part_table_offset, const int32_t* img_table_host,
                                          const int32_t* inst_table_host, const int32_t* part_table_host, const uint8_t* staged_host,
                                          int B, int N, int P, const float* mean, const float* std_, const float* pad_val, int to_rgb,
                                          int crop_h, int crop_w, float* img, uint8_t* masks, int32_t* stats, int H, int W,
                                          uint32_t* workspace, int64_t workspace_bytes, int force_workspace, cgg_stream_t stream) {
  const char* me = "cgg_train_prep_polygons_u8";
  int rc = tp_validate(me, true, staged, staged_bytes, img_table_offset, 0, img_table_host, nullptr, B, N, mean, std_, pad_val, 0, crop_h,
                       crop_w, img, masks, nullptr, stats, H, W);
  if (rc != CGG_OK) return rc;
  int64_t pw = 0;
  rc = pf_validate(me, staged, staged_bytes, img_table_offset, inst_table_offset, part_table_offset, img_table_host, inst_table_host,
                   part_table_host, staged_host, B, N, P, workspace, workspace_bytes, force_workspace, true, &pw);
  if (rc != CGG_OK) return rc;
  const int32_t* table = reinterpret_cast<const int32_t*>(staged + img_table_offset);
  rc = tp_launch_image(me, staged, table, B, mean, std_, pad_val, to_rgb, crop_h, crop_w, img, stats, H, W, stream);
  if (rc != CGG_OK) return rc;
  rc = pf_launch(me, staged, img_table_offset, inst_table_offset, part_table_offset, N, workspace, (int)pw, force_workspace, stream);
  if (rc != CGG_OK) return rc;
  if (N > 0) {
    const unsigned gx = (unsigned)((W + TP_TW - 1) / TP_TW), gy = (unsigned)((H + TP_TH - 1) / TP_TH);
    hipLaunchKernelGGL(cgg_train_prep_plane_bits_kernel, dim3(gx, gy, (unsigned)N), dim3(256), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int32_t*>(staged + inst_table_offset), workspace, (int)pw, masks, stats, N, H, W, crop_h,
                       crop_w);
    CGG_CHECK_LAUNCH(me);
  }
  return CGG_OK;
}
