// What the two uint8 image resizers share (cgg_image_prep_u8_kernel in image_prep.hip, cgg_train_prep_image_kernel in
// train_prep.hip): the tap rule, a tile's source bytes staged into LDS, the address of a tap, the three-plane store and the
// mean / 1 / std / pad constant. Each kernel keeps its own weights (11-bit integers or floats) and its own pixel formula. At the
// end, for the host: the checks of the staged-batch contract that the entry points of both files run before any launch.
//
// The rounding of (k + 0.5) * scale - 0.5 decides which source pixel a tap lands on, and the compiler would fuse exactly that
// pattern, so this header turns contraction off. The pragma is at file scope and therefore LEAKS into the rest of the including
// file. That is intended: both includers are built without contraction anyway (their build-flags line and their own pragma).
#pragma once
#include "cgg_common.h"

#pragma clang fp contract(off)

#define U8_LDS_BYTES 32768 /* the LDS image of a tile's source bytes; the kernel declares `__shared__ uint32_t lds[U8_LDS_BYTES / 4]` */

struct PrepConst {
  float mean[3], rstd[3], pad[3];   // per output plane; pad = the value of the padded region
  int to_rgb;
};

// pad_before_norm: Pad runs ahead of Normalize, so pad_val is in source channel order and is normalised like a pixel
static inline PrepConst u8_prep_const(const float* mean, const float* std_, const float* pad_val, int to_rgb, int pad_before_norm) {
  PrepConst cst;
  for (int q = 0; q < 3; ++q) {
    cst.mean[q] = mean[q];
    cst.rstd[q] = (float)(1.0 / (double)std_[q]);
    const float p = pad_val[(pad_before_norm && to_rgb) ? 2 - q : q];
    cst.pad[q] = pad_before_norm ? (p - cst.mean[q]) * cst.rstd[q] : p;
  }
  cst.to_rgb = to_rgb ? 1 : 0;
  return cst;
}

// The tap rule for one resized index k of an axis with source length s, scale = 1 / (d / s) in double:
// fx = float((k + 0.5) * scale - 0.5), two separately rounded double operations; i = floor(fx), fx -= i, clamped at both ends.
struct U8Tap {
  int i0, i1;   // the two source indices
  float fx;     // the fraction towards i1
};
__device__ __forceinline__ U8Tap u8_tap(int k, int s, double scale) {
  const double t = ((double)k + 0.5) * scale;
  float fx = (float)(t - 0.5);
  const float fl = floorf(fx);
  int i = (int)fl;
  fx -= fl;
  if (i < 0) {
    i = 0;
    fx = 0.f;
  }
  if (i >= s - 1) {
    i = s - 1;
    fx = 0.f;
  }
  U8Tap r;
  r.i0 = i;
  r.i1 = min(i + 1, s - 1);
  r.fx = fx;
  return r;
}

// A tile's source bytes: rows r0 .. of the image, bytes cb0 .. of each, in LDS when they fit U8_LDS_BYTES (workgroup-uniform).
struct U8Tile {
  int r0, cb0, ls;      // ls = row stride in LDS
  bool use_lds;
  const uint8_t* mem;   // the LDS image or src: one generic pointer, so a tap is one flat load whichever side holds it
};

// The span of the tile whose resized rows are ky0 .. ky1 and resized columns kx0 .. kx1 (inclusive) of an h x w HWC image at byte
// `off` of src, and its LDS image. A 3-byte pixel, a pitch that is no multiple of 4 and an arbitrary image offset make every row
// start at its own byte phase: rows are staged with aligned dword loads and the phase is added back by u8_tile_row. A dword that is
// not wholly inside the image's bytes is assembled from guarded byte loads: nothing outside off .. off + h * pitch is read.
// flip: source column c is read at w - 1 - c. inside = false: the tile holds no resized pixel and nothing is staged. All 256 threads
// call this; the caller's barrier follows when use_lds.
__device__ __forceinline__ U8Tile u8_tile_stage(uint32_t* __restrict__ lds, const uint8_t* __restrict__ src, bool inside, int off, int h,
                                                int w, int pitch, int ky0, int ky1, int kx0, int kx1, double sy, double sx, bool flip) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  U8Tile t = {0, 0, 0, false, src};
  if (!inside) return t;
  t.r0 = u8_tap(ky0, h, sy).i0;
  const int r1 = u8_tap(ky1, h, sy).i1;
  int lo_c = u8_tap(kx0, w, sx).i0, hi_c = u8_tap(kx1, w, sx).i1;
  if (flip) {                                       // columns lo_c .. hi_c of the mirrored image
    const int m = w - 1 - hi_c;
    hi_c = w - 1 - lo_c;
    lo_c = m;
  }
  t.cb0 = 3 * lo_c;
  const int nrows = r1 - t.r0 + 1, nbytes = 3 * (hi_c + 1) - t.cb0;
  t.ls = (nbytes + 6) & ~3;                         // the bytes, up to 3 of phase, rounded up to dwords
  t.use_lds = (long long)nrows * t.ls <= U8_LDS_BYTES;
  if (t.use_lds) {
    const int lo = off, hi = off + h * pitch;       // the image's bytes
    for (int rr = wv; rr < nrows; rr += 4) {
      const int a = off + (t.r0 + rr) * pitch + t.cb0, phase = a & 3, a4 = a - phase;
      const int ndw = (phase + nbytes + 3) >> 2;    // <= ls / 4
      for (int j = lane; j < ndw; j += 64) {
        const int g = a4 + 4 * j;
        uint32_t v;
        if (g >= lo && g <= hi - 4) {
          v = *reinterpret_cast<const uint32_t*>(src + g);
        } else {
          v = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (g + q >= lo && g + q < hi) v |= (uint32_t)src[g + q] << (8 * q);
        }
        lds[(rr * t.ls >> 2) + j] = v;
      }
    }
    t.mem = reinterpret_cast<const uint8_t*>(lds);
  }
  return t;
}

// index into t.mem of column-byte 0 of source row j, in LDS (phase included, relative to cb0) or in global memory:
// the byte of (column, channel) is t.mem[u8_tile_row(..) + 3 * column + channel]
__device__ __forceinline__ int u8_tile_row(const U8Tile& t, int off, int pitch, int j) {
  return t.use_lds ? (j - t.r0) * t.ls + ((off + j * pitch + t.cb0) & 3) - t.cb0 : off + j * pitch;
}

// A lane's four columns xl .. xl + 3 of the three planes (plane stride `plane`) at o = &plane 0 [y][xl], plane width Wb: non-temporal
// float4 stores when Wb % 4 == 0 (with xl % 4 == 0, xl < Wb implies xl + 3 < Wb), guarded scalar stores otherwise.
__device__ __forceinline__ void u8_store_planes(float* __restrict__ o, size_t plane, const float (&v)[3][4], int xl, int Wb) {
  if ((Wb & 3) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      f32x4 t = {v[q][0], v[q][1], v[q][2], v[q][3]};
      __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(o + q * plane));
    }
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (xl + c < Wb) o[q * plane + c] = v[q][c];
  }
}

// ---- the staged-batch contract, host side ----------------------------------------------------------------------------------------
// What every entry point of the two files checks, before any launch, about the staged bytes, the tables in them and the source
// images their rows describe. Each check sets the error string under the entry point's name `me` and answers the status.
#define U8_TRY(call)                     \
  do {                                   \
    const int rc__ = (call);             \
    if (rc__ != CGG_OK) return rc__;     \
  } while (0)

// the kernels form byte addresses up to 7 past an image's end in int arithmetic before they guard them
static inline int u8_check_staged_bytes(const char* me, int64_t staged_bytes) {
  CGG_REQUIRE(staged_bytes >= 1 && staged_bytes <= (int64_t)INT32_MAX - 8, staged_bytes < 1 ? CGG_EINVAL : CGG_EUNSUPPORTED,
              "%s: staged_bytes must be in 1 .. 2^31 - 9 (got %lld)", me, (long long)staged_bytes);
  return CGG_OK;
}

// the `name` table: `rows` rows of `cols` int32 at byte `off`, a multiple of 4, inside the staged bytes
static inline int u8_check_table(const char* me, const char* name, int64_t off, int64_t rows, int64_t cols, int64_t staged_bytes) {
  CGG_REQUIRE(off >= 0 && (off & 3) == 0 && off + rows * cols * 4 <= staged_bytes, CGG_EINVAL,
              "%s: the %s table (%lld rows at byte %lld, a multiple of 4) must lie inside the %lld staged bytes", me, name,
              (long long)rows, (long long)off, (long long)staged_bytes);
  return CGG_OK;
}

static inline int u8_check_norm3(const char* me, const float* mean, const float* std_, const float* pad_val) {
  for (int c = 0; c < 3; ++c)
    CGG_REQUIRE(std_[c] != 0.f && std_[c] == std_[c] && mean[c] == mean[c] && pad_val[c] == pad_val[c], CGG_EINVAL,
                "%s: mean / std / pad_val must be numbers and std non-zero (channel %d)", me, c);
  return CGG_OK;
}

// the sizes of image b's row: h x w resized to nh x nw, neither empty, the source within the index arithmetic of the kernels
static inline int u8_check_sizes(const char* me, int b, int64_t h, int64_t w, int64_t nh, int64_t nw) {
  CGG_REQUIRE(h >= 1 && w >= 1 && nh >= 1 && nw >= 1, CGG_EINVAL, "%s: image %d is zero-sized (%lld x %lld -> %lld x %lld)", me, b,
              (long long)h, (long long)w, (long long)nh, (long long)nw);
  CGG_REQUIRE(h <= CGG_IMAGE_PREP_MAX_DIM && w <= CGG_IMAGE_PREP_MAX_DIM, CGG_EUNSUPPORTED,
              "%s: image %d is %lld x %lld, larger than %d on a side", me, b, (long long)h, (long long)w, CGG_IMAGE_PREP_MAX_DIM);
  return CGG_OK;
}

// the bytes of image b's row: h rows of 3 w bytes, `pitch` apart from byte `off`, inside the staged bytes
static inline int u8_check_bytes(const char* me, int b, int64_t off, int64_t h, int64_t w, int64_t pitch, int64_t staged_bytes) {
  CGG_REQUIRE(pitch >= 3 * w, CGG_EINVAL, "%s: image %d: row pitch %lld < 3 * w = %lld", me, b, (long long)pitch, (long long)(3 * w));
  CGG_REQUIRE(off >= 0 && off + h * pitch <= staged_bytes, CGG_EINVAL,
              "%s: image %d (bytes %lld .. %lld) extends past the %lld staged bytes", me, b, (long long)off,
              (long long)(off + h * pitch), (long long)staged_bytes);
  return CGG_OK;
}
