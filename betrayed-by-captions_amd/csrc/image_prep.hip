// The reference's test pipeline on the device, one launch per batch: raw HWC uint8 images -> the (B, 3, Hb, Wb) float32 NCHW batch the
// stem reads. Replaces, per image, [3P] mmdet Resize (mmcv imrescale, 8-bit bilinear) -> Pad -> Normalize(to_rgb) -> ImageToTensor and
// the batch collation ([3P] mmcv collate of DataContainer(stack=True, padding_value=0)), which the reference runs on the CPU and ships
// as 12.6 MB of float32 per image. The arithmetic is the rule written down in image_prep.py (`prepare_host`), bit for bit:
//   taps      scale = 1 / (d / s) in double; fx = float((k + 0.5) * scale - 0.5), two separately rounded double operations;
//             i = floor(fx), fx -= i, clamped at both ends; a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048)
//   pixel     R = p[i] a0 + p[i + 1] a1 per source row; out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2
//   value     float(float(out - mean) * (1 / std)); the pad region holds one constant per plane, the collate region 0
// The rounding of (k + 0.5) * scale - 0.5 decides which source pixel a tap lands on, so nothing here may be contracted into a fused
// multiply-add: the file is built with contraction off (the flag below, and the pragma for a build that ignores the flag line).
//
// Geometry: a workgroup of 4 wavefronts owns an IP_TH x IP_TW = 16 x 256 tile of one image's output planes; a lane owns 4 consecutive
// columns, a wavefront one 256-column row segment at a time (1 KiB per plane per store instruction), 4 rows each. The source bytes the
// tile needs -- rows i(y0) .. i(y1) + 1, bytes 3 i(x0) .. 3 (i(x1) + 2) of each -- are staged into LDS (u8_resize.h), so each source
// byte crosses the memory pipeline once per tile instead of once per tap. A tile whose span does not fit U8_LDS_BYTES (downsampling
// by more than ~1.5 x) reads its taps from global memory instead.
// Every element of `out` is written exactly once, with non-temporal float4 stores when Wb % 4 == 0 (scalar stores otherwise).
//
// build-flags: -ffp-contract=off
#include "cgg_common.h"

// the tap rule, the tile's LDS image and the address of a tap in it, the three-plane store, PrepConst; the host checks of the staged bytes
#include "u8_resize.h"

#pragma clang fp contract(off)

#define IP_TW 256
#define IP_TH 16
#define IP_COLS CGG_IMAGE_PREP_TABLE_COLS

// rule 2 for one target index k of an axis with source length s: taps i0 / i1 and their 11-bit weights
__device__ __forceinline__ void ip_coef(int k, int s, double scale, int& i0, int& i1, int& a0, int& a1) {
  const U8Tap t = u8_tap(k, s, scale);
  a0 = (int)rintf((1.f - t.fx) * 2048.f);
  a1 = (int)rintf(t.fx * 2048.f);
  i0 = t.i0;
  i1 = t.i1;
}

__device__ __forceinline__ int ip_pixel(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  const int r0 = (p00 * a0 + p01 * a1) >> 4, r1 = (p10 * a0 + p11 * a1) >> 4;
  return (((b0 * r0) >> 16) + ((b1 * r1) >> 16) + 2) >> 2;
}

__global__ __launch_bounds__(256) void cgg_image_prep_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                                                 PrepConst cst, float* __restrict__ out, int Hb, int Wb) {
  __shared__ uint32_t lds[U8_LDS_BYTES / 4];
  const int b = blockIdx.z;
  const int32_t* d = table + IP_COLS * b;
  const int off = d[0], h = d[1], w = d[2], pitch = d[3], nh = d[4], nw = d[5], ph = d[6], pw = d[7];
  const int x0 = blockIdx.x * IP_TW, y0 = blockIdx.y * IP_TH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double sx = 1.0 / ((double)nw / (double)w), sy = 1.0 / ((double)nh / (double)h);

  // ---- the tile's source span (workgroup-uniform) and its LDS image -----------------------------------------------------------
  const bool resized = x0 < nw && y0 < nh;
  const U8Tile tile =
      u8_tile_stage(lds, src, resized, off, h, w, pitch, y0, min(y0 + IP_TH, nh) - 1, x0, min(x0 + IP_TW, nw) - 1, sy, sx, false);
  if (tile.use_lds) __syncthreads();               // uniform: every wavefront of the workgroup takes the same side

  // ---- this lane's 4 columns ----------------------------------------------------------------------------------------------------
  const int xl = x0 + 4 * lane;
  int xi0[4], xi1[4], xa0[4], xa1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    xi0[c] = xi1[c] = xa0[c] = xa1[c] = 0;
    if (resized && xl + c < nw) {
      ip_coef(xl + c, w, sx, xi0[c], xi1[c], xa0[c], xa1[c]);
      xi0[c] *= 3;
      xi1[c] *= 3;
    }
  }
  const size_t plane = (size_t)Hb * Wb;

#pragma unroll 1
  for (int r = 0; r < IP_TH / 4; ++r) {
    const int y = y0 + 4 * wv + r;
    if (y >= Hb || xl >= Wb) break;
    float v[3][4];
    const bool yin = y < nh;
    int j0 = 0, j1 = 0, b0 = 0, b1 = 0;
    if (resized && yin) ip_coef(y, h, sy, j0, j1, b0, b1);
    const int base0 = u8_tile_row(tile, off, pitch, j0), base1 = u8_tile_row(tile, off, pitch, j1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int x = xl + c;
      if (resized && yin && x < nw) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int ch = cst.to_rgb ? 2 - q : q;
          const int p00 = tile.mem[base0 + xi0[c] + ch], p01 = tile.mem[base0 + xi1[c] + ch];
          const int p10 = tile.mem[base1 + xi0[c] + ch], p11 = tile.mem[base1 + xi1[c] + ch];
          const int o = ip_pixel(p00, p01, p10, p11, xa0[c], xa1[c], b0, b1);
          v[q][c] = ((float)o - cst.mean[q]) * cst.rstd[q];
        }
      } else {
        const bool padded = y < ph && x < pw;
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q][c] = padded ? cst.pad[q] : 0.f;
      }
    }
    u8_store_planes(out + (size_t)b * 3 * plane + (size_t)y * Wb + xl, plane, v, xl, Wb);
  }
}

extern "C" int cgg_image_prep_u8(const uint8_t* staged, int64_t staged_bytes, int64_t table_offset, const int32_t* table_host, int B,
                                 const float* mean, const float* std_, const float* pad_val, int to_rgb, int pad_before_norm,
                                 float* out, int Hb, int Wb, cgg_stream_t stream) {
  const char* me = "cgg_image_prep_u8";
  CGG_REQUIRE(staged && table_host && mean && std_ && pad_val && out, CGG_EINVAL, "%s: null pointer", me);
  CGG_REQUIRE(B >= 1 && Hb >= 1 && Wb >= 1, CGG_EINVAL, "%s: B, Hb, Wb must be >= 1 (got %d, %d, %d)", me, B, Hb, Wb);
  CGG_REQUIRE(B <= CGG_IMAGE_PREP_MAX_DIM && Hb <= CGG_IMAGE_PREP_MAX_DIM && Wb <= CGG_IMAGE_PREP_MAX_DIM, CGG_EUNSUPPORTED,
              "%s: B, Hb, Wb must be <= %d (got %d, %d, %d)", me, CGG_IMAGE_PREP_MAX_DIM, B, Hb, Wb);
  U8_TRY(u8_check_staged_bytes(me, staged_bytes));
  U8_TRY(u8_check_table(me, "descriptor", table_offset, B, IP_COLS, staged_bytes));
  CGG_REQUIRE((((uintptr_t)staged) & 3u) == 0, CGG_EALIGN, "%s: staged must be 4-byte aligned", me);
  CGG_REQUIRE((Wb & 3) != 0 || cgg_aligned16(out), CGG_EALIGN, "%s: out must be 16-byte aligned when Wb %% 4 == 0", me);
  U8_TRY(u8_check_norm3(me, mean, std_, pad_val));
  for (int b = 0; b < B; ++b) {
    const int32_t* d = table_host + IP_COLS * b;
    const int64_t off = d[0], h = d[1], w = d[2], pitch = d[3], nh = d[4], nw = d[5], ph = d[6], pw = d[7];
    U8_TRY(u8_check_sizes(me, b, h, w, nh, nw));
    CGG_REQUIRE(nh <= ph && ph <= Hb && nw <= pw && pw <= Wb, CGG_EINVAL,
                "%s: image %d: need new <= pad <= batch, got rows %lld / %lld / %d, columns %lld / %lld / %d", me, b, (long long)nh,
                (long long)ph, Hb, (long long)nw, (long long)pw, Wb);
    U8_TRY(u8_check_bytes(me, b, off, h, w, pitch, staged_bytes));
  }
  const PrepConst cst = u8_prep_const(mean, std_, pad_val, to_rgb, pad_before_norm);
  const dim3 grid((unsigned)((Wb + IP_TW - 1) / IP_TW), (unsigned)((Hb + IP_TH - 1) / IP_TH), (unsigned)B);
  hipLaunchKernelGGL(cgg_image_prep_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, staged,
                     reinterpret_cast<const int32_t*>(staged + table_offset), cst, out, Hb, Wb);
  CGG_CHECK_LAUNCH(me);
  return CGG_OK;
}
