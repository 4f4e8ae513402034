// The resize arithmetic of the inference tail, shared by postproc.hip and panoptic_fuse.hip: torch's bilinear taps
// (align_corners=False), the four-sample blend and the (optionally two-stage) "upsample -> crop -> rescale" value of
// open_set/models/mask2former_head.py:960-964 + maskformer_fusion_head.py:414-425. cgg_bilerp / cgg_resized_logit read a
// plane in global memory and are postproc.hip's functions, text unchanged (routing them through the templates below
// changed how the compiler contracts a * b + c in its kernels, i.e. their rounding); cgg_bilerp_at /
// cgg_resized_logit_at are the same expressions over a sample source `Src` (global memory, or a footprint staged in LDS).
#pragma once
#include "cgg_common.h"

// torch upsample_bilinear2d (align_corners=False) source coordinate for output index `o`
struct BiTap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ BiTap cgg_bitap(int o, float scale, int in_size) {
  float f = scale * ((float)o + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  BiTap t;
  t.i0 = (int)f;
  if (t.i0 > in_size - 1) t.i0 = in_size - 1;
  t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
  t.l1 = f - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// sample sources: s(row, col) of one low-resolution plane
struct GlobalSrc {                       // a [*, W] plane in global memory
  const float* __restrict__ s;
  int W;
  __device__ __forceinline__ float operator()(int r, int c) const { return s[(size_t)r * W + c]; }
};
struct WindowSrc {                       // rows r0.., columns c0.. of the plane, copied to a [*, W] window (LDS)
  const float* s;
  int W, r0, c0;
  __device__ __forceinline__ float operator()(int r, int c) const { return s[(r - r0) * W + (c - c0)]; }
};

template <class Src>
__device__ __forceinline__ float cgg_bilerp_at(const Src& s, const BiTap& ty, const BiTap& tx) {
  return ty.l0 * (tx.l0 * s(ty.i0, tx.i0) + tx.l1 * s(ty.i0, tx.i1)) +
         ty.l1 * (tx.l0 * s(ty.i1, tx.i0) + tx.l1 * s(ty.i1, tx.i1));
}
__device__ __forceinline__ float cgg_bilerp(const float* __restrict__ s, int W, const BiTap& ty,
                                            const BiTap& tx) {
  return ty.l0 * (tx.l0 * s[(size_t)ty.i0 * W + tx.i0] + tx.l1 * s[(size_t)ty.i0 * W + tx.i1]) +
         ty.l1 * (tx.l0 * s[(size_t)ty.i1 * W + tx.i0] + tx.l1 * s[(size_t)ty.i1 * W + tx.i1]);
}

// value of the (optionally two-stage) resized logit at final pixel (oy, ox):
//   stage 1: [H, W] -> [up_h, up_w] (batch_input_shape), crop to [crop_h, crop_w] (img_shape)
//   stage 2 (if out != crop): [crop_h, crop_w] -> [out_h, out_w] (ori_shape, `rescale`)
struct ResizeGeom {
  int H, W, up_h, up_w, crop_h, crop_w, out_h, out_w;
  float s1y, s1x, s2y, s2x;
  int two_stage;
};
template <class Src>
__device__ __forceinline__ float cgg_resized_logit_at(const Src& s, const ResizeGeom& g, int oy, int ox) {
  if (!g.two_stage) {
    const BiTap ty = cgg_bitap(oy, g.s1y, g.H), tx = cgg_bitap(ox, g.s1x, g.W);
    return cgg_bilerp_at(s, ty, tx);
  }
  const BiTap uy = cgg_bitap(oy, g.s2y, g.crop_h), ux = cgg_bitap(ox, g.s2x, g.crop_w);
  float v[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const BiTap ty = cgg_bitap(a ? uy.i1 : uy.i0, g.s1y, g.H);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const BiTap tx = cgg_bitap(c ? ux.i1 : ux.i0, g.s1x, g.W);
      v[a][c] = cgg_bilerp_at(s, ty, tx);
    }
  }
  return uy.l0 * (ux.l0 * v[0][0] + ux.l1 * v[0][1]) + uy.l1 * (ux.l0 * v[1][0] + ux.l1 * v[1][1]);
}
__device__ __forceinline__ float cgg_resized_logit(const float* __restrict__ s, const ResizeGeom& g,
                                                   int oy, int ox) {
  if (!g.two_stage) {
    const BiTap ty = cgg_bitap(oy, g.s1y, g.H), tx = cgg_bitap(ox, g.s1x, g.W);
    return cgg_bilerp(s, g.W, ty, tx);
  }
  const BiTap uy = cgg_bitap(oy, g.s2y, g.crop_h), ux = cgg_bitap(ox, g.s2x, g.crop_w);
  float v[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const BiTap ty = cgg_bitap(a ? uy.i1 : uy.i0, g.s1y, g.H);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const BiTap tx = cgg_bitap(c ? ux.i1 : ux.i0, g.s1x, g.W);
      v[a][c] = cgg_bilerp(s, g.W, ty, tx);
    }
  }
  return uy.l0 * (ux.l0 * v[0][0] + ux.l1 * v[0][1]) + uy.l1 * (ux.l0 * v[1][0] + ux.l1 * v[1][1]);
}

__host__ __device__ static inline ResizeGeom make_geom(int H, int W, int up_h, int up_w, int crop_h, int crop_w,
                                                       int out_h, int out_w) {
  ResizeGeom g;
  g.H = H; g.W = W; g.up_h = up_h; g.up_w = up_w; g.crop_h = crop_h; g.crop_w = crop_w;
  g.out_h = out_h; g.out_w = out_w;
  g.s1y = (float)H / (float)up_h;
  g.s1x = (float)W / (float)up_w;
  g.two_stage = (out_h != crop_h || out_w != crop_w) ? 1 : 0;
  g.s2y = (float)crop_h / (float)out_h;
  g.s2x = (float)crop_w / (float)out_w;
  return g;
}

__device__ __forceinline__ float cgg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
