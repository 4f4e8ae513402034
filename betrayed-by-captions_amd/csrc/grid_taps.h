// The grid_sample rule of the point samplers, stated once: [3P] mmcv.ops.point_sample = F.grid_sample(points * 2 - 1, bilinear,
// zeros, align_corners=False). Same coordinate arithmetic and accumulation order as ATen's grid_sampler_2d kernel: unnormalise
// ((g + 1) * size - 1) / 2 on g = 2 p - 1, floor, the fractions towards the se and nw corners, then the taps nw, ne, sw, se with
// weight = (x fraction) * (y fraction). Every step is an explicit round-to-nearest intrinsic, so no includer's contraction setting
// can move a bit: the forward kernels, both backward kernels (postproc.hip) and the x3 packer (mask_logits.hip) sample at exactly
// the same place.
#pragma once
#include "cgg_common.h"

struct GridTaps {
  int x0, y0;              // the nw tap
  float tx, ty, ux, uy;    // ix - ix_nw, iy - iy_nw, ix_se - ix, iy_se - iy
};

// point (px, py) in [0, 1]^2 coordinates of an H x W map
__device__ __forceinline__ GridTaps cgg_grid_taps(float px, float py, int H, int W) {
  const float gx = __fsub_rn(__fmul_rn(px, 2.0f), 1.0f), gy = __fsub_rn(__fmul_rn(py, 2.0f), 1.0f);
  const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), (float)W), 1.f), 2.f);
  const float iy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), (float)H), 1.f), 2.f);
  const float fx = floorf(ix), fy = floorf(iy);
  GridTaps t;
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.tx = __fsub_rn(ix, fx);
  t.ty = __fsub_rn(iy, fy);
  t.ux = __fsub_rn(__fadd_rn(fx, 1.f), ix);
  t.uy = __fsub_rn(__fadd_rn(fy, 1.f), iy);
  return t;
}

// f(y, x, weight) for the taps inside rows [ylo, yhi) and columns [0, W), in nw, ne, sw, se order. The row range is the map's
// [0, H), or the band of rows a workgroup owns.
template <class F>
__device__ __forceinline__ void cgg_grid_taps_visit(const GridTaps& t, int ylo, int yhi, int W, F&& f) {
  const bool xin0 = t.x0 >= 0 && t.x0 < W, xin1 = t.x0 + 1 >= 0 && t.x0 + 1 < W;
  const bool yin0 = t.y0 >= ylo && t.y0 < yhi, yin1 = t.y0 + 1 >= ylo && t.y0 + 1 < yhi;
  if (xin0 && yin0) f(t.y0, t.x0, __fmul_rn(t.ux, t.uy));
  if (xin1 && yin0) f(t.y0, t.x0 + 1, __fmul_rn(t.tx, t.uy));
  if (xin0 && yin1) f(t.y0 + 1, t.x0, __fmul_rn(t.ux, t.ty));
  if (xin1 && yin1) f(t.y0 + 1, t.x0 + 1, __fmul_rn(t.tx, t.ty));
}
