// The 256-wide row LayerNorm, stated once: row statistics for the two lane layouts, the 4-wide row loads and the level-major
// K / V row table. The affine step (v * rstd * g + be, or an explicit fma) stays at the call sites: it differs by intent.
// Other rules, not here: the generic-N and half-wave bf16x8 kernels of linear_rows.hip, linear_rows2.hip's cross-wave and
// N <= 1024 forms, every GroupNorm (norm.hip, mask_feature_head.hip).
// The same rule, still written out: encoder_tail_x3.hip (both LayerNorms) and ln_bwd.hip. Through cgg_row16_norm the compiler
// packed and fused other products there (equal opcode counts, other bits: profiles/row_norm_refactor_ab.txt).
#pragma once
#include "cgg_common.h"

// 4 consecutive channels, f32 or bf16, as f32
__device__ __forceinline__ f32x4 cgg_row_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 cgg_row_load4(const uint16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
               __uint_as_float(u.y & 0xffff0000u)};
}

// ---- row statistics ------------------------------------------------------------------------------
// Both forms centre the lane's values in place (v -= mean) and return rstd = rsqrt(var + eps), in this order: pairwise
// (v0 + v1) + (v2 + v3), the reduction, mean = sum / 256, v -= mean, pairwise sum of the squares, the reduction. Every lane
// of the row (rows past the end included: hand them a clamped row) must call: the reductions are convergent.

// 16 lanes per row: lane sub = lane & 15 holds columns 4 sub + 64 k .. + 3, k = 0..3; cgg_row16_sum reduces.
// cgg_row16_norm_strict is the same text compiled with mul + add contraction off: a pragma at the call site does not reach an
// inlined callee, and under the default the compiler fuses some of the products into the sums (other roundings).
#define CGG_ROW16_NORM(NAME, CONTRACT)                                                                   \
  __device__ __forceinline__ float NAME(f32x4 (&v)[4], float eps) {                                      \
    CONTRACT                                                                                             \
    float sm = 0.f;                                                                                      \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) sm += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);       \
    sm = cgg_row16_sum(sm);                                                                              \
    const float mean = sm * (1.f / 256.f);                                                               \
    float q = 0.f;                                                                                       \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                      \
      v[k] = v[k] - mean;                                                                                \
      q += (v[k][0] * v[k][0] + v[k][1] * v[k][1]) + (v[k][2] * v[k][2] + v[k][3] * v[k][3]);            \
    }                                                                                                    \
    q = cgg_row16_sum(q);                                                                                \
    return rsqrtf(q * (1.f / 256.f) + eps);                                                              \
  }
CGG_ROW16_NORM(cgg_row16_norm, )
CGG_ROW16_NORM(cgg_row16_norm_strict, _Pragma("clang fp contract(off)"))
#undef CGG_ROW16_NORM

// one wave per row: lane holds columns 4 lane .. + 3; cgg_wave_sum reduces
__device__ __forceinline__ float cgg_wave_norm(f32x4& v, float eps) {
  float sm = (v[0] + v[1]) + (v[2] + v[3]);
  sm = cgg_wave_sum(sm);
  const float mean = sm * (1.f / 256.f);
  v = v - mean;
  float q = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  q = cgg_wave_sum(q);
  return rsqrtf(q * (1.f / 256.f) + eps);
}

// ---- level rows ----------------------------------------------------------------------------------
// The last encoder layer writes its K / V operands LEVEL-MAJOR ([level][image][hw_l][256]), so that each level is one
// contiguous (images * hw_l, 256) GEMM operand. start[l] = first row of level l inside an image of S rows, start[n] = S.
struct CggLevelRows { int n; int start[9]; };

// fills and validates the table for M = images * S rows
static inline int cgg_level_rows(CggLevelRows& lv, const int* level_start_host, int n_levels, int M, int S, const char* who) {
  CGG_REQUIRE(level_start_host, CGG_EINVAL, "%s: null pointer", who);
  CGG_REQUIRE(M > 0 && S > 0 && M % S == 0, CGG_EINVAL, "%s: M=%d not a multiple of S=%d", who, M, S);
  CGG_REQUIRE(n_levels >= 1 && n_levels <= 8, CGG_EUNSUPPORTED, "%s: n_levels=%d (1..8)", who, n_levels);
  lv.n = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    lv.start[l] = level_start_host[l];
    CGG_REQUIRE(lv.start[l] >= 0 && lv.start[l] < S && (l == 0 ? lv.start[l] == 0 : lv.start[l] > lv.start[l - 1]), CGG_EINVAL,
                "%s: level_start must start at 0 and increase (level %d: %d)", who, l, lv.start[l]);
  }
  lv.start[n_levels] = S;
  return CGG_OK;
}

// row si of image bi (of nimg) -> its level-major output row
__device__ __forceinline__ size_t cgg_level_row(const CggLevelRows& lv, int nimg, int bi, int si) {
  int l = 0;
  while (l + 1 < lv.n && si >= lv.start[l + 1]) ++l;
  return (size_t)nimg * lv.start[l] + (size_t)bi * (lv.start[l + 1] - lv.start[l]) + (si - lv.start[l]);
}
