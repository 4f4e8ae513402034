// Shared device/host helpers for libcgg_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/cgg_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;  // 4 x bf16 MFMA operand

#define CGG_WAVE 64

// ---- wave primitives ----------------------------------------------------------------------------
// One DPP move: every lane reads `v` from the lane that control CTRL names within its row of 16 (all rows
// and banks enabled; a lane whose source is invalid keeps 0). 0xB1 = quad_perm [1, 0, 3, 2].
template <int CTRL>
__device__ __forceinline__ int cgg_dpp(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float cgg_dpp(float v) {
  return __int_as_float(cgg_dpp<CTRL>(__float_as_int(v)));
}

// the value held by lane ^ 1, by one DPP move
__device__ __forceinline__ float cgg_lane_xor1(float x) { return cgg_dpp<0xB1>(x); }
__device__ __forceinline__ uint32_t cgg_lane_xor1(uint32_t x) { return (uint32_t)cgg_dpp<0xB1>((int)x); }

// Sum over each row of 16 lanes by four DPP moves, in this order: lane ^ 1 (0xB1), lane ^ 2 (0x4E),
// row_half_mirror (0x141), row_mirror (0x140). Every lane ends with its row's sum.
__device__ __forceinline__ float cgg_row16_sum(float v) {
  v += cgg_dpp<0xB1>(v);
  v += cgg_dpp<0x4E>(v);
  v += cgg_dpp<0x141>(v);
  v += cgg_dpp<0x140>(v);
  return v;
}

// Butterfly over each aligned group of W lanes (W = 64: the wave): __shfl_xor steps W / 2, W / 4, ..., 1.
// Every lane ends with the sum / maximum of its group.
template <int W = CGG_WAVE>
__device__ __forceinline__ float cgg_wave_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int W = CGG_WAVE>
__device__ __forceinline__ float cgg_wave_max(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// raw buffer descriptor over [p, p + bytes): out-of-range loads return 0, out-of-range stores are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t cgg_buffer_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// ---- error reporting (thread-local, no exceptions across the ABI) -------------------------------
void cgg_set_error(const char* fmt, ...);

#define CGG_REQUIRE(cond, code, ...)      \
  do {                                    \
    if (!(cond)) {                        \
      cgg_set_error(__VA_ARGS__);         \
      return (code);                      \
    }                                     \
  } while (0)

#define CGG_CHECK_LAUNCH(name)                                              \
  do {                                                                      \
    hipError_t e__ = hipGetLastError();                                     \
    if (e__ != hipSuccess) {                                                \
      cgg_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return (int)e__;                                                      \
    }                                                                       \
  } while (0)

// ---- dynamic LDS above 64 KiB ---------------------------------------------------------------------
// per-device state (overflow flag words, LDS limits already granted) is tabled for devices below this
#define CGG_MAX_DEVICES 16

// Call immediately before launching `kernel` with `bytes` of dynamic LDS. At most 64 KiB: nothing to do.
// Above: raises the function's limit on the current device unless a limit >= bytes was already granted
// there (the attribute belongs to the function on ONE device). Thread-safe; CGG_OK or the hipError_t.
int cgg_raise_dynamic_lds(const void* kernel, size_t bytes, const char* who);

#define CGG_RAISE_LDS(kernel, bytes, who)                                        \
  do {                                                                           \
    int rc__ = cgg_raise_dynamic_lds((const void*)(kernel), (bytes), (who));     \
    if (rc__ != CGG_OK) return rc__;                                             \
  } while (0)

static inline bool cgg_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// ---- bf16 helpers (round-to-nearest-even, NaN preserved) ----------------------------------------
// hardware conversion (the cast lowers to v_cvt_pk_bf16_f32 on gfx950, RNE); a software round costs
// ~15 VALU per element and made the conversion-heavy prologues latency-bound
__device__ __forceinline__ uint16_t cgg_f2bf(float f) {
  const __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float cgg_bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// split f into hi = bf16(f) and lo = bf16(f - hi): f ~= hi + lo with ~2^-17 relative residual
__device__ __forceinline__ void cgg_split_bf(float f, uint16_t& hi, uint16_t& lo) {
  hi = cgg_f2bf(f);
  lo = cgg_f2bf(f - cgg_bf2f(hi));
}

__device__ __forceinline__ uint32_t cgg_pack2(uint16_t a, uint16_t b) {
  return (uint32_t)a | ((uint32_t)b << 16);
}
// (bf16(a), bf16(b)) as one word, a in the low half: one v_cvt_pk_bf16_f32; the 4-wide form packs v[0..3] in order
__device__ __forceinline__ uint32_t cgg_pk_bf16(float a, float b) {
  const f32x2 pr = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(pr, bf16x2));
}
__device__ __forceinline__ uint2 cgg_pk_bf16(f32x4 v) { return make_uint2(cgg_pk_bf16(v[0], v[1]), cgg_pk_bf16(v[2], v[3])); }

// XCD-aware block remap: hardware places block b on XCD b % 8; give every XCD one contiguous chunk
// of the logical index space so neighbouring work shares that XCD's private L2 (bijective form,
// cdna_hip_programming.md "XCD swizzle must be bijective").
__device__ __forceinline__ int cgg_xcd_remap(int bid, int nwg) {
  const int nx = 8;
  int xcd = bid % nx, idx = bid / nx;
  int q = nwg / nx, r = nwg % nx;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}
