// Parity mode's mask-feature head of the pixel decoder as ONE launch (the end of [3P] MSDeformAttnPixelDecoder.forward:
// output ConvModule's GroupNorm + ReLU, the 1 x 1 mask_feature convolution; then the packed x3 images cgg_mask_logits' split mode
// reads, open_set/models/mask2former_head.py:787 / :801-823):
//
//     a  = relu((z - mean_bg) rstd_bg gamma + beta)           z = the raw 3 x 3 output, f32 channel-last [B, H W, 256]
//     mf = a Wm^T * colscale + bm                              f32-class f16 x 3 contraction of x3.h, 256 -> 256
//     images[pool] = split(pool == 1 ? mf : 2 x 2 centre mean of mf)      hi / lo [B][T][32 octets][32 pixels][8] f16 pieces
//
// replacing cgg_gn_nhwc_apply_kernel<false, true> (z f32 -> x3a), cgg_gemm_x3s (x3a -> mf f32) and cgg_pack_nhwc_f32_x3_kernel
// (mf -> images): the x3a form of a and the f32 mf had one consumer each, so 4 x 134 MB of HBM traffic at configs[1] existed only
// because the three steps were three kernels. The arithmetic is kept operation for operation -- the GroupNorm expression and its
// split, the three MFMAs per fragment pair in ascending k (cgg_gemm_x3s_kernel's order for K = 256: one k-group), the pre-scaled
// epilogue (acc * 16 colscale + 16 bias, clamp, / 16), the pack kernel's ((a + c) + (d + e)) * 0.25 -- so the images are
// bit-identical to the three-kernel path (tests/test_mask_feature_head_gpu.py).
//
// A workgroup owns an 8 x 8 pixel tile = 64 rows: the 2 x 2 centre blocks of every pool-2 / -4 / -8 pixel lie inside one tile
// (rows pool i + pool / 2 - 1, + 1), so a pooled image needs no neighbour's data. The rows are normalised and split into hi / lo
// A-fragment images in LDS (64 KiB, the bank swizzle of encoder_tail_x3.hip's row image); wave wn computes the 64 x (32 TN) block
// with the weight fragments streamed L2 -> registers MH_PF k-steps ahead; the f32 tile (64 x 260 floats) overlays the fragment
// images; every image piece leaves as 16 bytes per lane, 8 lanes = one 128-byte run of a pool-1 image. 65 KiB of LDS: two
// workgroups share a CU, one's load / store phase runs under the other's MFMAs.
//
// build-flags: -mllvm -amdgpu-mfma-vgpr-form=1
#include "x3.h"

#define MH_C 256
#define MH_STEPS 16
#define MH_RB 64               // rows per workgroup: 8 x 8 pixels
#define MH_TS 260              // f32 tile row stride
#define MH_IMG (2 * MH_STEPS * 64)          // u32x4 slots of one 64 x 256 image piece (32 KiB)

struct MhJobs {
  int n;
  int pool[4], Wp[4], npix[4], T[4];
  u32x4* hi[4];
  u32x4* lo[4];
};

template <int NWV>
__global__ __launch_bounds__(64 * NWV, NWV / 2) void cgg_mask_feature_head_x3_kernel(
    const float* __restrict__ z, const float* __restrict__ ws, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const CggX3W w, const float* __restrict__ bias, float lo_clamp, const MhJobs jobs, float* __restrict__ mf, int H, int W,
    int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mh_smem[];
  u32x4* xfrag = reinterpret_cast<u32x4*>(mh_smem);                    // row image: hi [2 m-tiles][16][64] | lo    64 KiB
  float* tile = reinterpret_cast<float*>(mh_smem);                           // [64][MH_TS] f32 output tile, overlays the image
  constexpr int NT = 64 * NWV;
  constexpr int TN = 8 / NWV;                                                // 32-column n-tiles per wave
  constexpr int MH_PF = NWV == 8 ? 2 : 4;                                    // B-fragment prefetch distance (k-steps)
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int j = lane & 31, hi5 = lane >> 5;
  const int b = blockIdx.y;
  const int tiles_x = W >> 3;
  const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const int y0 = by * 8, x0 = bx * 8;
  const size_t HW = (size_t)H * W;

  // weight stream: the first MH_PF k-steps are in flight while the rows are staged
  u32x4 qh[TN][MH_PF], ql[TN][MH_PF];
  const u32x4 *bh[TN], *bl[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const size_t o = ((size_t)(TN * wn + t) * MH_STEPS) * 64 + lane;
    bh[t] = w.hi + o;
    bl[t] = w.lo + o;
#pragma unroll
    for (int s = 0; s < MH_PF; ++s) {
      qh[t][s] = bh[t][s * 64];
      ql[t][s] = bl[t][s * 64];
    }
  }
  // ---- rows -> GroupNorm + ReLU -> split A-fragment images: 32-byte piece (row, k8) = the 8 channels of group k8 -> slot (mt,
  //      k-step = k8 / 2, (row % 32 + 32 (k8 & 1)) ^ k-step). All loads of a thread are issued before the first use. ----
  float am = 0.f;
  {
    constexpr int NP = MH_RB * 32 / NT;
    const int k8 = tid & 31;                          // NT % 32 == 0: one group per thread
    f32x4 v0[NP], v1[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (tid + i * NT) >> 5;
      const size_t pix = (size_t)(y0 + (row >> 3)) * W + x0 + (row & 7);
      const float* src = z + ((size_t)b * HW + pix) * MH_C + 8 * k8;
      v0[i] = *reinterpret_cast<const f32x4*>(src);
      v1[i] = *reinterpret_cast<const f32x4*>(src + 4);
    }
    const float mean = ws[((size_t)b * 32 + k8) * 2], var = ws[((size_t)b * 32 + k8) * 2 + 1];
    const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + k8 * 8), gb = *reinterpret_cast<const f32x4*>(gamma + k8 * 8 + 4);
    const f32x4 ba = *reinterpret_cast<const f32x4*>(beta + k8 * 8), bb = *reinterpret_cast<const f32x4*>(beta + k8 * 8 + 4);
    __builtin_amdgcn_sched_barrier(0);
    const float rstd = rsqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (tid + i * NT) >> 5;
      float f[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {                   // the expression of cgg_gn_nhwc_apply_kernel, then its ReLU
        f[k] = (v0[i][k] - mean) * rstd * ga[k] + ba[k];
        f[k + 4] = (v1[i][k] - mean) * rstd * gb[k] + bb[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        f[k] = fmaxf(f[k], 0.f);
        am = fmaxf(am, fabsf(f[k]));
      }
      u32x4 h, l;
      cgg_x3_split8(f32x4{f[0], f[1], f[2], f[3]}, f32x4{f[4], f[5], f[6], f[7]}, h, l);
      const int slot = ((row >> 5) * MH_STEPS + (k8 >> 1)) * 64 + (((row & 31) + 32 * (k8 & 1)) ^ (k8 >> 1));
      xfrag[slot] = h;
      xfrag[MH_IMG + slot] = l;
    }
  }
  // a normalised value beyond the x3a range: the flag the GroupNorm's x3a store raised
  if (flag && !(am * CGG_X3_ASCALE <= CGG_X3A_MAX)) atomicOr(flag, 1);
  f32x16 acc[2][TN];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][t][r] = 0.f;
  __syncthreads();
  // ---- 256 -> 256 contraction, k ascending; per accumulator and k-step: al bh, ah bl, ah bh ----
  {
    int xl = lane;
    asm volatile("" : "+v"(xl));
    auto load_a = [&](int s, u32x4& h0, u32x4& l0, u32x4& h1, u32x4& l1) {
      const int xo = xl ^ s;
      h0 = xfrag[s * 64 + xo];
      l0 = xfrag[MH_IMG + s * 64 + xo];
      h1 = xfrag[(MH_STEPS + s) * 64 + xo];
      l1 = xfrag[MH_IMG + (MH_STEPS + s) * 64 + xo];
    };
    u32x4 ah0, al0, ah1, al1;
    load_a(0, ah0, al0, ah1, al1);
#pragma unroll
    for (int s = 0; s < MH_STEPS; ++s) {
      u32x4 bhv[TN], blv[TN];
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        bhv[t] = qh[t][s % MH_PF];
        blv[t] = ql[t][s % MH_PF];
      }
      const u32x4 vah0 = ah0, val0 = al0, vah1 = ah1, val1 = al1;
      if (s + 1 < MH_STEPS) load_a(s + 1, ah0, al0, ah1, al1);
      if (s + MH_PF < MH_STEPS) {
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          qh[t][s % MH_PF] = bh[t][(s + MH_PF) * 64];
          ql[t][s % MH_PF] = bl[t][(s + MH_PF) * 64];
        }
      }
      __builtin_amdgcn_sched_barrier(0);                 // loads of the later steps issue BEFORE this step's MFMAs
#define MH_MF(A, B, C) C = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), C, 0, 0, 0)
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        MH_MF(val0, bhv[t], acc[0][t]);
        MH_MF(val1, bhv[t], acc[1][t]);
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        MH_MF(vah0, blv[t], acc[0][t]);
        MH_MF(vah1, blv[t], acc[1][t]);
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        MH_MF(vah0, bhv[t], acc[0][t]);
        MH_MF(vah1, bhv[t], acc[1][t]);
      }
#undef MH_MF
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();                                     // every wave is done with the row image: the tile overlays it
  // ---- epilogue of cgg_gemm_x3s_kernel (f32 output, no residual), in its pre-scaled domain: (acc * 16 cs + 16 bias) clamped, / 16 ----
#pragma unroll
  for (int nt = 0; nt < TN; ++nt) {
    const int col = 32 * TN * wn + 32 * nt + j;
    const float cs = w.scale[col] * CGG_X3_ASCALE;
    const float bs = bias ? bias[col] * CGG_X3_ASCALE : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = fmaxf(acc[mt][nt][r] * cs + bs, lo_clamp);
        tile[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hi5) * MH_TS + col] = v * CGG_X3_INV_ASCALE;
      }
  }
  __syncthreads();
  // ---- the images. Piece (pixel, octet kc) = 8 channels -> 16 bytes of hi and of lo at [b][p / 32][kc][p % 32]. ----
  for (int jb = 0; jb < jobs.n; ++jb) {
    const int pool = jobs.pool[jb], Wp = jobs.Wp[jb], T = jobs.T[jb];
    u32x4* __restrict__ dh = jobs.hi[jb];
    u32x4* __restrict__ dl = jobs.lo[jb];
    if (pool == 1) {
      // lanes (tx, kc): the 8 pixels of a tile row are 8 consecutive slots = one 128-byte run per octet (W % 8 == 0: inside one T tile)
#pragma unroll
      for (int it = 0; it < MH_RB * 32 / NT; ++it) {
        const int idx = tid + it * NT;
        const int tx = idx & 7, kc = (idx >> 3) & 31, ty = idx >> 8;
        const float* s = tile + (ty * 8 + tx) * MH_TS + kc * 8;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(s), v1 = *reinterpret_cast<const f32x4*>(s + 4);
        u32x4 h, l;
        cgg_x3_split8(v0, v1, h, l);
        const int p = (y0 + ty) * W + x0 + tx;
        const size_t slot = (((size_t)b * T + (p >> 5)) * 32 + kc) * 32 + (p & 31);
        dh[slot] = h;
        dl[slot] = l;
      }
    } else {
      // 2 x 2 centre mean of the pool x pool block, the pack kernel's association order; (8 / pool)^2 pooled pixels per tile
      const int ns = 8 / pool, npp = ns * ns;
      for (int idx = tid; idx < npp * 32; idx += NT) {
        const int pp = idx & (npp - 1), kc = idx / npp;
        const int ii = pp / ns, jj = pp - ii * ns;
        const int r0 = pool * ii + (pool >> 1) - 1, c0 = pool * jj + (pool >> 1) - 1;
        const float* s00 = tile + (r0 * 8 + c0) * MH_TS + kc * 8;
        const float* s10 = s00 + 8 * MH_TS;
        f32x4 m[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(s00 + 4 * h), c = *reinterpret_cast<const f32x4*>(s00 + MH_TS + 4 * h);
          const f32x4 d = *reinterpret_cast<const f32x4*>(s10 + 4 * h), e = *reinterpret_cast<const f32x4*>(s10 + MH_TS + 4 * h);
          m[h] = ((a + c) + (d + e)) * 0.25f;
        }
        u32x4 h, l;
        cgg_x3_split8(m[0], m[1], h, l);
        const int p = (y0 / pool + ii) * Wp + x0 / pool + jj;
        const size_t slot = (((size_t)b * T + (p >> 5)) * 32 + kc) * 32 + (p & 31);
        dh[slot] = h;
        dl[slot] = l;
      }
    }
    // padding slots of a ragged last 32-pixel tile hold zeros (the split of 0); the image's last workgroup writes them
    const int rag = jobs.npix[jb] & 31;
    if (rag && blockIdx.x == gridDim.x - 1) {
      const int cnt = 32 - rag;
      const u32x4 zero = {0u, 0u, 0u, 0u};
      for (int idx = tid; idx < cnt * 32; idx += NT) {
        const int kc = idx / cnt, pl = rag + (idx - kc * cnt);
        const size_t slot = (((size_t)b * T + (T - 1)) * 32 + kc) * 32 + pl;
        dh[slot] = zero;
        dl[slot] = zero;
      }
    }
  }
  if (mf) {                                            // the f32 map itself, for a caller that needs it
#pragma unroll
    for (int it = 0; it < MH_RB * 32 / NT; ++it) {
      const int idx = tid + it * NT;
      const int row = idx >> 5, c8 = idx & 31;
      const float* s = tile + row * MH_TS + c8 * 8;
      const size_t pix = (size_t)(y0 + (row >> 3)) * W + x0 + (row & 7);
      float* o = mf + ((size_t)b * HW + pix) * MH_C + c8 * 8;
      *reinterpret_cast<f32x4*>(o) = *reinterpret_cast<const f32x4*>(s);
      *reinterpret_cast<f32x4*>(o + 4) = *reinterpret_cast<const f32x4*>(s + 4);
    }
  }
}

int* cgg_x3_overflow_flag_ptr();       // x3s_gemm.hip

// cfg 0: four wavefronts per workgroup (two 32-column n-tiles each), 1: eight (one each); two workgroups per CU either way.
// -1 = the default
constexpr int MH_DEFAULT_CFG = 1;

template <int NWV>
static int mh_go(const char* who, const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps, const void* w_x3,
                 const float* bias, const MhJobs& jobs, float* mf, int B, int H, int W, hipStream_t stream) {
  constexpr size_t lds = (size_t)MH_RB * MH_TS * sizeof(float);              // the tile (>= the two row images)
  static_assert(lds >= (size_t)2 * MH_IMG * 16, "the tile must cover the row images");
  CGG_RAISE_LDS(cgg_mask_feature_head_x3_kernel<NWV>, lds, who);
  hipLaunchKernelGGL(cgg_mask_feature_head_x3_kernel<NWV>, dim3((unsigned)((H / 8) * (W / 8)), (unsigned)B), dim3(64 * NWV), lds, stream, z,
                     (const float*)gn_ws, gamma, beta, eps, cgg_x3_view(w_x3, MH_C, MH_C), bias, -__builtin_inff(), jobs, mf, H, W,
                     cgg_x3_overflow_flag_ptr());
  CGG_CHECK_LAUNCH(who);
  return CGG_OK;
}

static int mh_launch(const char* who, const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps, int groups,
                     const void* w_x3, const float* bias, void* const* hi_host, void* const* lo_host, const int* pools_host, int n,
                     float* mf, int B, int H, int W, int C, int N, int cfg, cgg_stream_t stream) {
  CGG_REQUIRE(z && gn_ws && gamma && beta && w_x3 && hi_host && lo_host && pools_host, CGG_EINVAL, "%s: null pointer", who);
  CGG_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && n >= 1 && n <= 4, CGG_EINVAL, "%s: bad sizes", who);
  CGG_REQUIRE(C == MH_C && N == MH_C && groups == 32, CGG_EUNSUPPORTED, "%s: C=%d N=%d groups=%d (only 256 / 256 / 32 is built)", who, C,
              N, groups);
  CGG_REQUIRE(H % 8 == 0 && W % 8 == 0, CGG_EUNSUPPORTED, "%s: %dx%d must be multiples of the 8 x 8 tile", who, H, W);
  CGG_REQUIRE((long long)H * W < (1ll << 31), CGG_EUNSUPPORTED, "%s: map too large", who);
  CGG_REQUIRE(cfg >= -1 && cfg <= 1, CGG_EINVAL, "%s: configuration %d (0, 1, or -1 = default)", who, cfg);
  CGG_REQUIRE(cgg_aligned16(z) && cgg_aligned16(gamma) && cgg_aligned16(beta) && cgg_aligned16(w_x3) && cgg_aligned16(mf) &&
                  (((uintptr_t)gn_ws) & 3u) == 0 && (((uintptr_t)bias) & 3u) == 0,
              CGG_EALIGN, "%s: 16-B alignment", who);
  MhJobs jobs;
  jobs.n = n;
  for (int i = 0; i < 4; ++i) {
    jobs.pool[i] = jobs.Wp[i] = jobs.npix[i] = jobs.T[i] = 0;
    jobs.hi[i] = jobs.lo[i] = nullptr;
  }
  for (int i = 0; i < n; ++i) {
    const int pool = pools_host[i];
    CGG_REQUIRE(pool == 1 || pool == 2 || pool == 4 || pool == 8, CGG_EUNSUPPORTED, "%s: pool=%d must be 1, 2, 4 or 8", who, pool);
    CGG_REQUIRE(hi_host[i] && lo_host[i] && cgg_aligned16(hi_host[i]) && cgg_aligned16(lo_host[i]), CGG_EALIGN, "%s: output %d", who, i);
    const int Hp = H / pool, Wp = W / pool;
    jobs.pool[i] = pool;
    jobs.Wp[i] = Wp;
    jobs.npix[i] = Hp * Wp;
    jobs.T[i] = (Hp * Wp + 31) / 32;
    jobs.hi[i] = (u32x4*)hi_host[i];
    jobs.lo[i] = (u32x4*)lo_host[i];
  }
  if ((cfg < 0 ? MH_DEFAULT_CFG : cfg) == 0)
    return mh_go<4>(who, z, gn_ws, gamma, beta, eps, w_x3, bias, jobs, mf, B, H, W, (hipStream_t)stream);
  return mh_go<8>(who, z, gn_ws, gamma, beta, eps, w_x3, bias, jobs, mf, B, H, W, (hipStream_t)stream);
}

extern "C" int cgg_mask_feature_head_x3(const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps, int groups,
                                        const void* w_x3, const float* bias, void* const* hi_host, void* const* lo_host,
                                        const int* pools_host, int n, float* mf, int B, int H, int W, int C, int N,
                                        cgg_stream_t stream) {
  return mh_launch("cgg_mask_feature_head_x3", z, gn_ws, gamma, beta, eps, groups, w_x3, bias, hi_host, lo_host, pools_host, n, mf, B, H,
                   W, C, N, -1, stream);
}

// ... with the wavefront configuration chosen by the caller: tests run both instantiations, the bench compares them
extern "C" int cgg_mask_feature_head_x3_cfg(const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps,
                                            int groups, const void* w_x3, const float* bias, void* const* hi_host, void* const* lo_host,
                                            const int* pools_host, int n, float* mf, int B, int H, int W, int C, int N, int cfg,
                                            cgg_stream_t stream) {
  return mh_launch("cgg_mask_feature_head_x3_cfg", z, gn_ws, gamma, beta, eps, groups, w_x3, bias, hi_host, lo_host, pools_host, n, mf,
                   B, H, W, C, N, cfg, stream);
}
