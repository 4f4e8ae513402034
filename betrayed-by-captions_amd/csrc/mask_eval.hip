// COCO mask evaluation on bit-packed planes (mask_eval.py states the rules in numpy; the kernels equal them exactly).
//
//   cgg_mask_intersections_bits   |d & g| for every detection plane d and ground-truth plane g of one image, and the areas |d|, |g|:
//     a binary GEMM over the pixel axis. A workgroup owns a block of up to 64 x 64 (d, g) pairs and walks over slabs of the
//     planes (a few rows of all its planes, at most MI_SLAB_WORDS 32-bit words per plane): it stages the slab in LDS with
//     16-byte loads (4-byte / byte loads for rows that are not 16-byte aligned), masking the pad bits of each row's last word
//     once, there; then thread (td, tg) of the 16 x 16 grid accumulates its 4 x 4 register tile -- pairs (td + 16 i, tg + 16 j)
//     -- with one AND and one count-add per 32 pixels and pair, reading the planes from LDS as 16-byte quads (the plane stride
//     of 17 quads keeps the 16 g planes a wave reads at once on distinct banks; its 4 d planes are broadcasts). Sub-tiles wholly
//     past D or G are skipped by wave-uniform tests. With D <= 64 and G <= 64 every plane byte is read from HBM once; beyond, a
//     plane is read once per block of 64 planes of the other side.
//     Sums across slabs are exact and order-free: slab group s of a pair block writes int32 partials to ws[s] and a second
//     kernel adds the groups. No atomics, no memset.
//   cgg_coco_match   the IoU quotient in double and the greedy matching of COCOeval.evaluateImg, one thread per (category, area
//     range, threshold): the scan is sequential by nature and the work is tiny. A workgroup serves one category and prepares its
//     detections, ground truths and IoU block in LDS first (a thread that walked all D x G pairs in global memory took 540 us).
//   cgg_coco_match_boxes   the same scan -- one kernel template, instantiated on its IoU source -- on box IoUs (`--eval bbox`):
//     the `bbIou` rule on xywh boxes in double, every operation rounded on its own (mask_eval.box_iou_host).
//   cgg_box_iou_f64   that rule alone: the (D, G) IoU matrix and the detections' areas.
#include "cgg_common.h"

namespace {

constexpr int MI_THREADS = 256;
constexpr int MI_BLOCK = 64;                         // planes of each side per workgroup
constexpr int MI_SLAB_WORDS = 64;                    // 32-bit words of one plane in a slab (64 beat 128 and 32 at 1024^2 and 480 x 640)
constexpr int MI_STRIDE_WORDS = MI_SLAB_WORDS + 4;   // LDS words between planes: 17 quads, odd
constexpr int MI_MAX_PLANES = CGG_MASK_EVAL_MAX_MASKS;
constexpr int MI_TARGET_GROUPS = 1024;               // workgroups aimed at: slab groups = TARGET / pair blocks

struct MiGeom {
  int db, gb;        // pair blocks along D and G (>= 1 each)
  int RW;            // words per row
  int CW;            // words of a row in one slab (RW, or MI_SLAB_WORDS for rows longer than a slab)
  int nchunks;       // slabs across a row
  int R;             // rows per slab
  int nslabs;
  int cap;           // bound on the slab groups, from D and G alone (the workspace is sized by it)
  int nsg;           // slab groups launched
};

inline int mi_cap(int D, int G) {
  const int db = D > 0 ? (D + MI_BLOCK - 1) / MI_BLOCK : 1, gb = G > 0 ? (G + MI_BLOCK - 1) / MI_BLOCK : 1;
  const int cap = MI_TARGET_GROUPS / (db * gb);
  return cap < 1 ? 1 : cap;
}

inline MiGeom mi_geom(int D, int G, int H, int row_bytes) {
  MiGeom g;
  g.db = D > 0 ? (D + MI_BLOCK - 1) / MI_BLOCK : 1;
  g.gb = G > 0 ? (G + MI_BLOCK - 1) / MI_BLOCK : 1;
  g.RW = (row_bytes + 3) / 4;
  g.CW = g.RW <= MI_SLAB_WORDS ? g.RW : MI_SLAB_WORDS;
  g.nchunks = (g.RW + g.CW - 1) / g.CW;
  g.R = g.RW <= MI_SLAB_WORDS ? MI_SLAB_WORDS / g.RW : 1;
  const int64_t nslabs = (int64_t)((H + g.R - 1) / g.R) * g.nchunks;
  g.nslabs = (int)nslabs;                              // <= H * ceil(row_bytes / 256): the caller bounds it
  g.cap = mi_cap(D, G);
  g.nsg = g.nslabs < g.cap ? g.nslabs : g.cap;
  return g;
}

// bits of word `wj` of a row that are pixels: the mask of the row's last word, all ones before it, zero after it
__device__ __forceinline__ uint32_t mi_word_mask(int wj, int W) {
  const int valid = W - wj * 32;
  return valid >= 32 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << valid) - 1u));
}

// One 32-bit word of a row from byte / 4-byte loads: word `wj` of row `row` (pad bits masked), 0 outside the planes
__device__ __forceinline__ uint32_t mi_load_word(const uint8_t* __restrict__ bits, int64_t stride, int plane, int total, int row, int wj,
                                                 int W, int row_bytes, int mode, bool inside) {
  uint32_t v = 0;
  if (inside && plane < total) {
    const uint8_t* src = bits + (int64_t)plane * stride + (int64_t)row * row_bytes + (int64_t)wj * 4;
    const int nb = row_bytes - wj * 4;                   // bytes of the row from this word on
    if (nb >= 4 && mode == 4) {
      v = *(const uint32_t*)src;
    } else {
      for (int b = 0; b < 4 && b < nb; ++b) v |= (uint32_t)src[b] << (8 * b);
    }
    v &= mi_word_mask(wj, W);
  }
  return v;
}

// Stage rows r0 .. r0 + nrows, words c0 .. c0 + CW of planes p0 .. p0 + nplanes (planes at or past `total` are zero) as
// lds[plane][row][CW], zero up to the next quad. A thread issues MI_BATCH loads before it stores the first: one round trip to
// memory per batch, not per item.
constexpr int MI_BATCH = 4;

__device__ __forceinline__ void mi_stage(uint32_t* lds, const uint8_t* __restrict__ bits, int64_t stride, int p0, int nplanes,
                                         int total, int r0, int nrows, int c0, int CW, int W, int row_bytes, int mode) {
  const int words = nrows * CW;
  const int quads = (words + 3) >> 2;
  if (mode == 16) {                                   // CW % 4 == 0, rows and planes 16-byte aligned
    const int qpr = CW >> 2;
    const int per_plane = nrows * qpr;
    const int items = nplanes * per_plane;
    for (int base = threadIdx.x; base < items; base += MI_THREADS * MI_BATCH) {
      u32x4 v[MI_BATCH];
      int off[MI_BATCH], wj[MI_BATCH];
#pragma unroll
      for (int u = 0; u < MI_BATCH; ++u) {
        const int idx = base + u * MI_THREADS;
        const int p = idx / per_plane, rem = idx - p * per_plane;
        const int r = rem / qpr, q = rem - r * qpr;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        wj[u] = c0 + q * 4;
        off[u] = p * MI_STRIDE_WORDS + rem * 4;
        if (idx < items && p0 + p < total)               // (row_bytes % 16 == 0: the quad lies inside the row)
          v[u] = *(const u32x4*)(bits + (int64_t)(p0 + p) * stride + (int64_t)(r0 + r) * row_bytes + (int64_t)wj[u] * 4);
      }
#pragma unroll
      for (int u = 0; u < MI_BATCH; ++u) {
        if (base + u * MI_THREADS >= items) break;
        v[u].x &= mi_word_mask(wj[u], W);
        v[u].y &= mi_word_mask(wj[u] + 1, W);
        v[u].z &= mi_word_mask(wj[u] + 2, W);
        v[u].w &= mi_word_mask(wj[u] + 3, W);
        *(u32x4*)(lds + off[u]) = v[u];
      }
    }
    return;
  }
  const int padded = quads * 4;
  const int items = nplanes * padded;
  for (int base = threadIdx.x; base < items; base += MI_THREADS * MI_BATCH) {
    uint32_t v[MI_BATCH];
    int off[MI_BATCH];
#pragma unroll
    for (int u = 0; u < MI_BATCH; ++u) {
      const int idx = base + u * MI_THREADS;
      const int p = idx / padded, rem = idx - p * padded;
      const int r = rem / CW;
      off[u] = p * MI_STRIDE_WORDS + rem;
      v[u] = mi_load_word(bits, stride, p0 + p, total, r0 + r, c0 + (rem - r * CW), W, row_bytes, mode, idx < items && rem < words);
    }
#pragma unroll
    for (int u = 0; u < MI_BATCH; ++u)
      if (base + u * MI_THREADS < items) lds[off[u]] = v[u];
  }
}

__global__ __launch_bounds__(MI_THREADS) void cgg_mi_partial_kernel(const uint8_t* __restrict__ det, int D, int64_t det_stride,
                                                                    const uint8_t* __restrict__ gt, int G, int64_t gt_stride, int H,
                                                                    int W, int row_bytes, MiGeom geom, int det_mode, int gt_mode,
                                                                    int32_t* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mi_lds[];
  uint32_t* lds_d = mi_lds;
  uint32_t* lds_g = mi_lds + MI_BLOCK * MI_STRIDE_WORDS;
  const int tg = threadIdx.x & 15, td = threadIdx.x >> 4;
  const int d0 = blockIdx.y * MI_BLOCK, g0 = blockIdx.z * MI_BLOCK;
  const int dvalid = D - d0 < MI_BLOCK ? D - d0 : MI_BLOCK;        // may be 0 (D == 0)
  const int gvalid = G - g0 < MI_BLOCK ? G - g0 : MI_BLOCK;
  const int ni = (dvalid + 15) >> 4, nj = (gvalid + 15) >> 4;      // 16-plane sub-tiles in use: uniform over the workgroup
  int32_t acc[4][4] = {};
  int32_t ad[4] = {}, ag[4] = {};
  for (int s = blockIdx.x; s < geom.nslabs; s += geom.nsg) {
    const int rs = s / geom.nchunks, c0 = (s - rs * geom.nchunks) * geom.CW;
    const int r0 = rs * geom.R;
    const int nrows = H - r0 < geom.R ? H - r0 : geom.R;
    const int cw = geom.RW - c0 < geom.CW ? geom.RW - c0 : geom.CW;  // (a 16-byte row keeps cw % 4 == 0)
    __syncthreads();                                               // the previous slab has been read
    mi_stage(lds_d, det, det_stride, d0, ni * 16, D, r0, nrows, c0, cw, W, row_bytes, det_mode);
    mi_stage(lds_g, gt, gt_stride, g0, nj * 16, G, r0, nrows, c0, cw, W, row_bytes, gt_mode);
    __syncthreads();
    const int quads = (nrows * cw + 3) >> 2;
    for (int q = 0; q < quads; ++q) {
      u32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < ni) {
          a[i] = *(const u32x4*)(lds_d + (td + 16 * i) * MI_STRIDE_WORDS + q * 4);
          ad[i] += __builtin_popcount(a[i].x) + __builtin_popcount(a[i].y) + __builtin_popcount(a[i].z) + __builtin_popcount(a[i].w);
        }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          b[j] = *(const u32x4*)(lds_g + (tg + 16 * j) * MI_STRIDE_WORDS + q * 4);
          ag[j] += __builtin_popcount(b[j].x) + __builtin_popcount(b[j].y) + __builtin_popcount(b[j].z) + __builtin_popcount(b[j].w);
        }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < ni) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nj) {
              int32_t c = acc[i][j];
              c = __builtin_popcount(a[i].x & b[j].x) + c;
              c = __builtin_popcount(a[i].y & b[j].y) + c;
              c = __builtin_popcount(a[i].z & b[j].z) + c;
              c = __builtin_popcount(a[i].w & b[j].w) + c;
              acc[i][j] = c;
            }
        }
    }
  }
  // partials of slab group blockIdx.x: [D][G] intersections, then [D] and [G] areas
  int32_t* part = ws + (int64_t)blockIdx.x * ((int64_t)D * G + D + G);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = d0 + td + 16 * i;
    if (d >= D) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = g0 + tg + 16 * j;
      if (g < G) part[(int64_t)d * G + g] = acc[i][j];
    }
    if (blockIdx.z == 0 && tg == 0) part[(int64_t)D * G + d] = ad[i];
  }
  if (blockIdx.y == 0 && td == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = g0 + tg + 16 * j;
      if (g < G) part[(int64_t)D * G + D + g] = ag[j];
    }
  }
}

// out[e] = sum over the slab groups of ws[s][e], e over [D][G] ++ [D] ++ [G]. A block takes MR_ELEMS consecutive elements; its
// MR_SUB sub-groups each add every MR_SUB-th slab group (independent loads, 128 bytes wide per sub-group), LDS adds the sub-groups.
constexpr int MR_ELEMS = 32, MR_SUB = 8;

__global__ __launch_bounds__(MR_ELEMS * MR_SUB) void cgg_mi_reduce_kernel(const int32_t* __restrict__ ws, int nsg, int D, int G,
                                                                         int32_t* __restrict__ inter, int32_t* __restrict__ area_d,
                                                                         int32_t* __restrict__ area_g) {
  __shared__ int32_t part[MR_SUB][MR_ELEMS];
  const int64_t N = (int64_t)D * G + D + G;
  const int le = threadIdx.x % MR_ELEMS, sub = threadIdx.x / MR_ELEMS;
  const int64_t e = (int64_t)blockIdx.x * MR_ELEMS + le;
  int32_t sum = 0;
  if (e < N) {
#pragma unroll 8
    for (int s = sub; s < nsg; s += MR_SUB) sum += ws[(int64_t)s * N + e];
  }
  part[sub][le] = sum;
  __syncthreads();
  if (sub != 0 || e >= N) return;
#pragma unroll
  for (int k = 1; k < MR_SUB; ++k) sum += part[k][le];
  if (e < (int64_t)D * G) inter[e] = sum;
  else if (e < (int64_t)D * G + D) area_d[e - (int64_t)D * G] = sum;
  else area_g[e - (int64_t)D * G - D] = sum;
}

inline int mi_load_mode(const uint8_t* p, int64_t stride, int row_bytes) {
  const uintptr_t all = (uintptr_t)p | (uintptr_t)stride | (uintptr_t)row_bytes;
  return (all & 15u) == 0 ? 16 : ((all & 3u) == 0 ? 4 : 1);
}

// ---- matching -------------------------------------------------------------------------------------------------------------------
// One workgroup per category, one thread per (area range, threshold). The first wave compacts, by ballots, the category's
// detections (score order, cut to max_det) and ground truths, and per area range the scan order of the ground truths (those that
// count first); all threads then fill the category's IoU block in LDS (CM_IOU_LDS entries: in chunks of detections when the block
// is larger) and each runs its sequential scan on LDS alone.
constexpr int CM_MAX_T = CGG_MASK_EVAL_MAX_THRS, CM_MAX_A = CGG_MASK_EVAL_MAX_AREAS, CM_MAX_K = CGG_MASK_EVAL_MAX_CATS;
constexpr int CM_IOU_LDS = 2048;

// The IoU source of the matching scan: what a (detection, ground truth) pair's IoU and a detection's own area are made from.
//   gt_key(g)                 what ground truth g contributes besides its index; the kernel stages it in LDS with the category
//   iou(d, g, key, crowd)     the pair's IoU in double
//   det_area(d)               the detection's area, for the area ranges
// Masks: the integer intersections and areas of cgg_mask_intersections_bits.
struct CmMaskIou {
  const int32_t* __restrict__ inter;
  const int32_t* __restrict__ area_d;
  const int32_t* __restrict__ area_g;
  int G;
  __device__ __forceinline__ int32_t gt_key(int g) const { return area_g[g]; }
  __device__ __forceinline__ double iou(int d, int g, int32_t ag, bool crowd) const {
    const int64_t i = inter[(int64_t)d * G + g];
    const int64_t u = crowd ? (int64_t)area_d[d] : (int64_t)area_d[d] + ag - i;
    return u == 0 ? 0.0 : (double)i / (double)u;
  }
  __device__ __forceinline__ double det_area(int d) const { return (double)area_d[d]; }
};

// Boxes (mask_eval.box_iou_host, the `bbIou` rule). A detection is a row (x0, y0, x1, y1, score) of float32 as the results hold
// it: every coordinate is widened to double, then w = x1 - x0 and h = y1 - y0 in double (mask_eval.det_boxes_xywh_host). A ground
// truth is (x, y, w, h) in double. Every operation below is an IEEE double operation of its own: contraction is off, since a
// product fused into the following add rounds once where the rule rounds twice.
struct CmBox {
  double x, y, w, h;
};

__device__ __forceinline__ CmBox cm_det_box(const float* __restrict__ det5, int d) {
#pragma clang fp contract(off)
  const float* b = det5 + (int64_t)d * 5;
  const double x0 = (double)b[0], y0 = (double)b[1], x1 = (double)b[2], y1 = (double)b[3];
  return CmBox{x0, y0, x1 - x0, y1 - y0};
}

__device__ __forceinline__ CmBox cm_gt_box(const double* __restrict__ gt4, int g) {
  const double* b = gt4 + (int64_t)g * 4;
  return CmBox{b[0], b[1], b[2], b[3]};
}

__device__ __forceinline__ double cm_box_area(const CmBox& b) {
#pragma clang fp contract(off)
  return b.w * b.h;
}

__device__ __forceinline__ double cm_box_iou(const CmBox& D, const CmBox& G, bool crowd) {
#pragma clang fp contract(off)
  const double da = D.w * D.h, ga = G.w * G.h;
  const double w = fmin(D.w + D.x, G.w + G.x) - fmax(D.x, G.x);
  if (w <= 0) return 0.0;
  const double h = fmin(D.h + D.y, G.h + G.y) - fmax(D.y, G.y);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : (da + ga) - i;
  return i / u;
}

struct CmBoxIou {
  const float* __restrict__ det5;
  const double* __restrict__ gt4;
  // nothing is staged per ground truth: its 32 bytes are read where the IoU block is filled (1024 of them do not fit the static LDS
  // besides that block and the scan orders; the scan itself reads no box)
  __device__ __forceinline__ int32_t gt_key(int) const { return 0; }
  __device__ __forceinline__ double iou(int d, int g, int32_t, bool crowd) const {
    return cm_box_iou(cm_det_box(det5, d), cm_gt_box(gt4, g), crowd);
  }
  __device__ __forceinline__ double det_area(int d) const { return cm_box_area(cm_det_box(det5, d)); }
};

template <class Iou>
__global__ __launch_bounds__(CM_MAX_T* CM_MAX_A) void cgg_coco_match_kernel(
    const Iou src, const int32_t* __restrict__ det_order, const int32_t* __restrict__ det_cats, const int32_t* __restrict__ gt_cats,
    const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area, const int32_t* __restrict__ cat_ids, int K,
    const double* __restrict__ area_rngs, int A, const double* __restrict__ iou_thrs, int T, int D, int G, int max_det,
    int class_agnostic, int32_t* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore, uint8_t* __restrict__ gt_ignore,
    int32_t* __restrict__ counts) {
  __shared__ uint16_t dsel[MI_MAX_PLANES];             // the category's detections, in score order
  __shared__ uint16_t gsel[MI_MAX_PLANES];             // its ground truths, in their order
  __shared__ uint16_t ord[CM_MAX_A][MI_MAX_PLANES];    // per area range: positions in gsel in scan order, bit 15 = crowd
  __shared__ int32_t g_key[MI_MAX_PLANES];             // src.gt_key of gsel[p] (masks: area_g)
  __shared__ uint8_t g_crowd[MI_MAX_PLANES];
  __shared__ double g_own_area[MI_MAX_PLANES];         // gt_area of gsel[p]
  __shared__ double iou_lds[CM_IOU_LDS];
  __shared__ int nreg[CM_MAX_A];                       // ground truths that count, per area range
  __shared__ int n_sel[2];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int cat = cat_ids[k];
  const uint64_t below = (1ull << lane) - 1ull;
  if (tid < 64) {                                      // (the block holds at least one full wave)
    int cnt = 0;
    for (int base = 0; base < D && cnt < max_det; base += 64) {
      const int o = base + lane;
      int d = 0;
      bool f = false;
      if (o < D) {
        d = det_order[o];
        f = class_agnostic || det_cats[d] == cat;
      }
      const uint64_t b = __ballot(f);
      const int pos = cnt + __popcll(b & below);
      if (f && pos < max_det) dsel[pos] = (uint16_t)d;
      cnt += __popcll(b);
    }
    const int Dk = cnt < max_det ? cnt : max_det;
    cnt = 0;
    for (int base = 0; base < G; base += 64) {
      const int g = base + lane;
      const bool f = g < G && gt_cats[g] == cat;
      const uint64_t b = __ballot(f);
      const int pos = cnt + __popcll(b & below);
      if (f) {
        gsel[pos] = (uint16_t)g;
        g_key[pos] = src.gt_key(g);
        g_crowd[pos] = gt_crowd[g] != 0;
        g_own_area[pos] = gt_area[g];
      }
      cnt += __popcll(b);
    }
    const int Gk = cnt;
    if (lane == 0) {
      n_sel[0] = Dk;
      n_sel[1] = Gk;
    }
    for (int a = 0; a < A; ++a) {
      const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
      int c = 0;
      for (int pass = 0; pass < 2; ++pass) {
        for (int base = 0; base < Gk; base += 64) {
          const int p = base + lane;
          bool f = false, crowd = false;
          if (p < Gk) {
            const double ga = g_own_area[p];           // (written by this wave, above)
            crowd = g_crowd[p] != 0;
            const bool ignored = crowd || ga < lo || ga > hi;
            f = ignored == (pass == 1);
          }
          const uint64_t b = __ballot(f);
          if (f) ord[a][c + __popcll(b & below)] = (uint16_t)(p | (crowd ? 0x8000 : 0));
          c += __popcll(b);
        }
        if (pass == 0 && lane == 0) nreg[a] = c;
      }
    }
  }
  __syncthreads();
  const int Dk = n_sel[0], Gk = n_sel[1];
  // what lies past D_k / G_k is written too, as zeros; the ignore flags of the ground truths in scan order; the counts
  int32_t* dtm_k = dt_match + (int64_t)k * A * T * D;
  uint8_t* dti_k = dt_ignore + (int64_t)k * A * T * D;
  const int tail = D - Dk;
  for (int e = tid; e < A * T * tail; e += blockDim.x) {
    const int row = e / tail, c = Dk + (e - row * tail);
    dtm_k[(int64_t)row * D + c] = 0;
    dti_k[(int64_t)row * D + c] = 0;
  }
  for (int e = tid; e < A * G; e += blockDim.x) {
    const int a = e / G, pos = e - a * G;
    gt_ignore[((int64_t)k * A + a) * G + pos] = (pos < Gk && pos >= nreg[a]) ? 1 : 0;
  }
  if (tid == 0) {
    counts[2 * k] = Dk;
    counts[2 * k + 1] = Gk;
  }
  // The scan, over chunks of detections whose IoU rows fit the LDS block (one chunk when D_k * G_k <= CM_IOU_LDS; G_k <= 1024, so
  // a chunk holds at least two detections): all threads fill the chunk's block, the scanning threads walk it. Every thread of the
  // workgroup stays for the barriers; Dk, Gk and the chunk are uniform.
  const bool scans = tid < A * T;
  const int a = scans ? tid / T : 0, t = scans ? tid - a * T : 0;
  const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
  const double thr = iou_thrs[t];
  const int n_count = nreg[a];
  uint32_t matched[MI_MAX_PLANES / 32];                 // per position in the scan order: matched at this threshold
  for (int w = 0; w < (Gk + 31) / 32; ++w) matched[w] = 0;
  int32_t* dtm = dtm_k + (int64_t)tid * D;
  uint8_t* dti = dti_k + (int64_t)tid * D;
  const int chunk = Gk > 0 && (int64_t)Dk * Gk > CM_IOU_LDS ? CM_IOU_LDS / Gk : Dk;
  for (int c0 = 0; c0 < Dk; c0 += chunk) {
    const int cn = Dk - c0 < chunk ? Dk - c0 : chunk;
    __syncthreads();                                    // the previous chunk has been scanned (first: dsel .. nreg are written)
    for (int e = tid; e < cn * Gk; e += blockDim.x) {
      const int ci = e / Gk, p = e - ci * Gk;
      iou_lds[e] = src.iou(dsel[c0 + ci], gsel[p], g_key[p], g_crowd[p] != 0);
    }
    __syncthreads();
    if (!scans) continue;
    for (int di = c0; di < c0 + cn; ++di) {
      double best = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
      int m = -1, m_gi = 0;
      bool m_ignored = false;
      const double* row = iou_lds + (di - c0) * Gk;
      // the scan's chain of dependent LDS reads is its cost: the order entry (which carries the crowd flag) is read one step ahead,
      // and the matched bits go by scan position, which all lanes share
      uint32_t o_next = Gk > 0 ? ord[a][0] : 0;
      for (int gi = 0; gi < Gk; ++gi) {
        const uint32_t o = o_next;
        o_next = ord[a][gi + 1 < Gk ? gi + 1 : gi];
        const bool ignored = gi >= n_count;
        if (ignored && m > -1 && !m_ignored) break;      // matched one that counts: the ignored ones are not scanned
        if (((matched[gi >> 5] >> (gi & 31)) & 1u) && !(o & 0x8000u)) continue;      // (matched and not crowd)
        const int p = (int)(o & 0x7fffu);
        const double v = row[p];
        if (v < best) continue;
        best = v;
        m = p;
        m_gi = gi;
        m_ignored = ignored;
      }
      if (m > -1) {
        matched[m_gi >> 5] |= 1u << (m_gi & 31);
        dtm[di] = (int32_t)gsel[m] + 1;
        dti[di] = m_ignored ? 1 : 0;
      } else {
        const double da = src.det_area(dsel[di]);
        dtm[di] = 0;
        dti[di] = (da < lo || da > hi) ? 1 : 0;
      }
    }
  }
}

// iou[d][g] and area_d[d] of cgg_box_iou_f64: one thread per pair (per detection when G = 0), the arithmetic of the matcher
constexpr int BI_THREADS = 256;

__global__ __launch_bounds__(BI_THREADS) void cgg_box_iou_kernel(const float* __restrict__ det5, int D, const double* __restrict__ gt4,
                                                                 const uint8_t* __restrict__ gt_crowd, int G, double* __restrict__ iou,
                                                                 double* __restrict__ area_d) {
  const int e = blockIdx.x * BI_THREADS + threadIdx.x;
  const int gn = G > 0 ? G : 1;
  if (e >= D * gn) return;
  const int d = e / gn, g = e - d * gn;
  const CmBoxIou src{det5, gt4};
  if (g == 0) area_d[d] = src.det_area(d);
  if (G > 0) iou[(int64_t)d * G + g] = src.iou(d, g, 0, gt_crowd[g] != 0);
}

}  // namespace

extern "C" int64_t cgg_mask_intersections_workspace_bytes(int D, int G, int H, int W) {
  if (D < 0 || G < 0 || H <= 0 || W <= 0 || D > MI_MAX_PLANES || G > MI_MAX_PLANES || (D == 0 && G == 0)) return 0;
  return (int64_t)mi_cap(D, G) * ((int64_t)D * G + D + G) * 4;
}

extern "C" int cgg_mask_intersections_bits(const uint8_t* det_bits, int D, int64_t det_stride_bytes, const uint8_t* gt_bits, int G,
                                           int64_t gt_stride_bytes, int H, int W, int row_bytes, void* ws, int32_t* inter,
                                           int32_t* area_d, int32_t* area_g, cgg_stream_t stream) {
  CGG_REQUIRE(D >= 0 && G >= 0 && H > 0 && W > 0 && row_bytes > 0 && (int64_t)row_bytes * 8 >= W, CGG_EINVAL,
              "cgg_mask_intersections_bits: bad sizes (D=%d G=%d H=%d W=%d row_bytes=%d)", D, G, H, W, row_bytes);
  CGG_REQUIRE(det_stride_bytes >= (int64_t)H * row_bytes && gt_stride_bytes >= (int64_t)H * row_bytes, CGG_EINVAL,
              "cgg_mask_intersections_bits: plane strides %lld / %lld below H * row_bytes = %lld", (long long)det_stride_bytes,
              (long long)gt_stride_bytes, (long long)H * row_bytes);
  CGG_REQUIRE(D <= MI_MAX_PLANES && G <= MI_MAX_PLANES, CGG_EUNSUPPORTED, "cgg_mask_intersections_bits: D=%d / G=%d above %d", D, G,
              MI_MAX_PLANES);
  CGG_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CGG_EUNSUPPORTED, "cgg_mask_intersections_bits: H * W = %lld does not fit 31 bits",
              (long long)H * W);
  CGG_REQUIRE((D == 0 || (det_bits && area_d)) && (G == 0 || (gt_bits && area_g)) && ((D == 0 && G == 0) || ws) &&
                  (D == 0 || G == 0 || inter),
              CGG_EINVAL, "cgg_mask_intersections_bits: null pointer");
  CGG_REQUIRE((((uintptr_t)ws) & 3u) == 0 && (((uintptr_t)inter) & 3u) == 0 && (((uintptr_t)area_d) & 3u) == 0 &&
                  (((uintptr_t)area_g) & 3u) == 0,
              CGG_EINVAL, "cgg_mask_intersections_bits: ws / inter / area_d / area_g must be 4-byte aligned");
  if (D == 0 && G == 0) return CGG_OK;
  const MiGeom geom = mi_geom(D, G, H, row_bytes);
  CGG_REQUIRE((int64_t)((H + geom.R - 1) / geom.R) * geom.nchunks <= (int64_t)0x7fffffff, CGG_EUNSUPPORTED,
              "cgg_mask_intersections_bits: too many slabs (H=%d row_bytes=%d)", H, row_bytes);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)2 * MI_BLOCK * MI_STRIDE_WORDS * sizeof(uint32_t);
  CGG_RAISE_LDS(cgg_mi_partial_kernel, lds, "cgg_mask_intersections_bits");
  hipLaunchKernelGGL(cgg_mi_partial_kernel, dim3(geom.nsg, geom.db, geom.gb), dim3(MI_THREADS), lds, s, det_bits, D, det_stride_bytes,
                     gt_bits, G, gt_stride_bytes, H, W, row_bytes, geom, D > 0 ? mi_load_mode(det_bits, det_stride_bytes, row_bytes) : 1,
                     G > 0 ? mi_load_mode(gt_bits, gt_stride_bytes, row_bytes) : 1, (int32_t*)ws);
  CGG_CHECK_LAUNCH("cgg_mask_intersections_bits(partial)");
  const int64_t N = (int64_t)D * G + D + G;
  hipLaunchKernelGGL(cgg_mi_reduce_kernel, dim3((unsigned)((N + MR_ELEMS - 1) / MR_ELEMS)), dim3(MR_ELEMS * MR_SUB), 0, s,
                     (const int32_t*)ws, geom.nsg, D, G, inter, area_d, area_g);
  CGG_CHECK_LAUNCH("cgg_mask_intersections_bits(reduce)");
  return CGG_OK;
}

extern "C" int cgg_coco_match(const int32_t* inter, const int32_t* area_d, const int32_t* area_g, const int32_t* det_order,
                              const int32_t* det_cats, const int32_t* gt_cats, const uint8_t* gt_crowd, const double* gt_area,
                              const int32_t* cat_ids, int K, const double* area_rngs, int A, const double* iou_thrs, int T, int D,
                              int G, int max_det, int class_agnostic, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore,
                              int32_t* counts, cgg_stream_t stream) {
  CGG_REQUIRE(D >= 0 && G >= 0 && K >= 1 && A >= 1 && T >= 1 && max_det >= 0, CGG_EINVAL,
              "cgg_coco_match: bad sizes (D=%d G=%d K=%d A=%d T=%d max_det=%d)", D, G, K, A, T, max_det);
  CGG_REQUIRE(T <= CM_MAX_T && A <= CM_MAX_A && K <= CM_MAX_K && D <= MI_MAX_PLANES && G <= MI_MAX_PLANES, CGG_EUNSUPPORTED,
              "cgg_coco_match: T=%d A=%d K=%d D=%d G=%d above %d / %d / %d / %d / %d", T, A, K, D, G, CM_MAX_T, CM_MAX_A, CM_MAX_K,
              MI_MAX_PLANES, MI_MAX_PLANES);
  CGG_REQUIRE(cat_ids && area_rngs && iou_thrs && counts && (D == 0 || (area_d && det_order && det_cats && dt_match && dt_ignore)) &&
                  (G == 0 || (area_g && gt_cats && gt_crowd && gt_area && gt_ignore)) && (D == 0 || G == 0 || inter),
              CGG_EINVAL, "cgg_coco_match: null pointer");
  CGG_REQUIRE((((uintptr_t)gt_area | (uintptr_t)area_rngs | (uintptr_t)iou_thrs) & 7u) == 0, CGG_EINVAL,
              "cgg_coco_match: gt_area / area_rngs / iou_thrs must be 8-byte aligned");
  const int threads = ((A * T + 63) / 64) * 64;         // one thread per (area range, threshold), whole waves
  hipLaunchKernelGGL(cgg_coco_match_kernel<CmMaskIou>, dim3((unsigned)K), dim3(threads), 0, (hipStream_t)stream,
                     CmMaskIou{inter, area_d, area_g, G}, det_order, det_cats, gt_cats, gt_crowd, gt_area, cat_ids, K, area_rngs, A,
                     iou_thrs, T, D, G, max_det, class_agnostic, dt_match, dt_ignore, gt_ignore, counts);
  CGG_CHECK_LAUNCH("cgg_coco_match");
  return CGG_OK;
}

extern "C" int cgg_box_iou_f64(const float* det_boxes5, int D, const double* gt_boxes_xywh, const uint8_t* gt_crowd, int G, double* iou,
                               double* area_d, cgg_stream_t stream) {
  CGG_REQUIRE(D >= 0 && G >= 0, CGG_EINVAL, "cgg_box_iou_f64: bad sizes (D=%d G=%d)", D, G);
  CGG_REQUIRE(D <= MI_MAX_PLANES && G <= MI_MAX_PLANES, CGG_EUNSUPPORTED, "cgg_box_iou_f64: D=%d / G=%d above %d", D, G, MI_MAX_PLANES);
  CGG_REQUIRE((D == 0 || (det_boxes5 && area_d)) && (G == 0 || (gt_boxes_xywh && gt_crowd)) && (D == 0 || G == 0 || iou), CGG_EINVAL,
              "cgg_box_iou_f64: null pointer");
  CGG_REQUIRE((((uintptr_t)det_boxes5) & 3u) == 0 && (((uintptr_t)gt_boxes_xywh | (uintptr_t)iou | (uintptr_t)area_d) & 7u) == 0,
              CGG_EINVAL, "cgg_box_iou_f64: det_boxes5 must be 4-byte, gt_boxes_xywh / iou / area_d 8-byte aligned");
  if (D == 0) return CGG_OK;
  const int n = D * (G > 0 ? G : 1);                    // (<= 2^20)
  hipLaunchKernelGGL(cgg_box_iou_kernel, dim3((unsigned)((n + BI_THREADS - 1) / BI_THREADS)), dim3(BI_THREADS), 0, (hipStream_t)stream,
                     det_boxes5, D, gt_boxes_xywh, gt_crowd, G, iou, area_d);
  CGG_CHECK_LAUNCH("cgg_box_iou_f64");
  return CGG_OK;
}

extern "C" int cgg_coco_match_boxes(const float* det_boxes5, const double* gt_boxes_xywh, const int32_t* det_order,
                                    const int32_t* det_cats, const int32_t* gt_cats, const uint8_t* gt_crowd, const double* gt_area,
                                    const int32_t* cat_ids, int K, const double* area_rngs, int A, const double* iou_thrs, int T, int D,
                                    int G, int max_det, int class_agnostic, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore,
                                    int32_t* counts, cgg_stream_t stream) {
  CGG_REQUIRE(D >= 0 && G >= 0 && K >= 1 && A >= 1 && T >= 1 && max_det >= 0, CGG_EINVAL,
              "cgg_coco_match_boxes: bad sizes (D=%d G=%d K=%d A=%d T=%d max_det=%d)", D, G, K, A, T, max_det);
  CGG_REQUIRE(T <= CM_MAX_T && A <= CM_MAX_A && K <= CM_MAX_K && D <= MI_MAX_PLANES && G <= MI_MAX_PLANES, CGG_EUNSUPPORTED,
              "cgg_coco_match_boxes: T=%d A=%d K=%d D=%d G=%d above %d / %d / %d / %d / %d", T, A, K, D, G, CM_MAX_T, CM_MAX_A, CM_MAX_K,
              MI_MAX_PLANES, MI_MAX_PLANES);
  CGG_REQUIRE(cat_ids && area_rngs && iou_thrs && counts && (D == 0 || (det_boxes5 && det_order && det_cats && dt_match && dt_ignore)) &&
                  (G == 0 || (gt_boxes_xywh && gt_cats && gt_crowd && gt_area && gt_ignore)),
              CGG_EINVAL, "cgg_coco_match_boxes: null pointer");
  CGG_REQUIRE((((uintptr_t)det_boxes5) & 3u) == 0 &&
                  (((uintptr_t)gt_boxes_xywh | (uintptr_t)gt_area | (uintptr_t)area_rngs | (uintptr_t)iou_thrs) & 7u) == 0,
              CGG_EINVAL, "cgg_coco_match_boxes: det_boxes5 must be 4-byte, gt_boxes_xywh / gt_area / area_rngs / iou_thrs 8-byte aligned");
  const int threads = ((A * T + 63) / 64) * 64;
  hipLaunchKernelGGL(cgg_coco_match_kernel<CmBoxIou>, dim3((unsigned)K), dim3(threads), 0, (hipStream_t)stream,
                     CmBoxIou{det_boxes5, gt_boxes_xywh}, det_order, det_cats, gt_cats, gt_crowd, gt_area, cat_ids, K, area_rngs, A,
                     iou_thrs, T, D, G, max_det, class_agnostic, dt_match, dt_ignore, gt_ignore, counts);
  CGG_CHECK_LAUNCH("cgg_coco_match_boxes");
  return CGG_OK;
}
