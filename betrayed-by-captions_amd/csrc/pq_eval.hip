// Panoptic-quality evaluation on id maps (pq_eval.py states the rules in numpy; the kernels equal `pq_image_host` exactly).
//
//   cgg_pq_confusion_i32   the confusion counts of one image: conf[g][p] = pixels whose ground-truth id has slot g and whose pred
//     value has slot p. Rows: 0 = VOID (id 0), 1 .. G = the staged ids in their order, G + 1 = an id that is not listed (the rule
//     skips it, and it is NOT void: only id 0 is subtracted from a union). Columns: 0 = void, 1 .. P = the rows of the pred
//     segment table; a row that is dropped (beyond *n_kept, value < 0, area <= 0) or repeats an earlier value owns no pixels: equal
//     values count into the first row of that value. Each workgroup builds both id -> slot tables in LDS (open addressing, the
//     slot of a key settled by an integer minimum, so it does not depend on the order of arrival), walks its share of the
//     pixels four at a time (16-byte loads of the int32 maps, three 4-byte loads of four RGB pixels), keeps a one-entry "same id
//     as the previous pixel" cache per lane and counts into an LDS table with LDS integer atomics -- one add per wave where all
//     its pixels fall into one cell, which is the common case inside a segment. The non-zero cells are then added to the global
//     table with integer atomics; a first launch zeroes that table (no memset node). Integer sums: bit-identical run to run.
//   cgg_pq_match   matching, false negatives' and false positives' inputs for one image, one workgroup: a thread per pred slot
//     (column sums = recounted areas), a thread per ground-truth slot (its match), a thread per pred slot again (ignored or not).
#include <limits.h>

#include "cgg_common.h"

namespace {

constexpr int PQ_THREADS = 256;
constexpr int PQ_MAX_SLOTS = CGG_PQ_EVAL_MAX_SEGMENTS;
constexpr int PQ_MAX_GROUPS = 256;
constexpr int PQ_INSTANCE_OFFSET = 1000;  // [3P] mmdet.core.evaluation.panoptic_utils.INSTANCE_OFFSET

inline int pq_hash_size(int n) {
  int s = 16;
  while (s < 2 * n) s *= 2;
  return s;
}

inline int64_t pq_lds_bytes(int G, int P) {
  return 4 * ((int64_t)(G + 2) * (P + 1)) + 8 * (int64_t)pq_hash_size(G) + 8 * (int64_t)pq_hash_size(P);
}

__global__ __launch_bounds__(PQ_THREADS) void cgg_pq_zero_kernel(int32_t* __restrict__ conf, int cells, int32_t* __restrict__ status) {
  const int i = blockIdx.x * PQ_THREADS + threadIdx.x;
  if (i < cells) conf[i] = 0;
  if (i == 0) {
    status[0] = 0;
    status[1] = INT_MAX;      // the smallest offending pred value
  }
}

// key -> slot in an open-addressing table of `size` (a power of two) entries, -1 when the key is absent
__device__ __forceinline__ int pq_find(const int32_t* key, const int32_t* slot, int mask, int id) {
  if (id < 0) return -1;                  // (-1 marks an empty entry)
  int h = id & mask;
  while (true) {
    const int k = key[h];
    if (k == id) return slot[h];
    if (k == -1) return -1;               // at most half of the entries are used: the probe ends
    h = (h + 1) & mask;
  }
}

__device__ __forceinline__ void pq_insert(int32_t* key, int32_t* slot, int mask, int id, int s) {
  int h = id & mask;
  while (true) {
    const int old = atomicCAS(&key[h], -1, id);
    if (old == -1 || old == id) {
      atomicMin(&slot[h], s);
      return;
    }
    h = (h + 1) & mask;
  }
}

struct PqLookup {
  const int32_t *gkey, *gslot, *pkey, *pslot;
  int gmask, pmask, G, C, num_classes;
  int32_t* status;
  int last_gid, last_g, last_pv, last_p;

  // confusion cell of one pixel
  __device__ __forceinline__ int cell(int gid, int pv) {
    if (gid != last_gid) {
      last_gid = gid;
      const int s = pq_find(gkey, gslot, gmask, gid);
      last_g = s >= 0 ? s : (gid == 0 ? 0 : G + 1);
    }
    if (pv != last_pv) {
      last_pv = pv;
      int s = 0;
      if (pv < 0 || pv % PQ_INSTANCE_OFFSET != num_classes) {
        s = pq_find(pkey, pslot, pmask, pv);
        if (s < 0) {
          s = 0;
          if (pv != 0) {                  // neither listed nor void
            atomicOr(&status[0], 1);
            atomicMin(&status[1], pv);
          }
        }
      }
      last_p = s;
    }
    return last_g * C + last_p;
  }
};

template <bool RGB>
__device__ __forceinline__ int pq_gt_id(const void* gt, int64_t i) {
  if (RGB) {
    const uint8_t* b = (const uint8_t*)gt + 3 * i;
    return (int)b[0] | ((int)b[1] << 8) | ((int)b[2] << 16);
  }
  return ((const int32_t*)gt)[i];
}

template <bool RGB>
__global__ __launch_bounds__(PQ_THREADS) void cgg_pq_confusion_kernel(const int32_t* __restrict__ pred, const void* __restrict__ gt,
                                                                      int64_t n, const int32_t* __restrict__ gt_ids, int G,
                                                                      const int32_t* __restrict__ table,
                                                                      const int32_t* __restrict__ n_kept_ptr, int P, int num_classes,
                                                                      int HG, int HP, int pred_wide, int gt_wide,
                                                                      int32_t* __restrict__ conf, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) int32_t pq_lds[];
  const int R = G + 2, C = P + 1, cells = R * C;
  int32_t* lconf = pq_lds;
  int32_t* gkey = lconf + cells;
  int32_t* gslot = gkey + HG;
  int32_t* pkey = gslot + HG;
  int32_t* pslot = pkey + HP;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < cells; i += PQ_THREADS) lconf[i] = 0;
  for (int i = tid; i < HG; i += PQ_THREADS) {
    gkey[i] = -1;
    gslot[i] = INT_MAX;
  }
  for (int i = tid; i < HP; i += PQ_THREADS) {
    pkey[i] = -1;
    pslot[i] = INT_MAX;
  }
  __syncthreads();
  for (int i = tid; i < G; i += PQ_THREADS) {
    const int id = gt_ids[i];
    if (id >= 0) pq_insert(gkey, gslot, HG - 1, id, i + 1);
  }
  int n_kept = *n_kept_ptr;
  n_kept = n_kept < 0 ? 0 : (n_kept > P ? P : n_kept);
  for (int k = tid; k < n_kept; k += PQ_THREADS) {
    const int value = table[4 * k], area = table[4 * k + 2];
    if (value >= 0 && area > 0) pq_insert(pkey, pslot, HP - 1, value, k + 1);
  }
  __syncthreads();
  PqLookup look{gkey, gslot, pkey, pslot, HG - 1, HP - 1, G, C, num_classes, status, -1, 0, INT_MIN, 0};
  const int64_t nvec = n >> 2;
  for (int64_t v0 = (int64_t)blockIdx.x * PQ_THREADS + (tid - lane); v0 < nvec; v0 += (int64_t)gridDim.x * PQ_THREADS) {
    const int64_t v = v0 + lane;
    const bool active = v < nvec;
    int pv[4] = {0, 0, 0, 0}, gid[4] = {0, 0, 0, 0};
    if (active) {
      if (pred_wide) {
        const u32x4 q = *(const u32x4*)(pred + 4 * v);
        pv[0] = (int)q.x, pv[1] = (int)q.y, pv[2] = (int)q.z, pv[3] = (int)q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] = pred[4 * v + j];
      }
      if (RGB && gt_wide) {               // four pixels = twelve bytes = three aligned words
        const uint32_t* w = (const uint32_t*)gt + 3 * v;
        const uint32_t a = w[0], b = w[1], c = w[2];
        gid[0] = (int)(a & 0xffffffu);
        gid[1] = (int)((a >> 24) | ((b & 0xffffu) << 8));
        gid[2] = (int)((b >> 16) | ((c & 0xffu) << 16));
        gid[3] = (int)(c >> 8);
      } else if (!RGB && gt_wide) {
        const u32x4 q = *(const u32x4*)((const int32_t*)gt + 4 * v);
        gid[0] = (int)q.x, gid[1] = (int)q.y, gid[2] = (int)q.z, gid[3] = (int)q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) gid[j] = pq_gt_id<RGB>(gt, 4 * v + j);
      }
    }
    int key[4] = {0, 0, 0, 0};
    if (active) {
#pragma unroll
      for (int j = 0; j < 4; ++j) key[j] = look.cell(gid[j], pv[j]);
    }
    const bool single = key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
    const int first = __builtin_amdgcn_readfirstlane(key[0]);      // (lane 0 is active whenever any lane is)
    const uint64_t act = __ballot(active);
    const uint64_t same = __ballot(active && single && key[0] == first);
    if (same == act) {
      if (lane == 0) atomicAdd(&lconf[first], 4 * __popcll(act));
    } else if (active) {
      int cnt = 1;
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        if (key[j] == key[j - 1]) {
          ++cnt;
        } else {
          atomicAdd(&lconf[key[j - 1]], cnt);
          cnt = 1;
        }
      }
      atomicAdd(&lconf[key[3]], cnt);
    }
  }
  if (blockIdx.x == 0 && tid < (int)(n & 3)) {        // the pixels past the last group of four
    const int64_t i = (nvec << 2) + tid;
    atomicAdd(&lconf[look.cell(pq_gt_id<RGB>(gt, i), pred[i])], 1);
  }
  __syncthreads();
  for (int i = tid; i < cells; i += PQ_THREADS) {
    const int c = lconf[i];
    if (c) atomicAdd(&conf[i], c);
  }
}

__global__ __launch_bounds__(PQ_THREADS) void cgg_pq_match_kernel(const int32_t* __restrict__ conf, const int32_t* __restrict__ ws_status,
                                                                  const int32_t* __restrict__ gt_cats, const uint8_t* __restrict__ gt_crowd,
                                                                  const int32_t* __restrict__ gt_area, int G,
                                                                  const int32_t* __restrict__ table, const int32_t* __restrict__ n_kept_ptr,
                                                                  int P, int32_t* __restrict__ status, double* __restrict__ gt_iou,
                                                                  int32_t* __restrict__ gt_match, int32_t* __restrict__ pred_area,
                                                                  int32_t* __restrict__ pred_value, int32_t* __restrict__ pred_cat,
                                                                  uint8_t* __restrict__ pred_flags) {
  __shared__ int32_t pflag[PQ_MAX_SLOTS];              // 1 = a segment, 2 = matched, 4 = ignored
  __shared__ int32_t parea[PQ_MAX_SLOTS];
  __shared__ int32_t pcat[PQ_MAX_SLOTS];
  __shared__ int32_t bits;
  const int tid = threadIdx.x;
  const int R = G + 2, C = P + 1;
  int n_kept = *n_kept_ptr;
  n_kept = n_kept < 0 ? 0 : (n_kept > P ? P : n_kept);
  if (tid == 0) bits = 0;
  __syncthreads();
  for (int k = tid; k < P; k += PQ_THREADS) {
    const int value = table[4 * k];
    bool valid = k < n_kept && value >= 0 && table[4 * k + 2] > 0;
    for (int j = 0; valid && j < k; ++j)               // an earlier row of the same value owns the pixels
      if (table[4 * j] == value && table[4 * j + 2] > 0) valid = false;
    int32_t a = 0;
    if (valid)
      for (int r = 0; r < R; ++r) a += conf[r * C + k + 1];
    pflag[k] = valid ? 1 : 0;
    parea[k] = a;
    pcat[k] = table[4 * k + 1];
    if (valid && a == 0) atomicOr(&bits, 2);
  }
  __syncthreads();
  for (int g = tid; g < G; g += PQ_THREADS) {
    int m = -1, nm = 0;
    double miou = 0.0;
    if (!gt_crowd[g]) {
      const int cat = gt_cats[g];
      const int64_t ag = gt_area[g];
      for (int k = 0; k < P; ++k) {
        if (!(pflag[k] & 1) || pcat[k] != cat) continue;
        const int64_t inter = conf[(g + 1) * C + k + 1];
        if (inter <= 0) continue;
        const int64_t un = (int64_t)parea[k] + ag - inter - (int64_t)conf[k + 1];
        const double iou = (double)inter / (double)un;
        if (iou > 0.5) {
          if (nm == 0) {
            m = k;
            miou = iou;
          }
          ++nm;
          atomicOr(&pflag[k], 2);
        }
      }
    }
    if (nm > 1) atomicOr(&bits, 4);
    gt_match[g] = m;
    gt_iou[g] = miou;
  }
  __syncthreads();
  for (int k = tid; k < P; k += PQ_THREADS) {
    int f = pflag[k];
    if ((f & 1) && !(f & 2)) {
      int crowd = -1;                                  // the last crowd of this category in record order
      for (int g = G - 1; g >= 0; --g)
        if (gt_crowd[g] && gt_cats[g] == pcat[k]) {
          crowd = g;
          break;
        }
      int64_t inter = conf[k + 1];
      if (crowd >= 0) inter += conf[(crowd + 1) * C + k + 1];
      if ((double)inter / (double)parea[k] > 0.5) f |= 4;
    }
    pred_flags[k] = (uint8_t)f;
    pred_area[k] = parea[k];
    pred_value[k] = (f & 1) ? table[4 * k] : -1;
    pred_cat[k] = pcat[k];
  }
  if (tid == 0) {
    status[0] = ws_status[0] | bits;
    status[1] = ws_status[1];
  }
}

inline int pq_check_sizes(const char* who, int G, int P) {
  CGG_REQUIRE(G >= 0 && P >= 0, CGG_EINVAL, "%s: bad sizes (G=%d P=%d)", who, G, P);
  CGG_REQUIRE(G <= PQ_MAX_SLOTS && P <= PQ_MAX_SLOTS, CGG_EUNSUPPORTED, "%s: G=%d / P=%d above %d", who, G, P, PQ_MAX_SLOTS);
  CGG_REQUIRE(pq_lds_bytes(G, P) <= cgg_dynamic_lds_limit(), CGG_EUNSUPPORTED,
              "%s: the confusion table of G=%d x P=%d and both id tables need %lld bytes of LDS, above %lld", who, G, P,
              (long long)pq_lds_bytes(G, P), (long long)cgg_dynamic_lds_limit());
  return CGG_OK;
}

}  // namespace

extern "C" int64_t cgg_pq_eval_lds_bytes(int G, int P) {
  if (G < 0 || P < 0 || G > PQ_MAX_SLOTS || P > PQ_MAX_SLOTS) return -1;
  return pq_lds_bytes(G, P);
}

extern "C" int64_t cgg_pq_confusion_workspace_bytes(int G, int P) {
  if (G < 0 || P < 0) return 0;
  return 4 * ((int64_t)(G + 2) * (P + 1) + 2);
}

extern "C" int cgg_pq_confusion_i32(const int32_t* pred, const void* gt, int gt_rgb, int H, int W, const int32_t* gt_ids, int G,
                                    const int32_t* table, const int32_t* n_kept, int P, int num_classes, int32_t* ws,
                                    cgg_stream_t stream) {
  const char* who = "cgg_pq_confusion_i32";
  CGG_REQUIRE(H > 0 && W > 0 && num_classes >= 0 && (gt_rgb == 0 || gt_rgb == 1), CGG_EINVAL,
              "%s: bad sizes (H=%d W=%d num_classes=%d gt_rgb=%d)", who, H, W, num_classes, gt_rgb);
  const int rc = pq_check_sizes(who, G, P);
  if (rc != CGG_OK) return rc;
  CGG_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CGG_EUNSUPPORTED, "%s: H * W = %lld does not fit 31 bits", who, (long long)H * W);
  CGG_REQUIRE(pred && gt && n_kept && ws && (G == 0 || gt_ids) && (P == 0 || table), CGG_EINVAL, "%s: null pointer", who);
  CGG_REQUIRE((((uintptr_t)pred | (uintptr_t)gt_ids | (uintptr_t)table | (uintptr_t)n_kept | (uintptr_t)ws) & 3u) == 0 &&
                  (gt_rgb || (((uintptr_t)gt) & 3u) == 0),
              CGG_EINVAL, "%s: int32 operands must be 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int cells = (G + 2) * (P + 1);
  int32_t* status = ws + cells;
  hipLaunchKernelGGL(cgg_pq_zero_kernel, dim3((unsigned)((cells + PQ_THREADS - 1) / PQ_THREADS)), dim3(PQ_THREADS), 0, s, ws, cells, status);
  CGG_CHECK_LAUNCH("cgg_pq_confusion_i32(zero)");
  const int64_t n = (int64_t)H * W, nvec = n >> 2;
  int64_t groups = (nvec + PQ_THREADS - 1) / PQ_THREADS;
  groups = groups < 1 ? 1 : (groups > PQ_MAX_GROUPS ? PQ_MAX_GROUPS : groups);
  const int HG = pq_hash_size(G), HP = pq_hash_size(P);
  const size_t lds = (size_t)pq_lds_bytes(G, P);
  const int pred_wide = cgg_aligned16(pred) ? 1 : 0;
  const int gt_wide = gt_rgb ? ((((uintptr_t)gt) & 3u) == 0 ? 1 : 0) : (cgg_aligned16(gt) ? 1 : 0);
  if (gt_rgb) {
    CGG_RAISE_LDS(cgg_pq_confusion_kernel<true>, lds, who);
    hipLaunchKernelGGL(cgg_pq_confusion_kernel<true>, dim3((unsigned)groups), dim3(PQ_THREADS), lds, s, pred, gt, n, gt_ids, G, table, n_kept,
                       P, num_classes, HG, HP, pred_wide, gt_wide, ws, status);
  } else {
    CGG_RAISE_LDS(cgg_pq_confusion_kernel<false>, lds, who);
    hipLaunchKernelGGL(cgg_pq_confusion_kernel<false>, dim3((unsigned)groups), dim3(PQ_THREADS), lds, s, pred, gt, n, gt_ids, G, table, n_kept,
                       P, num_classes, HG, HP, pred_wide, gt_wide, ws, status);
  }
  CGG_CHECK_LAUNCH("cgg_pq_confusion_i32");
  return CGG_OK;
}

extern "C" int cgg_pq_match(const int32_t* ws, const int32_t* gt_cats, const uint8_t* gt_crowd, const int32_t* gt_area, int G,
                            const int32_t* table, const int32_t* n_kept, int P, int32_t* status, double* gt_iou, int32_t* gt_match,
                            int32_t* pred_area, int32_t* pred_value, int32_t* pred_cat, uint8_t* pred_flags, cgg_stream_t stream) {
  const char* who = "cgg_pq_match";
  const int rc = pq_check_sizes(who, G, P);
  if (rc != CGG_OK) return rc;
  CGG_REQUIRE(ws && n_kept && status && (G == 0 || (gt_cats && gt_crowd && gt_area && gt_iou && gt_match)) &&
                  (P == 0 || (table && pred_area && pred_value && pred_cat && pred_flags)),
              CGG_EINVAL, "%s: null pointer", who);
  CGG_REQUIRE((((uintptr_t)gt_iou) & 7u) == 0, CGG_EINVAL, "%s: gt_iou must be 8-byte aligned", who);
  const int32_t* ws_status = ws + (G + 2) * (P + 1);
  hipLaunchKernelGGL(cgg_pq_match_kernel, dim3(1), dim3(PQ_THREADS), 0, (hipStream_t)stream, ws, ws_status, gt_cats, gt_crowd, gt_area, G, table,
                     n_kept, P, status, gt_iou, gt_match, pred_area, pred_value, pred_cat, pred_flags);
  CGG_CHECK_LAUNCH("cgg_pq_match");
  return CGG_OK;
}
