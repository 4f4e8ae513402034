// Batched panoptic fusion (open_set/models/maskformer_fusion_head.py:77-225) without a host read: which queries are
// kept, the per-pixel argmax, the segment decisions and the painted map of a whole batch in four launches whose
// data-dependent sizes are read from device memory, so a captured graph replays them on new data.
//   select : keep = label != num_classes && score > thr, compacted in query order (one wave per image)
//   argmax : a block owns a 32 x 16 tile of output pixels; the low-resolution samples the tile's taps can touch are
//            staged in LDS for a chunk of kept queries, every pixel then evaluates cgg_panoptic_argmax_kernel's
//            expressions (resize_taps.h) on that window
//   decide : `maskformer_fusion_head.panoptic_decide_host` on the three counters per kept query (one wave per image)
//   paint  : cgg_panoptic_paint_kernel's rule per image; void everywhere when nothing was kept
// The written rule is `panoptic_decide_host` (Python); cgg_panoptic_argmax / cgg_panoptic_paint are the comparison side.
#include "cgg_common.h"
#include "resize_taps.h"

#define PF_TW 32                 // tile width  (output pixels)
#define PF_TH 16                 // tile height
#define PF_PPT 2                 // pixels per thread: rows ly and ly + 8 of the tile
#define PF_STAGE_FLOATS 8192     // LDS window for one chunk of queries (32 KB)
#define PF_MIN_CHUNK 8           // a footprint that leaves room for fewer queries per chunk reads global memory instead
#define PF_MAX_Q CGG_PANOPTIC_FUSE_MAX_Q
#define PF_GEOM_COLS 5           // geometry row: crop_h, crop_w, out_h, out_w, pixel offset into the flat map
static_assert(PF_TW * PF_TH == 256 * PF_PPT, "one block covers its tile");
static_assert(sizeof(int32_t) * 3 * PF_MAX_Q + sizeof(float) * PF_STAGE_FLOATS <= 64 * 1024,
              "two blocks per CU: histogram + window within 64 KB");

struct PfImage {
  int crop_h, crop_w, out_h, out_w;
  long long off;
  bool ok;
};
// one image's row of the device geometry table; `ok` is false for a row the kernels must not act on (they exit, so a
// bad table can leave pixels unwritten but never writes outside the flat map or reads outside the logits)
__device__ __forceinline__ PfImage pf_image(const int64_t* __restrict__ geom, int b, int up_h, int up_w,
                                            int max_out_h, int max_out_w, long long total) {
  const int64_t* r = geom + (size_t)b * PF_GEOM_COLS;
  PfImage im;
  const long long ch = r[0], cw = r[1], oh = r[2], ow = r[3];
  im.off = r[4];
  im.ok = ch > 0 && ch <= up_h && cw > 0 && cw <= up_w && oh > 0 && oh <= max_out_h && ow > 0 && ow <= max_out_w &&
          im.off >= 0 && im.off <= total && oh * ow <= total - im.off;
  im.crop_h = (int)ch; im.crop_w = (int)cw; im.out_h = (int)oh; im.out_w = (int)ow;
  return im;
}

// ---- select ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cgg_pf_select_kernel(const float* __restrict__ score,
                                                           const int64_t* __restrict__ label,
                                                           int32_t* __restrict__ keep_idx, float* __restrict__ kscore,
                                                           int32_t* __restrict__ kclass, int32_t* __restrict__ n_kept,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ stats,
                                                           int Q, int num_classes, float thr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * Q;
  // the image's counters start at zero: this launch precedes the argmax in stream order
  for (int i = lane; i < 3 * Q; i += 64) counts[row * 3 + i] = 0;
  if (lane < 2) stats[b * 2 + lane] = 0;
  int base = 0;                                            // kept queries before this chunk (wave-uniform)
  for (int q0 = 0; q0 < Q; q0 += 64) {
    const int q = q0 + lane;
    float sc = 0.f;
    int64_t lb = num_classes;
    if (q < Q) { sc = score[row + q]; lb = label[row + q]; }
    const bool keep = q < Q && lb != (int64_t)num_classes && sc > thr;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int k = base + __popcll(m & ((1ull << lane) - 1ull));
      keep_idx[row + k] = q;
      kscore[row + k] = sc;
      kclass[row + k] = (int)lb;
    }
    base += __popcll(m);
  }
  for (int k = base + lane; k < Q; k += 64) {              // unused slots: fixed values, whatever an earlier replay kept
    keep_idx[row + k] = 0;
    kscore[row + k] = 0.f;
    kclass[row + k] = -1;
  }
  if (lane == 0) n_kept[b] = base;
}

// ---- argmax ------------------------------------------------------------------------------------------------------
// queries k0 .. k0 + kc of one image at this thread's pixels; `src_of(k)` gives query k's sample source
template <class SrcOf>
__device__ __forceinline__ void pf_scan(const SrcOf& src_of, int k0, int kc, const float* __restrict__ kscore,
                                        const ResizeGeom& g, const int (&oy)[PF_PPT], const int (&ox)[PF_PPT],
                                        const bool (&valid)[PF_PPT], float (&best)[PF_PPT], int (&bk)[PF_PPT],
                                        bool (&bhalf)[PF_PPT], int32_t* hist) {
  const int lane = threadIdx.x & 63;
  for (int k = k0; k < k0 + kc; ++k) {
    const float sc = kscore[k];
    const auto src = src_of(k);
#pragma unroll
    for (int j = 0; j < PF_PPT; ++j) {
      bool half = false;
      if (valid[j]) {
        const float v = cgg_resized_logit_at(src, g, oy[j], ox[j]);
        const float sg = cgg_sigmoid(v);
        half = sg >= 0.5f;
        const float pv = sc * sg;
        if (pv > best[j]) {
          best[j] = pv;
          bk[j] = k;
          bhalf[j] = half;
        }
      }
      // #(sigmoid_k >= 0.5): every thread of the block is at the same k, so one add per wave instead of one per pixel
      const unsigned long long m = __ballot(half);
      if (lane == 0 && m) atomicAdd(&hist[k * 3 + 1], __popcll(m));
    }
  }
}

__global__ __launch_bounds__(256) void cgg_pf_argmax_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ geom, const int32_t* __restrict__ n_kept,
    const int32_t* __restrict__ keep_idx, const float* __restrict__ kscore, int32_t* __restrict__ idmap,
    int32_t* __restrict__ counts, int32_t* __restrict__ stats, int Q, int H, int W, int up_h, int up_w,
    int max_out_h, int max_out_w, long long total) {
  extern __shared__ int32_t pf_smem[];                     // [3 * Q] histogram | [PF_STAGE_FLOATS] window
  int32_t* hist = pf_smem;
  float* stage = reinterpret_cast<float*>(pf_smem + 3 * Q);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(n_kept[b], Q);
  if (n <= 0) return;                                      // block-uniform; paint writes void
  const PfImage im = pf_image(geom, b, up_h, up_w, max_out_h, max_out_w, total);
  if (!im.ok) return;
  const int tiles_x = (im.out_w + PF_TW - 1) / PF_TW, tiles_y = (im.out_h + PF_TH - 1) / PF_TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;        // grid is sized for the largest image of the batch
  const int ty0 = ((int)blockIdx.x / tiles_x) * PF_TH, tx0 = ((int)blockIdx.x % tiles_x) * PF_TW;
  const ResizeGeom g = make_geom(H, W, up_h, up_w, im.crop_h, im.crop_w, im.out_h, im.out_w);
  const size_t row = (size_t)b * Q;
  const float* lg = logits + row * H * W;
  const int32_t* kidx = keep_idx + row;
  const float* ksc = kscore + row;

  for (int i = tid; i < 3 * n; i += 256) hist[i] = 0;

  // footprint: cgg_bitap's indices are non-decreasing in the output index, so the first pixel's i0 and the last
  // pixel's i1 (through both stages for `rescale`) bound every tap of the tile, clamps included
  const int oy1 = min(ty0 + PF_TH, im.out_h) - 1, ox1 = min(tx0 + PF_TW, im.out_w) - 1;
  int ya = ty0, yb = oy1, xa = tx0, xb = ox1;
  if (g.two_stage) {
    ya = cgg_bitap(ya, g.s2y, g.crop_h).i0; yb = cgg_bitap(yb, g.s2y, g.crop_h).i1;
    xa = cgg_bitap(xa, g.s2x, g.crop_w).i0; xb = cgg_bitap(xb, g.s2x, g.crop_w).i1;
  }
  const int r0 = cgg_bitap(ya, g.s1y, H).i0, r1 = cgg_bitap(yb, g.s1y, H).i1;
  const int c0 = cgg_bitap(xa, g.s1x, W).i0, c1 = cgg_bitap(xb, g.s1x, W).i1;
  const int Fh = r1 - r0 + 1, Fw = c1 - c0 + 1, F = Fh * Fw;
  const bool use_lds = (long long)F * PF_MIN_CHUNK <= PF_STAGE_FLOATS;
  if (tid == 0) atomicAdd(&stats[b * 2 + (use_lds ? 0 : 1)], 1);

  int oy[PF_PPT], ox[PF_PPT], bk[PF_PPT];
  bool valid[PF_PPT], bhalf[PF_PPT];
  float best[PF_PPT];
#pragma unroll
  for (int j = 0; j < PF_PPT; ++j) {
    oy[j] = ty0 + (tid >> 5) + j * (PF_TH / PF_PPT);
    ox[j] = tx0 + (tid & 31);
    valid[j] = oy[j] < im.out_h && ox[j] < im.out_w;
    best[j] = -INFINITY;
    bk[j] = 0;
    bhalf[j] = false;
  }
  __syncthreads();                                         // histogram is zero

  if (use_lds) {
    const int KC = PF_STAGE_FLOATS / F;                    // >= PF_MIN_CHUNK
    // a group of `gl` lanes copies one footprint row (contiguous in global memory), 256 / gl rows per pass
    int gl = 8;
    while (gl < Fw && gl < 64) gl <<= 1;
    const int rows_per_pass = 256 / gl, gr = tid / gl, gc = tid % gl;
    for (int k0 = 0; k0 < n; k0 += KC) {
      const int kc = min(KC, n - k0);
      for (int rr = gr; rr < kc * Fh; rr += rows_per_pass) {
        const int kq = rr / Fh, r = rr - kq * Fh;
        const float* src = lg + (size_t)kidx[k0 + kq] * H * W + (size_t)(r0 + r) * W + c0;
        float* dst = stage + kq * F + r * Fw;
        for (int c = gc; c < Fw; c += gl) dst[c] = src[c];
      }
      __syncthreads();
      pf_scan([&](int k) { return WindowSrc{stage + (k - k0) * F, Fw, r0, c0}; }, k0, kc, ksc, g, oy, ox, valid, best,
              bk, bhalf, hist);
      __syncthreads();                                     // the window is free for the next chunk
    }
  } else {
    pf_scan([&](int k) { return GlobalSrc{lg + (size_t)kidx[k] * H * W, W}; }, 0, n, ksc, g, oy, ox, valid, best, bk,
            bhalf, hist);
  }

#pragma unroll
  for (int j = 0; j < PF_PPT; ++j) {
    if (valid[j]) {
      idmap[im.off + (long long)oy[j] * im.out_w + ox[j]] = (bk[j] << 1) | (bhalf[j] ? 1 : 0);
      atomicAdd(&hist[bk[j] * 3], 1);
      if (bhalf[j]) atomicAdd(&hist[bk[j] * 3 + 2], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * n; i += 256)
    if (hist[i]) atomicAdd(&counts[row * 3 + i], hist[i]);
}

// ---- decide ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cgg_pf_decide_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ n_kept, const int32_t* __restrict__ keep_idx,
    const int32_t* __restrict__ kclass, int32_t* __restrict__ lut_val, int32_t* __restrict__ lut_half,
    int32_t* __restrict__ segments, int Q, int num_things, double iou_thr, int filter_low_score, int stuff_area_limit,
    int defer_stuff) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * Q;
  const int n = min(n_kept[b], Q);
  int things = 0;                                          // things accepted before this chunk (wave-uniform)
  for (int k0 = 0; k0 < Q; k0 += 64) {
    const int k = k0 + lane;
    int val = -1, half = 0, area = 0, cls = -1, qi = -1;
    bool thing = false;
    int a0 = 0, a2 = 0;
    if (k < n) {
      cls = kclass[row + k];
      qi = keep_idx[row + k];
      a0 = counts[(row + k) * 3];
      const int a1 = counts[(row + k) * 3 + 1];
      a2 = counts[(row + k) * 3 + 2];
      const bool pass = a0 > 0 && a1 > 0 && !((double)a0 / (double)a1 < iou_thr);
      thing = pass && cls < num_things;
      if (pass && !thing) {
        if (!defer_stuff) {
          val = cls;
          half = filter_low_score ? 1 : 0;
        } else if (a0 >= stuff_area_limit) {               // `_emb`: unfiltered area, painted without the 0.5 filter
          val = cls;
        }
      }
    }
    const unsigned long long m = __ballot(thing);
    if (thing) {                                           // instance id = 1 + things accepted earlier in query order
      val = cls + (1 + things + __popcll(m & ((1ull << lane) - 1ull))) * 1000;
      half = filter_low_score ? 1 : 0;
    }
    things += __popcll(m);
    if (val >= 0) area = half ? a2 : a0;
    if (k < Q) {
      lut_val[row + k] = val;
      lut_half[row + k] = half;
      int32_t* t = segments + (row + k) * 4;
      t[0] = val; t[1] = cls; t[2] = area; t[3] = qi;
    }
  }
}

// ---- paint -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cgg_pf_paint_kernel(const int32_t* __restrict__ idmap,
                                                           const int64_t* __restrict__ geom,
                                                           const int32_t* __restrict__ n_kept,
                                                           const int32_t* __restrict__ lut_val,
                                                           const int32_t* __restrict__ lut_half,
                                                           int32_t* __restrict__ seg, int Q, int up_h, int up_w,
                                                           int max_out_h, int max_out_w, long long total,
                                                           int void_label) {
  const int b = blockIdx.y;
  const PfImage im = pf_image(geom, b, up_h, up_w, max_out_h, max_out_w, total);
  if (!im.ok) return;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)im.out_h * im.out_w) return;
  int out = void_label;
  if (n_kept[b] > 0) {
    const int id = idmap[im.off + p];
    const int k = min(max(id >> 1, 0), Q - 1);
    const int v = lut_val[(size_t)b * Q + k];
    if (v >= 0 && (!lut_half[(size_t)b * Q + k] || (id & 1))) out = v;
  }
  seg[im.off + p] = out;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------
// workspace, in int32 units: stats [B, 2] | counts [B, Q, 3] | keep_idx | kclass | lut_val | lut_half [B, Q] each |
// idmap [total]; stats and counts are the counters the select kernel clears
extern "C" int64_t cgg_panoptic_fuse_batched_workspace_bytes(int B, int Q, int64_t total_out_pixels) {
  if (B <= 0 || Q <= 0 || total_out_pixels <= 0) return 0;
  return (int64_t)sizeof(int32_t) * ((int64_t)B * 2 + (int64_t)B * Q * 7 + total_out_pixels);
}

extern "C" int cgg_panoptic_fuse_batched(const float* logits, const float* score, const int64_t* label,
                                         const int64_t* geom, int32_t* seg, int32_t* n_kept, int32_t* segments,
                                         float* kept_score, void* ws, int64_t ws_bytes, int B, int Q, int H, int W,
                                         int up_h, int up_w, int max_out_h, int max_out_w, int64_t total_out_pixels,
                                         int num_classes, int num_things, float object_mask_thr, double iou_thr,
                                         int filter_low_score, int stuff_area_limit, int defer_stuff,
                                         cgg_stream_t stream) {
  CGG_REQUIRE(logits && score && label && geom && seg && n_kept && segments && kept_score && ws, CGG_EINVAL,
              "cgg_panoptic_fuse_batched: null pointer");
  CGG_REQUIRE(B > 0 && B <= 65535 && Q > 0 && H > 0 && W > 0 && up_h > 0 && up_w > 0 && max_out_h > 0 &&
                  max_out_w > 0 && total_out_pixels > 0 && num_classes > 0 && num_things >= 0,
              CGG_EINVAL, "cgg_panoptic_fuse_batched: bad sizes");
  CGG_REQUIRE(Q <= PF_MAX_Q, CGG_EUNSUPPORTED, "cgg_panoptic_fuse_batched: Q=%d queries (max %d)", Q, PF_MAX_Q);
  CGG_REQUIRE((int64_t)H * W <= 0x7fffffff && (int64_t)max_out_h * max_out_w <= 0x7fffffff, CGG_EUNSUPPORTED,
              "cgg_panoptic_fuse_batched: a plane of more than 2^31 pixels");
  CGG_REQUIRE(ws_bytes >= cgg_panoptic_fuse_batched_workspace_bytes(B, Q, total_out_pixels), CGG_EINVAL,
              "cgg_panoptic_fuse_batched: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t BQ = (size_t)B * Q;
  int32_t* stats = reinterpret_cast<int32_t*>(ws);
  int32_t* counts = stats + (size_t)B * 2;
  int32_t* keep_idx = counts + BQ * 3;
  int32_t* kclass = keep_idx + BQ;
  int32_t* lut_val = kclass + BQ;
  int32_t* lut_half = lut_val + BQ;
  int32_t* idmap = lut_half + BQ;
  const long long total = (long long)total_out_pixels;
  hipLaunchKernelGGL(cgg_pf_select_kernel, dim3(B), dim3(64), 0, s, score, label, keep_idx, kept_score, kclass, n_kept,
                     counts, stats, Q, num_classes, object_mask_thr);
  CGG_CHECK_LAUNCH("cgg_panoptic_fuse_batched(select)");
  const unsigned tiles = (unsigned)(((max_out_w + PF_TW - 1) / PF_TW) * (long long)((max_out_h + PF_TH - 1) / PF_TH));
  hipLaunchKernelGGL(cgg_pf_argmax_kernel, dim3(tiles, B), dim3(256),
                     sizeof(int32_t) * 3 * Q + sizeof(float) * PF_STAGE_FLOATS, s, logits, geom, n_kept, keep_idx,
                     kept_score, idmap, counts, stats, Q, H, W, up_h, up_w, max_out_h, max_out_w, total);
  CGG_CHECK_LAUNCH("cgg_panoptic_fuse_batched(argmax)");
  hipLaunchKernelGGL(cgg_pf_decide_kernel, dim3(B), dim3(64), 0, s, counts, n_kept, keep_idx, kclass, lut_val,
                     lut_half, segments, Q, num_things, iou_thr, filter_low_score, stuff_area_limit, defer_stuff);
  CGG_CHECK_LAUNCH("cgg_panoptic_fuse_batched(decide)");
  const long long max_npix = (long long)max_out_h * max_out_w;
  hipLaunchKernelGGL(cgg_pf_paint_kernel, dim3((unsigned)((max_npix + 255) / 256), B), dim3(256), 0, s, idmap, geom,
                     n_kept, lut_val, lut_half, seg, Q, up_h, up_w, max_out_h, max_out_w, total, num_classes);
  CGG_CHECK_LAUNCH("cgg_panoptic_fuse_batched(paint)");
  return CGG_OK;
}
