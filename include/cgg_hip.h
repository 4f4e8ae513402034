/*
 * cgg_hip.h -- C ABI of libcgg_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the hot path of
 * CGG ("Betrayed by Captions"): MSDeformAttn pixel decoder -> masked-cross-attention query decoder ->
 * mask_embed x mask_feature mask logits -> open-vocabulary post-processing.
 *
 * Conventions (every entry point):
 *   - extern "C", plain pointers and sizes; NO torch / C++ types cross this boundary.
 *   - every data pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator in
 *     this repo); the library never allocates or frees caller-visible memory. Its only state: one 64-byte
 *     overflow flag word per device (created by cgg_init(device), or thread-safely on first use -- call
 *     cgg_init before a hipGraph capture) and the read-only switches it took from the environment at load.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and NOTHING SYNCHRONISES, with
 *     exactly these exceptions, each of which copies a few bytes device->host and waits for them (not legal
 *     inside a graph capture): cgg_msda_read_levels, the mmcv-contract entries that take the DEVICE level
 *     table (cgg_msda_forward, cgg_msda_forward_fused, cgg_msda_backward -- each = cgg_msda_read_levels +
 *     the *_hostlevels entry), and cgg_x3_overflow_check.
 *   - return value: 0 (CGG_OK) on success, a negative CGG_E* for argument errors, or a positive
 *     hipError_t if the launch failed. No C++ exception crosses the ABI.
 *     cgg_last_error_string() gives a thread-local description of the last failure.
 *   - re-entrant and thread-safe (autograd / DDP threads pass their own stream).
 *
 * Each function names the reference interface it replaces (paths relative to the reference repo
 * jianzongwu/betrayed-by-captions; "[3P]" = upstream mmcv 1.7.1 / mmdet 2.28.2 symbol that the
 * reference selects through a `type=` string and whose source is not part of the reference tree).
 */
#ifndef CGG_HIP_H_
#define CGG_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGG_VERSION 100 /* 0.1.0 */

/* error codes (negative); positive return values are hipError_t */
#define CGG_OK 0
#define CGG_EINVAL (-1)       /* bad argument (null pointer, non-positive size, ...)            */
#define CGG_EUNSUPPORTED (-2) /* shape / dtype combination this build has no kernel for        */
#define CGG_EALIGN (-3)       /* pointer not aligned as the kernel requires (16 B)             */
#define CGG_ELIBRARY (-4)     /* a vendor library call (hipBLASLt) failed                      */

/* dtype tags */
#define CGG_F32 0
#define CGG_BF16 1
/* kv_dtype of cgg_masked_xattn_forward_lse / cgg_masked_xattn_backward only: f32 rows in memory, products on bf16 MFMA operands
 * (f32 accumulate) -- the throughput-mode training variant of the two kernels */
#define CGG_F32_BF16MFMA 2
#define CGG_F32_X3 3 /* cgg_masked_xattn_forward_lse (and cgg_masked_xattn_backward_x3): f32 rows, products on the f16 x 3 contraction (csrc/x3.h) */

typedef void* cgg_stream_t; /* hipStream_t */

int cgg_version(void);

/* Creates the library's per-device state (the 64-byte x3a overflow flag word) on `device`. Optional -- the first x3a producer on a
 * device creates it thread-safely -- but REQUIRED before capturing x3a kernels into a hipGraph on a device that has not run one yet
 * (the creation is a hipMalloc). Idempotent; restores the caller's current device. */
int cgg_init(int device);
const char* cgg_last_error_string(void);

/* ------------------------------------------------------------------------------------------------
 * K1/K2  Multi-scale deformable attention (sampling + aggregation).
 *
 * Replaces [3P] mmcv `ext_module.ms_deform_attn_forward(value, spatial_shapes, level_start_index,
 * sampling_locations, attention_weights, im2col_step)` / `ms_deform_attn_backward(...)`, i.e.
 * `MultiScaleDeformableAttnFunction`, selected by `type='MultiScaleDeformableAttention'` in
 * configs/instance/coco_b48n17.py:49-58 and executed 6x per forward by the pixel decoder built at
 * open_set/models/mask2former_head.py:112-117 (called :787).
 *
 *   value            [B, Nv, H, D]        f32 (CGG_F32) or bf16 (CGG_BF16); Nv = sum_l H_l*W_l
 *   spatial_shapes   [L, 2] int64 (H_l, W_l)        (device)
 *   level_start      [L]    int64                   (device)
 *   sampling_loc     [B, Nq, H, L, P, 2] f32, (x, y) in [0,1]
 *   attn_weight      [B, Nq, H, L, P]    f32 (already soft-maxed over L*P)
 *   out              [B, Nq, H*D]        f32
 * out[b,q,h*D+c] = sum_{l,p} w * bilinear_zero_pad(value_l[b,:,h,c]; x*W_l-0.5, y*H_l-0.5)
 * (grid_sample(align_corners=False, padding_mode='zeros') semantics).
 * Requires D % 4 == 0, L <= 8.
 * The level table, whichever way it arrives (device int64 or host int32), is held to ONE rule by every entry that gathers
 * (csrc/msda_common.h, msda_levels_from_host): H_l > 0, W_l > 0, level_start[l] >= 0, level_start[l] + H_l W_l <= Nv; anything else is
 * CGG_EINVAL "<entry>: level <l> does not fit Nv=<Nv>". The levels need not be ascending or gapless: the lane mappings that assume it
 * (4 x 4 / 8 x 8 tiles of the f32 stream forward, 8 x 4 patches of the gather backward) are chosen only where msda_levels_tile, next
 * to the reader, says the levels tile [0, Nq); the two geometry queries and the prologue entries read the table unchecked.
 * ---------------------------------------------------------------------------------------------- */
int cgg_msda_forward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start,
                     const float* sampling_loc, const float* attn_weight, float* out, int B, int Nv,
                     int H, int D, int L, int Nq, int P, int value_dtype, cgg_stream_t stream);

/* Fused variant: takes the RAW outputs of the `sampling_offsets` (H*L*P*2) and `attention_weights`
 * (H*L*P) linears and does `loc = ref + off / (W_l, H_l)` and the softmax over L*P in the kernel
 * prologue ([3P] MultiScaleDeformableAttention.forward). ref_points [Nq, 2] (x, y) in [0,1] are
 * shared by all levels and batch items (valid_ratios == 1, as in MSDeformAttnPixelDecoder).
 *   offs_logits  [B, Nq, ld]  f32, row = [H*L*P*2 offsets | H*L*P logits], ld >= H*L*P*3        */
int cgg_msda_forward_fused(const void* value, const int64_t* spatial_shapes,
                           const int64_t* level_start, const float* offs_logits, int ld,
                           const float* ref_points, float* out, int B, int Nv, int H, int D, int L,
                           int Nq, int P, int value_dtype, cgg_stream_t stream);

/* The one synchronising step of the mmcv contract, factored out: spatial_shapes [L,2] / level_start [L] (int64, DEVICE, as mmcv's
 * MultiScaleDeformableAttnFunction receives them) -> HOST int32 level_hw [2L] = (H_l, W_l) and level_start [L], validated against
 * Nv. A binding calls it ONCE per spatial_shapes tensor (once per forward pass: the 6 encoder layers and their backwards share the
 * tensor) and then uses the non-synchronising, graph-capturable *_hostlevels entries (INTEGRATION.md shows the stub). */
int cgg_msda_read_levels(const int64_t* spatial_shapes, const int64_t* level_start, int L, int Nv,
                         int32_t* level_hw_host, int32_t* level_start_host, cgg_stream_t stream);

/* Same kernels with the level table given as HOST int32 arrays (level_hw [L,2] = (H_l, W_l),
 * level_start [L]): no device->host read of the table, so the call is legal inside a hipGraph
 * capture. fused != 0 selects the cgg_msda_forward_fused argument meaning (sampling_loc =
 * offs_logits with row stride ld, attn_weight ignored, ref_points used).                          */
int cgg_msda_forward_hostlevels(const void* value, const int32_t* level_hw,
                                const int32_t* level_start, const float* sampling_loc,
                                const float* attn_weight, const float* ref_points, int ld,
                                float* out, int B, int Nv, int H, int D, int L, int Nq, int P,
                                int value_dtype, int fused, cgg_stream_t stream);

/* cgg_msda_forward_fused (host level table, f32) with `value` as the first H*D COLUMNS of wider rows (row stride vld floats, vld % 32
 * == 0): the x3a encoder stream (round 6) projects value, sampling offsets and attention logits of a layer with ONE GEMM whose rows
 * are [value 256 | offsets 192 | logits 96]; value_rows and offs_logits then point into the same (B, Nq, 544) buffer. H = 8, D = 32,
 * L = 3, P = 4 only (CGG_EUNSUPPORTED otherwise). */
int cgg_msda_forward_fused_vld(const float* value_rows, int vld, const int32_t* level_hw, const int32_t* level_start,
                               const float* offs_logits, int ld, const float* ref_points, float* out, int B, int Nv, int H, int D,
                               int L, int Nq, int P, cgg_stream_t stream);

/* Training: the MSDeformAttn prologue ([3P] MultiScaleDeformableAttention.forward: reference_points + offsets / (W_l, H_l),
 * softmax of the attention logits) and its backward as elementwise kernels on the raw rows [offsets H*L*P*2 | logits H*L*P]
 * (f32, row stride ld): loc (B, Nq, H, L, P, 2) / attn (B, Nq, H, L, P) out; backward: grad_rows (ld == 3 H L P) from the
 * gather's grad_loc / grad_attn, the softmax recomputed from the logits. level_hw host [L, 2] = (H_l, W_l); L * P <= 16. */
int cgg_msda_prologue(const float* rows, int ld, const float* ref_points, const int32_t* level_hw, float* loc, float* attn, int B,
                      int Nq, int H, int L, int P, cgg_stream_t stream);
int cgg_msda_prologue_backward(const float* grad_loc, const float* grad_attn, const float* rows, int ld, const int32_t* level_hw,
                               float* grad_rows, int B, int Nq, int H, int L, int P, cgg_stream_t stream);

/* Throughput-mode encoder stream: value bf16, offs_logits bf16 (the raw output of ONE bf16 GEMM over
 * [sampling_offsets; attention_weights]), out bf16 (input of the output_proj GEMM); host level table.    */
int cgg_msda_forward_fused_bf16(const void* value, const int32_t* level_hw, const int32_t* level_start,
                                const void* offs_logits, int ld, const float* ref_points, void* out, int B,
                                int Nv, int H, int D, int L, int Nq, int P, cgg_stream_t stream);
/* Same with `value` HEAD-MAJOR, (B, H, Nv, D): a 128-byte line then holds two x-neighbouring pixels of ONE head instead of
 * half-lines of two heads (H = 8, D = 32, L = 3, P = 4 only). */
int cgg_msda_forward_fused_bf16_hm(const void* value, const int32_t* level_hw, const int32_t* level_start,
                                const void* offs_logits, int ld, const float* ref_points, void* out, int B,
                                int Nv, int H, int D, int L, int Nq, int P, cgg_stream_t stream);

/* Backward of cgg_msda_forward (f32 value). grad_value / grad_loc / grad_attn must be ZEROED by the
 * caller and are accumulated in place (same contract as mmcv's ms_deform_attn_backward).           */
int cgg_msda_backward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const float* sampling_loc, const float* attn_weight, const float* grad_out,
                      float* grad_value, float* grad_loc, float* grad_attn, int B, int Nv, int H,
                      int D, int L, int Nq, int P, cgg_stream_t stream);

/* ... with the level table from the host (level_hw = [h0, w0, h1, w1, ...]): no device->host read-back per call, graph-capturable
 * (what the training-time autograd Function of the encoder calls). Round 5: grad_value comes from a sorted-scatter kernel
 * (csrc/msda_bwd.hip) whenever the queries are the pixels of the value pyramid (D == 32, integer scale between levels).
 * overwrite_loc_attn != 0: grad_loc / grad_attn are WRITTEN instead of accumulated (they need not be zeroed; grad_value still
 * must be) -- only valid where cgg_msda_backward_overwrites(...) returns 1 for the same geometry, CGG_EUNSUPPORTED otherwise. */
int cgg_msda_backward_hostlevels(const float* value, const int32_t* level_hw, const int32_t* level_start,
                                 const float* sampling_loc, const float* attn_weight, const float* grad_out,
                                 float* grad_value, float* grad_loc, float* grad_attn, int B, int Nv, int H, int D, int L,
                                 int Nq, int P, int overwrite_loc_attn, cgg_stream_t stream);
/* ... with a workspace (device, 16-B aligned, >= cgg_msda_backward_workspace_bytes(...) bytes; its contents need not be initialised)
 * for the TWO-PASS sorted scatter of grad_value: the first pass sums the corners inside a 4-pixel halo of 2 x 2-coarse-pixel tiles; a
 * tile with FEW corners outside it scatters them itself, a tile with many (>= 256 of its 1 344) flags itself and counts them per
 * region; a device-side classify step lists the regions that have something left, and persistent second-pass workgroups re-sort
 * exactly those corners on 4 x 4-coarse-pixel tiles with a 12-pixel halo (regions with < 768 corners left: straight to atomics). Offsets of several pixels (trained models) then cost a second sort instead of one 128-byte atomic
 * per corner (round 5: 8.5 ms per call at +-8 px against 2.0 ms at the initialisation's +-0.5 px). ws null or workspace_bytes == 0:
 * identical to cgg_msda_backward_hostlevels_2s. Same results as the single pass up to float summation order. */
/* vld: floats per pixel of the `value` AND `grad_value` rows (0 or H*D = packed (B, Nv, H, D)); a padded stride (e.g. 288 for H*D = 256)
 * keeps neighbouring pixels' lines / atomics off the same L2 channels. */
int cgg_msda_backward_hostlevels_ws(const float* value, int vld, const int32_t* level_hw, const int32_t* level_start,
                                    const float* sampling_loc, const float* attn_weight, const float* grad_out,
                                    float* grad_value, float* grad_loc, float* grad_attn, int B, int Nv, int H, int D, int L,
                                    int Nq, int P, int overwrite_loc_attn, void* ws, long long ws_bytes, cgg_stream_t stream,
                                    cgg_stream_t side_stream);
long long cgg_msda_backward_workspace_bytes(const int32_t* level_hw, const int32_t* level_start, int B, int Nv, int H, int D, int L,
                                            int Nq, int P);

/* ... with the split backward's two kernels on two streams (grad_value on `stream`, grad_loc / grad_attn on `side_stream`, forked
 * from and joined back into `stream` by events inside the call; side_stream null or == stream: the one-stream form). */
int cgg_msda_backward_hostlevels_2s(const float* value, const int32_t* level_hw, const int32_t* level_start,
                                 const float* sampling_loc, const float* attn_weight, const float* grad_out,
                                 float* grad_value, float* grad_loc, float* grad_attn, int B, int Nv, int H, int D, int L,
                                 int Nq, int P, int overwrite_loc_attn, cgg_stream_t stream, cgg_stream_t side_stream);
int cgg_msda_backward_overwrites(const int32_t* level_hw, const int32_t* level_start, int B, int Nv, int H, int D, int L, int Nq,
                                 int P);

/* ------------------------------------------------------------------------------------------------
 * K3/K4/K5  Mask logits: mask_pred[b,q,h,w] = sum_c mask_embed[b,q,c] * mask_feature[b,c,h,w]
 *
 * Replaces `torch.einsum('bqc,bchw->bqhw', mask_embed, mask_feature)` and the attention-mask rule
 * `sigmoid(interpolate(mask_pred, size_l, 'bilinear')) < 0.5` at
 * open_set/models/mask2former_head.py:748-759 (10x per forward), and the all-masked-row fix-up at
 * :825-826.
 *
 * mask_feature is packed ONCE per forward into an MFMA-fragment-major bf16 image
 *   packed[b][t][c/8][p%32][c%8]   (t = p/32, 16 B per (c/8, p) slot; tiles zero padded)
 * so that every `v_mfma_f32_32x32x16_bf16` B operand is one coalesced 1-KiB global_load_dwordx4.
 * `lo` (nullable) receives the bf16 residual f - bf16(f): with it the contraction runs as three
 * bf16 MFMAs (hi*hi + hi*lo + lo*hi), |err| ~1e-5 relative = f32-class accuracy; without it the
 * contraction is plain bf16 (north_star's MFMA bf16 path).
 * `pool` in {1,2,4,8}: pool == 1 packs the feature map itself; pool == s > 1 packs the map that
 * `F.interpolate(.., scale 1/s, bilinear, align_corners=False)` reads, i.e. the mean of the 2x2
 * block at rows/cols {s*i+s/2-1, s*i+s/2}: by linearity, logits of the pooled feature ARE the
 * interpolated logits, so the attention mask of a level needs a GEMM over H*W/s^2 pixels only.
 *   feat   [B, C, H, W] f32;  hi/lo  [B, ceil(H/s*W/s / 32), C/8, 32, 8] bf16
 * Requires C % 16 == 0, H % s == 0, W % s == 0.
 * ---------------------------------------------------------------------------------------------- */
int cgg_pack_mask_feature(const float* feat, void* hi, void* lo, int B, int C, int H, int W,
                          int pool, cgg_stream_t stream);

/*   embed   [B, Q, C] f32          (mask_embed MLP output)
 *   hi, lo  packed feature (lo nullable -> bf16 mode)        npix = number of (pooled) pixels
 *   out     [B, Q, npix] f32, nullable (logits not stored)
 *   bits    [B, Q, ceil(npix/32)] u32, nullable: bit (p%32) of word p/32 = (logit < 0), i.e. the
 *           boolean attention mask (True = blocked) shared by all heads -- never repeated x8.
 * Requires C == 256 (feat_channels of every shipped config), Q <= 256 (bf16); split mode: any Q (row groups of 128, in place).  */
int cgg_mask_logits(const float* embed, const void* hi, const void* lo, float* out, uint32_t* bits,
                    int B, int Q, int C, int npix, cgg_stream_t stream);
/* Exact-f32 variant for parity mode (f32 MFMA, f32 products): feat = the UN-packed f32 map [B, C, npix] (full resolution,
 * or the 2x2-mean map the pooled images are made of); same out / bits contract. Requires C == 256, Q <= 128.            */
int cgg_mask_logits_f32(const float* embed, const float* feat, float* out, uint32_t* bits, int B, int Q, int C, int npix,
                        cgg_stream_t stream);

/* Backward of K3 (the einsum of mask2former_head.py:748 differentiated on the training path :851-921):
 *   grad_feat [B, C, npix] f32 = sum_q embed[b][q][c] * grad_out[b][q][p]     (nullable: skipped)
 *   grad_embed[B, Q, C]   f32 = sum_p grad_out[b][q][p] * feat[b][c][p]       (nullable: skipped)
 * embed [B, Q, C] f32, feat [B, C, npix] f32 (the un-packed mask feature), grad_out [B, Q, npix] f32; outputs are written,
 * not accumulated. bf16 MFMA with f32 accumulation; split != 0 = 3 MFMAs on (hi, lo) bf16 pairs (f32-class accuracy).
 * Any Q: query rows are processed in groups of 128 (split) / 256 launches, a later group adding into grad_feat in place
 * (same lane, same element, fixed order). ws: cgg_mask_logits_backward_workspace_bytes(...) bytes (grad_embed partial
 * planes, summed in a fixed order: no atomics). Requires C == 256, npix % 8 == 0.                                     */
int64_t cgg_mask_logits_backward_workspace_bytes(int B, int Q, int C, int npix);
int cgg_mask_logits_backward(const float* embed, const float* feat, const float* grad_out, float* grad_embed,
                             float* grad_feat, void* ws, int B, int Q, int C, int npix, int split, cgg_stream_t stream);

/* rows of `bits` that block every key are cleared (open_set/models/mask2former_head.py:825-826).
 *   bits [rows, words] u32, npix valid bits per row.                                             */
/* Round 5: the consumer-fused form with the QUERY operand stationary in registers (csrc/mask_logits_astat.hip) -- bf16 MFMA,
 * attn-mask bits (logit < 0, mask2former_head.py:749-759) straight from the accumulators, the logits never stored: the form of the
 * einsum that is not bound by its f32 output (67.2 MB of algorithmic bytes at configs[1] instead of 119.6 MB).
 * embed (B, Q, 256) f32, hi = packed bf16 feature, bits (B, Q, ceil(npix / 32)) u32; Q <= 256. Same bits as cgg_mask_logits. */
int cgg_mask_logits_bits_astat(const float* embed, const void* hi, uint32_t* bits, int B, int Q, int C, int npix,
                               cgg_stream_t stream);
int cgg_attn_mask_fix_full_rows(uint32_t* bits, int rows, int npix, cgg_stream_t stream);

/* generic path for level sizes that are not an even integer divisor of the mask-feature size:
 * bilinear (align_corners=False) resize of stored logits [N, H, W] -> [N, h, w], then (x < 0) bits */
int cgg_attn_mask_from_logits(const float* logits, uint32_t* bits, int N, int H, int W, int h,
                              int w, cgg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K6  Masked multi-head cross-attention core (flash-style, split over keys).
 *
 * Replaces the `baddbmm + masked softmax + bmm` inside `nn.MultiheadAttention` reached through
 * [3P] mmcv MultiheadAttention <- DetrTransformerDecoderLayer, called at
 * open_set/models/mask2former_head.py:829-840 with attn_masks=[attn_mask, None].
 *
 *   q     [B, Q, H*D]  f32   (already projected, NOT yet scaled)
 *   kv    [B, S, 2*H*D] f32 or bf16: row = [K(H*D) | V(H*D)]  (projected keys / values)
 *   bits  [B, Q, ceil(S/32)] u32, nullable; bit set = key blocked; shared by heads. A row with all
 *         S bits set must have been cleared by cgg_attn_mask_fix_full_rows (else output is NaN,
 *         exactly like the reference). The unused bits of the last word (S % 32 != 0) are ignored by every consumer
 *         (forwards, backwards, the in-kernel full-row test) and written as 0 by every producer of `bits`.
 *   out   [B, Q, H*D]  f32   softmax(q k^T * scale + mask) v, heads concatenated
 *   ws    workspace, cgg_masked_xattn_workspace_bytes(...) bytes (split-K partials)
 * Requires D == 32, H*D <= 256, Q <= 128.
 * ---------------------------------------------------------------------------------------------- */
int64_t cgg_masked_xattn_workspace_bytes(int B, int Q, int H, int D, int S);
int cgg_masked_xattn_forward(const float* q, const void* kv, const uint32_t* bits, float* out,
                             void* ws, int B, int Q, int H, int D, int S, float scale,
                             int kv_dtype, cgg_stream_t stream);
/* Same, kv f32 rows [K | V] at row stride ldkv elements (>= 2 H D) and batch stride kv_bstride: a column slice of the merged
 * projection of several decoder layers (0 = dense). */
int cgg_masked_xattn_forward_strided(const float* q, const float* kv, int ldkv, int64_t kv_bstride, const uint32_t* bits,
                                     float* out, void* ws, int B, int Q, int H, int D, int S, float scale, cgg_stream_t stream);
/* cgg_masked_xattn_forward(_strided) with S^T = K Q^T and O^T = V^T P^T on the f32-class f16 x 3 contraction (csrc/xattn_x3.hip):
 * parity mode's inference path for mask2former_head.py:829-840. ldkv / kv_bstride = 0: contiguous (B, S, 2 E) rows. */
int cgg_masked_xattn_forward_x3(const float* q, const float* kv, int ldkv, int64_t kv_bstride, const uint32_t* bits, float* out,
                                void* ws, int B, int Q, int H, int D, int S, float scale, cgg_stream_t stream);
/* Throughput-mode variant: k [B, S, H*D] bf16 and the value projection TRANSPOSED, vt [B, H*D, S] bf16 (computed
 * as Wv x mem^T by the caller), bf16 MFMA for both contractions, f32 softmax statistics and accumulation.
 * Same mask / output / workspace contract. Requires D == 32, Q <= 128, S % 4 == 0.
 * ldk = row stride of k in elements (0 = H*D), vt_bstride = batch stride of vt in elements (0 = H*D*S): k may be a column
 * slice and vt a row block of the merged projection of all decoder layers that read the same level.
 * auto_unmask != 0: a query row whose mask blocks all S keys attends to all of them (mask2former_head.py:825-826) without
 * a prior cgg_attn_mask_fix_full_rows launch; `bits` is left untouched.                                            */
int cgg_masked_xattn_forward_bf16(const float* q, const void* k, const void* vt, const uint32_t* bits, float* out,
                                  void* ws, int B, int Q, int H, int D, int S, float scale, int ldk, int64_t vt_bstride,
                                  int auto_unmask, cgg_stream_t stream);

/* Training pair of K6 ("cgg_masked_xattn_forward ... + backward"): the forward that also saves the
 * log-sum-exp of every (image, head, query) row, and the backward of the attention core -- what autograd derives for the
 * `baddbmm + masked softmax + bmm` inside nn.MultiheadAttention on the training path
 * open_set/models/mask2former_head.py:829-840 (reached from forward_train, :851-921).
 *
 *   lse       [B, H, Q] f32   max + log(sum exp) of the masked, scaled scores (natural log)
 *   out       [B, Q, H*D] f32 the forward's output (delta = rowsum(grad_out o out) is recomputed from it)
 *   grad_out  [B, Q, H*D] f32
 *   grad_q    [B, Q, H*D] f32   d loss / d q      (written, not accumulated)
 *   grad_kv   [B, S, 2*H*D] f32 d loss / d [K | V] (written, not accumulated; every key row is written exactly once)
 *   ws        cgg_masked_xattn_backward_workspace_bytes(...) bytes (per-(chunk, wavefront) grad_q partial planes,
 *             summed in a fixed order: no floating-point atomics, bit-reproducible)
 * The bit mask is consumed as in the forward (bit set = blocked, shared by the heads); nothing of size Q x S is ever
 * stored. f32 MFMA (exact products). Requires D == 32, Q <= 128, kv_dtype == CGG_F32.                              */
int cgg_masked_xattn_forward_lse(const float* q, const void* kv, const uint32_t* bits, float* out, float* lse,
                                 void* ws, int B, int Q, int H, int D, int S, float scale, int kv_dtype,
                                 cgg_stream_t stream);
int64_t cgg_masked_xattn_backward_workspace_bytes(int B, int Q, int H, int D, int S);
int cgg_masked_xattn_backward(const float* q, const void* kv, const uint32_t* bits, const float* out,
                              const float* lse, const float* grad_out, float* grad_q, void* grad_kv, void* ws,
                              int B, int Q, int H, int D, int S, float scale, int kv_dtype, cgg_stream_t stream);
/* cgg_masked_xattn_backward on the f32-class f16 x 3 contraction of csrc/x3.h (parity-mode training, round 6): the five
 * contractions of the backward (scores, dP, dV, dK, dQ) as three v_mfma_f32_32x32x8_f16 per four f32 k-steps instead of four
 * v_mfma_f32_32x32x2_f32 -- as accurate as the f32 MFMA form (tests/test_kernels_gpu.py), 2.7 x less matrix-pipe time.
 * grad_out_amax = device scalar max |grad_out| (cgg_absmax_f32): the per-tensor pre-scale of the gradient operands; q, K, V
 * must be unit scale (|value| < 4094) like every x3 activation operand; inside that range and for a finite grad_out the
 * gradients are finite (dS is pre-scaled by a bound the kernel computes from max |grad_out|, the L1 norms of the V rows and
 * delta -- csrc/xattn_bwd.hip). Same tensors, workspace and limits otherwise. */
int cgg_masked_xattn_backward_x3(const float* q, const void* kv, const uint32_t* bits, const float* out, const float* lse,
                                 const float* grad_out, const float* grad_out_amax, float* grad_q, void* grad_kv, void* ws, int B,
                                 int Q, int H, int D, int S, float scale, cgg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K6w  Fused (shifted-)window multi-head self-attention of the Swin blocks, forward and backward (csrc/window_attn.hip).
 *
 * Replaces, per SwinBlock of [3P] mmdet 2.28 mmdet/models/backbones/swin.py (ShiftWindowMSA.forward -> WindowMSA.forward):
 * torch.roll, window partition, the (3, B_, heads, N, D) permute of qkv, the materialised (B_, heads, N, N) relative-position
 * bias + shifted-window mask, softmax(q k^T * scale + bias + mask) v, the transpose back, window reverse and the reverse roll.
 * All of the re-ordering is addressing: token (y, x) of the rolled map is token ((y + shift) % Hp, (x + shift) % Wp) of the
 * input, windows are ws x ws tiles of the rolled map, and every result goes back to the row its query came from.
 *
 *   qkv    [B, Hp*Wp, 3*C] f32  rows of the qkv linear over the PADDED, un-rolled, un-partitioned map, token-major (y * Wp + x);
 *                               columns [q | k | v], each heads x D
 *   table  [(2 ws - 1)^2, heads] f32  relative_position_bias_table; pair (i, j) of a window reads row
 *                               (yi - yj + ws - 1) * (2 ws - 1) + (xi - xj + ws - 1)
 *   out    [B, Hp*Wp, C] f32    softmax rows applied to v, heads concatenated, same token order as qkv
 *   lse    [B, heads, Hp*Wp] f32  max + log(sum exp) of each query's scores (natural log), consumed by the backward
 *   shift > 0: pairs whose rolled coordinates lie in different regions of the three-slice labelling [0, n - ws), [n - ws, n - shift),
 *   [n - shift, n) (per axis) get the reference's ADDITIVE -100 (not -inf).
 * Backward (recomputes the probabilities from qkv and lse; delta = rowsum(P o dP)):
 *   grad_out   [B, Hp*Wp, C] f32
 *   grad_qkv   [B, Hp*Wp, 3*C] f32  written, not accumulated: every token belongs to exactly one window
 *   grad_table [(2 ws - 1)^2, heads] f32  written; dS summed over batch, windows and index-equal pairs in a fixed order
 *                               (per-(window chunk, head) N x N partials in ws, folded by a second kernel): no floating-point
 *                               atomics, bit-reproducible
 *   ws         cgg_window_attn_backward_workspace_bytes(...) bytes
 * f32 MFMA (v_mfma_f32_16x16x4_f32: exact products, f32 accumulation); nothing of size N x N is read, and only the grad_table
 * partials are written. Requires D == 32 (C == heads * 32), ws * ws <= 144, Hp % ws == Wp % ws == 0, 0 <= shift < ws;
 * anything else returns CGG_EUNSUPPORTED, null pointers CGG_EINVAL, both before touching the device.             */
int cgg_window_attn_forward(const float* qkv, const float* table, float* out, float* lse, int B, int Hp, int Wp, int C,
                            int heads, int ws, int shift, float scale, cgg_stream_t stream);
int64_t cgg_window_attn_backward_workspace_bytes(int B, int Hp, int Wp, int heads, int ws);
int cgg_window_attn_backward(const float* qkv, const float* table, const float* lse, const float* grad_out, float* grad_qkv,
                             float* grad_table, void* ws_buf, int B, int Hp, int Wp, int C, int heads, int ws, int shift,
                             float scale, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K16 Caption-grounding pair costs and their backward.
 *
 * Replaces the body of open_set/models/losses/grounding_loss.py:32-58 (`grounding_loss`, evaluated for each of the 10
 * decoder outputs at open_set/models/mask2former_head.py:542-548): for every (caption i, image j) pair
 *     s = caption_i predictions_j^T * inv_temperature                                  (T x Q)
 *     cost[0][i][j] = sum_t mask[i][t] sum_q softmax_q(s)[t][q] * (-s[t][q]) / max(sum_t mask[i][t], 1)
 *     cost[1][i][j] = sum_q sum_t softmax_t(s)[t][q] * (-s[t][q]) / Q         (token softmax unmasked, as :44)
 * The reference's B-fold `repeat`s and its (B*B, T, Q) score / attention tensors are never materialised; the remaining
 * steps of the loss (the +100 fill of captions without nouns and the four log-softmax diagonals over the (Bc, Bp)
 * matrices, :60-77) are a few elementwise ops on B x B values and stay with the caller.
 *
 *   pred      [Bp, Q, d] f32   caption embeddings predicted by the head (all gathered images)
 *   cap       [Bc, T, d] f32   text embeddings of the caption nouns
 *   cap_mask  [Bc, T]   i32    1 = token present
 *   cost      [2, Bc, Bp] f32  (written)
 * backward: grad_cost [2, Bc, Bp] -> dsim [Bp, Bc*T, Q] f32 = d loss / d (caption_i[t] . pred_j[q]); the caller finishes
 * with ONE batched GEMM grad_pred[j] = dsim[j]^T x cap.reshape(Bc*T, d) (captions are constants: frozen text encoder).
 * f32 MFMA (exact products). Requires Q <= 256, T <= 64, d % 8 == 0.
 * ---------------------------------------------------------------------------------------------- */
int cgg_grounding_pair_costs(const float* pred, const float* cap, const int32_t* cap_mask, float* cost, int Bp, int Bc,
                             int Q, int T, int d, float inv_temperature, cgg_stream_t stream);
int cgg_grounding_pair_costs_backward(const float* pred, const float* cap, const int32_t* cap_mask,
                                      const float* grad_cost, float* dsim, int Bp, int Bc, int Q, int T, int d,
                                      float inv_temperature, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * K18  Row kernels of the caption generator + cross-entropy, so that the (B*34, 30522) logits of
 * open_set/models/mask2former_head.py:551-565 (`caption_generator(...)[1]` -> `loss_caption_generation`) are never
 * stored beyond one row chunk: the caller's library GEMM writes a chunk of logits, these kernels consume it.
 *
 *   logits  [M, ld] f32 or bf16 (dtype), N valid columns per row (N and ld multiples of 4 (f32) / 8 (bf16) elements:
 *           pad the vocabulary with -1e30 bias columns, which contribute exp(.) = 0)
 *   target  [M] i64; rows with target == ignore_index (or outside [0, N)) get loss 0 / gradient 0
 * forward : loss[row] = lse[row] - logits[row][target],  lse[row] = log sum_n exp(logits[row][n])  (both f32, written)
 * backward: logits[row][n] <- grad_rows[row] * (exp(logits[row][n] - lse[row]) - [n == target])   IN PLACE (same dtype)
 * ---------------------------------------------------------------------------------------------- */
int cgg_ce_rows_forward(const void* logits, const int64_t* target, float* loss, float* lse, int M, int N, int64_t ld,
                        int64_t ignore_index, int dtype, cgg_stream_t stream);
int cgg_ce_rows_backward(void* logits, const int64_t* target, const float* lse, const float* grad_rows, int M, int N,
                         int64_t ld, int64_t ignore_index, int dtype, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Prediction-only halves of the Hungarian matching costs on point-sampled mask logits, one pass.
 *
 * Replaces, per training step, the per-(layer, image) elementwise chain of open_set/models/mask2former_head.py:320-390
 * (`_get_target_single` -> mmdet CrossEntropyLossCost(use_sigmoid=True): pos = softplus(-x), neg = softplus(x),
 * einsum(pos, t) + einsum(neg, 1 - t); DiceCost(pred_act=True): sigmoid(x)). With softplus(-x) - softplus(x) = -x the pair of
 * contractions is sp_sum - x . t, so only row sums and sigmoid(x) are needed from the predictions:
 *   x        (rows, P) f32 logits, contiguous, 16-B aligned, P % 4 == 0
 *   sig      (rows, P) f32 out: sigmoid(x)
 *   sp_sum   (rows)    f32 out: sum_p softplus(x)
 *   sig_sum  (rows)    f32 out: sum_p sigmoid(x)   (square = 0)  |  sum_p sigmoid(x)^2   (square = 1: naive_dice = False)
 * ---------------------------------------------------------------------------------------------- */
int cgg_match_cost_rows(const float* x, float* sig, float* sp_sum, float* sig_sum, int rows, int P, int square,
                        cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * HOST function (no device work, no stream): COCO run-length encoding of bit-packed instance masks.
 *
 * Replaces, for the serving / evaluation path, the per-mask `.cpu().numpy()` of open_set/models/maskformer.py:205-208
 * followed by pycocotools `mask.encode` in the dataset's results2json: the (n, H, W/8) bit planes written by
 * cgg_instance_masks_picks(bitpack = 1) are copied to the host ONCE per batch and encoded here on `threads` host threads.
 *
 *   bits    host pointer, n planes of H rows x row_bytes bytes; pixel x of a row = bit (x & 7) of byte (x >> 3);
 *           plane i starts at bits + i * mask_stride_bytes
 *   out     host buffer of out_cap bytes receiving the n COCO "counts" strings back to back (compressed form of
 *           pycocotools' rleToString: column-major runs, first run = zeros); offsets[i] .. offsets[i+1] = string i
 *   offsets host int64[n + 1] (always written)
 * Returns the total number of bytes of all strings; if that exceeds out_cap nothing is copied (call again with a larger
 * buffer); negative = CGG_E*.
 * ---------------------------------------------------------------------------------------------- */
int64_t cgg_rle_encode_bitmasks(const uint8_t* bits, int n, int H, int W, int64_t mask_stride_bytes, int row_bytes,
                                int threads, uint8_t* out, int64_t out_cap, int64_t* offsets);

/* ----------------------------------------------------------------------------------------------
 * Device side of the same encoding: where the column-major bit stream of each mask changes value.
 *
 * A run-length code is determined by those positions; the format (delta coding, 5-bit groups) is per run and stays on
 * the host (cgg_rle_strings_from_transitions). `host_results.rle_transitions_host` states the rule in numpy and the
 * kernels equal it exactly: with p = x * H + y and v(p) the pixel (v(-1) = 0), p is a transition iff v(p) != v(p - 1) --
 * the bottom pixel of column x precedes the top pixel of column x + 1, and a mask whose pixel (0, 0) is set has a
 * transition at 0. The COCO counts of mask i are then t0, t1 - t0, ..., H * W - t_last ([H * W] for an empty mask).
 *
 *   bits      DEVICE pointer, as cgg_rle_encode_bitmasks reads it on the host: n planes of H rows x row_bytes bytes, plane i
 *             at bits + i * mask_stride_bytes, pixel x of a row = bit (x & 7) of byte (x >> 3); only the first W pixels of
 *             a row count, pad bits may hold anything
 *   ws        DEVICE, cgg_rle_transitions_workspace_bytes(n, H, W) bytes, 8-byte aligned. It BEGINS with the column-major
 *             planes `cols[i][x][by]` (uint64; x in [0, 64 * ceil(W / 64)), by in [0, ceil(H / 64))): bit r = pixel
 *             (by * 64 + r, x), bits beyond H or W zero. This layout is part of the contract (cgg_rle_encode_colmajor reads
 *             it); the per-(mask, 64-column strip) transition counts (uint32) and their exclusive scan (int64) follow.
 *   positions DEVICE uint32[capacity]: ascending per mask, packed mask after mask. The positions of mask i are written iff
 *             offsets[i + 1] <= capacity (so: a prefix of the masks); nothing is written at or past `capacity`.
 *   offsets   DEVICE int64[n + 1], always complete (also when the positions do not fit): mask i = offsets[i] .. offsets[i+1]
 * Three launches (transpose + count, scan, emit) on `stream`; no host read, no allocation, no atomics: legal under stream
 * capture. CGG_EINVAL before any device call: null pointer, n < 0, H, W < 1, row_bytes * 8 < W, mask_stride_bytes <
 * H * row_bytes, capacity < 0, H * W >= 2^31, misaligned ws / offsets / positions. No limit on H beyond H * W < 2^31.
 * ---------------------------------------------------------------------------------------------- */
int64_t cgg_rle_transitions_workspace_bytes(int n, int H, int W);
int cgg_rle_transitions(const uint8_t* bits, int n, int H, int W, int64_t mask_stride_bytes, int row_bytes, void* ws,
                        uint32_t* positions, int64_t capacity, int64_t* offsets, cgg_stream_t stream);

/* HOST functions for the two ways a mask leaves cgg_rle_transitions; out / out_cap / out_offsets and the return value as
 * in cgg_rle_encode_bitmasks (total bytes; > out_cap: nothing copied; negative = CGG_E*), strings byte-identical to it.
 *   cgg_rle_strings_from_transitions  positions (uint32, strictly ascending per mask, < H * W) + offsets (int64[n + 1])
 *                                     -> the n counts strings
 *   cgg_rle_encode_colmajor           n contiguous `cols` planes of the workspace layout above -> the n counts strings
 *                                     (the run peeling of cgg_rle_encode_bitmasks without its transposes), on `threads`
 *                                     host threads                                                                   */
int64_t cgg_rle_strings_from_transitions(const uint32_t* positions, const int64_t* offsets, int n, int H, int W,
                                         uint8_t* out, int64_t out_cap, int64_t* out_offsets);
int64_t cgg_rle_encode_colmajor(const uint64_t* cols, int n, int H, int W, int threads, uint8_t* out, int64_t out_cap,
                                int64_t* out_offsets);

/* ----------------------------------------------------------------------------------------------
 * Drawing a result over its image (csrc/paint.hip). `paint.py` states every rule in numpy (paint_instances_host,
 * components_host, paint_panoptic_host) and the kernels equal those bit for bit. All pointers DEVICE; everything runs on
 * `stream`; no host read, no allocation: legal under stream capture.
 *
 * The blend of a pixel value v (uint8) with a colour c (uint8) is the reference's numpy line
 * ([3P] open_set/core/visualization/image.py:199) in float64: (uint8) trunc(v * one_minus_alpha + c * alpha), two rounded
 * products and one rounded sum, no fused multiply-add. alpha and one_minus_alpha are both computed by the caller
 * (1 - 0.8 is 0.19999999999999996, not 0.2), each in [0, 1].
 *
 * cgg_paint_instances_u8: img, out (H, W, 3) uint8 (out may be img); bits as cgg_rle_transitions reads them (n planes of H rows x
 *   row_bytes, plane i at bits + i * mask_stride_bytes, pixel x = bit (x & 7) of byte (x >> 3), pad bits ignored); keep uint8[n];
 *   colors uint8[n][3], applied to the channels in stored order; boxes int32[n][4] (x0, y0, x1, y1, already truncated; they may
 *   reach outside the image) with box_colors uint8[n][3], or NULL for no boxes. One launch:
 *     1. for each kept mask in index order, every pixel of the mask is blended with the mask's colour at alpha;
 *     2. if `edges`: a pixel that lies in some kept mask i while one of its four neighbours does not (a neighbour outside the
 *        image never does) is blended ONCE with white at alpha 0.8;
 *     3. for each kept box in index order: the pixels of the rectangle x0..x1, y0..y1 (inclusive; empty when x1 < x0 or y1 < y0)
 *        nearer than `thickness` pixels to one of its four sides are blended once with the box's colour at alpha 0.8; pixels
 *        outside the image are not drawn.
 *   CGG_EINVAL: null pointer, H, W < 1, n < 0, thickness < 0, row_bytes * 8 < W, mask_stride_bytes < H * row_bytes, alpha or
 *   one_minus_alpha outside [0, 1]. CGG_EUNSUPPORTED: n > 1024, H * W * 3 > 2^31.
 *
 * cgg_label_components_i32: the 8-connected components of equal id of pan (H, W) int32, pixels equal to void_id (and negative
 *   ids) belonging to none. records int64[capacity][5] = [root, id, area, sum_x, sum_y], root = the smallest linear index
 *   y * W + x of the component, in NO particular order (sort by root for a canonical list); status int32[2]: [0] = the number of
 *   components (when it exceeds capacity, `records` holds any `capacity` of them), [1] = 0, or bit 0: a union-find loop hit its
 *   bound of H * W steps (a bug: the records are not to be used), bit 1: a negative id was met. ws: DEVICE,
 *   cgg_label_components_workspace_bytes(H, W) bytes, 8-byte aligned. Union-find with integer atomics only (min on labels, add
 *   on the sums), so the result does not depend on scheduling; no loop waits on another workgroup. Three memsets and four
 *   launches. CGG_EINVAL: null pointer, H, W < 1, capacity < 0, misalignment. CGG_EUNSUPPORTED: H * W >= 2^31.
 *
 * cgg_paint_panoptic_u8: pan (H, W) int32; ids int32[nids] strictly ascending with colors uint8[nids][3]. A pixel whose id is in
 *   the table is blended with that id's colour at alpha; if `edges`, such a pixel with a four-neighbour of another id, or on the
 *   frame, is then blended with white at alpha 0.8. One launch. CGG_EINVAL: null pointer, H, W < 1, nids < 0, alpha pair outside
 *   [0, 1]. CGG_EUNSUPPORTED: nids > 1024, H * W * 3 > 2^31.
 * ---------------------------------------------------------------------------------------------- */
#define CGG_PAINT_MAX_MASKS 1024 /* planes of one cgg_paint_instances_u8 call */
int cgg_paint_instances_u8(const uint8_t* img, uint8_t* out, int H, int W, const uint8_t* bits, int n, int64_t mask_stride_bytes,
                           int row_bytes, const uint8_t* keep, const uint8_t* colors, const int32_t* boxes,
                           const uint8_t* box_colors, double alpha, double one_minus_alpha, int thickness, int edges,
                           cgg_stream_t stream);
/* masks: `rows` rows of W bytes (torch.bool planes, non-zero = set) -> bits: `rows` rows of row_bytes bytes, pixel x = bit (x & 7) of
 * byte (x >> 3), bits past W zero. CGG_EINVAL: null pointer, rows < 0, W < 1, row_bytes * 8 < W. */
int cgg_pack_bool_rows_u8(const uint8_t* masks, int64_t rows, int W, int row_bytes, uint8_t* bits, cgg_stream_t stream);
int64_t cgg_label_components_workspace_bytes(int H, int W);
int cgg_label_components_i32(const int32_t* pan, int H, int W, int void_id, void* ws, int64_t* records, int capacity,
                             int32_t* status, cgg_stream_t stream);
#define CGG_PAINT_MAX_IDS 1024 /* ids of one cgg_paint_panoptic_u8 call */
int cgg_paint_panoptic_u8(const uint8_t* img, uint8_t* out, const int32_t* pan, int H, int W, const int32_t* ids,
                          const uint8_t* colors, int nids, double alpha, double one_minus_alpha, int edges, cgg_stream_t stream);

/* Throughput-mode self-attention of the query decoder ([3P] DetrTransformerDecoderLayer self_attn, no mask; S = Q <= 128):
 * q [B*Q, ldq] and kv = [k | v] [B*Q, ldkv] f32 rows (as written by the fused q|k|v projection) -> out [B*Q, H*D] f32 =
 * softmax(scale q k^T) v per head. bf16 MFMA operands, f32 accumulation and softmax; D == 32.                       */
int cgg_self_attn_rows_bf16(const float* q, int ldq, const float* kv, int ldkv, float* out, int B, int Q, int H, int D,
                            float scale, cgg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K7/K11  Skinny linear + fused residual LayerNorm for the QUERY side of the decoder (M = B*Q ~ 200 rows):
 * the q / out / self-attention projections and FFN of DetrTransformerDecoderLayer ([3P], called at
 * open_set/models/mask2former_head.py:829-840) and the cls / v2l / mask_embed MLPs of forward_head (:734-746).
 *   y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ res)      x row stride ldx, y row stride ldy, res stride ldr
 *   relu != 0 applies ReLU before the residual add; split == 1 -> 3 bf16 MFMAs on (hi, lo) pairs (~2e-5 of sum |x w|),
 *   split == 2 -> exact f32 (f32 MFMA on the un-rounded operands; what parity mode uses), split == 0 -> plain bf16.
 * Requires K % 16 == 0, ldx % 4 == 0.
 * cgg_add_layernorm: y = LayerNorm(a (+ b)) * gamma + beta over the last dim N (b nullable).
 * ---------------------------------------------------------------------------------------------- */
int cgg_linear_rows(const float* x, int ldx, const float* w, const float* bias, const float* res, int ldr,
                    float* y, int ldy, int M, int N, int K, int relu, int split, cgg_stream_t stream);
int cgg_add_layernorm(const float* a, const float* b, const float* gamma, const float* beta, float* y,
                      int rows, int N, float eps, cgg_stream_t stream);

/* Throughput-mode (bf16) successor of cgg_linear_rows. The weight is packed once by cgg_linear_rows_pack into bf16
 * MFMA-B-fragment order (cgg_linear_rows_packed_bytes(N, K) bytes) and then reused:
 *   y[M,N] = x[M,K] @ W^T + bias; ReLU on columns < relu_cols; + res[M,N];
 *   ln_gamma != NULL (N <= 256): y = LayerNorm(y) * gamma + beta in the epilogue;
 *   yp != NULL: yp = y + pos[row % pos_rows] (pos [pos_rows, N]) written in the same pass;
 *   ksplit > 1: K is split over ksplit workgroups; split z writes its partial sums to the plane y + z * M * ldy
 *   (y must hold ksplit planes; bias / res go into plane 0; no ReLU / LayerNorm / yp in that mode) and the consumer
 *   adds the planes (cgg_layernorm_chain with nsum = ksplit) -- deterministic, no atomics.
 *   x2 != NULL: output columns >= x2_col are computed from x2 [M, K] (row stride ldx2) instead of x, and
 *   y2 != NULL: output columns >= y2_col are stored to y2[m * ldy2 + (n - y2_col)] (x2_col, y2_col multiples of 256):
 *   the self-attention q | k | v projections (q, k from `query + query_pos`, v from `query`) as ONE launch.
 * Replaces, per decoder layer, the q/k/v/out projections, FFN, the three post-norm LayerNorms and the `x + pos`
 * adds of DetrTransformerDecoderLayer ([3P]; open_set/models/mask2former_head.py:829-840) and the cls / v2l /
 * mask_embed MLPs of forward_head (:734-746). Requires K % 16 == 0, ldx % 4 == 0.                               */
int64_t cgg_linear_rows_packed_bytes(int N, int K);
int cgg_linear_rows_pack(const float* w, void* packed, int N, int K, cgg_stream_t stream);
int cgg_linear_rows_bf16(const float* x, int ldx, const void* w_packed, const float* bias, const float* res,
                         int ldr, float* y, int ldy, const float* ln_gamma, const float* ln_beta, float ln_eps,
                         const float* pos, int pos_rows, float* yp, int ldyp, int M, int N, int K, int relu_cols,
                         int ksplit, const float* x2, int ldx2, int x2_col, float* y2, int ldy2, int y2_col,
                         cgg_stream_t stream);

/* y = LN_a(sum_{p < nsum} a[p * plane + ...]) ; yp = y + pos[row % pos_rows] (nullable) ; z = LN_b(y) (nullable): the
 * decoder layer's last norm (fed by the nsum split-K planes of cgg_linear_rows_bf16), the next layer's `query +
 * query_pos`, and the head's post_norm (mask2former_head.py:734) in one pass. N <= 1024.                          */
int cgg_layernorm_chain(const float* a, int lda, const float* gamma_a, const float* beta_a, float eps_a,
                        const float* pos, int pos_rows, const float* gamma_b, const float* beta_b, float eps_b,
                        float* y, float* yp, float* z, int rows, int N, int nsum, int64_t plane,
                        cgg_stream_t stream);

/* Tail of one query-decoder layer in ONE launch (C == 256), on the FFN's split-K planes [nsum][M][ld] (bias and
 * residual already in plane 0):  y = LN_a(sum planes) (the layer's last norm; [3P] DetrTransformerDecoderLayer),
 * yp = y + pos[row % pos_rows] (nullable), z = LN_b(y) (decoder post_norm, mask2former_head.py:734),
 * mask_embed = W3 relu(W2 relu(W1 z + b1) + b2) + b3 (:741-746) and, when wq != NULL, qn = Wq (y + pos) + bq -- the next
 * layer's cross-attention query projection (:829). w1 / w2 / w3 / wq: 256 x 256 weights packed by cgg_linear_rows_pack.
 * Same arithmetic per stage as cgg_layernorm_chain + 4 x cgg_linear_rows_bf16 (bf16 operands, f32 accumulate).
 * nsum <= 8 (F = 2048): more planes are CGG_EUNSUPPORTED -- cgg_layernorm_chain sums any number.                      */
#define CGG_DECODER_TAIL_MAX_PLANES 8 /* split-K planes held in registers per row (2048 / 256): more are refused (CGG_EUNSUPPORTED), not dropped */
int cgg_decoder_tail_bf16(const float* planes, int nsum, int64_t plane_stride, int ld, const float* gamma_a,
                          const float* beta_a, float eps_a, const float* pos, int pos_rows, const float* gamma_b,
                          const float* beta_b, float eps_b, const void* w1, const float* b1, const void* w2,
                          const float* b2, const void* w3, const float* b3, const void* wq, const float* bq, float* y,
                          float* yp, float* mask_embed, float* qn, int M, int C, cgg_stream_t stream);

/* Middle of a query-decoder layer in ONE launch (C == 256): x1 = LayerNorm(core Wo^T + bo + res) (attention output
 * projection, residual, post-norm; [3P] DetrTransformerDecoderLayer) and, when wqkv != NULL, the self-attention's fused
 * projection of the result: q = (x1 + pos) Wq^T + bq -> q [M, 256]; [k | v] = [(x1 + pos) Wk^T + bk | x1 Wv^T + bv] ->
 * kv [M, 512]. wo: 256 x 256, wqkv: 768 x 256 ([Wq; Wk; Wv] = in_proj_weight), packed by cgg_linear_rows_pack.    */
int cgg_decoder_mid_bf16(const float* core, int ldc, const void* wo, const float* bo, const float* res, int ldr,
                         const float* gamma, const float* beta, float eps, const float* pos, int pos_rows,
                         const void* wqkv, const float* bqkv, float* x1, float* q, float* kv, int M, int C,
                         cgg_stream_t stream);

/* The decoder layer's FFN ([3P] mmcv FFN: Linear(256, F) - ReLU - Linear(F, 256), + identity) in ONE launch: the split-K
 * partition of the second projection is the column partition of the first, so each workgroup keeps its 32 x 256 hidden
 * block in LDS. planes [F / 256][M][256] f32: partial sums of x + (relu(x W1^T + b1)) W2^T + b2 (b2 and x in plane 0),
 * to be added in plane order by cgg_decoder_tail_bf16 / cgg_layernorm_chain. w1: F x 256, w2: 256 x F, packed by
 * cgg_linear_rows_pack; F % 256 == 0.                                                                              */
int cgg_decoder_ffn_bf16(const float* x, int ldx, const void* w1, const float* b1, const void* w2, const float* b2,
                         float* planes, int M, int C, int F, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Parity mode ("x3"): the same query-side kernels on f32-class contractions. The reference runs every linear of
 * open_set/models/mask2former_head.py:711-761 and of the [3P] DetrTransformerDecoderLayer in f32; here each f32 operand is
 * split into two f16 pieces and every product is three v_mfma_f32_32x32x16_f16 into one f32 accumulator (csrc/x3.h:
 * 22-bit operands, pre-scaled by powers of two, f32-GEMM accuracy; activations must satisfy |x| < 4094). The weight is
 * packed once by cgg_x3_pack into an "x3 image" of cgg_x3_packed_bytes(N, K) bytes (hi fragments, lo fragments, per-column
 * un-scaling factors; K % 16 == 0). The *_x3 entry points take the argument lists of their *_bf16 twins with x3 images in
 * place of the bf16 packed weights.
 * ---------------------------------------------------------------------------------------------- */
int64_t cgg_x3_packed_bytes(int N, int K);
int cgg_x3_pack(const float* w, void* packed, int N, int K, cgg_stream_t stream);
int cgg_linear_rows_x3(const float* x, int ldx, const void* w_x3, const float* bias, const float* res,
                       int ldr, float* y, int ldy, const float* ln_gamma, const float* ln_beta, float ln_eps,
                       const float* pos, int pos_rows, float* yp, int ldyp, int M, int N, int K, int relu_cols,
                       int ksplit, const float* x2, int ldx2, int x2_col, float* y2, int ldy2, int y2_col,
                       cgg_stream_t stream);
int cgg_decoder_tail_x3(const float* planes, int nsum, int64_t plane_stride, int ld, const float* gamma_a,
                        const float* beta_a, float eps_a, const float* pos, int pos_rows, const float* gamma_b,
                        const float* beta_b, float eps_b, const void* w1, const float* b1, const void* w2,
                        const float* b2, const void* w3, const float* b3, const void* wq, const float* bq, float* y,
                        float* yp, float* mask_embed, float* qn, int M, int C, cgg_stream_t stream);
int cgg_decoder_mid_x3(const float* core, int ldc, const void* wo, const float* bo, const float* res, int ldr,
                       const float* gamma, const float* beta, float eps, const float* pos, int pos_rows,
                       const void* wqkv, const float* bqkv, float* x1, float* q, float* kv, int M, int C,
                       cgg_stream_t stream);
int cgg_decoder_ffn_x3(const float* x, int ldx, const void* w1, const float* b1, const void* w2, const float* b2,
                       float* planes, int M, int C, int F, cgg_stream_t stream);

/* Parity mode's large contractions (csrc/x3_gemm.hip), f32 in / f32 out, f32-class arithmetic, w_x3 = cgg_x3_pack image:
 *   cgg_gemm_x3:      out[M, N] (row stride ldc) = act(a[M, K] (row stride lda) W^T * colscale + bias (+ res[M, N], stride ldr));
 *                     relu != 0 applies max(., 0) last. K % 32 == 0, lda % 4 == 0, a 16-byte aligned. bias / res nullable.
 *   cgg_conv_x3_nhwc: the same contraction as an implicit GEMM over a channel-last map x [B, H, W, C] f32 (C % 32 == 0):
 *                     out [B, OH, OW, N] = act(conv(x, W, stride, pad) + bias (+ res [B, OH, OW, N])); W's x3 image is packed
 *                     from the filter re-laid-out as [N][KH][KW][C] (k = (ky, kx, c)). No im2col matrix is written.
 * Replace the f32 library GEMMs / convolutions under [3P] MSDeformAttnPixelDecoder, nn.MultiheadAttention's key / value
 * projections (mask2former_head.py:787, :829-840) and the ResNet backbone in parity mode.                          */
/* Channel-last pieces of parity mode's pixel decoder: cgg_group_norm_nhwc with an F32 input map x [B, HW, C] (same outputs
 * and options; y32 may alias x), and the x3 images of the channel-last f32 mask feature for cgg_mask_logits' split mode: up to
 * 4 pools (1 = full resolution, 2 / 4 / 8 = the 2x2-mean images of the decoder levels) from one launch; hi_host / lo_host /
 * pools_host are HOST arrays of n device pointers / ints, each image [B, ceil(npix / 32), C / 8, 32, 8] 16-bit pieces. */
int cgg_group_norm_nhwc_f32(const float* x, const float* gamma, const float* beta, void* ws, int B, int HW, int C, int groups,
                            float eps, int relu, const float* up_src, int up_h, int up_w, int64_t up_bstride, int W,
                            float* y32, int64_t y32_bstride, void* y16, const float* pos, void* yp16, int64_t y16_bstride,
                            cgg_stream_t stream);
int cgg_pack_mask_feature_nhwc_f32_x3(const float* feat, void* const* hi_host, void* const* lo_host, const int* pools_host,
                                      int n, int B, int C, int H, int W, cgg_stream_t stream);
/* Training (parity mode), matching costs: mask_embed . sample(mask_feature) at the P_group random points of each of the
 * P_total / P_group decoder layers (open_set/models/mask2former_head.py:899-921 samples the (B, Q, h, w) mask logits with [3P]
 * mmcv.ops.point_sample; sample(E F) = E sample(F)). feat [B, H, W, C] channel-last f32, pts [B, P_total, 2] in [0, 1] (x, y), the
 * points of layer g at [g P_group, (g + 1) P_group). Writes the SAMPLES as x3 images (the packed B operand of cgg_mask_logits'
 * split mode, as cgg_pack_mask_feature_nhwc_f32_x3 would from an f32 sample tensor that is never materialised): hi / lo
 * [P_total / P_group][B][P_group / 32][C / 8][32][8] 16-bit pieces -- image (g, b) holds layer g's samples of batch image b, so
 * cgg_mask_logits(embed_g, hi + g * B * image, lo + ..., npix = P_group) is that layer's (B, Q, P_group) point logits.
 * grid_sample arithmetic (bilinear, zeros padding, align_corners = False) in ATen's order. P_group % 32 == 0, C % 8 == 0. */
int cgg_point_sample_nhwc_x3(const float* feat, const float* pts, void* hi, void* lo, int B, int H, int W, int C, int P_total,
                             int P_group, cgg_stream_t stream);
/* Parity mode's twin of cgg_encoder_layer_tail_bf16: the whole post-attention half of an encoder layer as ONE launch on the
 * f32-class contraction (csrc/encoder_tail_x3.hip):
 *   x1 = LayerNorm0(x + a Wo^T + bo);   y = LayerNorm1(x1 + W2 relu(W1 x1 + b1) + b2)
 * a32 = attention rows (MSDeformAttn output before output_proj), x32 = layer input rows, both (M, 256) f32; wo / w1 / w2 = x3
 * images (cgg_x3_pack) of the (256 x 256), (F x 256), (256 x F) weights, F % 256 == 0. Outputs y32 = y and (nullable) yp32 =
 * y + pos[row % pos_rows], (M, 256) f32. x1 and the (M x F) hidden activation never reach memory. */
int cgg_encoder_layer_tail_x3(const float* a32, const float* x32, const void* wo_x3, const float* bo, const float* gamma0,
                              const float* beta0, float eps0, const void* w1_x3, const float* b1, const void* w2_x3,
                              const float* b2, const float* gamma1, const float* beta1, float eps1, const float* pos,
                              int pos_rows, float* y32, float* yp32, int M, int C, int F, cgg_stream_t stream);
int cgg_gemm_x3(const float* a, int lda, const void* w_x3, const float* bias, const float* res, int ldr, float* out, int ldc,
                int M, int N, int K, int relu, cgg_stream_t stream);
/* Parity mode's ResNet stem: cgg_stem_conv7x7_nchw on the f32-class contraction -- w_packed = hi | lo f16 A fragments of the
 * per-output-channel pre-scaled, BN-folded filter (2 x cgg_stem_conv7x7_packed_bytes() bytes), wscale[64] un-scales the
 * accumulators; out = RAW convolution (B, Ho, Wo, 64) f32 channel-last -- and the f32 (bias, ReLU, 3x3 / s2 / p1 max-pool) pass
 * over it (x (B, H, W, C) f32 -> y (B, Ho, Wo, C) f32, C % 4 == 0). Replace MIOpen's f32 stem + relu + max_pool + layout copy. */
int cgg_stem_conv7x7_x3_nchw(const float* img, const void* w_packed, const float* wscale, float* out, int B, int H, int W,
                             cgg_stream_t stream);
int cgg_bias_relu_maxpool_nhwc_f32(const float* x, const float* bias, float* y, int B, int H, int W, int C, cgg_stream_t stream);
/* cgg_gemm_x3 with a row-periodic residual (res_mod > 0: row m adds res[m % res_mod], e.g. a per-token table shared by the
 * images of a batch) and a column split (out2 != NULL: columns >= col2, a multiple of 32, are stored to out2[m * ldc2 + n - col2]):
 * the MSDeformAttn layer's value_proj and sampling_offsets | attention_weights projections as ONE launch over the rows x --
 * (x + pos) Wc^T + bc = x Wc^T + (pos Wc^T + bc), the bracket being a per-token table (mmcv MultiScaleDeformableAttention.forward). */
int cgg_gemm_x3_ex(const float* a, int lda, const void* w_x3, const float* bias, const float* res, int ldr, int res_mod, float* out,
                   int ldc, float* out2, int ldc2, int col2, int M, int N, int K, int relu, cgg_stream_t stream);
int cgg_conv_x3_nhwc(const float* x, const void* w_x3, const float* bias, const float* res, float* out, int B, int H, int W,
                     int C, int N, int KH, int KW, int stride, int pad, int relu, cgg_stream_t stream);

/* Round 4: the same contractions on PRE-SPLIT activation rows ("x3a", csrc/x3.h + csrc/x3s_gemm.hip). An x3a tensor has the shape,
 * bytes and addressing of the f32 tensor it stands for (channel-last, channels % 8 == 0), but every group of 8 consecutive
 * channels holds [8 x f16 hi | 8 x f16 lo] of 16 a -- the operand form of the f16 x 3 MFMA contraction -- so the GEMM moves both
 * operands HBM -> LDS by LDS-DMA with no conversion in its loop, and its epilogue can emit the next GEMM's A operand directly.
 *   cgg_gemm_x3s:      out[M, N] = act(a W^T * colscale + bias (+ res[m or m % res_mod])); a = x3a rows (row stride lda elements,
 *                      lda % 8 == 0), res_fmt 0 none / 1 f32 / 2 x3a, out_fmt 1 f32 / 2 x3a; K % 32 == 0, N % 8 == 0.
 *   cgg_conv_x3s_nhwc: implicit GEMM over a channel-last x3a map [B, H, W, C] (C % 32 == 0, KH * KW <= 32).
 *   cgg_x3a_encode / cgg_x3a_decode: f32 <-> x3a over n contiguous elements (n % 8 == 0): API edges and tests.
 *   cgg_x3_overflow_check: a stored x3a value must satisfy |a| < 4094 (f16 range of 16 a). Every x3a producer ORs 1 into a
 *                      per-device flag word when it sees a larger (or non-finite) value; this copies the word to *value_host
 *                      (synchronises the stream) and optionally clears it -- the caller turns it into an error instead of
 *                      letting inf / NaN masks through (open_set/models/mask2former_head.py:763-849 computes in f32, which
 *                      has no such limit).
 *   cgg_gemm_x3s_cfg / cgg_conv_x3s_nhwc_cfg: the same calls with the tile configuration (0 .. 17; -1 = by shape) as an ARGUMENT:
 *                      tests sweep every instantiation, benches compare them. (Round 4's process-global
 *                      cgg_gemm_x3s_force_config is gone: the library keeps no mutable state besides the overflow flag word.)
 *                      Configuration 18 is the halo-patch kernel of cgg_conv_x3s_nhwc for 3 x 3 / stride 1 / pad 1 convolutions
 *                      of 64, 128 or 256 channels without residual (the default for the ResNet's); forced for any other call
 *                      it returns CGG_EUNSUPPORTED.
 * Same reference call sites as cgg_gemm_x3 / cgg_conv_x3_nhwc above.                                                   */
int cgg_gemm_x3s(const void* a_x3a, int lda, const void* w_x3, const float* bias, const void* res, int ldr, int res_fmt,
                 int res_mod, void* out, int ldc, int out_fmt, int M, int N, int K, int relu, cgg_stream_t stream);
/* cgg_gemm_x3s over a stack of images: row m = row (m % rows_per_image) of image m / rows_per_image, image stride a_bstride elements. */
int cgg_gemm_x3s_batched(const void* a_x3a, int lda, int rows_per_image, int64_t a_bstride, const void* w_x3, const float* bias,
                         const void* res, int ldr, int res_fmt, int res_mod, void* out, int ldc, int out_fmt, int M, int N, int K,
                         int relu, cgg_stream_t stream);
int cgg_conv_x3s_nhwc(const void* x_x3a, const void* w_x3, const float* bias, const void* res, int res_fmt, void* out,
                      int out_fmt, int B, int H, int W, int C, int N, int KH, int KW, int stride, int pad, int relu,
                      cgg_stream_t stream);
int cgg_x3a_encode(const float* x, void* out_x3a, int64_t n, cgg_stream_t stream);
int cgg_x3a_decode(const void* x_x3a, float* out, int64_t n, cgg_stream_t stream);
int cgg_x3_overflow_check(int reset, int* value_host, cgg_stream_t stream);
int cgg_gemm_x3s_cfg(const void* a_x3a, int lda, const void* w_x3, const float* bias, const void* res, int ldr, int res_fmt,
                     int res_mod, void* out, int ldc, int out_fmt, int M, int N, int K, int relu, int cfg, cgg_stream_t stream);
int cgg_conv_x3s_nhwc_cfg(const void* x_x3a, const void* w_x3, const float* bias, const void* res, int res_fmt, void* out,
                          int out_fmt, int B, int H, int W, int C, int N, int KH, int KW, int stride, int pad, int relu, int cfg,
                          cgg_stream_t stream);
/* x3a-producing / -consuming twins of the stream's non-GEMM kernels (round 4):
 *   cgg_bias_relu_maxpool_nhwc_f32_x3a: the stem's (bias, ReLU, 3x3 / s2 max-pool) pass with the pooled map written as x3a (C % 8 == 0);
 *   cgg_group_norm_nhwc_f32_x3a:        cgg_group_norm_nhwc_f32 with y (and yp = y + pos[pixel], nullable) written as x3a rows at
 *                                       y + b * y_bstride; up_src_x3a (nullable) = the low-resolution x3a map whose bilinear x2
 *                                       up-sample is added before the ReLU (the FPN's `cur + F.interpolate(out)`);
 *   cgg_encoder_layer_tail_x3a:         cgg_encoder_layer_tail_x3 with the layer input x and both outputs as x3a rows.          */
int cgg_bias_relu_maxpool_nhwc_f32_x3a(const float* x, const float* bias, void* y_x3a, int B, int H, int W, int C,
                                       cgg_stream_t stream);
int cgg_group_norm_nhwc_f32_x3a(const float* x, const float* gamma, const float* beta, void* ws, int B, int HW, int C, int groups,
                                float eps, int relu, const void* up_src_x3a, int up_h, int up_w, int64_t up_bstride, int W,
                                void* y_x3a, int64_t y_bstride, const float* pos, void* yp_x3a, cgg_stream_t stream);

/* Backward of cgg_group_norm_nhwc_f32 (training, parity mode: the pixel decoder's finest FPN level kept channel-last; replaces
 * autograd's native_group_norm_backward + threshold_backward + upsample_bilinear2d_backward on NCHW copies behind the [3P]
 * MSDeformAttnPixelDecoder lateral / output ConvModules): x, dy (and y = the forward's output when relu) (B, HW, C) f32 channel-last,
 * stats = the forward workspace's head (B, groups, 2) = (mean, variance), ws >= cgg_group_norm_nhwc_backward_workspace_bytes.
 * -> dx (B, HW, C); tot (B, groups, 16): per-image pieces of (dgamma | dbeta) (dgamma[8 g + k] = sum_b tot[b][g][k], dbeta[8 g + k] =
 * sum_b tot[b][g][8 + k]); dlo (nullable, only without relu): gradient of the (B, lo_h, lo_w, C) map the forward up-sampled and added. */
int64_t cgg_group_norm_nhwc_backward_workspace_bytes(int B, int HW, int groups);
int cgg_group_norm_nhwc_f32_backward(const float* x, const float* y, const float* dy, const float* stats, const float* gamma, void* ws,
                                     int B, int HW, int C, int groups, float eps, int relu, float* dx, float* tot, float* dlo, int lo_h,
                                     int lo_w, int W, int dx_padded, cgg_stream_t stream);
/* cgg_group_norm_nhwc_f32 with y written into the interior of a (B, H + 2, W + 2, C) channel-last map whose one-pixel border the caller
 * zeroed (W = map width); dx_padded above is the same layout for the backward's dx: the padded maps of the x3 training convolution. */
int cgg_group_norm_nhwc_f32_padout(const float* x, const float* gamma, const float* beta, void* ws, int B, int HW, int C, int groups,
                                   float eps, int relu, const float* up_src, int up_h, int up_w, int64_t up_bstride, int W,
                                   float* y_padded, cgg_stream_t stream);
int cgg_encoder_layer_tail_x3a(const float* a32, const void* x_x3a, const void* wo_x3, const float* bo, const float* gamma0,
                               const float* beta0, float eps0, const void* w1_x3, const float* b1, const void* w2_x3,
                               const float* b2, const float* gamma1, const float* beta1, float eps1, const float* pos,
                               int pos_rows, void* y_x3a, void* yp_x3a, int M, int C, int F, cgg_stream_t stream);
/* The statistics passes of cgg_group_norm_nhwc_f32 alone: ws (>= cgg_group_norm_nhwc_workspace_bytes) receives (mean, variance) per
 * (b, group) at its head, exactly as the full call leaves them; nothing is normalised (the consumer applies it: below). */
int cgg_group_norm_nhwc_f32_stats(const float* x, void* ws, int B, int HW, int C, int groups, cgg_stream_t stream);
/* The mask-feature head of parity mode's pixel decoder as ONE launch (csrc/mask_feature_head.hip): GroupNorm apply + ReLU over the
 * raw 3 x 3 output z [B, H W, C] f32 channel-last (gn_ws = the (mean, variance) per (b, group) that cgg_group_norm_nhwc_f32*'s
 * statistics passes leave at the head of their workspace), the 1 x 1 mask_feature convolution on the f32-class contraction (w_x3 =
 * cgg_x3_pack of the (N x C) weight, bias nullable) and the x3 images of cgg_pack_mask_feature_nhwc_f32_x3 for n <= 4 pools out of
 * {1, 2, 4, 8} (hi_host / lo_host / pools_host as there). Bit-identical to cgg_group_norm_nhwc_f32_x3a(relu) -> cgg_gemm_x3s ->
 * cgg_pack_mask_feature_nhwc_f32_x3, whose x3a and f32 intermediates never reach memory here; mf (nullable) additionally receives
 * the f32 map [B, H, W, N]. C = N = 256, groups = 32, H % 8 == 0, W % 8 == 0. Raises the x3 overflow flag where the GroupNorm's
 * x3a store does. */
int cgg_mask_feature_head_x3(const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps, int groups,
                             const void* w_x3, const float* bias, void* const* hi_host, void* const* lo_host, const int* pools_host,
                             int n, float* mf, int B, int H, int W, int C, int N, cgg_stream_t stream);
/* ... with the wavefront configuration as an argument (0: four wavefronts per workgroup, 1: eight, -1: the default). */
int cgg_mask_feature_head_x3_cfg(const float* z, const void* gn_ws, const float* gamma, const float* beta, float eps, int groups,
                                 const void* w_x3, const float* bias, void* const* hi_host, void* const* lo_host,
                                 const int* pools_host, int n, float* mf, int B, int H, int W, int C, int N, int cfg,
                                 cgg_stream_t stream);

/* The reference's test pipeline for a batch of raw images as ONE launch (csrc/image_prep.hip): [3P] mmdet Resize (mmcv imrescale,
 * 8-bit bilinear) -> Pad -> Normalize(to_rgb) -> ImageToTensor per image and the [3P] mmcv collate of the batch, from HWC uint8 bytes
 * to out (B, 3, Hb, Wb) f32 contiguous NCHW -- what cgg_stem_conv7x7_nchw / cgg_stem_conv7x7_x3_nchw read. The arithmetic is the rule
 * of image_prep.py (`prepare_host`), bit for bit; it restates OpenCV's INTER_LINEAR for 8-bit images and claims equality with no
 * particular cv2 build.
 *   staged          DEVICE bytes (4-byte aligned base): the B images, 3-byte pixels, back to back at arbitrary byte offsets, and the
 *                   descriptor table at byte `table_offset` (a multiple of 4); staged_bytes = how many of them are valid
 *   table_host      HOST copy of the same B rows of 8 int32: byte offset, h, w, row pitch in bytes (>= 3 w), new_h, new_w, pad_h, pad_w.
 *                   It is read during the call, for validation only: the kernel reads the device rows
 *   mean, std, pad_val   HOST, 3 floats each; mean / std index the OUTPUT plane (after to_rgb). pad_before_norm != 0: Pad ran ahead of
 *                   Normalize -- pad_val indexes the SOURCE channel and the pad region holds (pad_val - mean) / std; 0: the pad
 *                   region holds pad_val[plane] itself. value = float(float(x - mean) * float(1 / std))
 *   out             every element is written exactly once: resized region (new_h x new_w), pad region (up to pad_h x pad_w), and 0.0
 *                   up to Hb x Wb (the collate padding); the caller does not clear it. 16-byte aligned when Wb % 4 == 0
 * Does not synchronise. Checked on the host before the launch: CGG_EINVAL for B < 1, a zero-sized image, new > pad or pad > batch on
 * either axis, pitch < 3 w, an image or the table extending past staged_bytes, std == 0; CGG_EUNSUPPORTED beyond the index arithmetic
 * of the kernel: B, h, w, Hb, Wb <= CGG_IMAGE_PREP_MAX_DIM and staged_bytes <= 2^31 - 9. The kernel reads no byte outside the table rows
 * and offset .. offset + h * pitch of each image. */
#define CGG_IMAGE_PREP_TABLE_COLS 8 /* descriptor row: byte offset, h, w, row pitch, new_h, new_w, pad_h, pad_w */
#define CGG_IMAGE_PREP_MAX_DIM 65535
int cgg_image_prep_u8(const uint8_t* staged, int64_t staged_bytes, int64_t table_offset, const int32_t* table_host, int B,
                      const float* mean, const float* std, const float* pad_val, int to_rgb, int pad_before_norm, float* out, int Hb,
                      int Wb, cgg_stream_t stream);

/* The reference's training pipeline (large-scale jitter) for a batch of raw samples in TWO launches (csrc/train_prep.hip): [3P] mmdet
 * RandomFlip -> Resize(ratio_range, keep_ratio) -> RandomCrop(absolute, recompute_bbox) -> FilterAnnotations(by_mask) -> Pad(size) ->
 * Normalize(to_rgb) per sample, from HWC uint8 images, uint8 instance bitmaps and uint8 semantic maps to img (B, 3, H, W) f32 NCHW,
 * masks (N, H, W) u8 (0 / 1), seg (B, 1, H, W) u8 and stats (N, 5) i32 = area, xmin, ymin, xmax, ymax of each output mask (an empty
 * one: 0, INT32_MAX, INT32_MAX, -1, -1). Flip, resize and crop are index arithmetic: each output pixel is one gather from the raw
 * sample, the resized sample never exists. The random decisions arrive in the table rows. The arithmetic is the rule of train_prep.py
 * (`prepare_train_host`), bit for bit: float32 bilinear taps for the image (no 8-bit rounding: the image is float from the loader on),
 * nearest for masks and semantic maps; it restates the [3P] steps from their published behaviour and claims equality with no
 * particular mmdet / mmcv / cv2 build.
 *   staged          DEVICE bytes (4-byte aligned base): the image table at byte `img_table_offset`, the instance table at byte
 *                   `inst_table_offset` (multiples of 4), and the images (3-byte pixels), instance bitmaps and semantic maps (1-byte
 *                   pixels, non-zero = set for a bitmap) back to back at arbitrary byte offsets; staged_bytes = how many are valid
 *   img_table_host  HOST copy of the B image rows of 12 int32: byte offset, h, w, row pitch in bytes (>= 3 w), new_h, new_w, oy, ox
 *                   (the window's corner in the resized image), flip (0 / 1: horizontal), first instance, instances (the images own
 *                   consecutive ranges of the N instances, in order), byte offset of the semantic map (rows of w bytes) or -1
 *   inst_table_host HOST copy of the N instance rows of 3 int32: image index, byte offset, row pitch in bytes (>= w); nullable when
 *                   N == 0. Both copies are read during the call, for validation only: the kernels read the device rows
 *   mean, std, pad_val   HOST, 3 floats each; mean / std index the OUTPUT plane (after to_rgb), pad_val the SOURCE channel: outside
 *                   the image's extent (min(new_h - oy, crop_h) x min(new_w - ox, crop_w)) img holds (pad_val - mean) / std, masks 0,
 *                   seg seg_pad. value = float(float(x - mean) * float(1 / std))
 *   img, masks, seg every element is written exactly once; the caller clears nothing, stats included (its rows are initialised by the
 *                   first launch and reduced into by the second with int32 atomicAdd / atomicMin / atomicMax, at most one each per
 *                   workgroup tile). masks / stats nullable when N == 0; seg nullable (no semantic maps: the table column is
 *                   ignored). img 16-byte, masks / seg 4-byte aligned when W % 4 == 0; stats 4-byte aligned
 * Does not synchronise. Checked on the host before the first launch: CGG_EINVAL for null pointers, B < 1, a zero-sized image, a
 * window outside the resized image (oy > max(new_h - crop_h, 0), likewise ox), a crop larger than the plane, a pitch too small, any
 * plane or table extending past staged_bytes, an instance whose image index is out of range or not the image that owns it, instance
 * ranges that do not tile 0 .. N, std == 0; CGG_EUNSUPPORTED beyond the index arithmetic of the kernels: B + N, h, w, H, W <=
 * CGG_IMAGE_PREP_MAX_DIM and staged_bytes <= 2^31 - 9; CGG_EALIGN as above. The kernels read no byte outside the table rows and
 * offset .. offset + h * pitch of each image, bitmap and map. */
#define CGG_TRAIN_PREP_IMG_COLS 12 /* byte offset, h, w, row pitch, new_h, new_w, oy, ox, flip, first instance, instances, semantic-map offset or -1 */
#define CGG_TRAIN_PREP_INST_COLS 3 /* image index, byte offset, row pitch */
int cgg_train_prep_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                      const int32_t* img_table_host, const int32_t* inst_table_host, int B, int N, const float* mean, const float* std,
                      const float* pad_val, int to_rgb, int seg_pad, int crop_h, int crop_w, float* img, uint8_t* masks, uint8_t* seg,
                      int32_t* stats, int H, int W, cgg_stream_t stream);

/* The same pipeline for PANOPTIC samples, from the id map instead of host-made bitmaps, in TWO launches (csrc/train_prep.hip): the
 * image kernel of cgg_train_prep_u8, then one kernel that gathers ONE id per output pixel (rule 3 of train_prep.py: nearest, flip,
 * window), looks it up in the image's segment rows and writes every plane the reference's LoadOpenPanopticAnnotations
 * (open_set/datasets/pipelines/loading.py:317-341) followed by the augmentation chain yields: the thing masks (1 where the pixel's
 * segment is thing slot t), the semantic byte (the segment's category; 255 for an id that no row lists) and the per-thing
 * statistics. Nearest gathers commute with "compare the id", so the result equals cgg_train_prep_u8 on the bitmaps and the semantic
 * map that `train_prep.load_panoptic_host` makes, bit for bit.
 *   staged          DEVICE bytes (4-byte aligned base): the three tables at bytes img / pan / seg_table_offset (multiples of 4), the
 *                   images and the id maps; staged_bytes = how many are valid
 *   img_table_host  HOST copy of the B image rows of cgg_train_prep_u8: first instance / instances count the image's THINGS (planes
 *                   of `masks`, rows of `stats`), the semantic-map offset is -1
 *   pan_table_host  HOST copy of the B rows of 5 int32: byte offset of the id map, row pitch in bytes, format (0: int32 ids, offset
 *                   and pitch multiples of 4, pitch >= 4 w; 1: 3 bytes R, G, B per pixel with id = R + 256 G + 65536 B, pitch >= 3 w),
 *                   first segment row, segment rows (<= CGG_TRAIN_PREP_MAX_SEGMENTS; the images own consecutive ranges of the S rows)
 *   seg_table_host  HOST copy of the S segment rows of 2 int32: id, and (slot << 8) | category with category <= 254 and slot = 0
 *                   for a segment that is no thing, t + 1 for the image's thing t. Within an image ids ascend strictly and the
 *                   non-zero slots are a permutation of 1 .. instances. Nullable when S == 0
 *   img, masks, seg, stats, mean, std, pad_val, seg_pad, crop   as for cgg_train_prep_u8; the caller clears nothing. seg nullable:
 *                   no semantic plane is written
 * Does not synchronise. Checked on the host before the first launch: everything cgg_train_prep_u8 checks for the image rows, and
 * CGG_EINVAL for a null table, a table or a map extending past staged_bytes, a pitch too small, a format other than 0 / 1, an
 * unaligned int32 map, a semantic-map offset other than -1, segment ranges that do not tile 0 .. S, ids that do not ascend, a
 * category > 254, slots that are no permutation; CGG_EUNSUPPORTED for more than CGG_TRAIN_PREP_MAX_SEGMENTS rows of one image;
 * CGG_EALIGN as for cgg_train_prep_u8. The kernels read no byte outside the table rows and offset .. offset + h * pitch of each
 * image and map. */
#define CGG_TRAIN_PREP_PAN_COLS 5 /* byte offset of the id map, row pitch in bytes, format (0: int32 ids, 1: R, G, B bytes), first segment row, segment rows */
#define CGG_TRAIN_PREP_SEG_COLS 2 /* id, (slot << 8) | category: slot 0 = no thing, t + 1 = the image's thing t */
#define CGG_TRAIN_PREP_MAX_SEGMENTS 256
int cgg_train_prep_panoptic_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t pan_table_offset,
                               int64_t seg_table_offset, const int32_t* img_table_host, const int32_t* pan_table_host,
                               const int32_t* seg_table_host, int B, int N, int S, const float* mean, const float* std,
                               const float* pad_val, int to_rgb, int seg_pad, int crop_h, int crop_w, float* img, uint8_t* masks,
                               uint8_t* seg, int32_t* stats, int H, int W, cgg_stream_t stream);

/* The same pipeline for INSTANCE samples whose masks arrive as COCO polygons (`ann_info['masks']`: per instance a list of parts, per
 * part a flat x0, y0, x1, y1, ... sequence), rasterised on the device (csrc/train_prep.hip): the image kernel of cgg_train_prep_u8,
 * one kernel that turns every instance's parts into a COLUMN-MAJOR BIT PLANE at source resolution (pixel p = x * h + y is bit p & 31
 * of word p >> 5), and the plane kernel of cgg_train_prep_u8 reading those bits instead of staged bytes -- rule 3 and the statistics
 * are the same code. The raster rule is rule 6 of train_prep.py (`polygon_mask_host`), a restatement of the published maskApi.c
 * (rleFrPoly, then merge with intersect = 0): vertices (int)(5 v + 0.5); the edge walk in steps of 1 / 5 pixel with
 * (int)(ys + s * t + 0.5), product and sums rounded on their own; a crossing wherever consecutive points change their column, at
 * the column-major index a = xd * h + yd; pixel p is set iff the number of crossings <= p is odd (one prefix parity over the whole
 * plane, carried across columns); an instance is the OR of its parts. It claims equality with no particular pycocotools build.
 * The fill kernel runs one workgroup per instance and takes the parts in turn: every point of every edge is closed-form in (edge, d),
 * so lanes stride over d and each crossing toggles one bit (atomic XOR) of a toggle plane -- in LDS when h * w <=
 * CGG_POLY_LDS_BITS, else in the workspace; then a prefix XOR over the plane in blocks of CGG_POLY_SCAN_BITS bits (shift-XOR inside
 * a word, the parity of the preceding words' population counts through a wave ballot and across the four waves as the carry).
 *   staged          DEVICE bytes (8-byte aligned base): the three tables at bytes img / inst / part_table_offset (multiples of 4), the
 *                   images and the coordinates as float64; no bitmap. staged_bytes = how many are valid
 *   img_table_host  HOST copy of the B image rows of cgg_train_prep_u8; the semantic-map offset is -1
 *   inst_table_host HOST copy of the N instance rows of 3 int32: image index, first part, parts (>= 0; the instances own consecutive
 *                   ranges of the P parts, in order). An instance without parts has an empty mask
 *   part_table_host HOST copy of the P part rows of 2 int32: byte offset of the part's 2 k float64 (a multiple of 8), vertex count k
 *   staged_host     HOST copy of the staged bytes; only the coordinates the part rows name are read, for validation
 *   workspace       DEVICE, 4-byte aligned, >= cgg_train_prep_polygons_workspace_bytes(...) bytes: the N bit planes first, each
 *                   max over the images of ceil(h * w / 32) words apart, then (workspace route) as many toggle planes. The kernels
 *                   write every word they read: the caller clears nothing
 *   force_workspace non-zero: toggle planes in the workspace whatever their size (for tests)
 *   img, masks, stats, mean, std, pad_val, crop   as for cgg_train_prep_u8 (there is no semantic plane)
 * cgg_polygon_fill_bits runs the fill kernel alone (same tables; of an image row only h, w, first instance, instances are used).
 * cgg_train_prep_polygons_workspace_bytes answers the bytes of workspace either needs, or a negative status.
 * Nothing synchronises. Checked on the host before the first launch: everything cgg_train_prep_u8 checks for the image rows, and
 * CGG_EINVAL for null pointers, a table or a part extending past staged_bytes, a part offset that is no multiple of 8, a vertex
 * count < 1, instance or part ranges that do not tile, a non-finite coordinate; CGG_EUNSUPPORTED for |coordinate| >
 * CGG_IMAGE_PREP_MAX_DIM (it bounds the edge walk), h * w > 2^31 - 32, a workspace that is too small; CGG_EALIGN as for
 * cgg_train_prep_u8, and for staged / workspace. */
#define CGG_TRAIN_PREP_POLY_INST_COLS 3 /* image index, first part, parts */
#define CGG_TRAIN_PREP_POLY_PART_COLS 2 /* byte offset of the part's 2 k float64 (a multiple of 8), vertex count k */
#define CGG_POLY_LDS_BITS 393216
#define CGG_POLY_SCAN_BITS 8192
int64_t cgg_train_prep_polygons_workspace_bytes(const int32_t* img_table_host, int B, int N, int force_workspace);
int cgg_polygon_fill_bits(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                          int64_t part_table_offset, const int32_t* img_table_host, const int32_t* inst_table_host,
                          const int32_t* part_table_host, const uint8_t* staged_host, int B, int N, int P, uint32_t* workspace,
                          int64_t workspace_bytes, int force_workspace, cgg_stream_t stream);
int cgg_train_prep_polygons_u8(const uint8_t* staged, int64_t staged_bytes, int64_t img_table_offset, int64_t inst_table_offset,
                               int64_t part_table_offset, const int32_t* img_table_host, const int32_t* inst_table_host,
                               const int32_t* part_table_host, const uint8_t* staged_host, int B, int N, int P, const float* mean,
                               const float* std, const float* pad_val, int to_rgb, int crop_h, int crop_w, float* img,
                               uint8_t* masks, int32_t* stats, int H, int W, uint32_t* workspace, int64_t workspace_bytes,
                               int force_workspace, cgg_stream_t stream);

/* One step of the caption beam search for a whole batch of images, decision and bookkeeping on the device (csrc/beam_step.hip):
 * the loop body of the reference's beam_search, open_set/utils/eval/inference.py:113-149 -- mean over the decoder blocks' generator
 * outputs, log-softmax, (log p + parent weight) / length^alpha, the top `beam` of an image's live rows, the walk over them that
 * finishes sequences at EOS and continues the others -- which the reference (and caption_search.beam_search) runs on the host for
 * one image. The rule, quirks included, is written down in caption_search.py (`beam_step_host`); equal candidates are ordered by
 * the smaller row * V + col. Two launches (per-chunk partials, then one workgroup per image); nothing is allocated, nothing
 * synchronises, the host reads no candidate.
 *   logits          (L, B * beam, V) f32 contiguous, 4-byte aligned: row b * beam + s = slot s of image b at the newest position
 *   state, all DEVICE, beam slots per image, rows of `state_max_len` tokens (<= CGG_BEAM_STEP_MAX_LEN):
 *     seqs (B, beam, state_max_len) i32 -- live sequences in slots 0 .. nlive - 1 in the order they were accepted; weights (B, beam)
 *     f32; nlive (B) i32; fin_seqs (B, beam, state_max_len) i32, fin_len / fin_score (B, beam) i32 / f32, nfin (B) i32 -- finished
 *     sequences in order; best_idx (B) i32; done (B) i32; ndone (1) i32 = how many images are done
 *   tokens, parents (B * beam) i64, written by every call: newest token and global parent row of each slot for the next decoder
 *                   step; dead slots (and every slot of a done image) get eos and their own row
 *   ws              cgg_beam_step_workspace_bytes(B, beam, V) bytes of scratch
 *   length          current length of every live sequence (1 at the BOS step); first != 0: the BOS step (every candidate becomes a
 *                   live sequence with its OWN weight, no EOS / max_len handling: inference.py:96-104)
 * An image whose `done` is set is left untouched. CGG_EINVAL: a null pointer, L < 1, B < 1, beam outside 1 .. CGG_BEAM_STEP_MAX_BEAM,
 * V < beam, max_len > state_max_len, length outside 1 .. state_max_len - 1; CGG_EUNSUPPORTED: state_max_len > CGG_BEAM_STEP_MAX_LEN. */
#define CGG_BEAM_STEP_MAX_BEAM 8
#define CGG_BEAM_STEP_MAX_LEN 256
int64_t cgg_beam_step_workspace_bytes(int B, int beam, int V);
int cgg_beam_step(const float* logits, int L, int B, int beam, int V, int32_t* seqs, float* weights, int32_t* nlive,
                  int32_t* fin_seqs, int32_t* fin_len, float* fin_score, int32_t* nfin, int32_t* best_idx, int32_t* done,
                  int32_t* ndone, int64_t* tokens, int64_t* parents, void* ws, int length, float alpha, int eos, int max_len,
                  int state_max_len, int first, cgg_stream_t stream);
/* ... one launch at a time, for measurements: passes = 1 the partials, 2 the decision over the partials that `ws` holds, 3 both. */
int cgg_beam_step_passes(const float* logits, int L, int B, int beam, int V, int32_t* seqs, float* weights, int32_t* nlive,
                         int32_t* fin_seqs, int32_t* fin_len, float* fin_score, int32_t* nfin, int32_t* best_idx, int32_t* done,
                         int32_t* ndone, int64_t* tokens, int64_t* parents, void* ws, int length, float alpha, int eos,
                         int max_len, int state_max_len, int first, int passes, cgg_stream_t stream);

/* Batched transpose of f32 matrices, in (B, R, C) -> out (B, C, R): the NCHW <-> NHWC layout changes around the x3 kernels under
 * autograd (torch `x.permute(0, 2, 3, 1).contiguous()` and back), 64 x 64 tiles through LDS. */
int cgg_transpose_f32(const float* in, float* out, int B, int R, int C, cgg_stream_t stream);
/* in (B, C, H, W) f32 contiguous -> the interior of out (B, H + 2, W + 2, C) (channel-last, one-pixel border NOT written: the caller
 * zeroes it): padded channel-last maps for the x3 training convolution's weight-gradient taps without a padding copy. */
int cgg_nchw_to_nhwc_pad1_f32(const float* in, float* out, int B, int C, int H, int W, cgg_stream_t stream);

/* Training in parity mode: the weight gradient of a linear layer, dW[n][k] = sum_m dy[m][n] x[m][k] -- autograd's
 * `grad_output.t() @ input` behind the F.linear calls of the [3P] MSDeformAttn encoder layers (mask2former_head.py:787) -- on the
 * f32-class f16 x 3 contraction; both row-major operands reach the MFMA through LDS transpose reads (csrc/wgrad_x3.hip). ws
 * (cgg_wgrad_x3_workspace_bytes) receives *splits_out partial (N, K) f32 matrices over contiguous row ranges; dW is their sum.
 * dy (M, N) rows at stride ldy, x (M, K) rows at stride ldx; N, K, ldy, ldx % 4 == 0; |values| < 4094. */
int64_t cgg_wgrad_x3_workspace_bytes(int M, int N, int K);
int cgg_wgrad_x3(const float* dy, int ldy, const float* x, int ldx, float* ws, int* splits_out, int M, int N, int K,
                 cgg_stream_t stream);
/* ... with the bias gradient db[n] = sum_m dy[m][n] (autograd's `grad_output.sum(0)`) from the same pass over dy: ws_bias
 * (>= splits x N floats, splits = workspace bytes / (4 N K)) receives one partial row per split. */
int cgg_wgrad_bias_x3(const float* dy, int ldy, const float* x, int ldx, float* ws, float* ws_bias, int* splits_out, int M, int N,
                      int K, cgg_stream_t stream);

/* Top-k SELECTION per row: idx[r, 0:k] = indices of the k largest x[r, 0:N] (row stride ld), in NO particular order, ties at the
 * threshold broken arbitrarily -- the importance sampling of the mask losses ([3P] mmdet get_uncertain_point_coords_with_randomness,
 * called at mask2former_head.py:605, keeps the 9 408 most uncertain of 37 632 random points per matched query; torch.topk sorts). */
int cgg_topk_select(const float* x, int ld, int rows, int N, int k, int64_t* idx, cgg_stream_t stream);

/* Per-tensor pre-scale of the x3 contractions' grad_output operands (round 5). The fixed 2^4 pre-scale of csrc/x3.h suits O(1)
 * activations; autograd's grad_output behind the F.linear / conv calls of mask2former_head.py:787 is not unit scale (|g| ~ 1e-6
 * keeps ~10 of the pair's 22 bits). cgg_absmax_f32 writes max |x| over an (M, N) f32 matrix (row stride ld; N, ld % 4 == 0) to the
 * device scalar *amax in one streaming pass; the *_scaled entry points pre-scale that operand by 2^(9 - floor(log2 amax)) instead
 * of 2^4 and fold the inverse into their epilogue (exact). amax pointers are nullable (= the fixed 2^4). Otherwise the
 * contracts of cgg_gemm_x3 / cgg_conv_x3_nhwc / cgg_wgrad_x3 / cgg_wgrad_bias_x3 (ws_bias nullable here). */
int cgg_absmax_f32(const float* x, int ld, int M, int N, float* amax, cgg_stream_t stream);
/* ReLU backward + the same maximum in one pass: g[i] = y[i] > 0 ? gy[i] : 0 (autograd's threshold_backward behind a ReLU whose
 * OUTPUT is y: the Bottleneck ReLUs of the trainable ResNet stage, [3P] mmdet ResNet under mask2former_head.py:787's inputs) and
 * *amax = max |g|. Dense f32 tensors of n elements, n % 4 == 0; g may alias gy. */
int cgg_relu_bwd_absmax_f32(const float* gy, const float* y, float* g, long long n, float* amax, cgg_stream_t stream);
/* cgg_gemm_x3_scaled for the backward of a fused training layer: `mask` (M, N; nullable) zeroes the result where mask <= 0 (the
 * ReLU backward of the layer whose output `mask` is), out_amax (device scalar, nullable) receives max |out| from the epilogue. */
int cgg_gemm_x3_bwd(const float* a, int lda, const float* a_amax, const void* w_x3, const float* mask, int ldm, float* out, int ldc,
                    float* out_amax, int M, int N, int K, cgg_stream_t stream);
int cgg_gemm_x3_scaled(const float* a, int lda, const float* a_amax, const void* w_x3, const float* bias, const float* res, int ldr,
                       float* out, int ldc, int M, int N, int K, int relu, cgg_stream_t stream);
int cgg_conv_x3_nhwc_scaled(const float* x, const float* x_amax, const void* w_x3, const float* bias, const float* res, float* out,
                            int B, int H, int W, int C, int N, int KH, int KW, int stride, int pad, int relu, cgg_stream_t stream);
int cgg_wgrad_x3_scaled(const float* dy, int ldy, const float* dy_amax, const float* x, int ldx, float* ws, float* ws_bias,
                        int* splits_out, int M, int N, int K, cgg_stream_t stream);

/* Encoder-stream residual LayerNorm (N == 256): y = LN(a + b) * gamma + beta, a / b f32 or bf16 (b nullable), with up
 * to three outputs written in the same pass: y32 (f32), y16 = bf16(y), yp16 = bf16(y + pos[row % pos_rows]).  */
int cgg_add_layernorm_ex(const void* a, int a_dtype, const void* b, int b_dtype, const float* gamma, const float* beta,
                         const float* pos, int pos_rows, float* y32, void* y16, void* yp16, int rows, int N,
                         float eps, cgg_stream_t stream);

/* Backward of y = LayerNorm(a + b) over N = 256 channels (training; forward = cgg_add_layernorm_ex): one pass over the rows,
 * statistics recomputed, upstream gradient = dy (f32) + dy16a + dy16b (bf16 gradients of the forward's bf16(y) / bf16(y + pos)
 * outputs; each nullable, at least one given), d/da = d/db = dx (f32; dx16 = optional bf16 copy for a bf16 `b`), per-workgroup partial sums of
 * (dgamma | dbeta): partial (cgg_add_layernorm_backward_partials(rows), 512) f32, to be summed over dim 0 by the caller.
 * Replaces autograd's add / layer_norm backward kernels on the encoder stream of [3P] BaseTransformerLayer. */
int64_t cgg_add_layernorm_backward_partials(int rows);
int cgg_add_layernorm_backward(const float* dy, const void* dy16a, const void* dy16b, const float* a, const void* b, int b_dtype,
                               const float* gamma, float eps, float* dx, void* dx16, float* partial, int rows, int N,
                               cgg_stream_t stream);
/* ... and max |dx| as a device scalar (dx_amax, written by the call; b nullable = plain LayerNorm(a)): the per-tensor pre-scale of
 * the f16 x 3 contractions that take dx as grad_output (cgg_gemm_x3_scaled / cgg_wgrad_x3_scaled) without a pass over dx. */
int cgg_add_layernorm_backward_amax(const float* dy, const void* dy16a, const void* dy16b, const float* a, const void* b, int b_dtype,
                                    const float* gamma, float eps, float* dx, void* dx16, float* partial, float* dx_amax, int rows,
                                    int N, cgg_stream_t stream);

/* Input projections of one MSDeformAttn encoder layer as ONE launch ([3P] MultiScaleDeformableAttention.forward:
 * value_proj / sampling_offsets / attention_weights; layers built at open_set/models/mask2former_head.py:112-117):
 *   value (M, 256) bf16 = x16 Wv^T + bv,   offs (M, NC) bf16 = xp16 Wc^T + bc   (Wc = [W_offsets; W_attention_weights],
 *   NC = 3 * heads * levels * points, 256 .. 384 in steps of 32: 288 for the 3-level encoder, 384 for 4 levels),
 * x16 / xp16 (M, 256) bf16 rows; xp16 == NULL: xp = bf16(x16 + pos16[row % pos_rows]) is formed in the kernel from the bf16
 * table pos16 (pos_rows, 256) and the `x + pos` rows are never stored. value_head_major_rows = N > 0: `value` is written
 * head-major, (M / N, 8, N, 32), for cgg_msda_forward_fused_bf16_hm; 0: (M, 256) rows. Biases f32; weights (N x 256 f32, N = 256 / NC) packed once by cgg_encoder_proj_pack
 * (bf16 MFMA-B fragments, cgg_linear_rows_packed_bytes(N, 256) bytes, output columns interleaved for wide stores). */
int cgg_encoder_proj_pack(const float* w, void* packed, int N, int K, cgg_stream_t stream);
int cgg_encoder_proj_bf16(const void* x16, const void* xp16, const void* pos16, int pos_rows, const void* wv_packed,
                          const float* bv, const void* wc_packed, const float* bc, void* value, void* offs, int M, int C, int NV,
                          int NC, int value_head_major_rows, cgg_stream_t stream);

/* K / V projections of the query decoder for one memory level, all decoder layers that read the level stacked (NK = n * 256
 * outputs; open_set/models/mask2former_head.py:795-812 feeding the cross-attention in_proj of [3P] nn.MultiheadAttention):
 *   k  (B * hw, NK) bf16 = mp16 Wk^T + bk;     vt (B, NK, hw) bf16 = Wv m16^T   (value projection transposed, no bias)
 * m16 / mp16 (B * hw, 256) bf16 rows, any hw (hw % 64 != 0 -- the 1050 / 4200 / 16800 keys of an 800 x 1333 input -- cuts the blocks
 * per image and masks the last one's stores: 4-byte vt stores for even hw, 2-byte for odd); wk packed by cgg_decoder_kv_pack_k, wv by cgg_linear_rows_pack (both
 * cgg_linear_rows_packed_bytes(NK, 256) bytes); bk f32. */
int cgg_decoder_kv_pack_k(const float* w, void* packed, int N, int K, cgg_stream_t stream);
int cgg_decoder_kv_proj_bf16(const void* m16, const void* mp16, const void* wk_packed, const float* bk, const void* wv_packed,
                             void* k, void* vt, int B, int hw, int C, int NK, cgg_stream_t stream);

/* ResNet-50 layer1 identity Bottleneck (mmdet ResNet `Bottleneck.forward`, configs/instance/coco_b48n17.py:17-26), BN folded,
 * channel-last bf16, as ONE launch: y = relu(conv1x1(relu(conv3x3(relu(conv1x1(x, W1) + b1), W2) + b2), W3) + b3 + x).
 * x / y (B, H, W, 256) bf16, H % 8 == 0, W % 16 == 0; all weights packed by cgg_linear_rows_pack: W1 (64 x 256), W2 as the
 * (64 x 576) matrix with K = (ky * 3 + kx) * 64 + c_in, W3 (256 x 64) with its ROWS permuted so that packed row 32 T + j is output
 * channel 64 (T / 2) + 4 (j / 2) + 2 (T & 1) + (j & 1) (see ops.pack_bottleneck64); biases f32. */
int cgg_bottleneck64_bf16(const void* x, const void* w1_packed, const float* b1, const void* w2_packed, const float* b2,
                          const void* w3_packed, const float* b3, void* y, int B, int H, int W, int C, int CMID, cgg_stream_t stream);

/* Encoder-stream FFN block of the pixel decoder as ONE launch ([3P] BaseTransformerLayer 'ffn' + 'norm' of the
 * MSDeformAttn encoder layers built at open_set/models/mask2former_head.py:112-117):
 *   y = LayerNorm(x + W2 relu(W1 x + b1) + b2);  x16 (M, 256) bf16 rows, w1 (F x 256) / w2 (256 x F) packed by
 *   cgg_linear_rows_pack, F % 256 == 0. Outputs (each nullable except one of y16 / y32): y16 = bf16(y),
 *   yp16 = bf16(y + pos[row % pos_rows]), y32 = y. The (M x F) hidden activation never reaches HBM. */
int cgg_encoder_ffn_ln_bf16(const void* x16, const void* w1_packed, const float* b1, const void* w2_packed,
                            const float* b2, const float* gamma, const float* beta, float eps, const float* pos,
                            int pos_rows, void* y16, void* yp16, float* y32, int M, int C, int F, cgg_stream_t stream);
/* Same block for the LAST encoder layer: the LayerNorm also emits the query decoder's K / V operands exactly as
 * cgg_add_layernorm_kv does (m16 = bf16(y + shift[s]), mp16 = bf16(y + shift[s] + pos[s]), level-major rows); y32 (nullable)
 * is the f32 memory at its natural rows. M = B * S rows, level_start_host[n_levels] ascending from 0. */
int cgg_encoder_ffn_ln_kv_bf16(const void* x16, const void* w1_packed, const float* b1, const void* w2_packed,
                               const float* b2, const float* gamma, const float* beta, float eps, const float* shift,
                               const float* pos, int S, const int* level_start_host, int n_levels, float* y32, void* m16,
                               void* mp16, int M, int C, int F, cgg_stream_t stream);
/* The whole post-attention half of an encoder layer as ONE launch ('self_attn' output projection + 'norm' + 'ffn' + 'norm' of
 * the [3P] BaseTransformerLayer, open_set/models/mask2former_head.py:112-117):
 *   x1 = LayerNorm0(x + a Wo^T + bo);   y = LayerNorm1(x1 + W2 relu(W1 x1 + b1) + b2)
 * a16 = attention rows (MSDeformAttn output before output_proj), x16 = layer input rows, both (M, 256) bf16; wo / w1 / w2 packed by
 * cgg_linear_rows_pack. x1 and the hidden activation never reach memory. Outputs as cgg_encoder_ffn_ln_bf16 (shift == NULL:
 * y16 / yp16 / y32, pos nullable) or as cgg_encoder_ffn_ln_kv_bf16 (shift != NULL: pos_rows = S, y16 = m16, yp16 = mp16,
 * level-major, level_start_host[n_levels]). */
int cgg_encoder_layer_tail_bf16(const void* a16, const void* x16, const void* wo_packed, const float* bo, const float* gamma0,
                                const float* beta0, float eps0, const void* w1_packed, const float* b1, const void* w2_packed,
                                const float* b2, const float* gamma1, const float* beta1, float eps1, const float* pos,
                                int pos_rows, const float* shift, const int* level_start_host, int n_levels, void* y16,
                                void* yp16, float* y32, int M, int C, int F, cgg_stream_t stream);

/* Last encoder layer of the stream: y = LN(a + b) as above (y32 nullable) plus the two bf16 operands of the query
 * decoder's K / V projections (mask2former_head.py:795-812), written LEVEL-MAJOR -- [level][batch][hw_l][256], level l =
 * rows level_start[l] .. level_start[l+1] of each batch's S rows -- so that every level is one contiguous GEMM operand:
 *   m16 = bf16(y + shift[s]),  mp16 = bf16((y + shift[s]) + pos[s]),  s = row % S;  shift, pos: [S, 256] f32.
 * level_start_host: n_levels ints on the HOST (start[0] == 0, increasing, < S).                                   */
int cgg_add_layernorm_kv(const void* a, int a_dtype, const void* b, int b_dtype, const float* gamma, const float* beta,
                         const float* shift, const float* pos, int S, const int* level_start_host, int n_levels,
                         float* y32, void* m16, void* mp16, int rows, int N, float eps, cgg_stream_t stream);

/* Throughput-mode (bf16, channel-last) variants used by the pixel decoder's inference stream.
 * cgg_group_norm_nhwc: GroupNorm over x [B, HW, C] bf16 with C / groups == 8 ([3P] MSDeformAttnPixelDecoder
 *   input_convs / lateral_convs / output_convs, norm_cfg GN-32), y = (x - mean) * rstd * gamma + beta
 *   (+ bilinear up-sample of up_src [B, up_h, up_w, C] f32 to the (HW / W, W) grid -- the FPN `cur +
 *   F.interpolate(outs[-1])` step) (+ ReLU); outputs (each nullable, at least one): y32 f32 with batch stride
 *   y32_bstride elements (writes straight into the (B, N, C) encoder stream), y16 = bf16(y) and yp16 =
 *   bf16(y + pos), pos [HW, C] f32, both with batch stride y16_bstride elements. ws:
 *   cgg_group_norm_nhwc_workspace_bytes(B, HW, groups) bytes of scratch (per-block partial statistics, no atomics).
 * cgg_pack_mask_feature_nhwc: cgg_pack_mask_feature for a [B, H, W, C] bf16 map (hi image only).              */
int64_t cgg_group_norm_nhwc_workspace_bytes(int B, int HW, int groups);
int cgg_group_norm_nhwc(const void* x, const float* gamma, const float* beta, void* ws, int B, int HW, int C,
                        int groups, float eps, int relu, const float* up_src, int up_h, int up_w,
                        int64_t up_bstride, int W, float* y32, int64_t y32_bstride, void* y16, const float* pos,
                        void* yp16, int64_t y16_bstride, cgg_stream_t stream);
int cgg_pack_mask_feature_nhwc(const void* feat, void* hi, int B, int C, int H, int W, int pool,
                               cgg_stream_t stream);
/* Same, up to 4 packed images from one launch (the full-resolution image and the pooled ones of the decoder levels):
 * hi_host[i] receives the pool = pools_host[i] image; both arrays (n <= 4 entries) live on the HOST.              */
int cgg_pack_mask_feature_nhwc_multi(const void* feat, void* const* hi_host, const int* pools_host, int n, int B, int C,
                                     int H, int W, cgg_stream_t stream);

/* f3  Channel-last epilogue of the BN-folded backbone convolutions ([3P] mmdet ResNet Bottleneck tail
 * `relu(bn3(conv3(x)) + identity)`, selected by configs/instance/coco_b48n17.py:17-26), in place:
 *   y[rows, C] bf16 <- act(y + bias[C] + res[rows, C]);  bias, res bf16, nullable;  relu != 0 -> max(., 0).
 * Requires C % 8 == 0 and 16-byte aligned pointers.                                                             */
int cgg_bias_act_nhwc(void* y, const void* bias, const void* res, int64_t rows, int C, int relu,
                      cgg_stream_t stream);

/* Library GEMM with the residual epilogue ATen does not expose, for `relu(conv3(x) + identity)` of a BN-folded
 * [3P] mmdet ResNet Bottleneck (1x1 convolution on channel-last bf16 rows):
 *   y[M, N] = act(x[M, K] w[N, K]^T + bias[N] + res[M, N])   (bf16 in / out, f32 accumulation; bias, res nullable; relu 0/1)
 * = ONE hipBLASLt matmul (beta = 1, HIPBLASLT_EPILOGUE_RELU_BIAS). cgg_blaslt_init(path) dlopens the hipBLASLt copy the
 * process already uses (NULL / "" = "libhipblaslt.so") and must be called once before.                              */
int cgg_blaslt_init(const char* libpath);
/* cgg_blaslt_set_tuning(n > 1): at the first use of a shape outside a stream capture, time the first n heuristic
 * candidates (2 warm + 5 timed launches each) and keep the fastest; cgg_blaslt_last_tuning reports (top-1, chosen) us. */
int cgg_blaslt_set_tuning(int n_candidates);
int cgg_blaslt_last_tuning(float* top1_us, float* chosen_us);
int cgg_gemm_bias_res_act_bf16(const void* x, const void* w, const void* bias, const void* res, void* y, int M, int N,
                               int K, int relu, cgg_stream_t stream);

/* Patch matrix of a 3x3 / padding 1 / stride 1|2 convolution on a channel-last bf16 map x[B, H, W, C]:
 * y[B * Ho * Wo, 9 * C], column (ky * 3 + kx) * C + c = x[b, oy * stride + ky - 1, ox * stride + kx - 1, c] (0 outside),
 * Ho = (H - 1) / stride + 1. With cgg_gemm_bias_res_act_bf16 it replaces the 3x3 convolutions of the deep stages of the
 * BN-folded [3P] mmdet ResNet (conv2 of the Bottlenecks of layer3 / layer4).                                        */
int cgg_im2col3x3_nhwc(const void* x, void* y, int B, int H, int W, int C, int stride, cgg_stream_t stream);

/* HOST function (no GPU work): rectangular linear sum assignment of n_problems f32 cost matrices (row-major, concatenated;
 * problem p is nr[p] x nc[p]) -- the Hungarian matching of open_set/assigners/mask_hungarian_assigner.py:126-131, which the
 * reference solves one matrix at a time with scipy.optimize.linear_sum_assignment. Same algorithm (Crouse 2016), scan order
 * and tie rule as scipy, so the INDICES agree, not only the cost. rows / cols: min(nr[p], nc[p]) pairs per problem,
 * concatenated, rows ascending. CGG_EINVAL for NaN / -inf entries, CGG_EUNSUPPORTED for an infeasible matrix.         */
int cgg_linear_sum_assignment_f32(const float* cost, int n_problems, const int* nr, const int* nc, int64_t* rows,
                                  int64_t* cols);

/* The same assignment on the DEVICE (csrc/lsap_device.hip): one launch, one wavefront per problem, the cost matrix and the
 * solver's state in LDS; same algorithm, f64 arithmetic, scan order and tie rule as the host function above, so the INDICES
 * are its (and scipy's). cost: flat f32 device buffer of cost_numel elements. desc: n_problems x 6 int64 on the device, per
 * problem: cost offset, nr, nc (1 .. 1024 each), output offset, label-row offset, gt-label offset (all in elements).
 * lds_bytes: the largest cgg_lsap_device_lds_bytes(nr, nc) of the table (<= cgg_dynamic_lds_limit()). Problem p writes
 * min(nr, nc) pairs at q_out / g_out[output offset ...], rows ascending as scipy returns them (out_numel elements each).
 * Optional epilogue (gt_labels, labels, weights all non-null): labels[label-row offset + q] = gt_labels[gt-label offset + g]
 * and weights[label-row offset + q] = 1 for every pair (gt_numel / rows_numel elements). status: two int32 words, 8-byte
 * aligned, that the caller zeroes; they keep [code, problem + 1] of the failing problem with the lowest index (a word that is
 * already non-zero is only replaced by a lower index): 1 = NaN / -inf entries, 2 = infeasible (both write the identity
 * pairing k -> (k, k), in range for every consumer), 3 = a descriptor that does not fit the buffers or lds_bytes (nothing
 * written). The other problems of the launch are unaffected; nothing here waits for the device.                          */
#define CGG_LSAP_MAX_SIDE 1024 /* sides of a problem */
int64_t cgg_lsap_device_lds_bytes(int nr, int nc);
int cgg_lsap_device_f32(const float* cost, int64_t cost_numel, const int64_t* desc, int n_problems, int64_t lds_bytes,
                        int64_t* q_out, int64_t* g_out, int64_t out_numel, const int64_t* gt_labels, int64_t gt_numel,
                        int64_t* labels, float* weights, int64_t rows_numel, int32_t* status, cgg_stream_t stream);
/* The most dynamic LDS a workgroup may request on the current device (160 KiB, gfx950's, when there is no device).      */
int64_t cgg_dynamic_lds_limit(void);

/* [3P] mmcv.ops.point_sample (= F.grid_sample(2 p - 1, bilinear, zeros, align_corners=False)) on a CHANNEL-LAST f32 map:
 * out[b, p, :] = bilinear sample of feat[b] (H, W, C) at pts[b, p] = (x, y) in [0, 1]; taps outside the map contribute 0.
 * Used for sample(E F) = E sample(F) at the matching points of all decoder layers (mask2former_head.py:357-366). C % 4 == 0. */
int cgg_point_sample_nhwc(const float* feat, const float* pts, float* out, int B, int H, int W, int C, int P,
                          cgg_stream_t stream);
/* Same sampling of single-channel f32 planes [N, H, W] with a plane index per output row: out[j, p] = sample of
 * planes[index[j]] at pts[j, p] (pts [rows, P, 2], out [rows, P]). Used for the matched queries' ground-truth mask targets
 * (mask2former_head.py:609-612): one launch per decoder layer for all images.                                          */
int cgg_point_sample_planes(const float* planes, const int32_t* index, const float* pts, float* out, int N, int H, int W,
                            int rows, int P, cgg_stream_t stream);
/* Backward of cgg_point_sample_planes wrt the planes (points are constants): grad_planes (N, H, W), ZEROED by the caller,
 * accumulates the tap weights x grad_out (rows, P) with f32 atomics; index nullable = row j samples plane j. Replaces
 * F.grid_sample's backward (which also computes the unused grid gradient) at open_set/models/mask2former_head.py:609-620. */
int cgg_point_sample_planes_backward(const float* grad_out, const int32_t* index, const float* pts, float* grad_planes, int N,
                                     int H, int W, int rows, int P, cgg_stream_t stream);
/* ... for rows that each have their OWN plane (the loss' mask planes of the positives): grad_planes (rows, H, W) is overwritten -- no
 * zero-fill, no global atomics (a workgroup accumulates a band of one plane in LDS and writes it once). */
int cgg_point_sample_planes_backward_rows(const float* grad_out, const float* pts, float* grad_planes, int H, int W, int rows, int P,
                                          cgg_stream_t stream);

/* Stem convolution of the BN-folded [3P] mmdet ResNet (conv1: 7x7, stride 2, padding 3, 3 -> 64 channels) straight from
 * the f32 NCHW image: out[B, Ho, Wo, 64] bf16 channel-last = RAW convolution (no bias; bf16 operands, f32 accumulation),
 * Ho = (H - 1) / 2 + 1. w_packed: cgg_stem_conv7x7_packed_bytes() bytes, bf16 MFMA A fragments
 * [2 m-tiles][11 k-steps][64 lanes][8] of W[64, 176] with k = ky * 24 + kx * 3 + c (zero elsewhere).              */
int64_t cgg_stem_conv7x7_packed_bytes(void);
int cgg_stem_conv7x7_nchw(const float* img, const void* w_packed, void* out, int B, int H, int W, cgg_stream_t stream);

/* y[B, Ho, Wo, C] = x[B, ::stride, ::stride, C] (channel-last bf16, Ho = (H - 1) / stride + 1): the input of a stride-2 1x1
 * downsample convolution ([3P] mmdet ResNet, style='pytorch') as a contiguous GEMM operand.                           */
int cgg_subsample_nhwc(const void* x, void* y, int B, int H, int W, int C, int stride, cgg_stream_t stream);

/* Stem tail of the BN-folded [3P] mmdet ResNet (`maxpool(relu(bn1(conv1(x))))`), channel-last bf16, one pass:
 *   y[B, Ho, Wo, C] = relu(maxpool3x3/s2/p1(x[B, H, W, C]) + bias[C]),  Ho = (H - 1) / 2 + 1 (same for W).          */
int cgg_bias_relu_maxpool_nhwc(const void* x, const void* bias, void* y, int B, int H, int W, int C,
                               cgg_stream_t stream);

/* K9  GroupNorm (+ optional ReLU) of the pixel decoder ConvModules ([3P] MSDeformAttnPixelDecoder,
 * norm_cfg=dict(type='GN', num_groups=32), configs/instance/coco_b48n17.py:40).
 *   x, y [B, C, H, W] f32 NCHW; gamma, beta [C]; ws = cgg_group_norm_workspace_bytes(...) bytes.
 * Requires C % groups == 0 (float4 path when H*W % 4 == 0).                                                    */
int64_t cgg_group_norm_workspace_bytes(int B, int C, int H, int W, int groups);
int cgg_group_norm(const float* x, const float* gamma, const float* beta, float* y, void* ws, int B, int C,
                   int H, int W, int groups, float eps, int relu, cgg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K19  Inference tail.
 *
 * cgg_upsample_bilinear: F.interpolate(x, (h, w), 'bilinear', align_corners=False) for
 * [N, H, W] -> [N, h, w] f32 (open_set/models/mask2former_head.py:960-964,
 * open_set/models/maskformer_fusion_head.py:421-425).
 *
 * cgg_instance_masks: fused "upsample -> (>0) -> mask score -> bbox" of
 * MaskFormerFusionHeadOpen.instance_postprocess_emb (maskformer_fusion_head.py:349-363) for the
 * selected queries, reading the LOW-RES logits, so the (Q, H_img, W_img) f32 tensor is never
 * written:
 *   logits [Q, H, W] f32;  sel [n] int32 query index per detection
 *   (up_h, up_w): batch_input_shape the head upsamples to (mask2former_head.py:957-964)
 *   (crop_h, crop_w): img_shape crop (maskformer_fusion_head.py:415-416)
 *   (out_h, out_w): ori_shape when `rescale` (:418-425), else == crop
 *   masks  [n, out_h, out_w] u8 (0/1);  mask_score [n] f32 = sum(sigmoid*[m>0]) / (sum[m>0]+1e-6);
 *   bbox [n, 4] f32 (x0, y0, x1+1, y1+1), zeros for an empty mask ([3P] mmdet mask2bbox)
 *   ws     scratch, n * 32 bytes
 *
 * cgg_panoptic_argmax: per-pixel argmax_k score[k] * sigmoid(resized logit[keep[k]])
 * (maskformer_fusion_head.py:100-120) fused with the resize; first max wins (torch.argmax).
 *   ids [out_h, out_w] int32 in [0, n);  win_half [out_h, out_w] u8 = winner's sigmoid >= 0.5
 *   counts [n, 3] int32: #(id == k), #(sigmoid_k >= 0.5), #(id == k && sigmoid_k >= 0.5)
 *   -- the three areas the segment loop of :122-157 needs (one D2H instead of 3 .item() per query)
 * cgg_panoptic_paint: seg[p] = lut_val[ids[p]] if lut_val >= 0 and (!lut_half[id] || win_half[p])
 *   else void_label  (the decisions of :129-157 applied in one pass).
 * ---------------------------------------------------------------------------------------------- */
int cgg_upsample_bilinear(const float* x, float* y, int N, int H, int W, int h, int w,
                          cgg_stream_t stream);
int cgg_instance_masks(const float* logits, const int32_t* sel, uint8_t* masks, float* mask_score,
                       float* bbox, void* ws, int Q, int H, int W, int up_h, int up_w, int crop_h,
                       int crop_w, int out_h, int out_w, int n, cgg_stream_t stream);
/* Multi-destination variant for the three evaluation types of one image (all / novel / base class sets,
 * maskformer_fusion_head.py:385-400): instance i is QUERY i (no `sel`), its mask is interpolated once and stored to every
 * slot dest_slot[dest_off[i] .. dest_off[i+1]) of masks [n_slots, out_h, out_w]; queries with no slot are skipped.
 * mask_score [Q], bbox [Q, 4] are per query (undefined for skipped queries); ws: Q * 32 bytes.                    */
int cgg_instance_masks_multi(const float* logits, const int32_t* dest_off, const int32_t* dest_slot, uint8_t* masks,
                             float* mask_score, float* bbox, void* ws, int Q, int H, int W, int up_h, int up_w,
                             int crop_h, int crop_w, int out_h, int out_w, cgg_stream_t stream);

/* Open-vocabulary (query, class) picks of MaskFormerFusionHeadOpen.instance_postprocess_emb
 * (open_set/models/maskformer_fusion_head.py:297-347) for all evaluation types and images in one launch.
 * dots [B*Q, ld] f32 = class-embedding predictions x concatenated class tables; type t owns columns
 * col0[t] .. col0[t] + ncols[t], the last one being the background class: prob = softmax over the type's columns,
 * background dropped, then the k best of the Q * (ncols[t] - 1) pairs. Outputs [B, n_types, k]: labels (class),
 * scores (class probability), qidx (query). topk(sorted=False) leaves order / ties open; here: descending score, ties
 * by ascending flat index. col0_host / ncols_host: n_types ints on the HOST. Limits: k <= 1024, n_types <= 8,
 * k <= Q * (ncols-1), 8k + 4Q * max(ncols-1) + 4Q <= 62 KiB of LDS (CGG_EUNSUPPORTED otherwise).                 */
int cgg_class_topk(const float* dots, int ld, int B, int Q, int n_types, const int* col0_host, const int* ncols_host,
                   int k, int64_t* labels, float* scores, int64_t* qidx, cgg_stream_t stream);

/* The rest of :349-363 for ONE image and all its picks (all evaluation types concatenated): every picked query's mask
 * is interpolated once and stored into each detection slot that picked it (as cgg_instance_masks_multi, the slot plan
 * now built on the device), then bboxes[j] = (box of query qidx[j], cls_scores[j] * mask_score[qidx[j]]).
 * masks [n_picks, out_h, out_w] u8, bboxes [n_picks, 5] f32, ws: cgg_instance_masks_picks_workspace_bytes(Q, n_picks).
 * bitpack != 0: masks [n_picks, out_h, out_w / 8] bytes, pixel x = bit (x & 7) of byte x >> 3 -- 8x fewer bytes for a
 * host-side consumer to copy (integer up-scale 2 / 4 / 8 without a second resize, out_w % 16 == 0; else CGG_EUNSUPPORTED). */
int64_t cgg_instance_masks_picks_workspace_bytes(int Q, int n_picks);
int cgg_instance_masks_picks(const float* logits, const int64_t* qidx, const float* cls_scores, int n_picks,
                             uint8_t* masks, float* bboxes, void* ws, int Q, int H, int W, int up_h, int up_w,
                             int crop_h, int crop_w, int out_h, int out_w, int bitpack, cgg_stream_t stream);
int cgg_panoptic_argmax(const float* logits, const int32_t* keep, const float* score, int32_t* ids,
                        uint8_t* win_half, int32_t* counts, int Q, int H, int W, int up_h, int up_w,
                        int crop_h, int crop_w, int out_h, int out_w, int n, cgg_stream_t stream);
int cgg_panoptic_paint(const int32_t* ids, const uint8_t* win_half, const int32_t* lut_val,
                       const int32_t* lut_half, int32_t* seg, int64_t npix, int void_label,
                       cgg_stream_t stream);

/* Batched panoptic fusion (maskformer_fusion_head.py:77-225) with no host read: select (keep = label != num_classes &&
 * score > object_mask_thr, compacted in query order), tiled argmax of score * sigmoid(resized logit) with the three areas
 * per kept query, the segment decisions (`maskformer_fusion_head.panoptic_decide_host` states the rule) and the painted
 * map, for B images in four launches (the select kernel zeroes the counters: no memset node). Every data-dependent size is
 * read from device memory by the kernels: no allocation, no synchronisation, legal under stream capture and replayable on
 * new data.
 *   logits [B, Q, H, W] f32;  score [B, Q] f32 and label [B, Q] int64 as cgg_rowwise_softmax_argmax writes them
 *   geom   DEVICE [B, 5] int64: crop_h, crop_w, out_h, out_w, first pixel of the image in `seg`. up_h, up_w, H, W are
 *          shared. A row with crop outside (up_h, up_w), out outside (max_out_h, max_out_w) or pixels outside
 *          [0, total_out_pixels) is skipped by every kernel (its pixels stay unwritten).
 *   seg    [total_out_pixels] int32, image b at geom[b][4] as [out_h, out_w]: category + instance_id * 1000 for things,
 *          the category for stuff, num_classes for void
 *   n_kept [B] int32;  kept_score [B, Q] f32 in slot order (0 past n_kept)
 *   segments [B, Q, 4] int32, row k = the image's k-th kept query: value in the map (-1: nothing painted), category,
 *          painted area, query index; rows past n_kept are -1, -1, 0, -1
 *   ws     cgg_panoptic_fuse_batched_workspace_bytes(B, Q, total_out_pixels) bytes (4-byte aligned); its first 2 * B
 *          int32 count, per image, the argmax blocks that staged their footprint in LDS and those that read global memory
 *          (a tile whose footprint leaves room for fewer than 8 queries in the 32 KB window)
 * defer_stuff = 1 is the `_emb` variant (stuff after the things, unfiltered area >= stuff_area_limit, painted without
 * the 0.5 filter); 0 paints stuff in query order. CGG_EINVAL: null pointer, bad sizes, workspace too small;
 * CGG_EUNSUPPORTED: Q > 1024 (the LDS histogram is sized by Q). */
#define CGG_PANOPTIC_FUSE_MAX_Q 1024 /* queries of one image */
int64_t cgg_panoptic_fuse_batched_workspace_bytes(int B, int Q, int64_t total_out_pixels);
int cgg_panoptic_fuse_batched(const float* logits, const float* score, const int64_t* label, const int64_t* geom,
                              int32_t* seg, int32_t* n_kept, int32_t* segments, float* kept_score, void* ws,
                              int64_t ws_bytes, int B, int Q, int H, int W, int up_h, int up_w, int max_out_h,
                              int max_out_w, int64_t total_out_pixels, int num_classes, int num_things,
                              float object_mask_thr, double iou_thr, int filter_low_score, int stuff_area_limit,
                              int defer_stuff, cgg_stream_t stream);

/* Row-wise softmax + max/argmax: scores = softmax(x) over the last dim, one wavefront per row
 * (MaskFormerFusionHeadOpen.get_cls_emb_scores, maskformer_fusion_head.py:297-315, and the
 * `.max(-1)` at :99).  x [rows, n] f32 -> prob [rows, n] f32 (nullable), maxv [rows] f32,
 * argmax [rows] int64 (first max wins). argmax always lies in [0, n): NaN entries take no part in
 * the maximum, and a row of nothing but NaN returns 0 (its maxv and prob are NaN).               */
int cgg_rowwise_softmax_argmax(const float* x, float* prob, float* maxv, int64_t* argmax, int rows,
                               int n, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * COCO mask evaluation on the device (csrc/mask_eval.hip). `mask_eval.py` states the rules in numpy
 * (mask_intersections_host, mask_iou_host, evaluate_img_host) and the kernels equal them exactly: integers, and IEEE double
 * operations in a fixed order. All pointers DEVICE; everything runs on `stream`; no host read, no allocation, no atomics:
 * legal under stream capture.
 *
 * cgg_mask_intersections_bits: inter[d][g] = set pixels of det plane d AND gt plane g, area_d[d], area_g[g] = set pixels of
 *   each plane. Planes as cgg_rle_transitions reads them: H rows x row_bytes bytes, plane i at bits + i * stride_bytes, pixel x
 *   of a row = bit (x & 7) of byte (x >> 3); only the first W pixels of a row count, pad bits may hold anything. Both sides share
 *   H, W and row_bytes. A workgroup stages a slab of rows of up to 64 + 64 planes in LDS (16-byte loads when pointer, stride
 *   and row_bytes are multiples of 16, 4-byte or byte loads otherwise; the pad bits are masked there, once) and each thread keeps
 *   a 4 x 4 register tile of pairs: one AND and one count-add per 32 pixels and pair. Slab groups write int32 partials to ws, a
 *   second launch adds them. ws: cgg_mask_intersections_workspace_bytes(D, G, H, W) bytes, 4-byte aligned.
 *   D = 0 or G = 0 is legal (the areas of the other side are still written; both 0: nothing is launched).
 *   CGG_EINVAL: null pointer, D, G < 0, H, W < 1, row_bytes * 8 < W, a stride below H * row_bytes, misaligned ws / outputs.
 *   CGG_EUNSUPPORTED: D > 1024, G > 1024, H * W >= 2^31.
 *
 * cgg_coco_match: COCOeval.evaluateImg for every (category k, area range a, threshold t) of one image, one thread each.
 *   inter / area_d / area_g as written above; det_order int32[D] = the detections in stable descending score order; det_cats
 *   int32[D], gt_cats int32[G], gt_crowd uint8[G], gt_area double[G] (the annotation's own area); cat_ids int32[K]; area_rngs
 *   double[A][2] = (lo, hi); iou_thrs double[T]. IoU = (double)inter / (double)(area_d + area_g - inter), for a crowd
 *   (double)inter / (double)area_d, 0 where the denominator is 0. Detections of category k (every detection when
 *   class_agnostic) in det_order, cut to max_det; ground truths of category k, those that count first, the ignored ones (crowd,
 *   or gt_area < lo or > hi) after them, original order within each group; greedy scan with best = min(t, 1 - 1e-10): a
 *   matched non-crowd ground truth is skipped, the ignored ones are not scanned once one that counts has matched, `iou < best`
 *   continues (a later equal IoU wins).
 *   dt_match int32[K][A][T][D]: row (k, a, t) holds, for the D_k detections in that order, 0 or 1 + the matched ground truth's
 *   index in the image; dt_ignore uint8[K][A][T][D]: the match is an ignored ground truth, or unmatched with area_d outside
 *   (lo, hi); gt_ignore uint8[K][A][G]: the G_k ground truths in scan order; counts int32[K][2] = (D_k, G_k). Entries past D_k /
 *   G_k are written as 0.
 *   CGG_EINVAL: null pointer, K, A, T < 1, D, G, max_det < 0, misaligned doubles. CGG_EUNSUPPORTED: T > 64, A > 8, K > 1024,
 *   D > 1024, G > 1024.
 *
 * cgg_box_iou_f64: the box side of COCOeval.computeIoU (`--eval bbox`), equal to mask_eval.box_iou_host bit for bit.
 *   det_boxes5 float[D][5] = (x0, y0, x1, y1, score) as the results hold them: every coordinate is widened to double, then the
 *   detection is (x0, y0, x1 - x0, y1 - y0) in double. gt_boxes_xywh double[G][4] = (x, y, w, h); gt_crowd uint8[G].
 *   Per pair, with D the detection and G the ground truth: da = D.w * D.h, ga = G.w * G.h;
 *   w = fmin(D.w + D.x, G.w + G.x) - fmax(D.x, G.x), 0 if w <= 0; h likewise on y, 0 if h <= 0; i = w * h;
 *   u = da for a crowd, else (da + ga) - i; iou = i / u. Every operation is an IEEE double operation of its own (no product is
 *   fused into an add). iou double[D][G]; area_d double[D] = da. D = 0 or G = 0 is legal (G = 0: the areas alone).
 *   CGG_EINVAL: null pointer, D, G < 0, misaligned pointers. CGG_EUNSUPPORTED: D > 1024, G > 1024.
 *
 * cgg_coco_match_boxes: cgg_coco_match with the IoU of cgg_box_iou_f64 in place of inter / area_d / area_g (the same kernel
 *   template: one scan, two IoU sources); the detection's own area, for the area ranges, is da. Every other argument, the
 *   outputs, their layouts and the error codes are those of cgg_coco_match. One launch, no workspace.
 * ---------------------------------------------------------------------------------------------- */
int cgg_box_iou_f64(const float* det_boxes5, int D, const double* gt_boxes_xywh, const uint8_t* gt_crowd, int G, double* iou,
                    double* area_d, cgg_stream_t stream);
#define CGG_MASK_EVAL_MAX_THRS 64    /* IoU thresholds, area ranges and categories of one cgg_coco_match / cgg_coco_match_boxes call */
#define CGG_MASK_EVAL_MAX_AREAS 8
#define CGG_MASK_EVAL_MAX_CATS 1024
int cgg_coco_match_boxes(const float* det_boxes5, const double* gt_boxes_xywh, const int32_t* det_order, const int32_t* det_cats,
                         const int32_t* gt_cats, const uint8_t* gt_crowd, const double* gt_area, const int32_t* cat_ids, int K,
                         const double* area_rngs, int A, const double* iou_thrs, int T, int D, int G, int max_det,
                         int class_agnostic, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, int32_t* counts,
                         cgg_stream_t stream);
#define CGG_MASK_EVAL_MAX_MASKS 1024 /* planes (or boxes) on each side of an intersection table */
int64_t cgg_mask_intersections_workspace_bytes(int D, int G, int H, int W);
int cgg_mask_intersections_bits(const uint8_t* det_bits, int D, int64_t det_stride_bytes, const uint8_t* gt_bits, int G,
                                int64_t gt_stride_bytes, int H, int W, int row_bytes, void* ws, int32_t* inter, int32_t* area_d,
                                int32_t* area_g, cgg_stream_t stream);
int cgg_coco_match(const int32_t* inter, const int32_t* area_d, const int32_t* area_g, const int32_t* det_order,
                   const int32_t* det_cats, const int32_t* gt_cats, const uint8_t* gt_crowd, const double* gt_area,
                   const int32_t* cat_ids, int K, const double* area_rngs, int A, const double* iou_thrs, int T, int D, int G,
                   int max_det, int class_agnostic, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, int32_t* counts,
                   cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Panoptic-quality evaluation on the device (csrc/pq_eval.hip). `pq_eval.py` states the rule in numpy (pq_image_host, a
 * restatement of the loop body of the reference's pq_compute_single_core) and the kernels equal it exactly: integer counts, and
 * one IEEE double quotient of two integers per pair. All pointers DEVICE; everything runs on `stream`; no host read, no
 * allocation, no memset node: legal under stream capture.
 *
 * cgg_pq_confusion_i32: ws[g][p] = pixels of an H x W image whose ground-truth id has slot g and whose pred value has slot p, an
 *   int32 table of (G + 2) x (P + 1) cells followed by two status words; ws: cgg_pq_confusion_workspace_bytes(G, P) bytes, which
 *   a first launch zeroes. pred: int32[H * W]. gt: int32[H * W] (gt_rgb = 0) or uint8[H * W * 3] RGB with id = R + 256 G +
 *   65536 B (gt_rgb = 1). Rows: 0 = id 0 (VOID), 1 + i = gt_ids[i] (ids >= 0; an id listed twice counts into its first slot),
 *   G + 1 = any other id. Columns: 0 = void, 1 + k = row k of `table`, int32[P][4] rows [value, category, area, query] as
 *   cgg_panoptic_fuse_batched writes them, of which the first *n_kept (read on the device, clamped to 0 .. P) are valid; rows
 *   with value < 0 or area <= 0 are dropped and equal values count into the first of their rows. A pred pixel is void iff
 *   value % 1000 == num_classes, or it is 0 and not in the table; any other value that is not in the table sets bit 1 of status
 *   word 0 and leaves the smallest such value in status word 1 (INT_MAX when there is none).
 *   Loads are 16 bytes wide where pred / gt are 16-byte aligned (RGB: 4-byte aligned), narrower otherwise.
 *   CGG_EINVAL: null or misaligned pointer, H, W < 1, G, P, num_classes < 0. CGG_EUNSUPPORTED: H * W >= 2^31, G or P > 4096, or
 *   cgg_pq_eval_lds_bytes(G, P) (the table and both id -> slot tables, held in LDS by every workgroup) above
 *   cgg_dynamic_lds_limit(); cgg_pq_eval_lds_bytes answers -1 for sizes outside 0 .. 4096.
 *
 * cgg_pq_match: from `ws` as written above, for one image: gt_cats int32[G] and the table's category column are compared as
 *   opaque integers; gt_crowd uint8[G]; gt_area int32[G] (the records' areas). Pred areas are the column sums. For a
 *   non-crowd ground truth g and a segment row k of equal category with inter = ws[1 + g][1 + k] > 0: iou = (double)inter /
 *   (double)(area_k + gt_area[g] - inter - ws[0][1 + k]), matched iff iou > 0.5. gt_match[g] = the matched row or -1, gt_iou[g]
 *   its iou (0 without a match). pred_flags[k]: 1 = row k is a segment (valid, first of its value), 2 = matched, 4 = unmatched
 *   and ignored: (ws[0][1 + k] + ws[1 + c][1 + k]) / area_k > 0.5 in double, c the LAST crowd of the row's category in gt order.
 *   pred_area[k], pred_value[k] (-1 for a row that is no segment), pred_cat[k]. status[0] = the confusion's status word, with
 *   bit 2 for a segment row without pixels and bit 4 for a ground truth with more than one match (gt_match keeps the first
 *   row); status[1] as above. gt_iou 8-byte aligned. Error codes as above.
 * ---------------------------------------------------------------------------------------------- */
#define CGG_PQ_EVAL_MAX_SEGMENTS 4096 /* G and P (the LDS limit binds first for all but very lopsided shapes) */
int64_t cgg_pq_eval_lds_bytes(int G, int P);
int64_t cgg_pq_confusion_workspace_bytes(int G, int P);
int cgg_pq_confusion_i32(const int32_t* pred, const void* gt, int gt_rgb, int H, int W, const int32_t* gt_ids, int G,
                         const int32_t* table, const int32_t* n_kept, int P, int num_classes, int32_t* ws, cgg_stream_t stream);
int cgg_pq_match(const int32_t* ws, const int32_t* gt_cats, const uint8_t* gt_crowd, const int32_t* gt_area, int G,
                 const int32_t* table, const int32_t* n_kept, int P, int32_t* status, double* gt_iou, int32_t* gt_match,
                 int32_t* pred_area, int32_t* pred_value, int32_t* pred_cat, uint8_t* pred_flags, cgg_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Caption metrics on the device (csrc/caption_eval.hip): the integer parts of BLEU-1..4 and ROUGE-L and the ordered double sums
 * of CIDEr. `caption_eval.py` states the rules in plain Python (bleu_components_host, lcs_host, ngram_df_host, cider_sums_host)
 * and the kernels equal them exactly: integers, and double sums whose every product and add is rounded on its own, in the
 * rule's order. All pointers DEVICE; everything runs on `stream`; no host read, no allocation.
 *
 * The corpus: N images, S sentences, the first sentence of an image its hypothesis, the others its references (P = S - N
 * pairs, pair p = sentence index - image index - 1). img_off int32[N + 1]: first sentence of every image, img_off[N] = S.
 * sent_off int32[S + 1]: first word of every sentence in `words` int32[W], token ids 1 .. 65535. One workgroup of one wave per
 * image, the image's words staged in LDS. The caps come from that layout and are not measured: a sentence holds at most
 * CGG_CAPTION_MAX_LEN tokens and an image at most CGG_CAPTION_MAX_REFS references, so that (32 + 1) * 128 staged words (16.5
 * KiB) and the other tables of a kernel -- the 129 x 64 uint16 LCS rows (16.1 KiB), or the term counts of one order (16.3 KiB)
 * -- stay under the 64 KiB of static LDS. An image beyond a cap, or whose offsets are not ascending within 0 .. W, is NOT
 * evaluated and touches nothing out of bounds: its int32 outputs are -1, its keys 0, its flags 0, its sums -1.0.
 *
 * cgg_caption_bleu_lcs_i32: bleu int32[N][10] = testlen, the closest reference length (min of (|l - testlen|, l): a tie takes
 *   the shorter; 0 without references), guess[k] = max(0, testlen - k), correct[k] = sum over the distinct hypothesis
 *   (k + 1)-grams of min(count, max over the references of their count), k = 0 .. 3, from `words` / `sent_off`; lcs int32[P] =
 *   the length of the longest common subsequence of hypothesis and reference in the second token stream `words_sp` /
 *   `sent_off_sp` (W_sp words), which cuts the same sentences differently.
 * cgg_caption_ngram_keys_i64: keys int64[W][4]: for the word at position i of its sentence and order k, the ids of words
 *   i .. i + k packed 16 bits each, the first lowest; 0 where the sentence ends before i + k. flags uint8[W][4]: 1 iff the
 *   position lies in a reference and no earlier position of the references of its image has the same key.
 * cgg_cider_sums_f64: gids int32[W][4] = an id in 0 .. U - 1 per key (ignored where the n-gram does not exist), df int32[U] the
 *   document frequency of every id, idf_by_df double[N + 1] the host-made table idf(df). With tf = the count of an n-gram in its
 *   sentence and v = (double)tf * idf: norm2 double[S][4] = sum of v * v over the sentence's distinct n-grams of that order in
 *   order of first occurrence; num double[P][4] = sum over the hypothesis' distinct n-grams, in that order, of
 *   min(v_hyp, v_ref) * v_ref, v_ref = 0.0 for an n-gram the reference lacks. No contraction. An id outside 0 .. U - 1 or a
 *   df outside 0 .. N reads entry 0.
 * CGG_EINVAL: a null pointer with work to do, a negative size, S < N, keys / sums not 8-byte aligned. CGG_EUNSUPPORTED: more than
 * 2^28 words or sentences (the [W][4] indices stay in int32). N = 0 is legal and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
#define CGG_CAPTION_MAX_LEN 128
#define CGG_CAPTION_MAX_REFS 32
int cgg_caption_bleu_lcs_i32(const int32_t* words, const int32_t* sent_off, int W, const int32_t* words_sp, const int32_t* sent_off_sp,
                             int W_sp, const int32_t* img_off, int N, int S, int32_t* bleu, int32_t* lcs, cgg_stream_t stream);
int cgg_caption_ngram_keys_i64(const int32_t* words, const int32_t* sent_off, int W, const int32_t* img_off, int N, int S,
                               int64_t* keys, uint8_t* flags, cgg_stream_t stream);
int cgg_cider_sums_f64(const int32_t* gids, const int32_t* df, int U, const double* idf_by_df, const int32_t* sent_off, int W,
                       const int32_t* img_off, int N, int S, double* norm2, double* num, cgg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CGG_HIP_H_ */
