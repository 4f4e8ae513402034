"""`MaskFormerFusionHeadOpen` -- open-vocabulary post-processing of the reference
(open_set/models/maskformer_fusion_head.py:15-464) on the HIP inference-tail kernels.

Class scores are `softmax(emb @ class_embs^T)` WITHOUT temperature (:312-313).
Differences in execution, not in results:
  * masks arrive as low-resolution logits + resize geometry (`LowResMasks`); "upsample to
    batch_input_shape -> crop img_shape -> (rescale to ori_shape)" is evaluated on the fly inside
    `cgg_instance_masks` / `cgg_panoptic_argmax`, so the (Q, H_img, W_img) f32 tensor is never stored;
  * the panoptic segment loop (:122-157) needs three areas per kept query; they come back from the
    device in ONE copy instead of three `.item()` syncs per query, and the decisions are painted by a
    LUT kernel (`panoptic_postprocess{,_emb}`, one image per call: the comparison side and the fallback);
  * `panoptic_postprocess_batched` (what `simple_test` uses for Q <= 1024) does the same for the whole batch with NO
    host read: (1) one matmul + one `rowwise_softmax_argmax` over B*Q rows, (2) a device geometry table built once per
    (metas, rescale), (3) `cgg_panoptic_fuse_batched`: the kept queries are selected and compacted on the device, the
    argmax stages each tile's low-resolution footprint in LDS, the segment loop runs as a kernel
    (`panoptic_decide_host` is its written rule) and the map is painted from its table -- four launches that a hipGraph
    can hold, (4) a segment table (value, category, area, query) per image comes back with the map
    (`with_segments`, `segments_info`);
  * `PER_IMAGE_PANOPTIC = True` (module attribute) makes `simple_test` take the per-image path.
"""
import json

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .config import to_config_dict
from .mask2former_head import LowResMasks
from .registry import HEADS

INSTANCE_OFFSET = 1000  # [3P] mmdet.core.evaluation.panoptic_utils.INSTANCE_OFFSET


PER_IMAGE_PANOPTIC = False  # True: `simple_test` runs `panoptic_postprocess{,_emb}` per image (tests: the comparison side)


def panoptic_decide_host(classes, counts, num_things, iou_thr, filter_low_score, stuff_area_limit, defer_stuff):
    """The segment loop of :122-157 (`defer_stuff=True`, the `_emb` variant) / :195-222 (False) on the three areas per kept
    query -- the written rule `cgg_panoptic_fuse_batched`'s decide kernel follows.

    classes: one class per kept query, in query order; counts (n, 3) as `cgg_panoptic_argmax` writes them: #(id == k),
    #(sigmoid_k >= 0.5), #(id == k and sigmoid_k >= 0.5). Returns (lut_val, lut_half, area), lists of n ints: the value the
    paint step writes for slot k (-1: nothing), whether it writes only where the winner's sigmoid >= 0.5, and how many pixels
    it writes (counts[k][2] where lut_half[k] is set, otherwise counts[k][0]; 0 where lut_val[k] < 0).

    What a kernel writer needs:
      * a slot passes when both areas are > 0 and not `mask_area / original_area < iou_thr` -- a float64 division compared
        with a float64 threshold (a ratio of exactly iou_thr passes);
      * the instance id of a thing is 1 + the number of things accepted EARLIER in query order;
      * a thing whose filtered area (counts[k][2]) is 0 still consumes an id: the test uses the unfiltered areas;
      * stuff of the plain variant is painted where it stands in query order, filtered like a thing;
      * stuff of the `_emb` variant is painted after all things, on still-void pixels -- the argmax partition is disjoint, so
        that is all of (id == k) -- when that UNFILTERED area is >= stuff_area_limit, and WITHOUT the 0.5 filter."""
    n = len(classes)
    cnt = [int(v) for row in counts for v in row]
    classes = [int(c) for c in classes]
    lut_val = [-1] * n
    lut_half = [0] * n
    instance_id = 1
    stuff = []
    for k in range(n):
        pred_class = classes[k]
        isthing = pred_class < num_things
        mask_area, original_area = cnt[3 * k], cnt[3 * k + 1]
        if mask_area > 0 and original_area > 0:
            if mask_area / original_area < iou_thr:
                continue
            if not isthing:
                if defer_stuff:
                    stuff.append(k)
                    continue
                lut_val[k] = pred_class
                lut_half[k] = 1 if filter_low_score else 0
            else:
                lut_val[k] = pred_class + instance_id * INSTANCE_OFFSET
                lut_half[k] = 1 if filter_low_score else 0
                instance_id += 1
    for k in stuff:
        # pasted onto still-void pixels only: the argmax partition is disjoint, so that is all of
        # (ids == k); the area test uses the UNFILTERED region (:151-157)
        if cnt[3 * k] < stuff_area_limit:
            continue
        lut_val[k] = classes[k]
        lut_half[k] = 0
    area = [0 if lut_val[k] < 0 else (cnt[3 * k + 2] if lut_half[k] else cnt[3 * k]) for k in range(n)]
    return lut_val, lut_half, area


def segments_info(table, n_kept, num_things, scores=None):
    """COCO-panoptic `segments_info` of one image from its segment table (rows [value, category, area, query index] of
    `panoptic_postprocess_batched(with_segments=True)`, the first `n_kept` are valid): stuff rows of one value merge (areas
    add; score and query are those of the first), rows that painted nothing (value < 0 or area 0) are dropped. Dicts
    id / category_id / isthing / area / score / query in order of first appearance."""
    rows = table.tolist() if hasattr(table, 'tolist') else [list(r) for r in table]
    sc = scores.tolist() if hasattr(scores, 'tolist') else scores
    out, by_id = [], {}
    for k in range(int(n_kept)):
        value, cat, area, query = (int(v) for v in rows[k])
        if value < 0 or area <= 0:
            continue
        if value in by_id:
            by_id[value]['area'] += area
            continue
        d = dict(id=value, category_id=cat, isthing=cat < num_things, area=area,
                 score=None if sc is None else float(sc[k]), query=query)
        by_id[value] = d
        out.append(d)
    return out


def _read_lines(path):
    with open(path, 'r', encoding='utf-8') as f:
        return f.read().split('\n')


@HEADS.register_module()
class MaskFormerFusionHeadOpen(nn.Module):

    def __init__(self, num_things_classes=65, num_stuff_classes=0, panoptic_mode=False, test_cfg=None,
                 loss_panoptic=None, init_cfg=None, **kwargs):
        super().__init__()
        # [3P] BasePanopticFusionHead
        self.num_things_classes = num_things_classes
        self.num_stuff_classes = num_stuff_classes
        self.num_classes = num_things_classes + num_stuff_classes
        self.test_cfg = to_config_dict(test_cfg) if test_cfg is not None else to_config_dict({})
        self.loss_panoptic = None
        if loss_panoptic:
            raise NotImplementedError('MaskFormerFusionHeadOpen has no training loss (forward_train -> {})')
        self.kwargs = kwargs
        self.panoptic_mode = panoptic_mode
        self.use_class_emb = kwargs.get('use_class_emb', False)
        self.known_file = kwargs.get('known_file', None)
        self.unknown_file = kwargs.get('unknown_file', None)
        if self.known_file is not None:
            self.known_cat_names = _read_lines(self.known_file)
        self.unknown_cat_names = _read_lines(self.unknown_file) if self.unknown_file is not None else []
        if self.use_class_emb:
            with open(kwargs['class_to_emb_file'], 'r') as f:
                class_to_emb = json.load(f)
            d = len(class_to_emb[0]['emb'])
            # buffer sizes exactly as :46-48 (incl. the trailing-'' quirk of unknown files)
            all_embs = torch.zeros((self.num_classes + 1, d), dtype=torch.float)
            novel_embs = torch.zeros((len(self.unknown_cat_names) + 1, d), dtype=torch.float)
            base_embs = torch.zeros((len(all_embs) - len(novel_embs) + 1, d), dtype=torch.float)
            names = []
            i = j = k = 0
            for cd in class_to_emb:
                if self.known_file and cd['name'] not in self.known_cat_names:
                    continue
                e = torch.FloatTensor(cd['emb'])
                if self.unknown_file:
                    if cd['name'] in self.unknown_cat_names:
                        novel_embs[j] = e
                        j += 1
                    else:
                        base_embs[k] = e
                        k += 1
                all_embs[i] = e
                names.append(cd['name'])
                i += 1
            self.register_buffer('all_class_embs', all_embs)
            self.register_buffer('novel_class_embs', novel_embs)
            self.register_buffer('base_class_embs', base_embs)
            self.all_classes = len(all_embs) - 1
            self.novel_classes = len(novel_embs) - 1
            self.base_classes = len(base_embs) - 1
            self.ordered_class_names = names

    @property
    def with_loss(self):
        return self.loss_panoptic is not None

    def forward_train(self, **kwargs):
        """MaskFormerFusionHead has no training loss."""
        return dict()

    # ------------------------------------------------------------------------------------------
    def get_cls_emb_scores(self, cls_emb_preds, gt_cls_embs):
        """:297-315 -- softmax(emb @ E^T), one wavefront per query row."""
        dots = torch.matmul(cls_emb_preds, gt_cls_embs.t()).contiguous()
        prob, _, _ = ops.rowwise_softmax_argmax(dots, want_prob=True)
        return prob

    @staticmethod
    def _geom(mask_pred, meta, rescale):
        """(logits (Q,h,w), up, crop, out) for one image."""
        if isinstance(mask_pred, LowResMasks):
            logits, up = mask_pred.logits, mask_pred.up_size
        else:  # an already-upsampled tensor: stage 1 degenerates to the identity
            logits, up = mask_pred, tuple(mask_pred.shape[-2:])
        crop = tuple(int(v) for v in meta['img_shape'][:2])
        crop = (min(crop[0], up[0]), min(crop[1], up[1]))
        out = tuple(int(v) for v in meta['ori_shape'][:2]) if rescale else crop
        return logits.contiguous(), up, crop, out

    def _topk(self, scores):
        """:340-347 given per-query class scores (Q, n) (background column already dropped):
        (labels, class scores, query indices) of the `max_per_image` best (query, class) pairs."""
        max_per_image = self.test_cfg.get('max_per_image', 100)
        n_cls = scores.shape[-1]
        flat = scores.flatten(0, 1)
        k = min(max_per_image, flat.numel())
        scores_per_image, top_indices = flat.topk(k, sorted=False)
        labels_per_image = top_indices % n_cls
        query_indices = torch.div(top_indices, n_cls, rounding_mode='floor')
        return labels_per_image, scores_per_image, query_indices

    def _batch_picks(self, emb_results, tables):
        """:297-347 for the whole batch and all evaluation types: ONE GEMM against the concatenated class tables and one
        `cgg_class_topk` launch -> (labels, class scores, query indices), each (B, T, k); None when the shapes are
        outside the kernel's limits (the per-type torch path then runs)."""
        if not (torch.is_tensor(emb_results) and emb_results.dim() == 3 and emb_results.is_cuda):
            return None
        B, Q, D = emb_results.shape
        ncols = [int(e.shape[0]) for e in tables]
        k = self.test_cfg.get('max_per_image', 100)
        if not ops.class_topk_supported(Q, ncols, k):
            return None
        from . import runtime
        cat = runtime.derived_cached('fusion_cls_cat', tuple(tables), lambda: torch.cat(list(tables), 0).float().contiguous())
        x = emb_results.reshape(B * Q, D).float()
        # 200 x 134 x 768: a BLAS library serves this with ONE workgroup (119 us measured); the skinny-linear kernel
        # (3 bf16 MFMAs on hi/lo operands, f32-class accuracy) spreads it over 10
        dots = ops.linear_rows(x, cat, split=True) if D % 16 == 0 else torch.matmul(x, cat.t())
        col0 = [sum(ncols[:t]) for t in range(len(ncols))]
        return ops.class_topk(dots, B, col0, ncols, k)

    def _instances_multi(self, picks, geom):
        """:349-363 for SEVERAL evaluation types of one image at once: picks = [(labels, class scores, query indices)];
        binary mask / mask score / bbox depend on the QUERY only, so every picked query's mask is interpolated once
        (`cgg_instance_masks_multi`) and stored straight into each type's detection slots -- no per-type gather pass
        over (n, H, W) masks. Returns [(labels, bboxes (n,5), masks (n,H,W) bool)] in the order of `picks`."""
        logits, up, crop, out = geom
        masks_l, qscores, qboxes = ops.instance_masks_multi(logits, [p[2] for p in picks], up, crop, out)
        res = []
        for (labels, cls_scores, qidx), masks in zip(picks, masks_l):
            det_scores = cls_scores * qscores.index_select(0, qidx)
            res.append((labels, torch.cat([qboxes.index_select(0, qidx), det_scores[:, None]], dim=-1), masks))
        return res

    def _geom_or_identity(self, mask_pred, meta, rescale):
        if meta is not None:
            return self._geom(mask_pred, meta, rescale)
        hw = tuple(mask_pred.shape[-2:])
        return mask_pred.contiguous(), hw, hw, hw

    def instance_postprocess_emb(self, mask_cls_emb, mask_pred, gt_cls_embs, meta=None, rescale=False):
        """:317-366 -> (labels (n,), bboxes (n,5) [x0,y0,x1,y1,score], masks (n,H,W) bool)."""
        geom = self._geom_or_identity(mask_pred, meta, rescale)
        scores = self.get_cls_emb_scores(mask_cls_emb, gt_cls_embs)[:, :-1]
        return self._instances_multi([self._topk(scores)], geom)[0]

    def instance_postprocess(self, mask_cls, mask_pred, meta=None, rescale=False):
        """:245-295 (closed-set variant on the classification logits)."""
        geom = self._geom_or_identity(mask_pred, meta, rescale)
        prob, _, _ = ops.rowwise_softmax_argmax(mask_cls.contiguous(), want_prob=True)
        labels, bboxes, masks = self._instances_multi([self._topk(prob[:, :-1])], geom)[0]
        is_thing = labels < self.num_things_classes
        return labels[is_thing], bboxes[is_thing], masks[is_thing]

    def _panoptic_from_scores(self, scores, labels, geom, defer_stuff):
        """shared body of :77-159 (defer_stuff=True) and :161-225 (False)."""
        logits, up, crop, out = geom
        thr = self.test_cfg.get('object_mask_thr', 0.8)
        iou_thr = self.test_cfg.get('iou_thr', 0.8)
        filter_low_score = self.test_cfg.get('filter_low_score', False)
        stuff_area_limit = self.test_cfg.get('stuff_area_limit', 4096)
        keep = labels.ne(self.num_classes) & (scores > thr)
        keep_idx = torch.nonzero(keep, as_tuple=False).squeeze(1)
        n = int(keep_idx.numel())                                   # host sync #1 (data-dependent size)
        if n == 0:
            return torch.full(out, self.num_classes, dtype=torch.int32, device=logits.device)
        cur_scores = scores[keep_idx].contiguous()
        ids, win_half, counts = ops.panoptic_argmax(logits, keep_idx.to(torch.int32).contiguous(),
                                                    cur_scores, up, crop, out)
        host = torch.cat([counts.flatten(), labels[keep_idx].to(torch.int32)]).cpu().tolist()  # sync #2
        cnt, classes = host[:3 * n], host[3 * n:]
        lut_val, lut_half, _ = panoptic_decide_host(classes, [cnt[3 * k:3 * k + 3] for k in range(n)], self.num_things_classes,
                                                    iou_thr, filter_low_score, stuff_area_limit, defer_stuff)
        dev = logits.device
        return ops.panoptic_paint(ids, win_half, torch.tensor(lut_val, dtype=torch.int32, device=dev),
                                  torch.tensor(lut_half, dtype=torch.int32, device=dev), self.num_classes)

    def panoptic_postprocess_emb(self, mask_cls_emb, mask_pred, gt_cls_embs, meta=None, rescale=False):
        """:77-159 -> (H,W) int32 map, `cls + instance_id * INSTANCE_OFFSET`, void = num_classes."""
        geom = self._geom(mask_pred, meta, rescale) if meta is not None else \
            (mask_pred.contiguous(), tuple(mask_pred.shape[-2:]), tuple(mask_pred.shape[-2:]),
             tuple(mask_pred.shape[-2:]))
        dots = torch.matmul(mask_cls_emb, gt_cls_embs.t()).contiguous()
        _, scores, labels = ops.rowwise_softmax_argmax(dots, want_prob=False)
        return self._panoptic_from_scores(scores, labels, geom, defer_stuff=True)

    def panoptic_postprocess(self, mask_cls, mask_pred, meta=None, rescale=False):
        """:161-225."""
        geom = self._geom(mask_pred, meta, rescale) if meta is not None else \
            (mask_pred.contiguous(), tuple(mask_pred.shape[-2:]), tuple(mask_pred.shape[-2:]),
             tuple(mask_pred.shape[-2:]))
        _, scores, labels = ops.rowwise_softmax_argmax(mask_cls.contiguous(), want_prob=False)
        return self._panoptic_from_scores(scores, labels, geom, defer_stuff=False)

    def _batched_geometry(self, up, img_metas, rescale, device):
        """`ops.panoptic_fuse_geometry` of (metas, rescale), built once and kept on the device: a pipeline's warm-up creates it
        before its graphs are captured, and the graphs replay its address."""
        crops, outs = [], []
        for meta in img_metas:
            crop = tuple(int(v) for v in meta['img_shape'][:2])
            crop = (min(crop[0], up[0]), min(crop[1], up[1]))
            crops.append(crop)
            outs.append(tuple(int(v) for v in meta['ori_shape'][:2]) if rescale else crop)
        key = (tuple(up), tuple(crops), tuple(outs), str(device))
        cache = self.__dict__.setdefault('_geometry_cache', {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) > 64:
                cache.clear()
            hit = cache[key] = ops.panoptic_fuse_geometry(outs, crops, device)
        from . import runtime
        runtime.keepalive(hit[0])
        return hit

    def panoptic_batched_supported(self, mask_pred_results):
        """the batched kernel's shape rules: (B, Q, h, w) logits with Q <= 1024 (the LDS histogram is sized by Q)"""
        logits = mask_pred_results.logits if isinstance(mask_pred_results, LowResMasks) else mask_pred_results
        return torch.is_tensor(logits) and logits.dim() == 4 and logits.is_cuda and logits.shape[1] <= ops.PANOPTIC_FUSE_MAX_Q

    def panoptic_postprocess_batched(self, scores_or_emb, mask_pred_results, img_metas, rescale=False, emb=True,
                                     with_segments=False, debug=False):
        """`panoptic_postprocess_emb` (emb=True: (B, Q, D) embeddings against `all_class_embs`) or `panoptic_postprocess`
        (emb=False: (B, Q, num_classes + 1) classification logits) of a whole batch without a host read. Returns the list of
        (out_h, out_w) int32 maps (views of one flat tensor; images differ in img_shape / ori_shape); with `with_segments`
        also a dict: n_kept (B,), table (B, Q, 4) int32 rows [value, category, area, query index] per kept query in query
        order, scores (B, Q) in the same slot order -- `segments_info` turns one image's block into COCO-panoptic dicts.
        `debug` adds the (B, 2) count of argmax blocks that ran from LDS / from global memory."""
        if isinstance(mask_pred_results, LowResMasks):
            logits, up = mask_pred_results.logits, mask_pred_results.up_size
        else:
            logits, up = mask_pred_results, tuple(mask_pred_results.shape[-2:])
        logits = logits.contiguous()
        B, Q = logits.shape[:2]
        x = scores_or_emb.reshape(B * Q, -1)
        dots = torch.matmul(x, self.all_class_embs.t()).contiguous() if emb else x.contiguous()
        _, scores, labels = ops.rowwise_softmax_argmax(dots, want_prob=False)
        geometry = self._batched_geometry(up, img_metas, rescale, logits.device)
        cfg = self.test_cfg
        res = ops.panoptic_fuse_batched(logits, scores.view(B, Q), labels.view(B, Q), geometry, up, self.num_classes,
                                        self.num_things_classes, cfg.get('object_mask_thr', 0.8), cfg.get('iou_thr', 0.8),
                                        cfg.get('filter_low_score', False), cfg.get('stuff_area_limit', 4096), defer_stuff=emb,
                                        debug=debug)
        seg, n_kept, table, kscore = res[:4]
        maps = [seg[off:off + oh * ow].view(oh, ow) for off, oh, ow in geometry[3]]
        if not (with_segments or debug):
            return maps
        info = dict(n_kept=n_kept, table=table, scores=kscore)
        if debug:
            info['blocks'] = res[4]
        return maps, info

    def semantic_postprocess(self, mask_cls, mask_pred):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------
    def simple_test(self, mask_cls_results, mask_cls_emb_results, mask_pred_results, img_metas, **kwargs):
        """:369-464 -> list (one dict per image) keyed by eval type."""
        eval_types = self.test_cfg.get('eval_types', [])
        rescale = kwargs.get('rescale', False)
        # this build's extension for index-parity checks: the (query, class) picks behind every detection, i.e. the
        # `top_indices // n_cls` of :344-347 that the reference computes and drops
        want_idx = bool(kwargs.get('with_query_indices', False))
        results = []
        todo = [(key, embs) for key, embs in (('all_results', getattr(self, 'all_class_embs', None)),
                                              ('novel_results', getattr(self, 'novel_class_embs', None)),
                                              ('base_results', getattr(self, 'base_class_embs', None)))
                if key in eval_types and not (key == 'all_results' and self.panoptic_mode)]
        batch_picks = self._batch_picks(mask_cls_emb_results, [e for _, e in todo]) if todo else None
        # panoptic maps of the whole batch without a host read (`panoptic_postprocess_batched`); PER_IMAGE_PANOPTIC or a shape
        # outside the kernel's rules takes the per-image entry points below. `with_segments` (this build's extension) adds
        # result['panoptic_segments']: the image's segment-table block {n_kept, table, scores} (`segments_info` reads it)
        want_seg = bool(kwargs.get('with_segments', False))
        pan_emb = 'all_results' in eval_types and self.panoptic_mode
        pan_cls = 'pan_results' in eval_types
        batched = (pan_emb or pan_cls) and not PER_IMAGE_PANOPTIC and self.panoptic_batched_supported(mask_pred_results)
        if want_seg and (pan_emb or pan_cls) and not batched:
            raise NotImplementedError('with_segments needs the batched panoptic path (Q <= 1024, PER_IMAGE_PANOPTIC off)')
        pan_maps = {}
        if batched and pan_emb:
            pan_maps['panoptic_all_results'] = self.panoptic_postprocess_batched(
                mask_cls_emb_results, mask_pred_results, img_metas, rescale, emb=True, with_segments=True)
        if batched and pan_cls:
            pan_maps['pan_results'] = self.panoptic_postprocess_batched(
                mask_cls_results, mask_pred_results, img_metas, rescale, emb=False, with_segments=True)
        for b, meta in enumerate(img_metas):
            mask_cls_result = mask_cls_results[b]
            emb = mask_cls_emb_results[b]
            mp = mask_pred_results[b]
            result = dict()
            if pan_emb and batched:
                result['panoptic_all_results'] = pan_maps['panoptic_all_results'][0][b]
            elif pan_emb:
                result['panoptic_all_results'] = self.panoptic_postprocess_emb(
                    emb, mp, self.all_class_embs, meta, rescale)
            # the embedding-based instance types of this image share ONE mask pass (same reference semantics as three
            # instance_postprocess_emb calls, :385-400)
            if todo and batch_picks is not None:
                # 4 launches per image: slot plan, one mask pass for all types, per-detection boxes / scores
                labels, cls_scores, qidx = batch_picks
                logits, up, crop, out = self._geom(mp, meta, rescale)
                # mask_bits (this build's extension): masks come back bit-packed, (n, H, W / 8) uint8 with pixel x in bit
                # x & 7 -- 8x fewer bytes for a host-side consumer to copy; callers unpack (detectors.simple_test does)
                bits = bool(kwargs.get('mask_bits', False)) and ops.instance_masks_bitpack_ok(logits.shape[-2:], up, crop, out)
                masks, bboxes = ops.instance_masks_picks(logits, qidx[b].reshape(-1), cls_scores[b].reshape(-1), up, crop,
                                                         out, bitpack=bits)
                k = labels.shape[-1]
                for t, (key, _) in enumerate(todo):
                    result[key] = (labels[b, t], bboxes[t * k:(t + 1) * k], masks[t * k:(t + 1) * k])
                if want_idx:
                    result['query_indices'] = {key: qidx[b, t].long() for t, (key, _) in enumerate(todo)}
                    result['class_scores'] = {key: cls_scores[b, t] for t, (key, _) in enumerate(todo)}
            elif todo:
                geom = self._geom(mp, meta, rescale)
                picks = [self._topk(self.get_cls_emb_scores(emb, embs)[:, :-1]) for _, embs in todo]
                for (key, _), r in zip(todo, self._instances_multi(picks, geom)):
                    result[key] = r
                if want_idx:
                    result['query_indices'] = {key: p[2].long() for (key, _), p in zip(todo, picks)}
                    result['class_scores'] = {key: p[1] for (key, _), p in zip(todo, picks)}
            if 'ins_results' in eval_types:
                result['ins_results'] = self.instance_postprocess(mask_cls_result, mp, meta, rescale)
            if pan_cls and batched:
                result['pan_results'] = pan_maps['pan_results'][0][b]
            elif pan_cls:
                result['pan_results'] = self.panoptic_postprocess(mask_cls_result, mp, meta, rescale)
            if want_seg and pan_maps:
                # the `_emb` map's table when both maps were asked for (it is the one `panoptic_mode` evaluates)
                info = pan_maps.get('panoptic_all_results', pan_maps.get('pan_results'))[1]
                result['panoptic_segments'] = dict(n_kept=info['n_kept'][b], table=info['table'][b], scores=info['scores'][b])
            results.append(result)
        return results
