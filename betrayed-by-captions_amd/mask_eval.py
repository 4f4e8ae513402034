"""COCO instance-mask evaluation (`--eval segm`) on bit-packed masks and COCO box evaluation (`--eval bbox`): the rules in numpy, and
`SegmEvaluator` / `BboxEvaluator`, which run them on the host or hand the costly steps to the device (csrc/mask_eval.hip through
`ops.mask_intersections` / `ops.coco_match`, and `ops.coco_match_boxes`).

The rules restate the reference's own evaluator, [3P] open_set/utils/eval/cocoeval.py (pycocotools' COCOeval with a `class_agnostic`
extension), and the base / novel / all average of open_set/datasets/coco_open.py:583-637:

  mask_intersections_host   |d & g| for every detection d and ground truth g of an image, and the areas
  mask_iou_host             pycocotools `rleIou`: inter / union, inter / area_d for a crowd, 0 where the denominator is 0
  det_boxes_xywh_host       coco_open.py:359-377 `xyxy2xywh` and the JSON round trip of the result file
  box_iou_host              the published maskApi.c `bbIou` on xywh boxes, every double operation rounded on its own
  evaluate_img_host         COCOeval.evaluateImg (cocoeval.py:244-325) for all (category, area range, threshold) of one image
  accumulate_host           COCOeval.accumulate (cocoeval.py:327-432)
  summarize_host            COCOeval._summarize, the twelve values of the standard COCO summary
  open_set_ap_host          coco_open.py:583-637

Masks are bit planes as `cgg_rle_transitions` reads them: (n, H, row_bytes) uint8, pixel x of a row = bit (x & 7) of byte (x >> 3);
only the first `width` pixels of a row count, pad bits may hold anything. The kernels equal the first five rules exactly (integers
and IEEE double operations in a fixed order, none fused); accumulation stays on the host, its input is small.
"""
import numpy as np

AREA_RNGS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))     # cocoeval.py:531
AREA_LABELS = ('all', 'small', 'medium', 'large')


def default_iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)             # cocoeval.py:528


def default_rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)             # cocoeval.py:529


_POP8 = np.array([bin(i).count('1') for i in range(256)], np.uint8)


def _check_bits(bits, width, name):
    bits = np.asarray(bits)
    if bits.dtype != np.uint8 or bits.ndim != 3:
        raise ValueError(f'{name}: (n, H, row_bytes) uint8 array expected')
    if width < 1 or bits.shape[2] * 8 < width:
        raise ValueError(f'{name}: width={width}, row_bytes={bits.shape[2]}')
    return bits


def _clear_pad_bits(bits, width):
    """a copy of the planes cut to ceil(width / 8) bytes per row with the bits past `width` cleared"""
    nb = (width + 7) // 8
    out = np.ascontiguousarray(bits[:, :, :nb])
    if out is bits or np.shares_memory(out, bits):
        out = out.copy()
    if width & 7 and out.size:
        out[:, :, nb - 1] &= np.uint8((1 << (width & 7)) - 1)
    return out


def _popcount_rows(a):
    """(n, m) uint8 -> (n,) int64 set bits per row"""
    if hasattr(np, 'bitwise_count'):
        return np.bitwise_count(a).sum(axis=1, dtype=np.int64)
    return _POP8[a].sum(axis=1, dtype=np.int64)


def mask_intersections_host(det_bits, gt_bits, width):
    """det_bits (D, H, row_bytes), gt_bits (G, H, row_bytes') uint8 bit planes of `width` pixels per row ->
    (inter int64 (D, G), area_d int64 (D,), area_g int64 (G,)): set pixels of d & g, of d and of g, pad bits ignored."""
    width = int(width)
    det_bits, gt_bits = _check_bits(det_bits, width, 'det_bits'), _check_bits(gt_bits, width, 'gt_bits')
    if det_bits.shape[1] != gt_bits.shape[1]:
        raise ValueError(f'mask_intersections_host: heights {det_bits.shape[1]} and {gt_bits.shape[1]} differ')
    D, G = det_bits.shape[0], gt_bits.shape[0]
    nbytes = det_bits.shape[1] * ((width + 7) // 8)
    d = _clear_pad_bits(det_bits, width).reshape(D, nbytes)
    g = _clear_pad_bits(gt_bits, width).reshape(G, nbytes)
    inter = np.zeros((D, G), np.int64)
    if D:
        for j in range(G):
            inter[:, j] = _popcount_rows(d & g[j])
    return inter, _popcount_rows(d), _popcount_rows(g)


def mask_iou_host(inter, area_d, area_g, gt_crowd):
    """float64 (D, G): inter / (area_d + area_g - inter), for a crowd ground truth inter / area_d, and 0.0 where the denominator is
    0 -- the rule of pycocotools `rleIou` (maskApi.c: `u = crowd ? area_d : area_d + area_g - i; o = u == 0 ? 0 : i / u`). One
    float64 division of two integers that float64 holds exactly."""
    inter = np.asarray(inter, np.int64)
    area_d = np.asarray(area_d, np.int64).reshape(-1, 1)
    area_g = np.asarray(area_g, np.int64).reshape(1, -1)
    crowd = np.asarray(gt_crowd).astype(bool).reshape(1, -1)
    den = np.where(crowd, area_d + 0 * area_g, area_d + area_g - inter)
    out = np.zeros(inter.shape, np.float64)
    np.divide(inter.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
    return out


def det_boxes_xywh_host(det_boxes5):
    """(D, 5) float32 (x0, y0, x1, y1, score), as the results hold them -> (D, 4) float64 (x, y, w, h): what the reference's
    `xyxy2xywh` (coco_open.py:359-377) writes into the result file and `loadRes` reads back. `tolist()` widens every float32
    coordinate to a Python float (float64), then x1 - x0 and y1 - y0 are float64 subtractions; JSON round-trips a float64."""
    b = np.asarray(det_boxes5).reshape(-1, 5)[:, :4].astype(np.float32).astype(np.float64)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


def box_iou_host(det_xywh, gt_xywh, gt_crowd):
    """float64 (D, G): the rule of `bbIou` in the published maskApi.c on (x, y, w, h) boxes. Per pair of detection D and ground
    truth G:

        da = D.w * D.h;  ga = G.w * G.h
        w = min(D.w + D.x, G.w + G.x) - max(D.x, G.x);  if w <= 0 the value is 0
        h = min(D.h + D.y, G.h + G.y) - max(D.y, G.y);  if h <= 0 the value is 0
        i = w * h;  u = da for a crowd ground truth, else (da + ga) - i;  the value is i / u

    Every operation is an IEEE float64 operation of its own: no product is fused into the following add (numpy does not fuse; the
    kernel is built with contraction off for this function). THE RULE IS WHAT IS PINNED, here and in the kernel, bit for bit; no
    equality with a particular pycocotools build is claimed (a C compiler is free to contract `da + ga - i` there)."""
    d = np.asarray(det_xywh, np.float64).reshape(-1, 1, 4)
    g = np.asarray(gt_xywh, np.float64).reshape(1, -1, 4)
    crowd = np.asarray(gt_crowd).astype(bool).reshape(1, -1)
    da = d[..., 2] * d[..., 3]
    ga = g[..., 2] * g[..., 3]
    w = np.minimum(d[..., 2] + d[..., 0], g[..., 2] + g[..., 0]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 3] + d[..., 1], g[..., 3] + g[..., 1]) - np.maximum(d[..., 1], g[..., 1])
    i = w * h
    u = np.where(crowd, da, (da + ga) - i)
    out = np.zeros(i.shape, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        np.divide(i, u, out=out, where=~((w <= 0) | (h <= 0)))
    return out


def evaluate_img_host(iou, det_scores, det_cats, gt_cats, gt_crowd, gt_area, area_d, cat_ids, area_rngs, iou_thrs, max_det,
                      class_agnostic):
    """COCOeval.evaluateImg of the reference (cocoeval.py:244-325) for every (category, area range, threshold) of one image.

    iou (D, G) float64 of ALL detections and ground truths of the image in their given order (`mask_iou_host`); det_scores,
    det_cats, area_d (D,); gt_cats, gt_crowd, gt_area (G,). Returns a list over `cat_ids` of lists over `area_rngs` of None (the
    category has neither a ground truth nor a detection in this image: the reference returns None) or a dict

      dt_match  int32 (T, D_k)  0 = unmatched, else 1 + the matched ground truth's index in the image. (The reference stores the
                                ground truth's `id` and tests `== 0`: ids are taken to be >= 1.)
      dt_ignore bool  (T, D_k)
      gt_ignore bool  (G_k,)    in scan order: the ground truths that count first, then the ignored ones
      dt_scores float64 (D_k,)
      dt_index  int64 (D_k,)    the detections' indices in the image

    Detections of a category: stable descending score order, cut to max_det; with class_agnostic every detection of the image
    is a candidate for every category's ground truths (the reference reads `_dts[imgId, 1]`: its caller gives every detection
    category 1). Ground truths: ignored (crowd, or area outside the range) last, original order within each group. Matching is
    the greedy scan with iou = min(t, 1 - 1e-10): a matched ground truth is skipped unless it is crowd; the scan stops when the
    best so far is a regular ground truth and the next one is ignored; `ious < iou` continues, so a later ground truth with an
    equal IoU replaces the earlier one. An unmatched detection whose own area is outside the range is ignored."""
    iou = np.asarray(iou, np.float64)
    det_scores = np.asarray(det_scores, np.float64)
    det_cats, gt_cats = np.asarray(det_cats), np.asarray(gt_cats)
    gt_crowd = np.asarray(gt_crowd).astype(bool)
    gt_area, area_d = np.asarray(gt_area, np.float64), np.asarray(area_d, np.float64)
    T = len(iou_thrs)
    order = np.argsort(-det_scores, kind='mergesort')
    out = []
    for cat in cat_ids:
        dsel = order if class_agnostic else order[det_cats[order] == cat]
        dsel = dsel[:max_det]
        gsel = np.nonzero(gt_cats == cat)[0]
        Dk, Gk = len(dsel), len(gsel)
        if Dk == 0 and Gk == 0:
            out.append([None] * len(area_rngs))
            continue
        per_area = []
        for lo, hi in area_rngs:
            gig = gt_crowd[gsel] | (gt_area[gsel] < lo) | (gt_area[gsel] > hi)
            gord = np.argsort(gig, kind='mergesort')
            g_idx, g_ig = gsel[gord], gig[gord]
            g_crowd = gt_crowd[g_idx]
            ious = iou[np.ix_(dsel, g_idx)]
            dtm = np.zeros((T, Dk), np.int32)
            gtm = np.zeros((T, Gk), bool)
            dtig = np.zeros((T, Dk), bool)
            if Dk and Gk:
                for ti, t in enumerate(iou_thrs):
                    for di in range(Dk):
                        best = min(t, 1 - 1e-10)
                        m = -1
                        for gi in range(Gk):
                            if gtm[ti, gi] and not g_crowd[gi]:
                                continue
                            if m > -1 and not g_ig[m] and g_ig[gi]:
                                break
                            if ious[di, gi] < best:
                                continue
                            best = ious[di, gi]
                            m = gi
                        if m == -1:
                            continue
                        dtig[ti, di] = g_ig[m]
                        dtm[ti, di] = g_idx[m] + 1
                        gtm[ti, m] = True
            outside = (area_d[dsel] < lo) | (area_d[dsel] > hi)
            dtig = dtig | ((dtm == 0) & outside[None, :])
            per_area.append(dict(dt_match=dtm, dt_ignore=dtig, gt_ignore=g_ig.copy(), dt_scores=det_scores[dsel],
                                 dt_index=dsel.astype(np.int64)))
        out.append(per_area)
    return out


def accumulate_host(records, K, A, max_dets, T, rec_thrs=None):
    """COCOeval.accumulate (cocoeval.py:327-432). records: one entry per image, each the [K][A] list of `evaluate_img_host`
    (evaluated at max_dets[-1]). Returns precision (T, R, K, A, M), recall (T, K, A, M), scores (T, R, K, A, M), -1 where a
    category has no ground truth that counts. As there: mergesort by -score over the images' concatenated detections,
    tp / (fp + tp + np.spacing(1)), the right-to-left precision envelope, `searchsorted(rc, rec_thrs, side='left')`."""
    rec_thrs = default_rec_thrs() if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    max_dets = sorted(int(m) for m in max_dets)
    R, M = len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            E = [img[k][a] for img in records if img[k][a] is not None]
            if not E:
                continue
            for m, max_det in enumerate(max_dets):
                dt_scores = np.concatenate([e['dt_scores'][:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e['dt_match'][:, :max_det] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e['dt_ignore'][:, :max_det] for e in E], axis=1)[:, inds]
                gtig = np.concatenate([e['gt_ignore'] for e in E])
                npig = np.count_nonzero(gtig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,)).tolist()
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side='left')):
                        if pi >= nd:           # (the reference leaves its loop through an IndexError here)
                            break
                        q[ri] = pr[pi]
                        ss[ri] = dt_scores_sorted[pi]
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, scores


def _summarize(precision, recall, iou_thrs, ap, iou_thr, a, m):
    s = precision if ap else recall
    if iou_thr is not None:
        s = s[np.where(iou_thr == np.asarray(iou_thrs))[0]]
    s = s[..., a, m]
    return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))


def summarize_host(precision, recall, iou_thrs, area_labels=AREA_LABELS):
    """COCOeval._summarize over the twelve lines of the standard COCO summary: AP, AP50, AP75, AP small / medium / large at the last
    max_dets entry, AR at each of the three max_dets entries, AR small / medium / large at the last. Mean over the entries > -1,
    -1 where there is none. `iou_thr == iou_thrs` is compared exactly, as there. Returns an ordered dict name -> value."""
    labels = list(area_labels)
    M = recall.shape[-1]
    last = M - 1
    al, sm, me, la = (labels.index(n) if n in labels else None for n in ('all', 'small', 'medium', 'large'))

    def S(ap, iou_thr, a, m):
        return -1.0 if a is None or m < 0 else _summarize(precision, recall, iou_thrs, ap, iou_thr, a, m)

    out = dict()
    out['AP'] = S(1, None, al, last)
    out['AP50'] = S(1, .5, al, last)
    out['AP75'] = S(1, .75, al, last)
    out['AP_small'], out['AP_medium'], out['AP_large'] = S(1, None, sm, last), S(1, None, me, last), S(1, None, la, last)
    for i in range(3):
        m = M - 3 + i
        out[f'AR_maxdets{i}'] = S(0, None, al, m)
    out['AR_small'], out['AR_medium'], out['AR_large'] = S(0, None, sm, last), S(0, None, me, last), S(0, None, la, last)
    return out


def open_set_ap_host(precision, pred_cats, unknown_cat_ids, all_cat_ids):
    """coco_open.py:583-637: per category of `pred_cats`, the mean over the entries > -1 of precision[0, :, idx, 0, -1] (first
    threshold -- 0.5 --, all areas, last max_dets); categories outside all_cat_ids, or with no entry, take no part. Returns
    (base, novel, all) in percent: the means over the categories outside / inside unknown_cat_ids and over both (NaN for an empty
    group, as numpy's mean of nothing)."""
    unknown, known = set(unknown_cat_ids or ()), set(all_cat_ids)
    base, novel = [], []
    for idx, cat in enumerate(pred_cats):
        r = precision[0, :, idx, 0, -1]
        r = r[r > -1]
        if r.size and cat in known:
            (novel if cat in unknown else base).append(np.mean(r))

    def mean100(v):
        return float(np.array(v).mean() * 100) if v else float('nan')

    return mean100(base), mean100(novel), mean100(base + novel)


# ------------------------------------------------------------------------------------------------
# the evaluator
# ------------------------------------------------------------------------------------------------
def _to_numpy(x):
    if x is None:
        return None
    if hasattr(x, 'detach'):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def pack_bool_rows_host(masks):
    """(n, H, W) bool / uint8 (non-zero = set) -> (n, H, ceil(W / 8)) uint8 bit planes, pad bits zero"""
    masks = np.asarray(masks) != 0
    return np.packbits(masks, axis=2, bitorder='little')


class _CocoEvaluator:
    """What `SegmEvaluator` and `BboxEvaluator` share: everything after an image's IoU matrix. The constructor, the record format
    (per image the [K][A] list of `evaluate_img_host`, or a pending device record), the one-buffer pinned copy of the device match
    records, `image_records` and `summarize`. A subclass adds `add`."""

    def __init__(self, cat_ids, unknown_cat_ids=None, all_cat_ids=None, max_dets=(100, 300, 1000), iou_thrs=None,
                 class_agnostic=False, device=None, skip_images_without_gt=False, max_in_flight=8):
        self.cat_ids = [int(c) for c in cat_ids]
        self.unknown_cat_ids = [] if unknown_cat_ids is None else [int(c) for c in unknown_cat_ids]
        self.all_cat_ids = [int(c) for c in (self.cat_ids if all_cat_ids is None else all_cat_ids)]
        self.max_dets = sorted(int(m) for m in max_dets)
        self.iou_thrs = default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64)
        self.class_agnostic = bool(class_agnostic)
        self.skip_images_without_gt = bool(skip_images_without_gt)
        self.area_rngs = np.asarray(AREA_RNGS, np.float64)
        self.device = device
        self.max_in_flight = int(max_in_flight)
        self.records = []          # per image, in `add` order: the [K][A] list of evaluate_img_host, or a pending device record
        self._in_flight = []       # indices into self.records of the device records not yet parsed
        self._pinned = {}          # bytes -> a pinned staging buffer that has been parsed (allocating one costs more than an `add`)
        self._dev = None
        if device is not None:
            import torch
            self.device = torch.device(device)
            self._dev = dict(
                cat_ids=torch.tensor(self.cat_ids, dtype=torch.int32, device=self.device),
                area_rngs=torch.tensor(self.area_rngs, dtype=torch.float64, device=self.device),
                iou_thrs=torch.tensor(self.iou_thrs, dtype=torch.float64, device=self.device))

    def _queue_match(self, match, D, G, order, det_cats, scores):
        """The device half of one `add` after its inputs are on the device: `match(out)` launches the matcher into the four output
        tensors; they, the score order, the categories and the scores share one byte buffer, so that one pinned copy carries all
        the host needs; an event follows the copy. Nothing waits (an `add` beyond `max_in_flight` queued copies waits for the
        oldest one)."""
        import torch
        dev = self.device
        K, A, T = len(self.cat_ids), len(self.area_rngs), len(self.iou_thrs)
        sizes = [('dt_match', 4 * K * A * T * D), ('counts', 4 * K * 2), ('order', 4 * D), ('det_cats', 4 * D), ('scores', 4 * D),
                 ('dt_ignore', K * A * T * D), ('gt_ignore', K * A * G)]
        offs, total = {}, 0
        for name, nbytes in sizes:
            offs[name] = (total, nbytes)
            total += (nbytes + 7) & ~7
        buf = torch.empty(max(total, 8), dtype=torch.uint8, device=dev)

        def part(name, dtype, shape):
            o, nb = offs[name]
            return buf[o:o + nb].view(dtype).view(shape)

        dt_match, counts = part('dt_match', torch.int32, (K, A, T, D)), part('counts', torch.int32, (K, 2))
        dt_ignore, gt_ignore = part('dt_ignore', torch.uint8, (K, A, T, D)), part('gt_ignore', torch.uint8, (K, A, G))
        match((dt_match, dt_ignore, gt_ignore, counts))
        part('order', torch.int32, (D,)).copy_(order)
        part('det_cats', torch.int32, (D,)).copy_(det_cats)
        part('scores', torch.float32, (D,)).copy_(scores)
        host = self._pinned.pop(buf.numel(), None)
        if host is None:
            host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.records.append(dict(pending=host, done=done, offs=offs, dims=(D, G, K, A, T)))
        self._in_flight.append(len(self.records) - 1)
        self._drain(keep=self.max_in_flight)

    def _drain(self, keep=0):
        """parse the queued device records whose copy has arrived; wait only for those beyond `keep`"""
        while self._in_flight:
            rec = self.records[self._in_flight[0]]
            if len(self._in_flight) > keep:
                rec['done'].synchronize()
            elif not rec['done'].query():
                break
            self.records[self._in_flight.pop(0)] = self._parse(rec)
            self._pinned[rec['pending'].numel()] = rec['pending']

    def _parse(self, rec):
        """pinned bytes of one image -> the [K][A] list `evaluate_img_host` returns"""
        raw = rec['pending'].numpy()
        D, G, K, A, T = rec['dims']

        def part(name, dtype, shape):
            o, nb = rec['offs'][name]
            return raw[o:o + nb].view(dtype).reshape(shape)

        return records_from_match(part('dt_match', np.int32, (K, A, T, D)), part('dt_ignore', np.uint8, (K, A, T, D)),
                                  part('gt_ignore', np.uint8, (K, A, G)), part('counts', np.int32, (K, 2)),
                                  part('order', np.int32, (D,)), part('det_cats', np.int32, (D,)),
                                  part('scores', np.float32, (D,)), self.cat_ids, self.class_agnostic)

    # -- the whole run -----------------------------------------------------------------------------
    def image_records(self):
        """every image's [K][A] record list, in `add` order (waits for the queued device copies); what a distributed run gathers"""
        self._drain()
        return self.records

    def summarize(self, extra_records=None):
        """-> dict(precision, recall, scores, stats (the twelve COCO summary values), base_ap50, novel_ap50, all_ap50).
        extra_records: further image records (of other ranks) to accumulate with this evaluator's own."""
        records = list(self.image_records()) + list(extra_records or ())
        K, A, T = len(self.cat_ids), len(self.area_rngs), len(self.iou_thrs)
        precision, recall, scores = accumulate_host(records, K, A, self.max_dets, T)
        base, novel, both = open_set_ap_host(precision, self.cat_ids, self.unknown_cat_ids, self.all_cat_ids)
        return dict(precision=precision, recall=recall, scores=scores, stats=summarize_host(precision, recall, self.iou_thrs),
                    base_ap50=base, novel_ap50=novel, all_ap50=both, images=len(records))


class SegmEvaluator(_CocoEvaluator):
    """COCO mask AP of a stream of images, from the device results of `simple_test(device_results=True, mask_bits=True)`.

    cat_ids: label -> category id of the detections' labels (the reference's `pred_cats`); ground-truth labels ARE category ids,
    and a ground truth of a category outside cat_ids takes no part (the reference loads ground truth by `catIds`).
    unknown_cat_ids / all_cat_ids: the novel categories and the categories present in the dataset, for base / novel / all AP50
    (`open_set_ap_host`); both default to "no novel category, every category present".

    device=None: the host rule on numpy arrays -- the comparison side and the CPU path. With a device, `add` launches
    `ops.mask_intersections` and `ops.coco_match` on the current stream and queues one pinned device-to-host copy of the match
    records; no mask leaves the device and nothing synchronises before `summarize()` (an `add` beyond `max_in_flight` queued
    copies waits for the oldest one). Shapes outside `ops.mask_eval_ok` take the host rule.

    skip_images_without_gt: leave out an image that has no ground truth of cat_ids, as the reference's `_get_valid_imgs` does
    for its per-split runs (coco_open.py:567)."""

    # -- one image ---------------------------------------------------------------------------------
    def add(self, det_labels, det_boxes5, det_masks, gt_masks, gt_labels, gt_crowd=None, gt_area=None):
        """det_labels (D,) labels into cat_ids, det_boxes5 (D, 5) with the score last, det_masks (D, H, row_bytes) uint8 bit planes (or
        (D, H, W) bool bitmaps, which are packed first);
        gt_masks (G, H, W) bool / uint8 bitmaps (host or device; W is the image's width), gt_labels (G,) category ids, gt_crowd
        (G,) or None (no crowd), gt_area (G,) the annotations' own `area` or None (the pixel count)."""
        W = int(gt_masks.shape[2])
        H = int(gt_masks.shape[1])
        if len(det_masks.shape) != 3:
            raise ValueError('SegmEvaluator.add: det_masks must be (D, H, row_bytes) bit planes (mask_bits=True)')
        if str(det_masks.dtype).endswith('bool'):
            # `mask_bits=True` is a request: geometries outside `ops.instance_masks_bitpack_ok` come back as (D, H, W) bool bitmaps
            if self.device is not None and hasattr(det_masks, 'is_cuda') and det_masks.is_cuda:
                from . import ops
                det_masks = ops.pack_bool_masks(det_masks)
            else:
                det_masks = pack_bool_rows_host(_to_numpy(det_masks))
        if int(det_masks.shape[1]) != H or int(det_masks.shape[2]) * 8 < W:
            raise ValueError(f'SegmEvaluator.add: det_masks {tuple(det_masks.shape)} do not cover ground truth of {H} x {W}')
        if self.skip_images_without_gt:
            gl = _to_numpy(gt_labels)
            if not np.isin(gl, self.cat_ids).any():
                return
        use_device = False
        if self.device is not None:
            from . import ops
            use_device = ops.mask_eval_ok(int(det_masks.shape[0]), int(gt_masks.shape[0]), H, W)
        if use_device:
            self._add_device(det_labels, det_boxes5, det_masks, gt_masks, gt_labels, gt_crowd, gt_area, H, W)
        else:
            self._add_host(det_labels, det_boxes5, det_masks, gt_masks, gt_labels, gt_crowd, gt_area, W)

    def _add_host(self, det_labels, det_boxes5, det_masks, gt_masks, gt_labels, gt_crowd, gt_area, W):
        det_bits = _to_numpy(det_masks)
        if det_bits.dtype != np.uint8:
            raise ValueError('SegmEvaluator.add: det_masks must be uint8 bit planes (mask_bits=True)')
        gt_bits = pack_bool_rows_host(_to_numpy(gt_masks))
        G = gt_bits.shape[0]
        scores = _to_numpy(det_boxes5).reshape(-1, 5)[:, 4].astype(np.float64)
        det_cats = np.asarray(self.cat_ids, np.int64)[_to_numpy(det_labels).astype(np.int64)] if len(scores) else np.zeros(0, np.int64)
        crowd = np.zeros(G, bool) if gt_crowd is None else _to_numpy(gt_crowd).astype(bool)
        inter, area_d, area_g = mask_intersections_host(det_bits, gt_bits, W)
        area = area_g.astype(np.float64) if gt_area is None else _to_numpy(gt_area).astype(np.float64)
        iou = mask_iou_host(inter, area_d, area_g, crowd)
        self.records.append(evaluate_img_host(iou, scores, det_cats, _to_numpy(gt_labels), crowd, area, area_d, self.cat_ids,
                                              self.area_rngs, self.iou_thrs, self.max_dets[-1], self.class_agnostic))

    def _add_device(self, det_labels, det_boxes5, det_masks, gt_masks, gt_labels, gt_crowd, gt_area, H, W):
        import torch
        from . import ops
        dev = self.device
        D, G = int(det_masks.shape[0]), int(gt_masks.shape[0])

        def on_device(x, dtype):
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            return t.to(device=dev, dtype=dtype, non_blocking=True)

        gm = gt_masks if torch.is_tensor(gt_masks) else torch.from_numpy(np.ascontiguousarray(gt_masks))
        if gm.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'SegmEvaluator.add: gt_masks must be bool or uint8 bitmaps (got {gm.dtype})')
        gm = gm.to(dev, non_blocking=True)                                      # host arrays: one H2D, packed on the device
        gt_bits = ops.pack_bool_masks(gm.view(torch.bool) if gm.dtype == torch.uint8 else gm)      # (the kernel reads non-zero = set)
        scores = on_device(det_boxes5, torch.float32).reshape(-1, 5)[:, 4].contiguous()
        det_cats = self._dev['cat_ids'][on_device(det_labels, torch.int64)] if D else torch.zeros(0, dtype=torch.int32, device=dev)
        order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32)
        gt_cats = on_device(gt_labels, torch.int32)
        crowd = torch.zeros(G, dtype=torch.uint8, device=dev) if gt_crowd is None else on_device(gt_crowd, torch.uint8)
        det_masks = det_masks if torch.is_tensor(det_masks) else torch.from_numpy(np.ascontiguousarray(det_masks))
        if det_masks.dtype != torch.uint8:
            raise ValueError(f'SegmEvaluator.add: det_masks must be uint8 bit planes or bool bitmaps (got {det_masks.dtype})')
        inter, area_d, area_g = ops.mask_intersections(det_masks.to(dev, non_blocking=True), gt_bits, W)
        area = area_g.to(torch.float64) if gt_area is None else on_device(gt_area, torch.float64)
        self._queue_match(lambda out: ops.coco_match(inter, area_d, area_g, order, det_cats, gt_cats, crowd, area, self._dev['cat_ids'],
                                                     self._dev['area_rngs'], self._dev['iou_thrs'], self.max_dets[-1],
                                                     self.class_agnostic, out=out), D, G, order, det_cats, scores)


class BboxEvaluator(_CocoEvaluator):
    """COCO box AP of a stream of images (`--eval bbox`), from the `(labels, bboxes (n, 5), masks)` tuples of the results: the
    constructor, records and `summarize` of `SegmEvaluator`, with `box_iou_host` in place of the mask IoU. A detection is the box
    `det_boxes_xywh_host` makes of its row, and its area -- for the area ranges -- is that box's w * h, which is what `loadRes`
    stores for box results. The reference's `evaluate_det_segm` runs `proposal` as this very evaluation under another name.

    device=None: the host rule. With a device, `add` uploads the small ground-truth arrays, launches `ops.coco_match_boxes` once on
    the current stream and queues one pinned copy of the match records; nothing synchronises before `summarize()`. Shapes outside
    `ops.box_eval_ok` take the host rule."""

    def add(self, det_labels, det_boxes5, gt_boxes_xywh, gt_labels, gt_crowd=None, gt_area=None):
        """det_labels (D,) labels into cat_ids, det_boxes5 (D, 5) float32 (x0, y0, x1, y1, score); gt_boxes_xywh (G, 4) float64, the
        annotations' own `bbox`, gt_labels (G,) category ids, gt_crowd (G,) or None (no crowd), gt_area (G,) the annotations' own
        `area` or None (the ground-truth box's w * h)."""
        if len(det_boxes5.shape) != 2 or int(det_boxes5.shape[1]) != 5:
            raise ValueError(f'BboxEvaluator.add: det_boxes5 must be (D, 5) (got {tuple(det_boxes5.shape)})')
        gt_boxes = _to_numpy(gt_boxes_xywh).astype(np.float64).reshape(-1, 4)
        gl = _to_numpy(gt_labels).reshape(-1)
        D, G = int(det_boxes5.shape[0]), gt_boxes.shape[0]
        if len(gl) != G or int(det_labels.shape[0]) != D:
            raise ValueError(f'BboxEvaluator.add: {D} boxes with {int(det_labels.shape[0])} labels, {G} ground-truth boxes with {len(gl)}')
        if self.skip_images_without_gt and not np.isin(gl, self.cat_ids).any():
            return
        crowd = np.zeros(G, bool) if gt_crowd is None else _to_numpy(gt_crowd).astype(bool).reshape(-1)
        area = gt_boxes[:, 2] * gt_boxes[:, 3] if gt_area is None else _to_numpy(gt_area).astype(np.float64).reshape(-1)
        use_device = False
        if self.device is not None:
            from . import ops
            use_device = ops.box_eval_ok(D, G)
        if use_device:
            self._add_device(det_labels, det_boxes5, gt_boxes, gl, crowd, area, D, G)
        else:
            self._add_host(det_labels, det_boxes5, gt_boxes, gl, crowd, area)

    def _add_host(self, det_labels, det_boxes5, gt_boxes, gt_labels, crowd, area):
        boxes5 = _to_numpy(det_boxes5).astype(np.float32).reshape(-1, 5)
        scores = boxes5[:, 4].astype(np.float64)
        det_cats = np.asarray(self.cat_ids, np.int64)[_to_numpy(det_labels).astype(np.int64)] if len(scores) else np.zeros(0, np.int64)
        det = det_boxes_xywh_host(boxes5)
        iou = box_iou_host(det, gt_boxes, crowd)
        self.records.append(evaluate_img_host(iou, scores, det_cats, gt_labels, crowd, area, det[:, 2] * det[:, 3], self.cat_ids,
                                              self.area_rngs, self.iou_thrs, self.max_dets[-1], self.class_agnostic))

    def _add_device(self, det_labels, det_boxes5, gt_boxes, gt_labels, crowd, area, D, G):
        import torch
        from . import ops
        dev = self.device

        def on_device(x, dtype):
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            return t.to(device=dev, dtype=dtype, non_blocking=True)

        # the ground truth of one image in ONE host-to-device copy: G rows of (x, y, w, h, area, category, crowd) in float64
        # (category ids and flags are small integers: exact)
        gt = np.empty((G, 7), np.float64)
        gt[:, :4], gt[:, 4], gt[:, 5], gt[:, 6] = gt_boxes, area, gt_labels, crowd
        gt = on_device(gt, torch.float64)
        gt_xywh, gt_area = gt[:, :4].contiguous(), gt[:, 4].contiguous()
        gt_cats, gt_crowd = gt[:, 5].to(torch.int32), gt[:, 6].to(torch.uint8)
        boxes5 = on_device(det_boxes5, torch.float32).contiguous()
        scores = boxes5[:, 4].contiguous()
        det_cats = self._dev['cat_ids'][on_device(det_labels, torch.int64)] if D else torch.zeros(0, dtype=torch.int32, device=dev)
        order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32)
        self._queue_match(lambda out: ops.coco_match_boxes(boxes5, gt_xywh, order, det_cats, gt_cats, gt_crowd, gt_area,
                                                           self._dev['cat_ids'], self._dev['area_rngs'], self._dev['iou_thrs'],
                                                           self.max_dets[-1], self.class_agnostic, out=out), D, G, order, det_cats, scores)


def records_from_match(dt_match, dt_ignore, gt_ignore, counts, order, det_cats, scores, cat_ids, class_agnostic):
    """The arrays `ops.coco_match` wrote for one image ((K, A, T, D), (K, A, T, D), (K, A, G), (K, 2)) with the image's score order,
    categories and scores (D,) -> the [K][A] list `evaluate_img_host` returns (copies: the staging buffer may be dropped)."""
    order = np.asarray(order, np.int64)
    cats_sorted = np.asarray(det_cats)[order]
    out = []
    for k, cat in enumerate(cat_ids):
        Dk, Gk = int(counts[k, 0]), int(counts[k, 1])
        if Dk == 0 and Gk == 0:
            out.append([None] * dt_match.shape[1])
            continue
        dsel = (order if class_agnostic else order[cats_sorted == cat])[:Dk]
        sc = np.asarray(scores)[dsel].astype(np.float64)
        out.append([dict(dt_match=dt_match[k, a, :, :Dk].copy(), dt_ignore=dt_ignore[k, a, :, :Dk].astype(bool),
                         gt_ignore=gt_ignore[k, a, :Gk].astype(bool), dt_scores=sc, dt_index=dsel.copy())
                    for a in range(dt_match.shape[1])])
    return out


def format_summary(name, res, metric='segm'):
    """the printed form of one evaluator's `summarize()` result; `metric` names the evaluation in the first line"""
    lines = [f'{metric} {name}: {res["images"]} images']
    lines += [f'  {k:<12} = {v:0.3f}' for k, v in res['stats'].items()]
    lines.append(f'  AP50: base {res["base_ap50"]:0.1f}, novel {res["novel_ap50"]:0.1f}, all {res["all_ap50"]:0.1f}')
    return '\n'.join(lines)
