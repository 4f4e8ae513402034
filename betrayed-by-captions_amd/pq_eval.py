"""Panoptic quality (`--eval PQ`): PQ / SQ / RQ over All, Known Things, Unknown Things and Stuff. The rules in numpy, and
`PQEvaluator`, which runs them on the host or hands the two per-pixel steps to the device (csrc/pq_eval.hip through
`ops.pq_confusion` / `ops.pq_match`).

The rules restate the reference's evaluator, open_set/utils/eval/pq_evaluation.py, and the parts of
open_set/datasets/coco_panoptic_open.py around it, without importing either:

  pan_result_segments_host   `_pan2json` (coco_panoptic_open.py:512-550) without files: the records of a result map, void -> 0
  pq_image_host              the loop body of `pq_compute_single_core` (pq_evaluation.py:97-174) for one image -> an image record
  pq_accumulate_host         the sums that loop keeps in `PQStat`, from the image records, in the order of ONE core
  pq_average_host            `PQStat.pq_average` (pq_evaluation.py:47-84)
  parse_pq_results_host      `parse_pq_results` and the `PQ_copypaste` string (coco_panoptic_open.py:617-626, 683-698)

An id map is what `train_prep` stages as `pan_seg`: (h, w) int32 ids, or (h, w, 3) uint8 RGB with id = R + 256 G + 65536 B.
Nothing here decodes a PNG, and nothing is claimed about `panopticapi`. The kernels equal `pq_image_host` exactly: integer counts,
and one IEEE double quotient of two integers per pair; accumulation stays on the host, its input is a few hundred bytes per image.
"""
import numpy as np

from .train_prep import _check_pan_seg, _pan_ids

INSTANCE_OFFSET = 1000       # [3P] mmdet.core.evaluation.panoptic_utils.INSTANCE_OFFSET
OFFSET = 256 * 256 * 256     # pq_evaluation.py:14
VOID = 0                     # pq_evaluation.py:15

STATUS_UNLISTED_PRED = 1     # status word of the device route: a pred value in the map that is neither listed nor void
STATUS_NO_PIXELS = 2         # a listed pred segment without a pixel
STATUS_MULTI_MATCH = 4       # a ground truth that matches more than one pred (the record keeps one match per ground truth)

METRICS = (('All', None, None), ('Known Things', True, False), ('Unknown Things', True, True), ('Stuff', False, None))


def _to_numpy(x):
    if hasattr(x, 'detach'):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _id_map(pan, name):
    """(h, w) int64 ids of an id map in either accepted form (`train_prep._check_pan_seg` / `_pan_ids` decide)"""
    arr, fmt = _check_pan_seg(_to_numpy(pan))
    return _pan_ids(arr, fmt).astype(np.int64)


def pan_result_segments_host(pan, num_classes, all_cat_ids, isthing):
    """A RESTATEMENT of `CocoPanopticDatasetOpen._pan2json` (coco_panoptic_open.py:512-550) for one result map, without files. The
    dataset class cannot be imported in this build (mmdet is absent), so no execution of it is claimed.

    pan (h, w) integer map of `label + instance * INSTANCE_OFFSET`, void = num_classes; all_cat_ids[label] -> category id;
    isthing[label]. Returns (ids, segments): the map with the void pixels set to 0 (int64, a copy), and for every value of
    `np.unique(pan)` whose label is not num_classes a dict(id, category_id, isthing, area) with area = (pan == value).sum(), in
    ascending value order. As there, a value 0 (label 0 without an instance number) and the void share the id 0 afterwards."""
    pan = np.array(_to_numpy(pan), dtype=np.int64)
    segments = []
    for value in np.unique(pan):
        sem = int(value) % INSTANCE_OFFSET
        if sem == num_classes:
            continue
        segments.append(dict(id=int(value), category_id=int(all_cat_ids[sem]), isthing=int(bool(isthing[sem])),
                             area=int((pan == value).sum())))
    pan[pan % INSTANCE_OFFSET == num_classes] = VOID
    return pan, segments


def _by_id(segments, name):
    out = {}
    for el in segments:
        if int(el['id']) in out:
            raise ValueError(f'pq_image_host: {name} holds the id {int(el["id"])} twice')
        out[int(el['id'])] = el
    return out


def pq_image_host(pan_gt, gt_segments, pan_pred, pred_segments, image_id=None):
    """The loop body of `pq_compute_single_core` (pq_evaluation.py:97-174) for one image, restated literally.

    pan_gt, pan_pred: id maps (either accepted form) of one size, the pred's void pixels already 0. gt_segments: the dataset's
    records (id, category_id, iscrowd, area); pred_segments: records with id and category_id. An id may appear once per list.

    Pred areas are recounted from the map; ground-truth areas are taken from the records. The confusion counts are keyed by
    gt * 256^3 + pred. A pair is skipped for an id absent from either record list, for a crowd ground truth, or for unequal
    categories; union = area_pred + area_gt - inter - inter(VOID, pred), iou = inter / union in float64, matched iff iou > 0.5.
    Every unmatched non-crowd ground truth is a false negative. Of the crowds of one category the LAST in record order counts;
    an unmatched pred is ignored iff (inter(VOID, pred) + inter(that crowd, pred)) / area_pred > 0.5, else a false positive.
    KeyError, in the reference's words: a pred id in the map without a record (other than 0), a pred record without pixels.

    Returns the image record, slots in record order, no pixels:
      gt_id, gt_cat int64 (G,), gt_crowd bool (G,), gt_match int32 (G,) the matched pred slot or -1, gt_iou float64 (G,)
      pred_id, pred_cat, pred_area int64 (P,), pred_matched, pred_ignored bool (P,)
      extra: [(gt slot, pred slot, iou)] -- further matches of a ground truth that already has one, in ascending pred id. Empty
             unless a record's area understates the segment's pixels (with true areas two preds cannot both cover more than
             half of a union); the device route reports such an image instead of recording it."""
    gt = _id_map(pan_gt, 'pan_gt')
    pred = _id_map(pan_pred, 'pan_pred')
    if gt.shape != pred.shape:
        raise ValueError(f'pq_image_host: pan_gt {gt.shape} and pan_pred {pred.shape} differ')
    gt_segms, pred_segms = _by_id(gt_segments, 'gt_segments'), _by_id(pred_segments, 'pred_segments')
    gt_slot = {k: i for i, k in enumerate(gt_segms)}
    pred_slot = {k: i for i, k in enumerate(pred_segms)}
    G, P = len(gt_segms), len(pred_segms)
    # predicted segments area calculation + prediction sanity checks
    pred_area = np.zeros(P, np.int64)
    pred_labels_set = set(pred_segms)
    labels, labels_cnt = np.unique(pred, return_counts=True)
    for label, label_cnt in zip(labels.tolist(), labels_cnt.tolist()):
        if label not in pred_segms:
            if label == VOID:
                continue
            raise KeyError('In the image with ID {} segment with ID {} is presented in PNG and not presented in JSON.'.format(
                image_id, label))
        pred_area[pred_slot[label]] = label_cnt
        pred_labels_set.remove(label)
    if len(pred_labels_set) != 0:
        raise KeyError('In the image with ID {} the following segment IDs {} are presented in JSON and not presented in PNG.'.format(
            image_id, list(pred_labels_set)))
    # confusion matrix calculation
    gt_pred_map = {}
    labels, labels_cnt = np.unique(gt.astype(np.uint64) * np.uint64(OFFSET) + pred.astype(np.uint64), return_counts=True)
    for label, intersection in zip(labels.tolist(), labels_cnt.tolist()):
        gt_pred_map[(label // OFFSET, label % OFFSET)] = intersection
    rec = dict(gt_id=np.array(list(gt_segms), np.int64).reshape(G), gt_cat=np.array([int(e['category_id']) for e in gt_segms.values()], np.int64).reshape(G),
               gt_crowd=np.array([e['iscrowd'] == 1 for e in gt_segms.values()], bool).reshape(G),
               gt_match=np.full(G, -1, np.int32), gt_iou=np.zeros(G, np.float64),
               pred_id=np.array(list(pred_segms), np.int64).reshape(P),
               pred_cat=np.array([int(e['category_id']) for e in pred_segms.values()], np.int64).reshape(P), pred_area=pred_area,
               pred_matched=np.zeros(P, bool), pred_ignored=np.zeros(P, bool), extra=[])
    # count all matched pairs (ascending key order: numpy's unique sorts, and the dict keeps it)
    for (gt_label, pred_label), intersection in gt_pred_map.items():
        if gt_label not in gt_segms or pred_label not in pred_segms:
            continue
        if gt_segms[gt_label]['iscrowd'] == 1:
            continue
        if gt_segms[gt_label]['category_id'] != pred_segms[pred_label]['category_id']:
            continue
        g, p = gt_slot[gt_label], pred_slot[pred_label]
        union = int(pred_area[p]) + gt_segms[gt_label]['area'] - intersection - gt_pred_map.get((VOID, pred_label), 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = np.float64(intersection) / np.float64(union)          # (numpy integers there: a zero union gives inf, no error)
        if iou > 0.5:
            if rec['gt_match'][g] < 0:
                rec['gt_match'][g], rec['gt_iou'][g] = p, iou
            else:
                rec['extra'].append((g, p, float(iou)))
            rec['pred_matched'][p] = True
    # the crowd that counts for a category: the last one in record order
    crowd_labels_dict = {}
    for gt_label, gt_info in gt_segms.items():
        if gt_info['iscrowd'] == 1:
            crowd_labels_dict[gt_info['category_id']] = gt_label
    # unmatched preds: ignored, or false positives
    for pred_label, pred_info in pred_segms.items():
        p = pred_slot[pred_label]
        if rec['pred_matched'][p]:
            continue
        intersection = gt_pred_map.get((VOID, pred_label), 0)
        if pred_info['category_id'] in crowd_labels_dict:
            intersection += gt_pred_map.get((crowd_labels_dict[pred_info['category_id']], pred_label), 0)
        rec['pred_ignored'][p] = np.float64(intersection) / np.float64(pred_area[p]) > 0.5
    return rec


def pq_accumulate_host(records):
    """Image records -> {category id: dict(tp, fp, fn (int), iou (float64))}, the sums `pq_compute_single_core` keeps.

    The order of the float64 sum is the reference's with ONE core: images in order, within an image the matches in ascending
    (ground-truth id, pred id). The reference's own result depends on `multiprocessing.cpu_count()`: `pq_compute_multi_core` splits
    the images over that many processes and adds each core's partial iou sums afterwards, so its last bits differ from machine to
    machine. This build pins the single-core order."""
    stats = {}

    def cat(c):
        return stats.setdefault(int(c), dict(tp=0, fp=0, fn=0, iou=np.float64(0.0)))

    for rec in records:
        extra = {}
        for g, p, iou in rec.get('extra', ()):
            extra.setdefault(int(g), []).append((int(rec['pred_id'][p]), iou))
        for g in np.argsort(rec['gt_id'], kind='mergesort').tolist():
            if rec['gt_match'][g] < 0:
                continue
            matches = [(int(rec['pred_id'][rec['gt_match'][g]]), rec['gt_iou'][g])] + extra.get(g, [])
            for _, iou in sorted(matches, key=lambda m: m[0]):
                c = cat(rec['gt_cat'][g])
                c['tp'] += 1
                c['iou'] = c['iou'] + np.float64(iou)
        for g in range(len(rec['gt_id'])):
            if rec['gt_match'][g] < 0 and not rec['gt_crowd'][g]:
                cat(rec['gt_cat'][g])['fn'] += 1
        for p in range(len(rec['pred_id'])):
            if not rec['pred_matched'][p] and not rec['pred_ignored'][p]:
                cat(rec['pred_cat'][p])['fp'] += 1
    return stats


def pq_average_host(stats, categories, isthing, isunknown, unknown_cat_ids):
    """`PQStat.pq_average` (pq_evaluation.py:47-84). stats: `pq_accumulate_host`'s; categories {id: dict(id, isthing)} in the
    dataset's order; isthing / isunknown None = both. Returns (dict(pq, sq, rq, n, precision, recall), per-class results); a
    category with tp + fp + fn = 0 is left out of n."""
    precision, recall, pq, sq, rq, n = 0.0, 0.0, 0, 0, 0, 0
    per_class_results = {}
    for label, label_info in categories.items():
        cat_isthing = label_info['isthing'] == 1
        cat_isunknown = label_info['id'] in unknown_cat_ids
        if isthing is not None and isthing != cat_isthing:
            continue
        if isunknown is not None and isunknown != cat_isunknown:
            continue
        s = stats.get(label) or dict(tp=0, fp=0, fn=0, iou=0.0)
        iou, tp_class, fp_class, fn_class = s['iou'], s['tp'], s['fp'], s['fn']
        if tp_class + fp_class + fn_class == 0:
            per_class_results[label] = {'pq': 0.0, 'sq': 0.0, 'rq': 0.0, 'precision': 0.0, 'recall': 0.0}
            continue
        precision_class = tp_class / (tp_class + fp_class) if (tp_class + fp_class) > 0 else 0.0
        recall_class = tp_class / (tp_class + fn_class) if (tp_class + fn_class) > 0 else 0.0
        pq_class = iou / (tp_class + 0.5 * fp_class + 0.5 * fn_class)
        sq_class = iou / tp_class if tp_class != 0 else 0
        rq_class = tp_class / (tp_class + 0.5 * fp_class + 0.5 * fn_class)
        per_class_results[label] = {'pq': pq_class, 'sq': sq_class, 'rq': rq_class, 'precision': precision_class, 'recall': recall_class}
        n += 1
        precision += precision_class
        recall += recall_class
        pq += pq_class
        sq += sq_class
        rq += rq_class
    if n == 0:
        return {'pq': 0, 'sq': 0, 'rq': 0, 'n': 0, 'precision': 0, 'recall': 0}, per_class_results
    return {'pq': pq / n, 'sq': sq / n, 'rq': rq / n, 'n': n, 'precision': precision / n, 'recall': recall / n}, per_class_results


def pq_splits_host(stats, categories, unknown_cat_ids):
    """the four splits of `evaluate_pan_json` (coco_panoptic_open.py:595-602): {'All', 'Known Things', 'Unknown Things', 'Stuff':
    averaged dict, 'classwise': the per-class results of 'All'}"""
    pq_results = {}
    for name, isthing, isunknown in METRICS:
        pq_results[name], classwise = pq_average_host(stats, categories, isthing, isunknown, unknown_cat_ids)
        if name == 'All':
            pq_results['classwise'] = classwise
    return pq_results


def parse_pq_results_host(pq_results):
    """`parse_pq_results` (coco_panoptic_open.py:683-698) and the `PQ_copypaste` string of :618-626: the twelve numbers in percent"""
    result = dict()
    for tag, name in (('', 'All'), ('_kth', 'Known Things'), ('_ukth', 'Unknown Things'), ('_st', 'Stuff')):
        for m in ('PQ', 'SQ', 'RQ'):
            result[m + tag] = 100 * pq_results[name][m.lower()]
    result['PQ_copypaste'] = (
        f'{result["PQ"]:.3f} {result["SQ"]:.3f} {result["RQ"]:.3f} '
        f'{result["PQ_kth"]:.3f} {result["SQ_kth"]:.3f} {result["RQ_kth"]:.3f} '
        f'{result["PQ_ukth"]:.3f} {result["SQ_ukth"]:.3f} {result["RQ_ukth"]:.3f} '
        f'{result["PQ_st"]:.3f} {result["SQ_st"]:.3f} {result["RQ_st"]:.3f}')
    return result


def format_pq_summary(pq_results):
    """the table `print_panoptic_table` prints (coco_panoptic_open.py:700-720), as plain text"""
    rows = [['', 'PQ', 'SQ', 'RQ', 'Precision', 'Recall', 'categories']]
    for name, _, _ in METRICS:
        rows.append([name] + [f'{(pq_results[name][k] * 100):0.3f}' for k in ('pq', 'sq', 'rq', 'precision', 'recall')]
                    + [str(pq_results[name]['n'])])
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    lines = ['Panoptic Evaluation Results:', rule]
    for i, r in enumerate(rows):
        lines.append('|' + '|'.join(' ' + v.ljust(w) + ' ' for v, w in zip(r, width)) + '|')
        if i == 0:
            lines.append(rule)
    lines.append(rule)
    return '\n'.join(lines)


# ------------------------------------------------------------------------------------------------
# the evaluator
# ------------------------------------------------------------------------------------------------
def _is_table(x):
    return isinstance(x, dict) and 'table' in x and 'n_kept' in x


def _align(n, a=16):
    return (n + a - 1) // a * a


class PQEvaluator:
    """PQ of a stream of images, from the panoptic maps of `simple_test(device_results=True, with_segments=True)`.

    all_cat_ids: label -> category id (the dataset's `all_cat_ids`); isthing: per label; unknown_cat_ids: the novel categories;
    num_classes: the void label of a result map (default len(all_cat_ids)).

    add(pan_pred, pred_segments_or_table, pan_gt, gt_segments)
      pan_pred   (h, w) integer result map (`label + instance * INSTANCE_OFFSET`, void = num_classes), host or device. A pixel is
                 void iff value % INSTANCE_OFFSET == num_classes, or the value is 0 and not listed.
      pred_segments_or_table   the image's segment table dict(n_kept, table[, scores]) of the batched fusion (device or host), a
                 list of records (id, category_id), or None: the records `pan_result_segments_host` finds in the map.
      pan_gt     the ground-truth id map, (h, w) int32 or (h, w, 3) uint8 RGB;  gt_segments: records id, category_id, iscrowd, area.

    device=None: the numpy rules (`pan_result_segments_host` for a table or None, then `pq_image_host`). With a device, `add` stages
    the ground truth in pinned memory, makes one host-to-device copy, launches `ops.pq_confusion` and `ops.pq_match` on the current
    stream and queues one small pinned device-to-host copy of the record; the table's `n_kept` is read through its device pointer
    and nothing synchronises before `summarize()` (an `add` beyond `max_in_flight` queued copies waits for the oldest). An image
    outside `ops.pq_eval_ok`, with a ground-truth record of id 0, with non-integer areas, or without a table or a list, takes the
    host rule. The records of the two routes are equal, bit for bit."""

    def __init__(self, all_cat_ids, isthing, unknown_cat_ids=None, num_classes=None, device=None, max_in_flight=8):
        self.all_cat_ids = [int(c) for c in all_cat_ids]
        self.isthing = [int(bool(t)) for t in isthing]
        if len(self.isthing) != len(self.all_cat_ids):
            raise ValueError(f'PQEvaluator: {len(self.all_cat_ids)} categories, {len(self.isthing)} isthing flags')
        self.unknown_cat_ids = [] if unknown_cat_ids is None else [int(c) for c in unknown_cat_ids]
        self.num_classes = len(self.all_cat_ids) if num_classes is None else int(num_classes)
        self.categories = {c: dict(id=c, isthing=t) for c, t in zip(self.all_cat_ids, self.isthing)}
        self._label_of = {c: i for i, c in enumerate(self.all_cat_ids)}
        self.device = None
        self.max_in_flight = int(max_in_flight)
        self.records = []
        self._in_flight = []
        self._pinned = {}
        self.device_images = 0     # images that took the device route
        if device is not None:
            import torch
            self.device = torch.device(device)

    # -- one image ---------------------------------------------------------------------------------
    def add(self, pan_pred, pred_segments_or_table, pan_gt, gt_segments):
        if len(pan_pred.shape) != 2:
            raise ValueError(f'PQEvaluator.add: pan_pred must be an (h, w) map (got shape {tuple(pan_pred.shape)})')
        H, W = int(pan_pred.shape[0]), int(pan_pred.shape[1])
        gt_arr, fmt = _check_pan_seg(_to_numpy(pan_gt), (H, W))
        gt_segments = list(gt_segments)
        image_id = len(self.records)
        if self.device is not None and self._device_ok(pred_segments_or_table, gt_segments, H, W):
            self._add_device(pan_pred, pred_segments_or_table, gt_arr, fmt, gt_segments, H, W, image_id)
        else:
            self._add_host(pan_pred, pred_segments_or_table, gt_arr, gt_segments, image_id)

    def _device_ok(self, pred, gt_segments, H, W):
        from . import ops
        if pred is None:
            return False
        P = int(pred['table'].shape[0]) if _is_table(pred) else len(pred)
        if not ops.pq_eval_ok(len(gt_segments), P, H, W, bool(self.isthing and self.isthing[0])):
            return False
        for el in gt_segments:
            a = el['area']
            if int(el['id']) == VOID or int(a) != a or not 0 <= int(a) < (1 << 31) or not 0 <= int(el['id']) < (1 << 31):
                return False
        if not _is_table(pred):
            for el in pred:
                if not 0 <= int(el['id']) < (1 << 31):
                    return False
        return True

    def _add_host(self, pan_pred, pred, gt_arr, gt_segments, image_id):
        pan = _to_numpy(pan_pred)
        if pred is None or _is_table(pred):
            pan, pred = pan_result_segments_host(pan, self.num_classes, self.all_cat_ids, self.isthing)
        else:
            pan = np.array(pan, dtype=np.int64)
            pan[pan % INSTANCE_OFFSET == self.num_classes] = VOID
        self.records.append(pq_image_host(gt_arr, gt_segments, pan.astype(np.int32), pred, image_id))

    def _codes(self):
        """category id -> the int32 code the kernel compares: the label for a category of all_cat_ids, else a negative code of its own
        (within one image: a ground truth and a pred of one unlisted category still compare equal, as in the host rule)"""
        other = {}
        return lambda c: self._label_of[int(c)] if int(c) in self._label_of else other.setdefault(int(c), -2 - len(other))

    def _add_device(self, pan_pred, pred, gt_arr, fmt, gt_segments, H, W, image_id):
        import torch
        from . import ops
        dev = self.device
        by_id = _by_id(gt_segments, 'gt_segments')
        G = len(by_id)
        code = self._codes()
        is_table = _is_table(pred)
        pred_host = None if torch.is_tensor(pan_pred) and pan_pred.is_cuda else np.ascontiguousarray(_to_numpy(pan_pred), dtype=np.int32)
        table_host = None
        if is_table and not (torch.is_tensor(pred['table']) and pred['table'].is_cuda):
            table_host = np.ascontiguousarray(_to_numpy(pred['table']), dtype=np.int32).reshape(-1, 4)
            n_kept_host = int(_to_numpy(pred['n_kept']))
        elif not is_table:
            plist = _by_id(pred, 'pred_segments')
            table_host = np.array([[int(k), code(e['category_id']), 1, i] for i, (k, e) in enumerate(plist.items())], np.int32).reshape(-1, 4)
            n_kept_host = len(plist)
        P = int(pred['table'].shape[0]) if is_table else len(plist)
        # one pinned buffer, one copy: the ground-truth map, its id / category / area / crowd lists, and what of the pred is on the host
        parts, total = {}, 0
        for name, nbytes in (('gt_map', gt_arr.nbytes), ('gt_ids', 4 * G), ('gt_cats', 4 * G), ('gt_area', 4 * G), ('gt_crowd', G),
                             ('pred_map', 0 if pred_host is None else pred_host.nbytes),
                             ('table', 0 if table_host is None else table_host.nbytes), ('n_kept', 0 if table_host is None else 4)):
            parts[name] = (total, nbytes)
            total += _align(nbytes)
        total = max(total, 16)
        stage = self._pinned.pop(('in', total), None)
        if stage is None:
            stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        raw = stage.numpy()

        def put(name, arr):
            o, nb = parts[name]
            raw[o:o + nb] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)

        put('gt_map', gt_arr)
        put('gt_ids', np.array(list(by_id), np.int32))
        put('gt_cats', np.array([code(e['category_id']) for e in by_id.values()], np.int32))
        put('gt_area', np.array([int(e['area']) for e in by_id.values()], np.int32))
        put('gt_crowd', np.array([e['iscrowd'] == 1 for e in by_id.values()], np.uint8))
        if pred_host is not None:
            put('pred_map', pred_host)
        if table_host is not None:
            put('table', table_host)
            put('n_kept', np.array([n_kept_host], np.int32))
        dbuf = stage.to(dev, non_blocking=True)

        def dpart(name, dtype, shape):
            o, nb = parts[name]
            return dbuf[o:o + nb].view(dtype).view(shape)

        gt_map = dpart('gt_map', torch.int32, (H, W)) if fmt == 0 else dpart('gt_map', torch.uint8, (H, W, 3))
        pmap = pan_pred if pred_host is None else dpart('pred_map', torch.int32, (H, W))
        if pmap.dtype != torch.int32:
            pmap = pmap.to(torch.int32)
        if table_host is None:
            table, n_kept = pred['table'], pred['n_kept'].reshape(1)
        else:
            table, n_kept = dpart('table', torch.int32, (P, 4)), dpart('n_kept', torch.int32, (1,))
        gt_ids, gt_cats = dpart('gt_ids', torch.int32, (G,)), dpart('gt_cats', torch.int32, (G,))
        conf = ops.pq_confusion(pmap.contiguous(), table, n_kept, gt_map, gt_ids, self.num_classes)
        rec_dev, offs = ops.pq_match(conf, gt_cats, dpart('gt_crowd', torch.uint8, (G,)), dpart('gt_area', torch.int32, (G,)), table, n_kept)
        host = self._pinned.pop(('out', rec_dev.numel()), None)
        if host is None:
            host = torch.empty(rec_dev.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(rec_dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.records.append(dict(pending=host, done=done, offs=offs, dims=(G, P), stage=stage, image_id=image_id, is_table=is_table,
                                 gt=by_id, pred=None if is_table else plist))
        self._in_flight.append(len(self.records) - 1)
        self.device_images += 1
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
            self._pinned[('out', rec['pending'].numel())] = rec['pending']
            self._pinned[('in', rec['stage'].numel())] = rec['stage']

    def _parse(self, rec):
        """pinned bytes of one image -> the record `pq_image_host` returns; the status word becomes the reference's errors"""
        raw = rec['pending'].numpy()
        G, P = rec['dims']

        def part(name, dtype, n):
            o, nb = rec['offs'][name]
            return raw[o:o + nb].view(dtype)[:n].copy()

        status, bad = (int(v) for v in part('status', np.int32, 2))
        flags = part('pred_flags', np.uint8, P)
        value, cat, area = part('pred_value', np.int32, P), part('pred_cat', np.int32, P), part('pred_area', np.int32, P)
        if status & STATUS_UNLISTED_PRED:
            raise KeyError('In the image with ID {} segment with ID {} is presented in PNG and not presented in JSON.'.format(
                rec['image_id'], bad))
        valid = (flags & 1) != 0
        if status & STATUS_NO_PIXELS:
            raise KeyError('In the image with ID {} the following segment IDs {} are presented in JSON and not presented in PNG.'.format(
                rec['image_id'], [int(v) for v in value[valid & (area == 0)]]))
        if status & STATUS_MULTI_MATCH:
            raise ValueError(f'PQEvaluator: image {rec["image_id"]}: a ground-truth segment matches more than one prediction (a recorded '
                             'area understates its pixels); the device record keeps one match per ground truth -- evaluate with device=None')
        slots = np.nonzero(valid)[0]                       # table rows that are segments (dropped and merged rows are not)
        if rec['is_table']:                                # in ascending value order, as `pan_result_segments_host` lists them
            slots = slots[np.argsort(value[slots], kind='mergesort')]
        new_slot = np.full(P + 1, -1, np.int32)
        new_slot[slots] = np.arange(len(slots), dtype=np.int32)
        gt_match = part('gt_match', np.int32, G)
        gt = rec['gt']
        if rec['is_table']:
            pred_cat = np.asarray(self.all_cat_ids, np.int64)[cat[slots]] if len(slots) else np.zeros(0, np.int64)
        else:
            pred_cat = np.array([int(e['category_id']) for e in rec['pred'].values()], np.int64).reshape(-1)[slots]
        return dict(gt_id=np.array(list(gt), np.int64).reshape(G), gt_cat=np.array([int(e['category_id']) for e in gt.values()], np.int64).reshape(G),
                    gt_crowd=np.array([e['iscrowd'] == 1 for e in gt.values()], bool).reshape(G),
                    gt_match=new_slot[gt_match], gt_iou=part('gt_iou', np.float64, G),
                    pred_id=value[slots].astype(np.int64), pred_cat=pred_cat, pred_area=area[slots].astype(np.int64),
                    pred_matched=(flags[slots] & 2) != 0, pred_ignored=(flags[slots] & 4) != 0, extra=[])

    # -- the whole run -----------------------------------------------------------------------------
    def image_records(self):
        """every image's record, in `add` order (waits for the queued device copies); what a distributed run gathers"""
        self._drain()
        return self.records

    def summarize(self, extra_records=None):
        """-> dict(stats {category: tp, fp, fn, iou}, pq_results (the four splits and 'classwise'), results (the twelve numbers and
        PQ_copypaste), images). extra_records: further image records (of other ranks) accumulated after this evaluator's own."""
        records = list(self.image_records()) + list(extra_records or ())
        stats = pq_accumulate_host(records)
        pq_results = pq_splits_host(stats, self.categories, self.unknown_cat_ids)
        return dict(stats=stats, pq_results=pq_results, results=parse_pq_results_host(pq_results), images=len(records))
