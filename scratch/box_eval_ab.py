"""A/B of the two ways to evaluate one image's boxes, in ONE process, alternating: the device route (`BboxEvaluator.add` on the device
results: one upload of the ground truth, one kernel and one small pinned copy of the match records, waited for) against the host
route (the (D, 5) boxes copied out, then `mask_eval.det_boxes_xywh_host` + `box_iou_host` + `evaluate_img_host`), at configs[1]
geometry: 1024 x 1024, the first D = 100 detections the random-weight model returns, G = 30 synthetic ground truths (jittered
copies of detections' boxes with two-decimal coordinates, two of them crowd). Median [min .. max] over --reps alternating
repetitions after a warm-up; then the matching kernel alone (HIP events).

    python scratch/box_eval_ab.py [--reps 20] [--out profiles/box_eval_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def med(v):
    return f'{statistics.median(v):9.3f} [{min(v):.3f} .. {max(v):.3f}] ms'


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cgg_amd import mask_eval, ops, runtime, synthetic
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.WORKLOADS['cfg1']
    args = argparse.Namespace(backbone=wl['backbone'], panoptic=wl['panoptic'], hw=wl['hw'], queries=wl['queries'], batch=1)
    _, model = bench.build_model(args, dev)
    H, W = args.hw
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(1234)).to(dev)
    with torch.no_grad(), runtime.precision_scope('fp32'):
        res = model.simple_test(img, synthetic.img_metas(1, H, W), rescale=True, device_results=True, mask_bits=True)[0]
    labels, boxes, _ = (t[:100].contiguous() for t in res['all_results'])
    D, G = int(boxes.shape[0]), 30
    K = int(model.panoptic_fusion_head.all_classes)
    cat_ids = list(range(1, K + 1))
    rs = np.random.RandomState(7)
    det = mask_eval.det_boxes_xywh_host(boxes.cpu().numpy())
    src = rs.randint(0, D, size=G)
    gt = np.round(np.stack([det[src, 0] + rs.uniform(-4, 4, G), det[src, 1] + rs.uniform(-4, 4, G),
                            np.maximum(det[src, 2] + rs.uniform(-4, 4, G), 1), np.maximum(det[src, 3] + rs.uniform(-4, 4, G), 1)], axis=1), 2)
    gt_cats = np.asarray(cat_ids)[labels.cpu().numpy()[src]]
    crowd = np.zeros(G, bool)
    crowd[-2:] = True
    area = gt[:, 2] * gt[:, 3]
    on_dev = mask_eval.BboxEvaluator(cat_ids, device=dev)
    on_host = mask_eval.BboxEvaluator(cat_ids, device=None)

    def device_route():
        on_dev.add(labels, boxes, gt, gt_cats, crowd)
        return on_dev.image_records()[-1]            # waits for the pinned copy and parses it

    def host_copy():
        return labels.cpu().numpy(), boxes.cpu().numpy()

    def host_rules(lab, b5):
        d = mask_eval.det_boxes_xywh_host(b5)
        iou = mask_eval.box_iou_host(d, gt, crowd)
        return mask_eval.evaluate_img_host(iou, b5[:, 4].astype(np.float64), np.asarray(cat_ids)[lab], gt_cats, crowd, area,
                                           d[:, 2] * d[:, 3], cat_ids, on_host.area_rngs, on_host.iou_thrs, on_host.max_dets[-1], False)

    for _ in range(2):
        d = device_route()
        h = host_rules(*host_copy())
    for k in range(K):
        for ar in range(4):
            assert (d[k][ar] is None) == (h[k][ar] is None)
            if d[k][ar] is not None:
                assert all(np.array_equal(d[k][ar][n], h[k][ar][n]) for n in ('dt_match', 'dt_ignore', 'gt_ignore', 'dt_scores'))
    td, tc, tr = [], [], []
    for _ in range(a.reps):
        td.append(timed(device_route)[0])
        t, arrays = timed(host_copy)
        tc.append(t)
        tr.append(timed(lambda: host_rules(*arrays))[0])
        on_dev.records.clear()
    n_match = sum(int((r['dt_match'] > 0).sum()) for per_area in h for r in per_area if r is not None)
    det_cats_host = np.asarray(cat_ids)[labels.cpu().numpy()]
    pairs = max(int((det_cats_host == c).sum()) * int((gt_cats == c).sum()) for c in cat_ids)
    lines = [f'box_eval_ab: device route (BboxEvaluator.add + wait for its records) vs host route (copy of the boxes + numpy rules), '
             f'{a.reps} alternating repetitions after 2 warm-up rounds, one process; median [min .. max]',
             f'configs[1] {H}x{W}, D = {D} detections of the random-weight model, G = {G} synthetic ground truths, K = {K} categories, '
             f'T = 10, A = 4 ({n_match} matched entries; detections in {len(np.unique(det_cats_host))} of them, the largest '
             f'category has D_k x G_k = {pairs} pairs)',
             f'  device route (ground truth from the host)    {med(td)}',
             f'  host route: D2H of labels and boxes          {med(tc)}',
             f'  host route: xywh + box_iou + evaluate_img    {med(tr)}',
             f'  host route, both                             {med([x + y for x, y in zip(tc, tr)])}']
    t64 = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)        # noqa: E731
    order = torch.sort(boxes[:, 4].contiguous(), descending=True, stable=True).indices.to(torch.int32)
    det_cats = on_dev._dev['cat_ids'][labels.to(torch.int64)]
    fixed = (t64(gt, torch.float64), order, det_cats, t64(gt_cats, torch.int32), t64(crowd, torch.uint8), t64(area, torch.float64),
             on_dev._dev['cat_ids'], on_dev._dev['area_rngs'], on_dev._dev['iou_thrs'], on_dev.max_dets[-1], False)
    out = ops.coco_match_boxes(boxes, *fixed)
    tk = []
    for _ in range(a.reps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.coco_match_boxes(boxes, *fixed, out=out)
        e.record()
        e.synchronize()
        tk.append(s.elapsed_time(e))
    lines.append(f'  cgg_coco_match_boxes alone ({K} workgroups, HIP events around the wrapper) {med(tk[3:])}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
