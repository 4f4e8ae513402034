"""A/B of the two ways to score one image's panoptic map, in ONE process, alternating: the device route (`PQEvaluator.add` on the
device map and segment table: one pinned H2D copy of the ground truth, the confusion and matching kernels, one small pinned copy of
the record, waited for) against the host route (the map copied out, then `pq_eval.pan_result_segments_host` + `pq_image_host`), at
configs[4] geometry, 800 x 1344. Two inputs: the map and table the random-weight model returns (it holds one id), and a synthetic
pair of maps with about 30 ground-truth and 40 predicted segments. Median [min .. max] over --reps alternating repetitions after a
warm-up; the device route's parts (copy, confusion, match) by HIP events on their own.

    python scratch/pq_eval_ab.py [--reps 10] [--out profiles/pq_eval_ab.txt]
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


def events(fn, reps):
    out = []
    for _ in range(reps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out[3:]


def synthetic_pair(H, W, n_gt, n_pred, num_things, num_classes, seed):
    """ground truth of n_gt rectangles over VOID (24-bit ids, one crowd) and a raw result map of n_pred shifted copies and noise"""
    rs = np.random.RandomState(seed)
    gt = np.zeros((H, W), np.int32)
    ids = rs.choice(np.arange(1, 2 ** 24), size=n_gt, replace=False)
    rects, labels = [], rs.randint(0, num_classes, size=n_gt)
    for k in range(n_gt):
        r0, c0 = rs.randint(0, H - 40), rs.randint(0, W - 40)
        rects.append((r0, min(H, r0 + rs.randint(40, 400)), c0, min(W, c0 + rs.randint(40, 400))))
        gt[rects[k][0]:rects[k][1], rects[k][2]:rects[k][3]] = ids[k]
    segments = [dict(id=int(ids[k]), category_id=int(labels[k]) + 1, iscrowd=int(k == 3 and labels[k] < num_things),
                     area=int((gt == ids[k]).sum())) for k in range(n_gt)]
    pan = np.full((H, W), num_classes, np.int32)
    for k in range(n_pred):
        if k < n_gt:
            r0, r1, c0, c1 = rects[k]
            r0, c0, label = r0 + rs.randint(0, 8), c0 + rs.randint(0, 8), int(labels[k])
        else:
            r0, c0, label = rs.randint(0, H - 40), rs.randint(0, W - 40), int(rs.randint(0, num_classes))
            r1, c1 = r0 + rs.randint(20, 200), c0 + rs.randint(20, 200)
        pan[r0:r1, c0:c1] = label + (1000 * (k + 1) if label < num_things else 0)
    return pan, gt, segments


def table_of(pan, Q, num_classes):
    rows = [[int(v), int(v) % 1000, int((pan == v).sum()), k] for k, v in enumerate(np.unique(pan)) if int(v) % 1000 != num_classes]
    table = np.zeros((Q, 4), np.int32)
    table[:len(rows)] = np.array(rows, np.int32).reshape(-1, 4)
    return table, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cgg_amd import ops, pq_eval, runtime, synthetic
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.WORKLOADS['cfg4']
    args = argparse.Namespace(backbone=wl['backbone'], panoptic=wl['panoptic'], hw=wl['hw'], queries=wl['queries'], batch=1)
    _, model = bench.build_model(args, dev)
    H, W = args.hw
    fh = model.panoptic_fusion_head
    n, things = int(fh.num_classes), int(fh.num_things_classes)
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(1234)).to(dev)
    with torch.no_grad(), runtime.precision_scope('bf16'):
        res = model.simple_test(img, synthetic.img_metas(1, H, W), rescale=True, device_results=True, with_segments=True)[0]
    model_pan, model_seg = res['panoptic_all_results'], res['panoptic_segments']
    Q = int(model_seg['table'].shape[0])
    pan_np, gt_map, gt_segments = synthetic_pair(H, W, 30, 40, things, n, seed=7)
    table_np, n_kept = table_of(pan_np, Q, n)
    syn_pan = torch.from_numpy(pan_np).to(dev)
    syn_seg = dict(n_kept=torch.tensor(n_kept, dtype=torch.int32, device=dev), table=torch.from_numpy(table_np).to(dev))
    cats, isthing = list(range(1, n + 1)), [int(k < things) for k in range(n)]
    lines = [f'pq_eval_ab: device route (PQEvaluator.add + wait for its record) vs host route (map copy + numpy rules), {a.reps} '
             f'alternating repetitions after 2 warm-up rounds, one process; median [min .. max]',
             f'configs[4] geometry {H}x{W}, {n} classes ({things} things), segment table of Q = {Q} rows; ground truth: (h, w) int32 map '
             f'on the host with {len(gt_segments)} records']
    for name, pan, seg in (('map of the random-weight model', model_pan, model_seg), ('synthetic pair of maps', syn_pan, syn_seg)):
        on_dev = pq_eval.PQEvaluator(cats, isthing, device=dev)
        on_host = pq_eval.PQEvaluator(cats, isthing)

        def device_route():
            on_dev.add(pan, seg, gt_map, gt_segments)
            return on_dev.image_records()[-1]            # waits for the pinned copy and parses it

        def host_copy():
            return pan.cpu().numpy()

        def host_segments(m):
            return pq_eval.pan_result_segments_host(m, n, cats, isthing)

        def host_image(m, segs):
            return pq_eval.pq_image_host(gt_map, gt_segments, m.astype(np.int32), segs)

        for _ in range(2):
            d = device_route()
            h = host_image(*host_segments(host_copy()))
        assert on_dev.device_images == 2
        for k in h:
            assert (list(d[k]) == list(h[k])) if k == 'extra' else np.array_equal(d[k], h[k]), k
        assert d['gt_iou'].tobytes() == h['gt_iou'].tobytes()
        td, tc, ts, ti = [], [], [], []
        for _ in range(a.reps):
            td.append(timed(device_route)[0])
            t, m = timed(host_copy)
            tc.append(t)
            t, (m0, segs) = timed(lambda: host_segments(m))
            ts.append(t)
            ti.append(timed(lambda: host_image(m0, segs))[0])
            on_dev.records.clear()
        # the device route's parts on their own
        G = len(gt_segments)
        stage = torch.empty(gt_map.nbytes + 16 * G + 64, dtype=torch.uint8, pin_memory=True)
        t_copy = events(lambda: stage.to(dev, non_blocking=True), a.reps)
        gt_dev = torch.from_numpy(gt_map).to(dev)
        gt_ids = torch.tensor([s['id'] for s in gt_segments], dtype=torch.int32, device=dev)
        gt_cats = torch.tensor([s['category_id'] - 1 for s in gt_segments], dtype=torch.int32, device=dev)
        gt_crowd = torch.tensor([s['iscrowd'] for s in gt_segments], dtype=torch.uint8, device=dev)
        gt_area = torch.tensor([s['area'] for s in gt_segments], dtype=torch.int32, device=dev)
        kept = seg['n_kept'].reshape(1)
        ws = ops.pq_confusion(pan, seg['table'], kept, gt_dev, gt_ids, n)
        t_conf = events(lambda: ops.pq_confusion(pan, seg['table'], kept, gt_dev, gt_ids, n, ws=ws), a.reps)
        t_match = events(lambda: ops.pq_match(ws, gt_cats, gt_crowd, gt_area, seg['table'], kept), a.reps)
        nbytes = H * W * 8
        lines += [f'{name}: {len(h["pred_id"])} predicted segments, {int((h["gt_match"] >= 0).sum())} matches, '
                  f'{int(h["pred_ignored"].sum())} ignored preds',
                  f'  device route, per add (staging, H2D, 3 launches, D2H, parse)   {med(td)}',
                  f'    its H2D copy of the staged ground truth alone ({stage.numel() / 1e6:.1f} MB)   {med(t_copy)}',
                  f'    cgg_pq_confusion_i32 alone (zero + count, 2 launches)       {med(t_conf)}   reads {nbytes / 1e6:.1f} MB -> '
                  f'{nbytes / 1e6 / statistics.median(t_conf):.0f} GB/s',
                  f'    cgg_pq_match alone (1 launch)                               {med(t_match)}',
                  f'  host route: D2H of the map ({H * W * 4 / 1e6:.1f} MB)                            {med(tc)}',
                  f'  host route: pan_result_segments_host                          {med(ts)}',
                  f'  host route: pq_image_host                                     {med(ti)}',
                  f'  host route, all three                                         {med([x + y + z for x, y, z in zip(tc, ts, ti)])}']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
