"""A/B of the two ways to evaluate one image's instance masks, in ONE process, alternating: the device route (`SegmEvaluator.add` on
the device results: two kernels and one small pinned copy of the match records, waited for) against the host route (the bit planes
copied out, then `mask_eval.mask_intersections_host` + `mask_iou_host` + `evaluate_img_host`), at configs[1] geometry: 1024 x 1024,
the first D = 100 masks the random-weight model returns, G = 30 synthetic ground truths (rectangles, two of them crowd). Median
[min .. max] over --reps alternating repetitions after a warm-up; then the intersection kernel alone (HIP events) with its achieved
bytes/s against its one-pass traffic, (D + G) x H x W / 8.

    python scratch/mask_eval_ab.py [--reps 20] [--out profiles/mask_eval_ab.txt]
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

HBM_GBS = 8000.0        # MI355X peak


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
    labels, boxes, bits = (t[:100].contiguous() for t in res['all_results'])
    D, G = int(bits.shape[0]), 30
    K = int(model.panoptic_fusion_head.all_classes)
    cat_ids = list(range(1, K + 1))
    rs = np.random.RandomState(7)
    gt = np.zeros((G, H, W), bool)
    for g in range(G):
        r0, c0 = rs.randint(0, H - 64), rs.randint(0, W - 64)
        gt[g, r0:r0 + rs.randint(16, 400), c0:c0 + rs.randint(16, 400)] = True
    gt_cats = rs.randint(1, K + 1, size=G)
    crowd = np.zeros(G, bool)
    crowd[-2:] = True
    gt_dev = torch.from_numpy(gt).to(dev)
    on_dev = mask_eval.SegmEvaluator(cat_ids, device=dev)
    on_host = mask_eval.SegmEvaluator(cat_ids, device=None)
    scores = boxes[:, 4].cpu().numpy().astype(np.float64)
    det_cats = np.asarray(cat_ids)[labels.cpu().numpy()]
    gt_bits_host = mask_eval.pack_bool_rows_host(gt)

    def device_route():
        on_dev.add(labels, boxes, bits, gt_dev, gt_cats, crowd)
        return on_dev.image_records()[-1]            # waits for the pinned copy and parses it

    def device_route_host_gt():                       # ground truth arrives as a host bool array: 31 MB H2D first
        on_dev.add(labels, boxes, bits, gt, gt_cats, crowd)
        return on_dev.image_records()[-1]

    def host_copy():
        return bits.cpu().numpy()

    def host_inter(planes):
        return mask_eval.mask_intersections_host(planes, gt_bits_host, W)

    def host_match(inter, area_d, area_g):
        iou = mask_eval.mask_iou_host(inter, area_d, area_g, crowd)
        return mask_eval.evaluate_img_host(iou, scores, det_cats, gt_cats, crowd, area_g.astype(np.float64), area_d, cat_ids,
                                           on_host.area_rngs, on_host.iou_thrs, on_host.max_dets[-1], False)

    for _ in range(2):
        d = device_route()
        device_route_host_gt()
        h = host_match(*host_inter(host_copy()))
    for k in range(K):
        for ar in range(4):
            assert (d[k][ar] is None) == (h[k][ar] is None)
            if d[k][ar] is not None:
                assert all(np.array_equal(d[k][ar][n], h[k][ar][n]) for n in ('dt_match', 'dt_ignore', 'gt_ignore', 'dt_scores'))
    td, tdh, tc, ti, tm = [], [], [], [], []
    for _ in range(a.reps):
        td.append(timed(device_route)[0])
        tdh.append(timed(device_route_host_gt)[0])
        t, planes = timed(host_copy)
        tc.append(t)
        t, inter = timed(lambda: host_inter(planes))
        ti.append(t)
        tm.append(timed(lambda: host_match(*inter))[0])
        on_dev.records.clear()
    n_match = sum(int((r['dt_match'] > 0).sum()) for per_area in h for r in per_area if r is not None)
    lines = [f'mask_eval_ab: device route (SegmEvaluator.add + wait for its records) vs host route (plane copy + numpy rules), '
             f'{a.reps} alternating repetitions after 2 warm-up rounds, one process; median [min .. max]',
             f'configs[1] {H}x{W}, D = {D} masks of the random-weight model, G = {G} synthetic ground truths, K = {K} categories, '
             f'T = 10, A = 4 ({n_match} matched entries)',
             f'  device route, ground truth on the device   {med(td)}',
             f'  device route, ground truth from the host   {med(tdh)}   ({G * H * W / 1e6:.0f} MB of bool bitmaps H2D first)',
             f'  host route: D2H of the planes              {med(tc)}   ({D * H * bits.shape[2] / 1e6:.1f} MB)',
             f'  host route: mask_intersections_host        {med(ti)}',
             f'  host route: mask_iou + evaluate_img_host   {med(tm)}',
             f'  host route, all three                      {med([x + y + z for x, y, z in zip(tc, ti, tm)])}']
    gt_bits = ops.pack_bool_masks(gt_dev)
    ws = torch.empty(int(ops._lib_().cgg_mask_intersections_workspace_bytes(D, G, H, W)), dtype=torch.uint8, device=dev)
    tk = []
    for _ in range(a.reps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.mask_intersections(bits, gt_bits, W, ws=ws)
        e.record()
        e.synchronize()
        tk.append(s.elapsed_time(e))
    tk = tk[3:]
    nbytes = (D + G) * H * bits.shape[2]
    lines.append(f'  cgg_mask_intersections_bits alone (2 launches) {med(tk)}   one-pass traffic {nbytes / 1e6:.1f} MB -> '
                 f'{nbytes / 1e6 / statistics.median(tk):.0f} GB/s = {nbytes / 1e4 / statistics.median(tk) / HBM_GBS:.1f} % of HBM peak '
                 f'(the planes were just written / read: they may be served from the 256 MiB cache)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
