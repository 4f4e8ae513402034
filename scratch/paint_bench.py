"""A/B of the two ways to paint a result, in ONE process, alternating: the device route (`model.show_result(show_labels=False)` on
device results: the masks are never copied) against the host route (the masks copied out and unpacked as `simple_test`'s host form
does it, then `paint.paint_instances_host` / `paint.paint_panoptic_host`), at configs[1] (1024 x 1024 instance, the masks one
`simple_test` returns, score_thr 0 and 0.3) and configs[4] (800 x 1344 panoptic). Median [min .. max] over --reps alternating
repetitions after a warm-up, and the device time of the paint / labelling launches alone (HIP events) with their bytes against HBM.

    python scratch/paint_bench.py [--reps 20] [--out profiles/paint_ab.txt]
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
    return f'{statistics.median(v):8.2f} [{min(v):.2f} .. {max(v):.2f}] ms'


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def events(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def model_of(name, dev):
    from cgg_amd import synthetic
    wl = bench.WORKLOADS[name]
    args = argparse.Namespace(backbone=wl['backbone'], panoptic=wl['panoptic'], hw=wl['hw'], queries=wl['queries'], batch=1)
    _, model = bench.build_model(args, dev)
    H, W = args.hw
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(1234)).to(dev)
    return model, img, synthetic.img_metas(1, H, W), (H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cgg_amd import ops, paint, runtime
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = [f'paint_ab: device route (show_result(show_labels=False) on device results) vs host route (mask copy + unpack + numpy rule), '
             f'{a.reps} alternating repetitions after 3 warm-up rounds, one process; median [min .. max]']
    with torch.no_grad(), runtime.precision_scope('fp32'):
        # ---- configs[1]: instances ------------------------------------------------------------------------------------------------
        model, x, metas, (H, W) = model_of('cfg1', dev)
        res = model.simple_test(x, metas, rescale=True, device_results=True, mask_bits=True)[0]
        labels_t, boxes_t, bits = res['all_results']
        frame = np.random.default_rng(3).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        n = int(labels_t.numel())
        scores = boxes_t[:, 4].cpu().numpy()
        for thr in (0.0, 0.3):
            def device_route():
                return model.show_result(frame, res, score_thr=thr, show_labels=False)

            def host_copy():
                return np.unpackbits(bits.cpu().numpy(), axis=-1, bitorder='little')[:, :, :W].view(np.bool_)

            def host_paint(masks):
                labels, boxes, _, order, keep = paint.instance_draw_list(res, thr)
                colors = np.zeros((n, 3), np.uint8)
                colors[keep] = paint.instance_colors_host(labels[keep], paint.get_palette(None, int(labels.max()) + 1))
                bc = paint.get_palette((72, 101, 241), int(labels.max()) + 1)[labels]
                return paint.paint_instances_host(frame, masks[order], colors, keep, boxes, bc)
            for _ in range(3):
                d = device_route()
                h = host_paint(host_copy())
            assert np.array_equal(d, h), 'the two routes paint different images'
            td, tc, tp = [], [], []
            for _ in range(a.reps):
                td.append(timed(device_route)[0])
                t, masks = timed(host_copy)
                tc.append(t)
                tp.append(timed(lambda: host_paint(masks))[0])
            kept = int((scores > thr).sum()) if thr > 0 else n
            lines += [f'configs[1] {H}x{W}, {n} masks, score_thr {thr}: {kept} drawn',
                      f'  device route                      {med(td)}',
                      f'  host route: mask copy + unpack    {med(tc)}   ({n * H * W / 1e6:.0f} MB of bool planes)',
                      f'  host route: numpy paint           {med(tp)}',
                      f'  host route, both                  {med([x_ + y_ for x_, y_ in zip(tc, tp)])}']
        dimg = torch.from_numpy(frame).to(dev)
        keep = torch.ones(n, dtype=torch.uint8, device=dev)
        colors = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
        dboxes = torch.from_numpy(paint.truncate_boxes(boxes_t.cpu().numpy())).to(dev)
        out = torch.empty_like(dimg)
        tk = events(lambda: ops.paint_instances(dimg, bits, keep, colors, dboxes, colors, out=out), a.reps)
        nbytes = n * H * bits.shape[2] + 2 * dimg.numel()
        lines.append(f'  cgg_paint_instances_u8 alone      {med(tk)}   {nbytes / 1e6:.1f} MB (packed masks read + image read/write) -> '
                     f'{nbytes / 1e6 / statistics.median(tk):.0f} GB/s = {nbytes / 1e4 / statistics.median(tk) / HBM_GBS:.1f} % of HBM peak')
        del model, res, bits
        # ---- configs[4]: panoptic -------------------------------------------------------------------------------------------------
        model, x, metas, (H, W) = model_of('cfg4', dev)
        res = model.simple_test(x, metas, rescale=True, device_results=True)[0]
        pan = res['panoptic_all_results']
        frame = np.random.default_rng(4).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        void = model.num_classes

        def device_route():
            return model.show_result(frame, res, show_labels=False)

        def host_route():
            p = pan.cpu().numpy()
            ids = np.unique(p)[::-1]
            ids = ids[ids != void]
            colors = paint.instance_colors_host(ids % 1000, paint.get_palette(None, int((ids % 1000).max()) + 1 if len(ids) else 0))
            return paint.paint_panoptic_host(frame, p, ids, colors, void)
        for _ in range(3):
            d, h = device_route(), host_route()
        assert np.array_equal(d, h), 'the two routes paint different images'
        td, th = [], []
        for _ in range(a.reps):
            td.append(timed(device_route)[0])
            th.append(timed(host_route)[0])
        p = pan.cpu().numpy()
        ids = np.unique(p)
        ids = ids[ids != void]
        lines += [f'configs[4] {H}x{W} panoptic map as the random-weight model returns it: {len(ids)} id(s) (the host route grows with '
                  f'the number of ids: one full-image pass each)',
                  f'  device route                      {med(td)}',
                  f'  host route (copy + unique + paint){med(th)}']
        # the same shape with a map of many segments (64-pixel blocks of 40 thing / stuff ids, some void), as a trained model's would be
        rng = np.random.default_rng(5)
        pool = np.concatenate([np.arange(20) + 1000 * np.arange(1, 21), 80 + np.arange(20), [void]]).astype(np.int32)
        coarse = pool[rng.integers(0, len(pool), size=((H + 63) // 64, (W + 63) // 64))]
        res_many = dict(panoptic_all_results=torch.from_numpy(np.kron(coarse, np.ones((64, 64), np.int32))[:H, :W].copy()).to(dev))
        res0, pan0 = res, pan
        res, pan = res_many, res_many['panoptic_all_results']          # the two closures above read these
        for _ in range(3):
            d, h = device_route(), host_route()
        assert np.array_equal(d, h), 'the two routes paint different images'
        td2, th2 = [], []
        for _ in range(a.reps):
            td2.append(timed(device_route)[0])
            th2.append(timed(host_route)[0])
        lines += [f'{H}x{W} synthetic map of 64 x 64 blocks, {len(np.unique(pan.cpu().numpy())) - 1} ids',
                  f'  device route                      {med(td2)}',
                  f'  host route (copy + unique + paint){med(th2)}']
        res, pan = res0, pan0
        dpan = pan.to(torch.int32).contiguous()
        dimg = torch.from_numpy(frame).to(dev)
        tl = events(lambda: ops.label_components(dpan, void), a.reps)
        dids = torch.from_numpy(np.sort(ids).astype(np.int32)).to(dev)
        dcol = torch.randint(0, 256, (len(ids), 3), dtype=torch.uint8, device=dev)
        out = torch.empty_like(dimg)
        tq = events(lambda: ops.paint_panoptic(dimg, dpan, dids, dcol, out=out), a.reps)
        nbytes = dpan.numel() * 4 + 2 * dimg.numel()
        rec, status = ops.label_components(dpan, void)
        lines += [f'  cgg_label_components_i32 alone    {med(tl)}   ({int(status[0])} components; workspace alloc + 3 memsets + 4 launches)',
                  f'  cgg_paint_panoptic_u8 alone       {med(tq)}   {nbytes / 1e6:.1f} MB (id map read + image read/write) -> '
                  f'{nbytes / 1e6 / statistics.median(tq):.0f} GB/s = {nbytes / 1e4 / statistics.median(tq) / HBM_GBS:.1f} % of HBM peak']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
