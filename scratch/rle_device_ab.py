"""A/B of the two RleCollector modes (host encoder on the copied bit planes vs run boundaries found on the device) in ONE
process: the loop of bench.py's `host_results_rate` on configs[1], the two collectors alternating, ROUNDS rounds each, for
the masks as produced (noise: the random-weight model) and for the filled disks (trained-like). Reports median [min .. max]
images/s, D2H bytes per image, the share of masks that took the column-plane fallback, the device time of the
`ops.rle_transitions` launches of one batch (HIP events) and the time from `submit` to the `copied` event on an idle device.

    python scratch/rle_device_ab.py [--steps 20] [--rounds 10] [--out profiles/rle_device_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def disks_like(results, cache):
    """bench.py's `with_disks`: the same result tensors with every mask replaced by a filled disk (made once, on the device)"""
    out = []
    for res in results:
        per = {}
        for key, val in res.items():
            if isinstance(val, (tuple, list)) and len(val) == 3 and torch.is_tensor(val[2]) and val[2].dtype == torch.uint8:
                m = val[2]
                k = (tuple(m.shape), m.device)
                if k not in cache:
                    n, Hh, Wb = m.shape
                    yy = torch.arange(Hh, device=m.device).view(1, Hh, 1).float()
                    xx = torch.arange(Wb * 8, device=m.device).view(1, 1, Wb * 8).float()
                    g = torch.Generator(device='cpu').manual_seed(11)
                    cy = (torch.rand(n, 1, 1, generator=g) * Hh).to(m.device)
                    cx = (torch.rand(n, 1, 1, generator=g) * Wb * 8).to(m.device)
                    rr = (torch.rand(n, 1, 1, generator=g) * 0.25 + 0.05).to(m.device) * Hh
                    on = ((yy - cy) ** 2 + (xx - cx) ** 2) <= rr ** 2
                    w = (on.view(n, Hh, Wb, 8).to(torch.uint8) << torch.arange(8, device=m.device, dtype=torch.uint8)).sum(-1)
                    cache[k] = w.to(torch.uint8).contiguous()
                per[key] = (val[0], val[1], cache[k])
            else:
                per[key] = val
        out.append(per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cgg_amd import ops, runtime
    from cgg_amd.host_results import RleCollector, fusion_class_counts
    from cgg_amd.pipeline import detector_pipeline
    wl = bench.WORKLOADS['cfg1']
    args = argparse.Namespace(backbone=wl['backbone'], panoptic=wl['panoptic'], hw=wl['hw'], queries=wl['queries'], batch=wl['batch'],
                              pipeline=3, defer_tail=0)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    runtime.set_precision('fp32')
    _, model = bench.build_model(args, dev)
    B, (H, W) = args.batch, args.hw
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1234)).to(dev)
    metas = bench.workload_metas(args, B)
    nstage = 3
    pipe = detector_pipeline(model, img, metas, stages=nstage, defer_tail=0, rescale=True, device_results=True, mask_bits=True)
    ncls = fusion_class_counts(model.panoptic_fusion_head)
    cols = dict(host=RleCollector(dev, ncls), device=RleCollector(dev, ncls, device_rle=True))
    cache = {}

    def run(col, n, smooth):
        # bench.py host_results_rate.run, with the collector as a parameter
        depth = nstage - 1
        futs, in_copy, pending, copied = [], [], [], {}
        tally = dict(images=0, masks=0, nbytes=0)

        def drain(block):
            while futs and (block or futs[0].done()):
                for im in futs.pop(0).result():
                    tally['images'] += 1
                    for key in im:
                        for cls in im[key][1]:
                            tally['masks'] += len(cls)
                            tally['nbytes'] += sum(len(r['counts']) for r in cls)
        for _ in range(n):
            while len(in_copy) > depth + 1:
                RleCollector.wait_copied(in_copy.pop(0))
            ev = copied.pop(pipe._n % pipe.slots, None)
            if ev is not None:
                pipe.streams[-1].wait_event(ev)
            pending.append(pipe.submit(img))
            while len(pending) > depth:
                old = pending.pop(0)
                r = pipe.wait(old)
                f = col.submit(disks_like(r, cache) if smooth else r)
                futs.append(f)
                in_copy.append(f)
                copied[old] = f.copied
            drain(False)
        for old in pending:
            r = pipe.wait(old)
            futs.append(col.submit(disks_like(r, cache) if smooth else r))
        drain(True)
        return tally

    lines = [f'rle_device_ab: configs[1] ({H}x{W}, batch {B}, {args.queries} queries, fp32), {nstage}-stage pipeline, {a.steps} steps per round, '
             f'{a.rounds} rounds per mode alternating in one process; rle_threads={cols["host"].rle_threads}, '
             f'cpu_quota={runtime.effective_cpu_count()}, run_capacity=default ({RleCollector.RUNS_PER_MASK} per mask)']
    with runtime.precision_scope('fp32'):
        for smooth, label in ((True, 'filled disks (trained-like)'), (False, 'masks as produced (noise)')):
            rates = dict(host=[], device=[])
            before = {k: dict(c.stats) for k, c in cols.items()}
            images = dict(host=0, device=0)
            per_mask = 0.0
            for k, c in cols.items():
                run(c, 3, smooth)
            for k, c in cols.items():                     # the warm-up does not count
                before[k] = dict(c.stats)
            for _ in range(a.rounds):
                for k, c in cols.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    t = run(c, a.steps, smooth)
                    torch.cuda.synchronize()
                    rates[k].append(t['images'] / (time.perf_counter() - t0))
                    images[k] += t['images']
                    per_mask = t['nbytes'] / max(t['masks'], 1)
                    masks_per_image = t['masks'] / max(t['images'], 1)
            lines.append(f'\n{label}: {masks_per_image:.0f} masks per image, {per_mask:.0f} bytes of RLE per mask')
            for k, c in cols.items():
                d = {s: c.stats[s] - before[k][s] for s in c.stats}
                r = rates[k]
                share = f', fallback share {d["fallback_masks"] / max(d["masks"], 1):.3f}' if k == 'device' else ''
                lines.append(f'  {k:6s} {statistics.median(r):7.1f} images/s [{min(r):.1f} .. {max(r):.1f}]   '
                             f'D2H {d["d2h_bytes"] / max(images[k], 1) / 1e6:.3f} MB per image{share}')
            # one batch on an idle device: the kernels' device time and submit -> copied
            old = pipe.submit(img)
            r = pipe.wait(old)
            r = disks_like(r, cache) if smooth else r
            torch.cuda.synchronize()
            tensors = [v[2] for im in r for v in im.values() if isinstance(v, (tuple, list)) and len(v) == 3]
            bufs = [ops.rle_transitions(m, m.shape[-1] * 8, capacity=RleCollector.RUNS_PER_MASK * m.shape[0]) for m in tensors]
            torch.cuda.synchronize()
            kern = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for m, (p, o, w) in zip(tensors, bufs):
                    ops.rle_transitions(m, m.shape[-1] * 8, positions=p, offsets=o, ws=w)
                e1.record()
                e1.synchronize()
                kern.append(e0.elapsed_time(e1))
            lines.append(f'  device time of the rle_transitions launches of one batch ({len(tensors)} tensors, '
                         f'{sum(m.shape[0] for m in tensors)} masks, 3 launches each): median {statistics.median(kern):.3f} ms '
                         f'[{min(kern):.3f} .. {max(kern):.3f}]')
            for k, c in cols.items():
                lat = []
                for _ in range(10):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f = c.submit(r)
                    f.copied.synchronize()
                    lat.append((time.perf_counter() - t0) * 1e3)
                    f.result()
                lines.append(f'  {k:6s} submit -> copied event, idle device, one batch: median {statistics.median(lat):.3f} ms '
                             f'[{min(lat):.3f} .. {max(lat):.3f}]')
    for c in cols.values():
        c.close()
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
