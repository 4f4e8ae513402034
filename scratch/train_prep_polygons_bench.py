"""Instance samples with polygon annotations through the device-side training pipeline, two ways, at the shape an instance-config
user runs: B = 16 raw samples of 480 x 640, the reference pipeline's 1024 x 1024 output, 15 instances of 1 to 3 parts and about 40
vertices each, ratios drawn from (0.1, 2.0).

  (a) the route before `cgg_train_prep_polygons_u8`: bitmaps made beforehand (NOT timed here: see the last line) and staged,
      `TrainPrep.prep` on them (`cgg_train_prep_u8`);
  (b) `TrainPrep.prep` on the raw polygon samples: the coordinates staged, the masks rasterised on the device.

One process; after a warm-up the sides alternate, ten repeats each. Per side: bytes staged, device time of the launches (HIP events
around the op, after the H2D copy on the same stream), wall time of `prep` (it returns after its one synchronisation), each as
median [min .. max] over the repeats. The host time of `polygon_mask_host` over the batch is reported on a line of its own: it is
THIS BUILD'S numpy statement of the rule, not pycocotools' C -- it says what the rule costs in numpy, not what the reference's
loader costs, and is no speed-up figure.

    python scratch/train_prep_polygons_bench.py [out.txt]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402
import cgg_amd              # noqa: E402,F401
from cgg_amd import ops, synthetic, train_prep as tp  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
SPEC = tp.TrainPrepSpec(img_scale=(1024, 1024), ratio_range=(0.1, 2.0), flip_ratio=0.5, crop_size=(1024, 1024), size=(1024, 1024),
                        pad_val=((128.0, 128.0, 128.0), 0, 255), mean=MEAN, std=STD, to_rgb=True, with_seg=False)
B, HW, INSTANCES, REPEATS = 16, (480, 640), 15, 10
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def main():
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    raw = [synthetic.polygon_sample(HW, 80, seed=100 + i, extra=INSTANCES - 4, vertices=(36, 44)) for i in range(B)]
    params = [tp.draw_train_params(rng, HW, SPEC) for _ in raw]
    parts = [len(p) for s in raw for p in s['gt_polygons']]
    verts = [len(xy) // 2 for s in raw for p in s['gt_polygons'] for xy in p]
    say(f'B = {B}, {HW[0]} x {HW[1]} sources -> 1024 x 1024, {INSTANCES} instances per image, parts per instance {min(parts)} .. '
        f'{max(parts)}, vertices per part {min(verts)} .. {max(verts)} ({sum(verts)} in all); drawn ratios '
        f'{min(p.scale[0] for p in params) / 1024:.2f} .. {max(p.scale[0] for p in params) / 1024:.2f}')

    t0 = time.perf_counter()
    bitmaps = [tp.polygons_to_bitmap_sample(s) for s in raw]
    host_ms = (time.perf_counter() - t0) * 1e3

    events = []
    for name in ('train_prep_u8', 'train_prep_polygons_u8'):     # HIP events around the launches of either entry point
        def timed(*a, _f=getattr(ops, name), **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = _f(*a, **kw)
            e1.record()
            events.append((e0, e1))
            return out
        setattr(ops, name, timed)

    prep = tp.TrainPrep(SPEC, dev)

    def side(samples):
        t1 = time.perf_counter()
        out = prep.prep(samples, params)
        return out, (time.perf_counter() - t1) * 1e3

    sides = [('(a)  bitmaps staged, cgg_train_prep_u8', lambda: side(bitmaps)),
             ('(b)  polygons staged, cgg_train_prep_polygons_u8', lambda: side(raw))]
    ref = None
    for _ in range(2):                                           # warm-up: slots allocated, kernels loaded; and the sides agree
        for _, f in sides:
            (kw, kept), _ = f()
            torch.cuda.synchronize()
            got = (kept, [m.cpu() for m in kw['gt_masks']], [x.cpu() for x in kw['gt_bboxes']], kw['img'].cpu())
            if ref is None:
                ref = got
            assert got[0] == ref[0] and all(torch.equal(x, y) for x, y in zip(got[1], ref[1])) and torch.equal(got[3], ref[3]) \
                and all(torch.equal(x, y) for x, y in zip(got[2], ref[2])), 'the sides disagree'
    say(f'both sides give equal images, masks and boxes; kept {sum(ref[0])} of {B * INSTANCES} instances')
    events.clear()
    rows = {name: dict(wall=[], dev=[], staged=0) for name, _ in sides}
    for _ in range(REPEATS):
        for name, f in sides:
            _, wall = f()
            torch.cuda.synchronize()
            (e0, e1), = events
            events.clear()
            r = rows[name]
            r['wall'].append(wall)
            r['dev'].append(e0.elapsed_time(e1))
            r['staged'] = prep.last_staged_bytes

    def fmt(v, d=2):
        return f'{np.median(v):.{d}f} [{min(v):.{d}f} .. {max(v):.{d}f}]'
    launches = {sides[0][0]: 2, sides[1][0]: 3}
    say(f'median [min .. max] over {REPEATS} alternating repeats, ms')
    say(f'{"side":<50} {"staged MB":>10} {"launches":>9} {"device, all launches":>26} {"per launch":>11} {"prep wall":>24}')
    for name, _ in sides:
        r = rows[name]
        say(f'{name:<50} {r["staged"] / 1e6:>10.2f} {launches[name]:>9} {fmt(r["dev"], 3):>26} '
            f'{np.median(r["dev"]) / launches[name]:>11.3f} {fmt(r["wall"]):>24}')
    a, b = rows[sides[0][0]], rows[sides[1][0]]
    say(f'(b): staged bytes x {b["staged"] / a["staged"]:.3f} of (a); device time {np.median(b["dev"]) - np.median(a["dev"]):+.3f} ms '
        f'against (a), whose own spread is {max(a["dev"]) - min(a["dev"]):.3f} ms; prep wall '
        f'{np.median(b["wall"]) - np.median(a["wall"]):+.2f} ms')
    say(f'host, not part of either side: polygon_mask_host over the batch ({B * INSTANCES} instances) took {host_ms:.1f} ms once -- this '
        "build's numpy statement of rule 6, NOT pycocotools' C: it is no measure of the reference's loader and no speed-up figure")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
