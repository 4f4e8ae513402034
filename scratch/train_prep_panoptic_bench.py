"""Panoptic samples through the device-side training pipeline, two ways, at the shape a panoptic user runs: B = 16 raw samples of
480 x 640, the reference pipeline's 1024 x 1024 output, about 30 records with 15 things per image, ratios drawn from (0.1, 2.0).

  (a) the path before `cgg_train_prep_panoptic_u8`: `load_panoptic_host` per sample on the host (the reference loader's loop), then
      `TrainPrep.prep` on the bitmaps and the semantic map (`cgg_train_prep_u8`);
  (b) `TrainPrep.prep` on the raw panoptic samples (int32 id maps), (b') the same with RGB id maps.

One process; after a warm-up the sides alternate, ten repeats each. Per side: host time of the loader step, bytes staged, device time
of the launches (HIP events around the op, after the H2D copy on the same stream), wall time of `prep` (it returns after its one
synchronisation), each as median [min .. max] over the repeats.

    python scratch/train_prep_panoptic_bench.py [out.txt]
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
                        pad_val=((128.0, 128.0, 128.0), 0, 255), mean=MEAN, std=STD, to_rgb=True, with_seg=True)
B, HW, THINGS, REPEATS = 16, (480, 640), 15, 10
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def raw_sample(seed, rgb):
    s = synthetic.panoptic_sample(HW, 80, 53, seed=seed, rgb=rgb, blocks=(4, 8))        # 32 blocks, 30 records
    seen = 0
    for r in s['segments']:                                      # exactly 15 things: the others become stuff
        if r['is_thing']:
            seen += 1
            if seen > THINGS:
                r['is_thing'], r['category'] = False, 80 + seen
    s['gt_labels'] = np.array([r['category'] for r in s['segments'] if r['is_thing']], dtype=np.int64)
    return s


def main():
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    seeds = [100 + i for i in range(B)]
    raw = {False: [raw_sample(k, False) for k in seeds], True: [raw_sample(k, True) for k in seeds]}
    params = [tp.draw_train_params(rng, HW, SPEC) for _ in seeds]
    recs = [len(s['segments']) for s in raw[False]]
    things = [len(s['gt_labels']) for s in raw[False]]
    say(f'B = {B}, {HW[0]} x {HW[1]} sources -> 1024 x 1024, records per image {min(recs)} .. {max(recs)}, things {min(things)} .. '
        f'{max(things)}; drawn ratios {min(p.scale[0] for p in params) / 1024:.2f} .. {max(p.scale[0] for p in params) / 1024:.2f}')

    events = []
    for name in ('train_prep_u8', 'train_prep_panoptic_u8'):     # HIP events around the launches of either entry point
        def timed(*a, _f=getattr(ops, name), **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = _f(*a, **kw)
            e1.record()
            events.append((e0, e1))
            return out
        setattr(ops, name, timed)

    prep = tp.TrainPrep(SPEC, dev)

    def bitmaps(samples):
        out = []
        for s in samples:
            b = {k: v for k, v in s.items() if k not in ('pan_seg', 'segments')}
            b['gt_masks'], b['gt_semantic_seg'] = tp.load_panoptic_host(s['pan_seg'], s['segments'])
            out.append(b)
        return out

    def side_a():
        t0 = time.perf_counter()
        bm = bitmaps(raw[False])
        t1 = time.perf_counter()
        out = prep.prep(bm, params)
        return out, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def side_b(rgb):
        t1 = time.perf_counter()
        out = prep.prep(raw[rgb], params)
        return out, 0.0, (time.perf_counter() - t1) * 1e3

    sides = [('(a)  host loader + cgg_train_prep_u8', side_a), ('(b)  cgg_train_prep_panoptic_u8, int32 maps', lambda: side_b(False)),
             ("(b') cgg_train_prep_panoptic_u8, RGB maps", lambda: side_b(True))]
    ref = None
    for _ in range(2):                                           # warm-up: slots allocated, kernels loaded; and the sides agree
        for _, f in sides:
            (kw, kept), _, _ = f()
            torch.cuda.synchronize()
            got = (kept, [m.cpu() for m in kw['gt_masks']], kw['gt_semantic_seg'].cpu(), [x.cpu() for x in kw['gt_bboxes']])
            if ref is None:
                ref = got
            assert got[0] == ref[0] and all(torch.equal(x, y) for x, y in zip(got[1], ref[1])) and torch.equal(got[2], ref[2]) \
                and all(torch.equal(x, y) for x, y in zip(got[3], ref[3])), 'the sides disagree'
    say(f'all sides give equal masks, semantic maps and boxes; kept {sum(ref[0])} of {sum(things)} things')
    events.clear()
    rows = {name: dict(load=[], wall=[], dev=[], staged=0) for name, _ in sides}
    for _ in range(REPEATS):
        for name, f in sides:
            _, load, wall = f()
            torch.cuda.synchronize()
            (e0, e1), = events
            events.clear()
            r = rows[name]
            r['load'].append(load)
            r['wall'].append(wall)
            r['dev'].append(e0.elapsed_time(e1))
            r['staged'] = prep.last_staged_bytes

    def fmt(v, d=2):
        return f'{np.median(v):.{d}f} [{min(v):.{d}f} .. {max(v):.{d}f}]'
    say(f'median [min .. max] over {REPEATS} alternating repeats, ms')
    say(f'{"side":<44} {"host loader":>24} {"staged MB":>10} {"device, 2 launches":>26} {"prep wall":>24}')
    for name, _ in sides:
        r = rows[name]
        say(f'{name:<44} {fmt(r["load"]):>24} {r["staged"] / 1e6:>10.2f} {fmt(r["dev"], 3):>26} {fmt(r["wall"]):>24}')
    a = rows[sides[0][0]]
    for name, _ in sides[1:]:
        r = rows[name]
        per = 7 if 'int32' in name else 6
        say(f'{name.strip()}: staged bytes x {r["staged"] / a["staged"]:.3f} of (a) (derived per source pixel: {per} / (4 + {THINGS}) = '
            f'{per / (4 + THINGS):.3f}); device time {np.median(r["dev"]) - np.median(a["dev"]):+.3f} ms against (a), whose own spread '
            f'is {max(a["dev"]) - min(a["dev"]):.3f} ms')
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
