"""Times the kernels that share csrc/grid_taps.h, csrc/u8_resize.h and the instance-mask reduction tail, through ONE given build of
libcgg_hip.so, at sizes a user runs: device events around one call, 10 warm-up calls, the median / min / p90 of 60. Run it once per
library, each in a fresh process, alternating (before, after, before, after): the two runs of one library give the spread that a
difference between the libraries has to exceed. -> profiles/sampling_refactor_ab.txt
usage: sampling_refactor_ab.py <path of libcgg_hip.so> <result .json>"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
assert _lib._lib is None
from cgg_amd import ops
from cgg_amd._lib import dev_ptr, stream_ptr

dev = torch.device('cuda:0')
WARM, REPS = 10, 60
RES = {}


def timed(name, fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    RES[name] = dict(median_us=statistics.median(ts), min_us=ts[0], p90_us=ts[int(0.9 * len(ts))])
    print(f'{name:46s} median {RES[name]["median_us"]:9.1f} us   min {ts[0]:9.1f}   p90 {RES[name]["p90_us"]:9.1f}', flush=True)


g = torch.Generator().manual_seed(1)

# ---- 100 picks at 1024^2 from 256^2 logits (three launches: plan, masks, final) -------------------------------------------------
logits = (torch.randn(100, 256, 256, generator=g) * 3).to(dev)
qidx = torch.arange(100).to(dev)
cls = torch.rand(100, generator=g).to(dev)
hw = (1024, 1024)
timed('instance_masks_picks 100 x 1024^2 bytes', lambda: ops.instance_masks_picks(logits, qidx, cls, hw, hw, hw))
timed('instance_masks_picks 100 x 1024^2 bit-packed', lambda: ops.instance_masks_picks(logits, qidx, cls, hw, hw, hw, bitpack=True))
# the generic kernel: a crop width that is no multiple of 16
hw2 = (1024, 1000)
timed('instance_masks_picks 100 x 1024x1000 generic', lambda: ops.instance_masks_picks(logits, qidx, cls, hw, hw2, hw2))
del logits

# ---- point samplers at the loss shapes of the R50 training step: batch 16, 256^2 x 256 mask feature, 12 544 points, 184 positives ----
B, Hf, C, P, ROWS = 16, 256, 256, 12544, 184
feat = torch.randn(B, Hf, Hf, C, generator=g).to(dev)
pts = torch.rand(B, P, 2, generator=g).to(dev)
timed('point_sample_nhwc 16 x 256^2 x 256, P 12544', lambda: ops.point_sample_nhwc(feat, pts))
del feat
planes = (torch.rand(64, 1024, 1024, generator=g) > 0.5).float().to(dev)
index = torch.randint(0, 64, (ROWS,), generator=g).to(torch.int32).to(dev)
rpts = torch.rand(ROWS, P, 2, generator=g).to(dev)
timed('point_sample_planes 184 rows of 1024^2, P 12544', lambda: ops.point_sample_planes(planes, index, rpts))
del planes
gout = torch.randn(ROWS, P, generator=g).to(dev)
gp = torch.zeros(ROWS, Hf, Hf, device=dev)


def bwd_atomic():
    ops._call('cgg_point_sample_planes_backward', dev_ptr(gout, 'grad', torch.float32), None, dev_ptr(rpts, 'points', torch.float32),
              dev_ptr(gp), ROWS, Hf, Hf, ROWS, P, stream_ptr(dev))


def bwd_rows():
    ops._call('cgg_point_sample_planes_backward_rows', dev_ptr(gout, 'grad', torch.float32), dev_ptr(rpts, 'points', torch.float32),
              dev_ptr(gp), Hf, Hf, ROWS, P, stream_ptr(dev))


timed('planes_backward (atomic) 184 x 256^2, P 12544', bwd_atomic)
timed('planes_backward_rows (tiled) 184 x 256^2, P 12544', bwd_rows)

# ---- image prep and train prep: a batch of 8 planes of 1024^2 -------------------------------------------------------------------
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
Bi = 8
rng = np.random.default_rng(5)


def stage(h, w, rows):
    """Bi images of h x w x 3 back to back, the table behind them -> (staged, host table, table offset)"""
    n = h * w * 3
    table_off = (Bi * n + 3) & ~3
    t = torch.tensor([[b * n, h, w, 3 * w] + rows(b) for b in range(Bi)], dtype=torch.int32)
    buf = np.zeros(table_off + t.numel() * 4, dtype=np.uint8)
    buf[:Bi * n] = rng.integers(0, 256, size=Bi * n, dtype=np.uint8)
    buf[table_off:].view(np.int32)[:] = t.numpy().reshape(-1)
    return torch.from_numpy(buf).to(dev), t, table_off


out = torch.empty(Bi, 3, 1024, 1024, device=dev)
for label, (h, w) in (('up 768x1024 -> 1024^2 (LDS taps)', (768, 1024)), ('down 2048x2048 -> 1024^2 (global taps)', (2048, 2048))):
    staged, table, toff = stage(h, w, lambda b: [1024, 1024, 1024, 1024])
    timed(f'image_prep_u8 8 x {label}', lambda: ops.image_prep_u8(staged, table, out, MEAN, STD, 114.0, table_offset=toff))
for label, (h, w, nh, o) in (('up 640^2 -> 1280^2, window 1024^2 (LDS taps)', (640, 640, 1280, 128)),
                             ('down 2560^2 -> 1280^2, window 1024^2 (global taps)', (2560, 2560, 1280, 128))):
    staged, table, toff = stage(h, w, lambda b: [nh, nh, o, o, b & 1, 0, 0, -1])
    inst = torch.zeros(0, 3, dtype=torch.int32)
    masks, stats = torch.empty(0, 1024, 1024, dtype=torch.uint8, device=dev), torch.empty(0, 5, dtype=torch.int32, device=dev)
    timed(f'train_prep_u8 8 x {label}',
          lambda: ops.train_prep_u8(staged, table, inst, out, masks, None, stats, MEAN, STD, 114.0, img_table_offset=toff,
                                    inst_table_offset=toff))

torch.cuda.synchronize()
assert os.path.abspath(_lib.LIB_PATH) == os.path.abspath(sys.argv[1]) and _lib._lib is not None
with open(sys.argv[2], 'w') as f:
    json.dump(RES, f, indent=1)
