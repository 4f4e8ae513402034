"""The device-side training pipeline (train_prep.py / csrc/train_prep.hip) against the host rule, at the reference's training shape:
B = 16 raw samples of 480 x 640 with 7 instance bitmaps each, the 1024 x 1024 large-scale-jitter pipeline, ratios drawn from
(0.1, 2.0) by `draw_train_params`.

  1. `TrainPrep.prep` per batch: wall time of the whole call (host staging copy, H2D, two launches, the statistics D2H and the one
     synchronisation), and the device time of the two launches alone (HIP events around `ops.train_prep_u8` on an already staged
     buffer).
  2. `prepare_train_host` for the same batches on 16 threads (one sample per task; numpy releases the GIL in its loops).

Set beside the training step of `python bench.py --gpus 1 --workload cfg2` (R50, batch 16, 1024 x 1024) from the same session.

    python scratch/train_prep_bench.py [out.txt]
"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402
import cgg_amd              # noqa: E402,F401
from cgg_amd import ops, synthetic, train_prep as tp  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
SPEC = tp.TrainPrepSpec(img_scale=(1024, 1024), ratio_range=(0.1, 2.0), flip_ratio=0.5, crop_size=(1024, 1024), size=(1024, 1024),
                        pad_val=((128.0, 128.0, 128.0), 0, 255), mean=MEAN, std=STD, to_rgb=True)
B, HW, N_INST, BATCHES, THREADS = 16, (480, 640), 7, 6, 16
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def raw_sample(seed):
    b = synthetic.train_batch(1, HW[0], HW[1], num_classes=80, max_inst=N_INST, seed=seed)
    masks = b['gt_masks'][0].numpy()
    while len(masks) < N_INST:                                   # exactly 7 instances: repeat the drawn ones
        masks = np.concatenate([masks, masks])[:N_INST]
    rng = np.random.default_rng(seed)
    return dict(img=rng.integers(0, 256, size=HW + (3,), dtype=np.uint8), gt_masks=np.ascontiguousarray(masks),
                gt_labels=rng.integers(0, 80, size=(N_INST,)))


def main():
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    batches = []
    for k in range(BATCHES):
        samples = [raw_sample(100 * k + i) for i in range(B)]
        batches.append((samples, [tp.draw_train_params(rng, HW, SPEC) for _ in samples]))
    ratios = [p.scale[0] / 1024 for _, ps in batches for p in ps]
    say(f'{BATCHES} batches of B = {B}, {HW[0]} x {HW[1]} sources, {N_INST} instances each; drawn ratios {min(ratios):.2f} .. '
        f'{max(ratios):.2f}, mean {np.mean(ratios):.2f}')

    prep = tp.TrainPrep(SPEC, dev)
    for samples, params in batches[:2]:                          # warm-up: slots allocated, kernels loaded
        prep.prep(samples, params)
    torch.cuda.synchronize()
    walls = []
    for samples, params in batches:
        t0 = time.perf_counter()
        kw, kept = prep.prep(samples, params)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    say(f'TrainPrep.prep, wall per batch (staging copy + H2D + 2 launches + D2H + sync): median {np.median(walls):.2f} ms '
        f'(min {min(walls):.2f}, max {max(walls):.2f}); kept {sum(kept)} of {B * N_INST} instances in the last batch')

    # the two launches alone, on the staged bytes of the last call
    slot = prep._ring.slots[(prep._ring.n - 1) % len(prep._ring.slots)]
    samples, params = batches[-1]
    N = B * N_INST
    img_table = slot.pinned[:4 * ops.TRAIN_PREP_IMG_COLS * B].view(torch.int32).view(B, -1).clone()
    inst_off = 4 * ops.TRAIN_PREP_IMG_COLS * B
    inst_table = slot.pinned[inst_off:inst_off + 4 * ops.TRAIN_PREP_INST_COLS * N].view(torch.int32).view(N, -1).clone()
    nbytes = inst_off + 4 * ops.TRAIN_PREP_INST_COLS * N + B * HW[0] * HW[1] * (3 + N_INST)
    img = torch.empty((B, 3, 1024, 1024), device=dev)
    masks = torch.empty((N, 1024, 1024), dtype=torch.uint8, device=dev)
    stats = torch.empty((N, 5), dtype=torch.int32, device=dev)

    def launch():
        ops.train_prep_u8(slot.dev, img_table, inst_table, img, masks, None, stats, MEAN, STD, SPEC.pad_val[0], to_rgb=True,
                          crop_size=SPEC.crop_size, staged_bytes=nbytes)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 10)
    out_bytes = img.numel() * 4 + masks.numel()
    say(f'cgg_train_prep_u8, device time per batch (2 launches, HIP events, 10 back to back x 5): median {np.median(times):.3f} ms '
        f'(min {min(times):.3f}); {out_bytes / 1e6:.0f} MB written + {nbytes / 1e6:.0f} MB staged -> '
        f'{(out_bytes + nbytes) / np.median(times) / 1e9:.2f} TB/s')

    # the host rule on 16 threads
    def one(args):
        return tp.prepare_train_host([args[0]], [args[1]], SPEC)
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(one, zip(*batches[0])))
        host = []
        for samples, params in batches:
            t0 = time.perf_counter()
            list(pool.map(one, zip(samples, params)))
            host.append((time.perf_counter() - t0) * 1e3)
    say(f'prepare_train_host, wall per batch on {THREADS} threads: median {np.median(host):.1f} ms (min {min(host):.1f}, max {max(host):.1f})')
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
