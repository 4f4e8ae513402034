"""cgg_image_prep_u8 (csrc/image_prep.hip: Resize + Pad + Normalize(to_rgb) + collate of a batch of raw uint8 images in one launch):

1. the kernel alone, at 2 x (480 x 640 -> 800 x 1067, padded 800 x 1088) and 2 x (1024 x 1024 -> 800 x 800), against
     - its byte floor: source bytes read once + B * 3 * Hb * Wb * 4 written, at the 6.29 TB/s a float4 copy reaches on this chip;
     - the same preparation composed from ATen ops on the device from the same uint8 bytes (to float, F.interpolate bilinear,
       channel flip, normalise, pad into the batch). That side interpolates in float32, so it is NOT the pinned rule: its distance
       from the rule is printed (<= 1.3 levels expected), it is the speed that is compared.
   Two timings, both with HIP events, the two sides alternated over 5 rounds:
     - "graph": 100 launches captured into one hipGraph and replayed, per launch -- back-to-back device time with no host enqueue
       in it; this is the figure compared with the byte floor;
     - "eager": 50 launches through the Python wrapper, per launch -- what a caller pays when the host enqueue is the limit;
   (warm: the 1.8 / 6.3 MB source stays in cache, as it does behind its own H2D copy), and one cold eager launch each per round
   behind a 1 GiB fill that evicts the caches.
2. end to end: tools/test.py on 480 x 640 frames, three ways: --synthetic-u8 (raw frames from a PINNED pool), raw frames as pageable
   numpy arrays (what a decoder hands over), and the same frames prepared by `prepare_host` as pinned float tensors (prepared ONCE,
   outside the timed loop: the float side's best case, it only pays the 12.6 MB copy per image). ImagePrep stages every host image
   with a CPU copy into its pinned slot; that copy is timed alone from pageable and from pinned memory. Last, the per-image host
   time of `prepare_host` on one thread, which a user preparing on the host pays on top of the float path.

    python scratch/image_prep_bench.py [out.txt]
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402
import torch.nn.functional as F  # noqa: E402
import cgg_amd              # noqa: E402,F401
from cgg_amd import image_prep as ip, ops, synthetic  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PIPELINE = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(1333, 800), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Pad', size_divisor=32, pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
                             dict(type='Normalize', mean=list(MEAN), std=list(STD), to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
N_LAUNCH, N_GRAPH, ROUNDS, HBM_COPY_TBS = 50, 100, 5, 6.29
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def u8_pool(hw, seed=11, pool=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (hw[0], hw[1], 3), dtype=torch.uint8, generator=g) for _ in range(pool)]


def float_stream(cfg, rank, world):
    """`--data` hook of part 2: the --synthetic-u8 frames, prepared on the host once, as pinned float tensors"""
    spec = ip.parse_test_pipeline(PIPELINE)
    n = int(os.environ['IMAGE_PREP_BENCH_N'])
    pool = []
    for t in u8_pool((480, 640)):
        batch, metas = ip.prepare_host([t.numpy()], spec)
        t = torch.from_numpy(batch[0])
        pool.append((t.pin_memory() if torch.cuda.is_available() else t, metas[0]))
    for i in range(n):
        if i % world == rank:
            yield pool[i % len(pool)][0], dict(pool[i % len(pool)][1], filename=f'synthetic_{i}.jpg')


def u8_stream(cfg, rank, world):
    """`--data` hook of part 2: the same frames as pageable numpy arrays, as a decoder would hand them over (ImagePrep stages those
    through its pinned slot with a host copy; --synthetic-u8's pinned pool is read by the copy engine directly)"""
    n = int(os.environ['IMAGE_PREP_BENCH_N'])
    pool = [t.numpy().copy() for t in u8_pool((480, 640))]
    for i in range(n):
        if i % world == rank:
            yield pool[i % len(pool)], dict(filename=f'synthetic_{i}.jpg')


def timeit(fn, n):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def kernel_case(dev, hw, B=2):
    spec = ip.parse_test_pipeline(PIPELINE)
    imgs = [t.numpy() for t in u8_pool(hw, seed=hw[0], pool=B)]
    want, _ = ip.prepare_host(imgs, spec)
    geoms = [ip.image_geometry(hw, spec) for _ in imgs]
    Hb, Wb = want.shape[-2:]
    nsrc = hw[0] * hw[1] * 3
    table = torch.tensor([[32 * B + b * nsrc, hw[0], hw[1], 3 * hw[1], *geoms[b]] for b in range(B)], dtype=torch.int32)
    staged_h = np.empty(32 * B + B * nsrc, dtype=np.uint8)
    staged_h[:32 * B].view(np.int32)[:] = table.numpy().reshape(-1)
    for b, im in enumerate(imgs):
        staged_h[32 * B + b * nsrc:32 * B + (b + 1) * nsrc] = im.reshape(-1)
    staged = torch.from_numpy(staged_h).to(dev)
    out = torch.empty((B, 3, Hb, Wb), dtype=torch.float32, device=dev)
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    padv = ((128.0 - mean_t) / std_t).view(3, 1, 1)
    out_aten = torch.empty_like(out)

    def kernel():
        ops.image_prep_u8(staged, table, out, MEAN, STD, (128.0, 128.0, 128.0), to_rgb=True, pad_before_norm=True)

    def aten():
        for b in range(B):
            nh, nw, ph, pw = geoms[b]
            x = staged[32 * B + b * nsrc:32 * B + (b + 1) * nsrc].view(hw[0], hw[1], 3).permute(2, 0, 1)[None].float()
            x = F.interpolate(x, size=(nh, nw), mode='bilinear', align_corners=False)
            x = (x.flip(1) - mean_t) / std_t
            out_aten[b] = padv                       # the pad region (Hb x Wb = this image's padded shape here)
            out_aten[b, :, :nh, :nw] = x[0]

    kernel()
    aten()
    torch.cuda.synchronize()
    same = torch.equal(out.cpu(), torch.from_numpy(want))
    dist = ((out - out_aten) * std_t).abs().max().item()
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    t = dict(kernel=[], aten=[])
    cold = dict(kernel=[], aten=[])
    tg = dict(kernel=[], aten=[])
    for _ in range(3):
        kernel(), aten()
    graphs = {}
    try:
        for k, f in (('kernel', kernel), ('aten', aten)):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                f()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(N_GRAPH):
                    f()
            torch.cuda.synchronize()
            gr.replay()
            graphs[k] = gr
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for k in ('kernel', 'aten'):
                tg[k].append(timeit(graphs[k].replay, 1) / N_GRAPH)
    except Exception as exc:      # a measurement aid: the eager figures below still stand
        say(f'  graph timing unavailable: {type(exc).__name__}: {exc}')
        tg = None
    for _ in range(ROUNDS):
        for k, f in (('kernel', kernel), ('aten', aten)):
            t[k].append(timeit(f, N_LAUNCH))
        for k, f in (('kernel', kernel), ('aten', aten)):
            flush.fill_(1.0)
            cold[k].append(timeit(f, 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    medc = {k: sorted(v)[len(v) // 2] for k, v in cold.items()}
    byts = B * nsrc + out.numel() * 4
    floor = byts / (HBM_COPY_TBS * 1e12) * 1e6
    say(f'{B} x ({hw[0]} x {hw[1]} -> {geoms[0][0]} x {geoms[0][1]}, padded {Hb} x {Wb}); kernel == prepare_host bit for bit: {same}; '
        f'ATen composition differs from the rule by at most {dist:.2f} levels')
    say(f'  bytes: {B * nsrc / 1e6:.2f} MB read + {out.numel() * 4 / 1e6:.2f} MB written = {byts / 1e6:.2f} MB; floor at {HBM_COPY_TBS} TB/s '
        f'= {floor:.1f} us')
    for k in ('kernel', 'aten'):
        say(f'  {k:6s} warm median {med[k]:7.1f} us (runs ' + ' '.join(f'{x:.1f}' for x in t[k]) + f'); cold median {medc[k]:7.1f} us (runs '
            + ' '.join(f'{x:.1f}' for x in cold[k]) + ')')
    say(f'  eager (host enqueue included): ATen / kernel = {med["aten"] / med["kernel"]:.2f} x warm, {medc["aten"] / medc["kernel"]:.2f} x cold '
        f'(slowest kernel run {max(t["kernel"]):.1f} us vs fastest ATen run {min(t["aten"]):.1f} us)')
    if tg:
        mg = {k: sorted(v)[len(v) // 2] for k, v in tg.items()}
        for k in ('kernel', 'aten'):
            say(f'  {k:6s} graph median {mg[k]:7.2f} us per launch (runs ' + ' '.join(f'{x:.2f}' for x in tg[k]) + ')')
        say(f'  graph (device time): kernel {byts / mg["kernel"] / 1e6:.2f} TB/s = {100 * floor / mg["kernel"]:.0f} % of the floor rate; '
            f'ATen / kernel = {mg["aten"] / mg["kernel"]:.2f} x')
    return same and med['kernel'] < med['aten']


def end_to_end(n=96):
    import importlib.util
    tmp = tempfile.mkdtemp(prefix='image_prep_bench_')
    cfg = synthetic.model_config(num_things=65, num_stuff=0, num_unknown=17, num_queries=100, depth=50)
    cfg_file = os.path.join(tmp, 'configs1.py')
    with open(cfg_file, 'w') as f:
        f.write('model = ' + repr(cfg) + '\ndata = dict(test=dict(pipeline=' + repr(PIPELINE) + '))\n')
    spec = importlib.util.spec_from_file_location('cgg_tools_test_bench', os.path.join(ROOT, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    os.environ['IMAGE_PREP_BENCH_N'] = str(n)
    common = [cfg_file, 'none', '--num-images', str(n), '--samples-per-gpu', '2', '--mask-bits']
    rates = {}
    for name, extra in (('pinned uint8 frames (--synthetic-u8), device-side preparation', ['--synthetic-u8', '480x640']),
                        ('pageable uint8 arrays, device-side preparation', ['--data', 'scratch.image_prep_bench:u8_stream']),
                        ('float tensors prepared on the host beforehand', ['--data', 'scratch.image_prep_bench:float_stream'])):
        runs = []
        for _ in range(2):
            torch.manual_seed(0)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                drv.main(common + extra)
            rec = json.loads([ln for ln in buf.getvalue().splitlines() if ln.startswith('{')][-1])
            runs.append(rec['images_per_sec_this_rank'])
        rates[name] = runs
        say(f'  tools/test.py, {n} images of 480 x 640 (batch 2, parity mode, --mask-bits), {name}: '
            + ' / '.join(f'{r:.1f}' for r in runs) + ' images/s (two runs)')
    img = u8_pool((480, 640))[0].numpy()
    sp = ip.parse_test_pipeline(PIPELINE)
    # the host copy of one frame into pinned staging, from pageable and from pinned memory (CPU reads of pinned memory can be slow)
    stage = torch.empty(img.size, dtype=torch.uint8).pin_memory().numpy().reshape(img.shape)
    pinned_src = torch.from_numpy(img).pin_memory().numpy()
    for name, src in (('pageable', img), ('pinned', pinned_src)):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            np.copyto(stage, src)
            ts.append((time.perf_counter() - t0) * 1e6)
        say(f'  host copy of one 480 x 640 frame (0.92 MB) from {name} memory into the pinned staging slot: {min(ts):.0f} us best of 5')
    best = {k: max(v) for k, v in rates.items()}
    names = list(best)
    say(f'  best runs: pinned uint8 {best[names[0]]:.1f}, pageable uint8 {best[names[1]]:.1f}, prepared float {best[names[2]]:.1f} images/s; '
        f'uint8 / float = {best[names[0]] / best[names[2]]:.2f} (pinned), {best[names[1]] / best[names[2]]:.2f} (pageable)')
    torch.set_num_threads(1)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ip.prepare_host([img], sp)
        ts.append((time.perf_counter() - t0) * 1e3)
    say(f'  prepare_host (numpy, one thread), one 480 x 640 image: {min(ts):.1f} ms best of 3 = {1e3 / min(ts):.1f} images/s per core; '
        'the reference prepares with cv2, which was not available to time')
    return rates


if __name__ == '__main__':
    dev = torch.device('cuda')
    ok = True
    for hw in ((480, 640), (1024, 1024)):
        ok = kernel_case(dev, hw) and ok
    say('end to end (the synthetic flagship detector, R50 / 100 queries, random weights):')
    end_to_end()
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0 if ok else 1)
