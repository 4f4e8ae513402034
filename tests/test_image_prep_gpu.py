"""csrc/image_prep.hip against the rule of image_prep.py (`prepare_host`), and `inference_detector` end to end.

Stage 1 -- mean 0, std 1, no channel flip: the floats are the integer levels, and the kernel must EQUAL the host rule (bit-exact).
Stage 2 -- the shipped mean / std with to_rgb: atol 1e-6 against the float64 formula (x - mean) / std on the host rule's levels. For
these constants: mean rounding 6.7e-8, subtract rounding 1.3e-7, reciprocal-std rounding 1.6e-7, multiply rounding 1.2e-7 -- about
4.5e-7 in all for |v| <= 2.65; the tolerance leaves a 2 x margin. (Both sides also apply the same two float32 operations, so they are
equal as well; that is asserted too.)

The kernel's tile is TH x TW = 16 x 256 output pixels per workgroup. The shapes are the smallest at which it can go wrong:
  1 x 6 -> 4 x 9        a single source row: both vertical taps clamp
  7 x 5 -> 14 x 10      upsampling: source rows shared between output rows
  40 x 56 -> 17 x 23    more than 2 x down: taps skip source pixels; 17 = TH + 1 rows
  33 x 31 -> 64 x 61    a 93-byte pitch: no source row is dword-aligned
  50 x 70 -> 130 x 300  8 TH + 2 rows and TW + 44 columns: several tiles each way, both last tiles ragged
  200 x 1200 -> 16 x 256   one full tile whose source span (200 rows x 3.6 KB) exceeds the 32 KB LDS image: the global-memory tap path
each without Pad (Wb = new_w: the scalar-store path unless new_w % 4 == 0) and padded to a multiple of 32 (the float4-store path).
"""
import os
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import image_prep as ip, ops, synthetic
from cgg_amd.config import Config

pytestmark = pytest.mark.gpu

TH, TW = 16, 256
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
SHAPES = [((1, 6), (4, 9)), ((7, 5), (14, 10)), ((40, 56), (TH + 1, 23)), ((33, 31), (64, 61)), ((50, 70), (8 * TH + 2, TW + 44)),
          ((200, 1200), (TH, TW))]


def _rand_img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _spec(new_hw, **kw):
    d = dict(img_scale=(new_hw[1], new_hw[0]), keep_ratio=False, size_divisor=None)
    d.update(kw)
    return ip.PrepSpec(**d)


def _device_batch(dev, imgs, spec, **kw):
    """ImagePrep into a NaN-filled caller-owned buffer: every element has to be written"""
    want, metas = ip.prepare_host(imgs, spec)
    out = torch.full(want.shape, float('nan'), dtype=torch.float32, device=dev)
    got, got_metas = ip.ImagePrep(spec, dev, **kw)(imgs, out=out)
    assert got is out
    got = got.cpu()
    assert not torch.isnan(got).any(), 'an element of the output was not written'
    for a, b in zip(metas, got_metas):
        assert a.keys() == b.keys() and a['img_shape'] == b['img_shape'] and a['pad_shape'] == b['pad_shape']
        assert np.array_equal(a['scale_factor'], b['scale_factor'])
    return got, torch.from_numpy(want)


@pytest.mark.parametrize('divisor', [None, 32])
@pytest.mark.parametrize('src, dst', SHAPES)
def test_stage1_levels_equal_the_host_rule(dev, src, dst, divisor):
    img = _rand_img(src[0], src[1], 100 + src[0])
    got, want = _device_batch(dev, [img], _spec(dst, size_divisor=divisor, pad_val=(3.0, 5.0, 7.0)))
    assert torch.equal(got, want)
    assert torch.equal(got[0, :, :dst[0], :dst[1]], got[0, :, :dst[0], :dst[1]].round())


@pytest.mark.parametrize('pad_before_norm', [True, False])
@pytest.mark.parametrize('src, dst', SHAPES)
def test_stage2_shipped_constants(dev, src, dst, pad_before_norm):
    img = _rand_img(src[0], src[1], 200 + src[0])
    spec = _spec(dst, size_divisor=32, pad_val=(128.0, 64.0, 32.0), mean=MEAN, std=STD, to_rgb=True, pad_before_norm=pad_before_norm)
    got, want = _device_batch(dev, [img], spec)
    levels = ip.resize_u8(img, *dst)[:, :, ::-1].astype(np.float64)                      # the host rule's levels, RGB
    f64 = ((levels - np.array(MEAN)) / np.array(STD)).transpose(2, 0, 1)
    assert np.abs(got[0, :, :dst[0], :dst[1]].double().numpy() - f64).max() <= 1e-6
    pad = np.array((32.0, 64.0, 128.0)) if pad_before_norm else np.array((128.0, 64.0, 32.0))    # source order ahead of the flip
    padv = (pad - np.array(MEAN)) / np.array(STD) if pad_before_norm else pad
    below, right = got[0, :, dst[0]:, :].double().numpy(), got[0, :, :dst[0], dst[1]:].double().numpy()
    assert below.size + right.size > 0
    for region in (below, right):
        assert region.size == 0 or np.abs(region - padv[:, None, None]).max() <= 1e-6
    assert torch.equal(got, want)


def test_batch_of_three_sizes_in_one_launch(dev):
    """keep_ratio=True; the staged images start at bytes 96, 201 (odd) and 552 behind the 96-byte table; pad and collate regions
    by value, the collate region on the right of images 0 and 1 and below image 2"""
    imgs = [_rand_img(7, 5, 1), _rand_img(13, 9, 2), _rand_img(20, 41, 3)]
    spec = ip.PrepSpec(img_scale=(96, 64), keep_ratio=True, size_divisor=32, pad_val=128.0, mean=MEAN, std=STD, to_rgb=True)
    got, want = _device_batch(dev, imgs, spec)
    assert torch.equal(got, want)
    geoms = [ip.image_geometry(i.shape[:2], spec) for i in imgs]
    assert geoms == [(90, 64, 96, 64), (92, 64, 96, 64), (47, 96, 64, 96)] and tuple(got.shape) == (3, 3, 96, 96)
    padv = torch.tensor([(128.0 - m) / s for m, s in zip(MEAN, STD)], dtype=torch.float64)
    for b, (nh, nw, ph, pw) in enumerate(geoms):
        if nw < pw:
            assert (got[b, :, :ph, nw:pw].double() - padv[:, None, None]).abs().max() <= 1e-6
        assert nh < ph and (got[b, :, nh:ph, :pw].double() - padv[:, None, None]).abs().max() <= 1e-6
        assert torch.all(got[b, :, :, pw:] == 0) and torch.all(got[b, :, ph:, :] == 0)
    assert got[0, :, :, 64:].numel() > 0 and got[2, :, 64:, :].numel() > 0       # collate regions on the right and at the bottom


def test_entry_with_pitched_rows_and_a_table_behind_the_images(dev):
    """the C-ABI layout in full: an image at byte 1 with a row pitch of 3 w + 5, a second one behind it, the table last"""
    a, b = _rand_img(9, 11, 4), _rand_img(6, 17, 5)
    spec = ip.PrepSpec(img_scale=(40, 24), keep_ratio=True, size_divisor=8, pad_val=0.0, mean=MEAN, std=STD, to_rgb=False,
                       pad_before_norm=False)
    want, _ = ip.prepare_host([a, b], spec)
    pa = 3 * 11 + 5
    off_a, off_b = 1, 1 + 9 * pa
    table_off = (off_b + 6 * 51 + 3) & ~3
    staged = np.full(table_off + 64, 255, dtype=np.uint8)
    staged[off_a:off_a + 9 * pa].reshape(9, pa)[:, :33] = a.reshape(9, 33)
    staged[off_b:off_b + 6 * 51] = b.reshape(-1)
    ga, gb = ip.image_geometry((9, 11), spec), ip.image_geometry((6, 17), spec)
    table = torch.tensor([[off_a, 9, 11, pa, *ga], [off_b, 6, 17, 51, *gb]], dtype=torch.int32)
    staged[table_off:].view(np.int32)[:] = table.numpy().reshape(-1)
    out = torch.full(want.shape, float('nan'), device=dev)
    ops.image_prep_u8(torch.from_numpy(staged).to(dev), table, out, MEAN, STD, 0.0, to_rgb=False, pad_before_norm=False,
                      table_offset=table_off)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


def test_slot_reuse_without_synchronisation(dev):
    """7 calls on 2 staging slots, different images and sizes, nothing synchronised in between: each batch equals its own host result"""
    spec = ip.PrepSpec(img_scale=(320, 200), keep_ratio=True, size_divisor=32, pad_val=128.0, mean=MEAN, std=STD, to_rgb=True)
    prep = ip.ImagePrep(spec, dev, slots=2)
    batches = [[_rand_img(60 + 7 * k, 90 + 5 * k, 10 + k), _rand_img(80 - 3 * k, 70 + 11 * k, 30 + k)] for k in range(7)]
    batches[3] = [torch.from_numpy(batches[3][0]), torch.from_numpy(batches[3][1]).to(dev)]       # CPU and device tensors
    batches[4] = [torch.from_numpy(batches[4][0]).pin_memory(), batches[4][1]]                     # a pinned source
    batches[5] = [_rand_img(200, 300, 50), _rand_img(150, 280, 51)]                                # outgrows the 64 KiB first slot
    got = [prep(b)[0] for b in batches]
    torch.cuda.synchronize()
    for g, b in zip(got, batches):
        assert torch.equal(g.cpu(), torch.from_numpy(ip.prepare_host(b, spec)[0]))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
PIPELINE = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(192, 128), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Pad', size_divisor=32, pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
                             dict(type='Normalize', mean=list(MEAN), std=list(STD), to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


@pytest.fixture(scope='module')
def model(dev):
    from util import randomize
    cfg = Config(dict(model=synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2,
                                                   dec_layers=3, vocab=500, num_points=256),
                      data=dict(test=dict(pipeline=PIPELINE))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = cgg_amd.init_detector(cfg, None, device=dev)
    randomize(m, seed=9)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.fill_(1.0)
            mod.running_mean.zero_()
    assert m.cfg is cfg and not m.training
    return m


def _diff(a, b, path='result'):
    """where two results differ (None: nowhere): same structure, same dtypes, same bits"""
    if isinstance(a, dict):
        if not isinstance(b, dict) or a.keys() != b.keys():
            return f'{path}: keys'
        return next((d for d in (_diff(a[k], b[k], f'{path}[{k!r}]') for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return f'{path}: length'
        return next((d for d in (_diff(x, y, f'{path}[{i}]') for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if torch.is_tensor(a):
        return None if torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b) else f'{path}: tensor'
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.dtype != b.dtype or a.shape != b.shape:
            return f'{path}: array type / shape'
        return None if np.array_equal(a, b) else f'{path}: {int((a != b).sum())} of {a.size} values, max |a - b| = {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3g}'
    return None if a == b else f'{path}: {a!r} != {b!r}'


def _structured_u8(h, w, seed):
    x = synthetic.structured_images(1, h, w, seed=seed, shapes=8)[0]
    return ((x - x.min()) / (x.max() - x.min()) * 255).round().byte().permute(1, 2, 0).contiguous().numpy()


def test_inference_detector_equals_simple_test_on_the_host_batch(dev, model):
    """The float inputs are identical (asserted), so the results are compared for EXACT equality. One thing in the detector is not
    a function of its input alone: the mask score is a float atomic sum over workgroups of 4096 output pixels
    (csrc/postproc.hip), whose order changes from run to run. Two terms have one order only, so the sources here have at most
    2 x 4096 pixels (results are rescaled to the source size): 64 x 96 and 90 x 64. Their padded shapes, 128 x 192 and 192 x 128,
    also give both images a collate region."""
    a, b = _structured_u8(64, 96, 1), _structured_u8(90, 64, 2)
    spec = ip.parse_test_pipeline(PIPELINE)
    host, metas = ip.prepare_host([a, b], spec)
    assert host.shape == (2, 3, 192, 192) and [m['pad_shape'] for m in metas] == [(128, 192, 3), (192, 128, 3)]
    seen = []
    real = model.simple_test
    model.simple_test = lambda imgs, img_metas, **kw: (seen.append((imgs.clone(), kw)), real(imgs, img_metas, **kw))[1]
    try:
        got = cgg_amd.inference_detector(model, [a, b])
    finally:
        del model.simple_test
    assert isinstance(got, list) and len(got) == 2
    assert torch.equal(seen[0][0].cpu(), torch.from_numpy(host)) and seen[0][1] == dict(rescale=True)
    for m in metas:
        m['batch_input_shape'] = (192, 192)
    with torch.no_grad():
        want = model.simple_test(torch.from_numpy(host).to(dev), metas, rescale=True)
    assert _diff(got, want) is None
    assert any(len(m) for r in got for m in r['all_results'][1]), 'no detection at all: the comparison is empty'


def test_inference_detector_at_the_head_tests_size(dev, model):
    """B = 2 at 128 x 192, the size of the head tests: 24 576 output pixels = 6 workgroups per mask in the score sum, so the scores
    may differ between two runs in the order of a 6-term float sum. Labels (the per-class lists), box corners and masks are exact.
    Score tolerance, relative: two orders of a sum of n = 6 positive float32 terms differ by at most 2 (n - 1) 2^-24, and the
    division by the pixel count and the product with the class score that follow round once more each: 12 x 2^-24 = 7.2e-7."""
    a, b = _structured_u8(128, 192, 5), _structured_u8(128, 192, 6)
    spec = ip.parse_test_pipeline(PIPELINE)
    host, metas = ip.prepare_host([a, b], spec)
    assert host.shape == (2, 3, 128, 192)
    got = cgg_amd.inference_detector(model, [a, b])
    for m in metas:
        m['batch_input_shape'] = (128, 192)
    with torch.no_grad():
        want = model.simple_test(torch.from_numpy(host).to(dev), metas, rescale=True)
    assert len(got) == len(want) == 2
    rtol, n_masks = 12 * 2.0**-24, 0
    for g, w in zip(got, want):
        assert g.keys() == w.keys()
        for k in g:
            (gb, gm), (wb, wm) = g[k], w[k]
            assert len(gb) == len(wb) and len(gm) == len(wm)
            for c, (x, y) in enumerate(zip(gb, wb)):
                assert x.shape == y.shape and np.array_equal(x[:, :4], y[:, :4]), (k, c)
                worst = np.abs(x[:, 4] - y[:, 4]) / np.maximum(np.abs(y[:, 4]), 1e-30)
                assert worst.size == 0 or worst.max() <= rtol, (k, c, float(worst.max()))
            assert _diff(gm, wm, f'masks[{k!r}]') is None
            n_masks += sum(len(c) for c in gm)
    assert n_masks > 0, 'no detection at all: the comparison is empty'


def test_single_image_and_keywords_pass_through(dev, model):
    a = _structured_u8(100, 150, 3)
    seen = []
    real = model.simple_test
    model.simple_test = lambda imgs, img_metas, **kw: (seen.append(kw), real(imgs, img_metas, **kw))[1]
    try:
        got = cgg_amd.inference_detector(model, torch.from_numpy(a), with_caption=True)
        dev_res = cgg_amd.inference_detector(model, (a,), device_results=True, mask_bits=True)
    finally:
        del model.simple_test
    assert isinstance(got, dict) and 'all_results' in got
    assert seen[0] == dict(rescale=True, with_caption=True) and seen[1] == dict(rescale=True, device_results=True, mask_bits=True)
    assert isinstance(dev_res, list) and len(dev_res) == 1
    labels, boxes, masks = dev_res[0]['all_results']
    assert torch.is_tensor(labels) and torch.is_tensor(masks) and masks.is_cuda           # device results: nothing was copied out


# ---- tools/test.py on raw uint8 frames -------------------------------------------------------------------------------------------------
def _frames():
    return [_structured_u8(100, 150, 20 + i) for i in range(6)] + [_structured_u8(110, 120, 30)]


def u8_stream(cfg, rank, world):
    """`--data` hook: six 100 x 150 frames (three pipelined batches: the first is the example the graphs are captured on, the later
    ones are written into the pipeline's own input buffers) and one 110 x 120 frame of another padded shape (a trailing short batch);
    with a dict of extra meta keys, with None, and bare"""
    for i, f in enumerate(_frames()):
        if i % world == rank:
            yield (f, dict(filename=f'u8_{i}.jpg')) if i % 3 == 0 else ((torch.from_numpy(f), None) if i % 3 == 1 else f)


def float_stream(cfg, rank, world):
    """the same frames prepared on the host: the driver's float path"""
    spec = ip.parse_test_pipeline(PIPELINE)
    for i, f in enumerate(_frames()):
        if i % world == rank:
            batch, metas = ip.prepare_host([f], spec)
            yield torch.from_numpy(batch[0]), metas[0]


def test_test_driver_serves_raw_uint8_frames(dev, tmp_path):
    """tools/test.py --data with raw uint8 frames returns, image by image and in order, what it returns for the same frames prepared
    by `prepare_host` and fed as float tensors; --synthetic-u8 runs."""
    import importlib.util
    import sys
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = cgg_amd.registry.build_detector(cfg)
    randomize(m, seed=21)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.fill_(1.0)
            mod.running_mean.zero_()
    ck = save_checkpoint(m, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny_u8.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\ndata = dict(test=dict(pipeline=' + repr(PIPELINE) + '))\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tests'))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_u8', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    a = drv.main([str(cfg_file), ck, '--data', 'test_image_prep_gpu:u8_stream'])
    b = drv.main([str(cfg_file), ck, '--data', 'test_image_prep_gpu:float_stream'])
    assert len(a) == 7 and len(b) == 7
    shapes = [(100, 150)] * 6 + [(110, 120)]
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert set(ra) == set(rb)
        for k in ra:
            assert tuple(ra[k][2].shape[-2:]) == shapes[i] == tuple(rb[k][2].shape[-2:]), (i, k)      # rescaled to the source, in order
            assert sorted(ra[k][0].tolist()) == sorted(rb[k][0].tolist()), (i, k)
            assert int(ra[k][2].sum()) == int(rb[k][2].sum()), (i, k)
    c = drv.main([str(cfg_file), ck, '--synthetic-u8', '100x150', '--num-images', '4'])
    assert len(c) == 4 and all(tuple(r[k][2].shape[-2:]) == (100, 150) for r in c for k in r)
