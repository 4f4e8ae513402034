"""csrc/train_prep.hip against the rule of train_prep.py (`prepare_train_host`): every output of `TrainPrep.prep` EQUALS the host
rule's (torch.equal on image, masks, semantic maps, boxes, labels; the kept counts and the metas), the C ABI's layout and error
codes, and the path from raw samples to a training step (forward_train, tools/train.py --synthetic-u8, the re-sampling of empty
samples).

Both kernels work on TH x TW = 16 x 256 tiles with 4 columns per lane. The shapes are the smallest at which they can go wrong:
  sources 37 x 53, 48 x 64 (twice, once without an instance, in the middle of the batch) and 5 x 7 in ONE batch: 3-byte pixels, odd
  pitches and 1-byte mask rows put images and masks at every byte phase of the staged buffer
  planes (64, 64): 4 row tiles; (32, 48); (30, 50) with a (24, 50) window: W % 4 != 0 (the scalar stores) and a pad below the window
  x 2 upsampling at offset 0 and at the full margin, unflipped and flipped (the LDS image of a tile and the clamped last taps; the
  bottom-right source pixel is outside the window at offset 0 = dropped, and unflipped it touches the window's last row and column at
  the full margin), ~0.1 downsampling (a 4 x 6 resized image: the plane is all pad), a short-side fit that crops one axis and pads
  the other, flip on odd (53, 7) and even (64) widths, with and without semantic maps; 120 x 400 -> 12 x 40: a tile whose source
  span exceeds the LDS image (taps from global memory).
"""
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, synthetic, train_prep as tp
from cgg_amd._lib import CggError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PLANES = [((64, 64), (64, 64)), ((32, 48), (32, 48)), ((24, 50), (30, 50))]          # (crop_size, size)
MODES = ['up2_origin', 'up2_margin', 'up2_margin_flip', 'down_flip', 'short_side']


def _spec(crop, size, seg=False):
    return tp.TrainPrepSpec(img_scale=(64, 64), crop_size=crop, size=size, pad_val=((128.0, 64.0, 32.0), 0, 255), mean=MEAN, std=STD,
                            to_rgb=True, with_seg=seg)


def _raw(h, w, n, seed, seg=False):
    """instance 0: the top-left source pixel; 1: the bottom-right one; 2: everything; 3 ..: random rectangles (bool / 255 / 1)"""
    r = np.random.default_rng(seed)
    masks = np.zeros((n, h, w), dtype=np.uint8)
    for i in range(n):
        if i == 0:
            masks[i, 0, 0] = 1
        elif i == 1:
            masks[i, h - 1, w - 1] = 255
        elif i == 2:
            masks[i] = 1
        else:
            y, x = int(r.integers(0, h)), int(r.integers(0, w))
            masks[i, y:y + int(r.integers(1, h // 2 + 2)), x:x + int(r.integers(1, w // 2 + 2))] = 3
    s = dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), gt_masks=masks.astype(bool) if seed % 2 else masks,
             gt_labels=r.integers(0, 10, size=(n,)), filename=f'raw_{seed}.jpg', gt_caption_ids=r.integers(1, 500, size=(8,)),
             gt_caption_mask=np.ones(8, dtype=np.int64), gt_caption_nouns_ids=r.integers(1, 500, size=(8,)),
             gt_caption_nouns_mask=np.ones(8, dtype=np.int64))
    if seg:
        s['gt_semantic_seg'] = r.integers(0, 134, size=(h, w), dtype=np.uint8)
    return s


def _batch(seg, seed=0):
    return [_raw(37, 53, 5, seed + 1, seg), _raw(48, 64, 0, seed + 2, seg), _raw(48, 64, 4, seed + 3, seg), _raw(5, 7, 3, seed + 4, seg)]


def _params(samples, mode, spec):
    ch, cw = spec.crop_size
    out = []
    for s in samples:
        h, w = s['img'].shape[:2]
        if mode.startswith('up2'):
            scale = (2 * w, 2 * h)
        elif mode == 'down_flip':
            scale = (6, 6)
        else:
            scale = (10000, ch - 3)                              # the short side becomes ch - 3 rows (or columns): pads that axis
        nh, nw = tp.resized_hw((h, w), scale)
        margin = (max(nh - ch, 0), max(nw - cw, 0))
        out.append(tp.TrainParams('flip' in mode, scale, margin if mode.startswith('up2_margin') else
                                  (margin[0] // 2, margin[1] // 2) if mode == 'short_side' else (0, 0)))
    return out


def _assert_equal(got, kept, want, want_kept, dev):
    assert kept == want_kept
    assert set(got) == set(want)
    for k in want:
        if k == 'img_metas':
            for a, b in zip(got[k], want[k]):
                assert a.keys() == b.keys()
                for f in a:
                    if f == 'scale_factor':
                        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f])
                    elif f == 'img_norm_cfg':
                        assert np.array_equal(a[f]['mean'], b[f]['mean']) and np.array_equal(a[f]['std'], b[f]['std']) \
                            and a[f]['to_rgb'] == b[f]['to_rgb']
                    else:
                        assert a[f] == b[f], f
            continue
        gs, ws = (got[k], want[k]) if isinstance(want[k], list) else ([got[k]], [want[k]])
        assert len(gs) == len(ws), k
        for i, (g, w) in enumerate(zip(gs, ws)):
            w = torch.as_tensor(w)
            assert g.device.type == 'cuda' and g.dtype == w.dtype and g.shape == w.shape, (k, i, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(g.cpu(), w), (k, i)


@pytest.mark.parametrize('seg', [False, True])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('crop, size', PLANES)
def test_prep_equals_the_host_rule(dev, crop, size, mode, seg):
    spec = _spec(crop, size, seg)
    samples = _batch(seg)
    params = _params(samples, mode, spec)
    want, want_kept = tp.prepare_train_host(samples, params, spec)
    got, kept = tp.TrainPrep(spec, dev).prep(samples, params)
    _assert_equal(got, kept, want, want_kept, dev)
    assert got['img'].shape == (4, 3) + size and kept[1] == 0 and got['gt_masks'][1].shape == (0,) + size


@pytest.mark.parametrize('flip', [False, True])
def test_taps_from_global_memory_when_a_tile_spans_more_than_the_lds_image(dev, flip):
    """120 x 400 -> 12 x 40: the one tile reads 120 source rows of 1200 bytes, 144 KB > the 32 KB LDS image, so its taps come from
    global memory (every other case here fits); next to it a sample that takes the LDS path in the same launch"""
    spec = _spec((32, 48), (32, 48), True)
    samples = [_raw(120, 400, 4, 61, True), _raw(37, 53, 5, 62, True)]
    params = [tp.TrainParams(flip, (40, 40), (0, 0)), tp.TrainParams(flip, (106, 74), (20, 30))]
    assert tp.resized_hw((120, 400), (40, 40)) == (12, 40) and 120 * 1200 > 32768
    want, want_kept = tp.prepare_train_host(samples, params, spec)
    got, kept = tp.TrainPrep(spec, dev).prep(samples, params)
    _assert_equal(got, kept, want, want_kept, dev)
    assert kept[0] >= 1


def test_the_cases_cover_what_they_claim():
    """host arithmetic only: the geometry the docstring lists is present in the cases above"""
    seen = set()
    for (crop, size), mode in ((p, m) for p in PLANES for m in MODES):
        spec = _spec(crop, size)
        samples = _batch(False)
        params = _params(samples, mode, spec)
        want, kept = tp.prepare_train_host(samples, params, spec)
        for b, (s, p) in enumerate(zip(samples, params)):
            h, w = s['img'].shape[:2]
            nh, nw, oy, ox, eh, ew = tp.sample_geometry((h, w), p, spec)
            n = len(s['gt_masks'])
            if (nh, nw) == (2 * h, 2 * w):
                seen.add('up2')
                if (oy, ox) == (0, 0) and nh > crop[0] and nw > crop[1]:
                    seen.add('origin')
                    assert n == 0 or kept[b] < n                 # the bottom-right pixel lies outside the window: dropped
                if oy > 0 and ox > 0 and (oy, ox) == (nh - crop[0], nw - crop[1]):
                    seen.add('full margin')
                    touching = int((want['gt_bboxes'][b][:, 2:] == np.array([ew, eh])).all(axis=1).sum()) if n else None
                    assert n == 0 or touching >= (1 if p.flip else 2)      # "everything", and unflipped the bottom-right pixel
            if (nh, nw) == (4, 6):
                seen.add('4 x 6')
            if (nh < crop[0]) != (nw < crop[1]):
                seen.add('crop one axis, pad the other')
            if p.flip:
                seen.add('flip odd' if w % 2 else 'flip even')
            if eh < size[0] and ew < size[1]:
                seen.add('pad both')
    assert seen == {'up2', 'origin', 'full margin', '4 x 6', 'crop one axis, pad the other', 'flip odd', 'flip even', 'pad both'}


def test_slot_reuse_without_synchronisation_by_the_caller(dev):
    """5 calls on ONE staging slot, different batches, the results read only at the end: each equals its own host result"""
    spec = _spec((32, 48), (32, 48), True)
    prep = tp.TrainPrep(spec, dev, slots=1)
    runs = []
    for k in range(5):
        samples = _batch(True, seed=10 * k)[::-1] if k % 2 else _batch(True, seed=10 * k)
        if k == 3:
            samples = [_raw(200, 150, 6, 77, True)] + samples      # outgrows the 64 KiB first slot
        params = _params(samples, MODES[k], spec)
        runs.append((prep.prep(samples, params), samples, params))
    torch.cuda.synchronize()
    for (got, kept), samples, params in runs:
        want, want_kept = tp.prepare_train_host(samples, params, spec)
        _assert_equal(got, kept, want, want_kept, dev)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _pitched_layout():
    """two samples: image rows of 3 w + 5 bytes from byte 1 on, bitmap rows of w + 3 bytes, a semantic map, the tables LAST"""
    a, b = _raw(9, 11, 3, 41, True), _raw(6, 17, 2, 42, True)
    spec = tp.TrainPrepSpec(img_scale=(32, 32), crop_size=(16, 20), size=(16, 24), pad_val=((1.0, 2.0, 3.0), 0, 255), mean=MEAN, std=STD,
                            to_rgb=False, with_seg=True)
    params = [tp.TrainParams(False, (30, 30), (0, 0)), tp.TrainParams(True, (40, 40), (0, 20))]      # 25 x 30 and 14 x 40 resized
    buf = np.full(4096, 0xCC, dtype=np.uint8)
    n, img_rows, inst_rows, first = 1, [], [], 0
    for bi, (s, p) in enumerate(zip((a, b), params)):
        h, w = s['img'].shape[:2]
        nh, nw, oy, ox, _, _ = tp.sample_geometry((h, w), p, spec)
        pitch = 3 * w + 5
        off = n
        buf[off:off + h * pitch].reshape(h, pitch)[:, :3 * w] = s['img'].reshape(h, 3 * w)
        n += h * pitch
        masks = np.asarray(s['gt_masks']).astype(np.uint8)
        for m in masks:
            mp = w + 3
            buf[n:n + h * mp].reshape(h, mp)[:, :w] = m
            inst_rows.append((bi, n, mp))
            n += h * mp
        soff = n
        buf[n:n + h * w] = s['gt_semantic_seg'].reshape(-1)
        n += h * w
        img_rows.append((off, h, w, pitch, nh, nw, oy, ox, int(p.flip), first, len(masks), soff))
        first += len(masks)
    inst_off = (n + 3) & ~3
    img_off = inst_off + 12 * len(inst_rows)
    end = img_off + 48 * 2
    img_table, inst_table = torch.tensor(img_rows, dtype=torch.int32), torch.tensor(inst_rows, dtype=torch.int32)
    buf[inst_off:img_off].view(np.int32)[:] = inst_table.numpy().reshape(-1)
    buf[img_off:end].view(np.int32)[:] = img_table.numpy().reshape(-1)
    return (a, b), params, spec, buf[:end].copy(), img_table, inst_table, img_off, inst_off


def test_entry_with_pitched_rows_and_tables_behind_the_planes(dev):
    """the C-ABI layout in full, into dirty outputs: every element is written, the statistics rows included"""
    samples, params, spec, buf, img_table, inst_table, img_off, inst_off = _pitched_layout()
    want, kept = tp.prepare_train_host(list(samples), params, spec)
    N = inst_table.shape[0]
    img = torch.full((2, 3, 16, 24), float('nan'), device=dev)
    masks = torch.full((N, 16, 24), 7, dtype=torch.uint8, device=dev)
    seg = torch.full((2, 1, 16, 24), 7, dtype=torch.uint8, device=dev)
    stats = torch.full((N, 5), 12345, dtype=torch.int32, device=dev)
    ops.train_prep_u8(torch.from_numpy(buf).to(dev), img_table, inst_table, img, masks, seg, stats, MEAN, STD, (1.0, 2.0, 3.0),
                      to_rgb=False, crop_size=(16, 20), seg_pad=255, img_table_offset=img_off, inst_table_offset=inst_off)
    assert torch.equal(img.cpu(), torch.from_numpy(want['img'])) and torch.equal(seg.cpu(), torch.from_numpy(want['gt_semantic_seg']))
    st, m = stats.cpu().numpy(), masks.cpu().numpy()
    assert m.max() <= 1
    first = 0
    for b, s in enumerate(samples):
        n = len(s['gt_masks'])
        eh, ew = want['img_metas'][b]['img_shape'][:2]
        rows = [tp.mask_stats(m[first + i], eh, ew) for i in range(n)]
        assert st[first:first + n].tolist() == [list(r) for r in rows]
        keep = [i for i in range(n) if rows[i][0] >= 1]
        assert len(keep) == kept[b] and np.array_equal(m[first:first + n][keep], want['gt_masks'][b])
        assert np.array_equal(tp.stats_to_boxes(st[first:first + n][keep]), want['gt_bboxes'][b])
        first += n
    assert sum(kept) >= 3


def test_error_codes_without_a_launch():
    """every refusal is decided on the host, before anything is launched: the buffers here are HOST memory"""
    lib = _lib.load()
    _, _, _, buf, img_table, inst_table, img_off, inst_off = _pitched_layout()
    N = inst_table.shape[0]
    staged = np.zeros(buf.size + 64, dtype=np.uint8)
    staged[:buf.size] = buf
    outs = np.zeros(1 << 16, dtype=np.uint8)
    import ctypes
    f3 = ctypes.c_float * 3
    base = dict(staged=staged.ctypes.data, staged_bytes=buf.size, img_off=img_off, inst_off=inst_off, it=img_table, nt=inst_table, B=2, N=N,
                mean=f3(*MEAN), std=f3(*STD), pad=f3(0, 0, 0), to_rgb=1, seg_pad=255, ch=16, cw=20, img=outs.ctypes.data,
                masks=outs.ctypes.data + 16384, seg=outs.ctypes.data + 32768, stats=outs.ctypes.data + 49152, H=16, W=24)
    assert base['staged'] % 16 == 0 and base['img'] % 16 == 0

    def call(**kw):
        a = dict(base, **kw)
        vp = ctypes.c_void_p
        it, nt = a['it'], a['nt']
        return lib.cgg_train_prep_u8(vp(a['staged']), a['staged_bytes'], a['img_off'], a['inst_off'],
                                     vp(it.data_ptr()) if it is not None else None, vp(nt.data_ptr()) if nt is not None else None,
                                     a['B'], a['N'], a['mean'], a['std'], a['pad'], a['to_rgb'], a['seg_pad'], a['ch'], a['cw'], vp(a['img']),
                                     vp(a['masks']), vp(a['seg']), vp(a['stats']), a['H'], a['W'], None)

    def edited(table, row, col, val):
        t = table.clone()
        t[row, col] = val
        return t

    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    cases = [
        (EINVAL, dict(staged=None)), (EINVAL, dict(it=None)), (EINVAL, dict(img=None)), (EINVAL, dict(nt=None)), (EINVAL, dict(masks=None)),
        (EINVAL, dict(stats=None)), (EINVAL, dict(mean=None)),
        (EINVAL, dict(B=0)),
        (EINVAL, dict(it=edited(img_table, 0, 1, 0))),                                   # a zero-sized image
        (EINVAL, dict(it=edited(img_table, 1, 5, 0))),                                   # ... resized to nothing
        (EINVAL, dict(it=edited(img_table, 0, 6, int(img_table[0, 4]) - 16 + 1))),       # oy one past max(nh - ch, 0)
        (EINVAL, dict(it=edited(img_table, 1, 7, int(img_table[1, 5]) - 20 + 1))),       # ox likewise
        (EINVAL, dict(it=edited(img_table, 0, 6, -1))),
        (EINVAL, dict(it=edited(img_table, 0, 3, 3 * 11 - 1))),                          # image pitch < 3 w
        (EINVAL, dict(nt=edited(inst_table, 1, 2, 10))),                                 # bitmap pitch < w
        (EINVAL, dict(it=edited(img_table, 1, 0, buf.size - 10))),                       # an image past staged_bytes
        (EINVAL, dict(nt=edited(inst_table, 4, 1, buf.size - 10))),                      # a bitmap past staged_bytes
        (EINVAL, dict(it=edited(img_table, 1, 11, buf.size - 10))),                      # a semantic map past staged_bytes
        (EINVAL, dict(staged_bytes=img_off + 95)),                                       # the image table past staged_bytes
        (EINVAL, dict(inst_off=buf.size - 8)),                                           # the instance table past staged_bytes
        (EINVAL, dict(img_off=img_off + 2)),                                             # a table offset that is no multiple of 4
        (EINVAL, dict(nt=edited(inst_table, 0, 0, 2))),                                  # an image index out of range
        (EINVAL, dict(nt=edited(inst_table, 0, 0, -1))),
        (EINVAL, dict(nt=edited(inst_table, 0, 0, 1))),                                  # ... in range, but not the owner
        (EINVAL, dict(it=edited(img_table, 1, 9, 2))),                                   # instance ranges that leave a gap
        (EINVAL, dict(N=N - 1)),
        (EINVAL, dict(std=f3(1.0, 0.0, 1.0))),
        (EINVAL, dict(ch=17)),                                                           # a window larger than the plane
        (EINVAL, dict(staged_bytes=0)),
        (EUNSUPPORTED, dict(staged_bytes=2**31 - 8)),
        (EUNSUPPORTED, dict(H=65536)), (EUNSUPPORTED, dict(W=65536, cw=20)),
        (EUNSUPPORTED, dict(it=edited(img_table, 0, 2, 65536))),
        (EUNSUPPORTED, dict(B=40000, N=30000)),
        (EALIGN, dict(staged=base['staged'] + 2)), (EALIGN, dict(img=base['img'] + 4)), (EALIGN, dict(masks=base['masks'] + 1)),
        (EALIGN, dict(seg=base['seg'] + 2)), (EALIGN, dict(stats=base['stats'] + 2)),
    ]
    for i, (code, kw) in enumerate(cases):
        rc = call(**kw)
        assert rc == code, (i, sorted(kw), rc, lib.cgg_last_error_string())
        assert b'cgg_train_prep_u8' in lib.cgg_last_error_string()
    assert not outs.any(), 'a refused call wrote to its outputs'


def test_wrapper_refuses_host_tensors_and_wrong_shapes(dev):
    _, _, _, buf, img_table, inst_table, img_off, inst_off = _pitched_layout()
    N = inst_table.shape[0]
    mk = lambda d: (torch.empty((2, 3, 16, 24), device=d), torch.empty((N, 16, 24), dtype=torch.uint8, device=d),       # noqa: E731
                    torch.empty((2, 1, 16, 24), dtype=torch.uint8, device=d), torch.empty((N, 5), dtype=torch.int32, device=d))
    staged = torch.from_numpy(buf)
    with pytest.raises(CggError, match='ROCm device'):
        ops.train_prep_u8(staged, img_table, inst_table, *mk('cpu'), MEAN, STD, img_table_offset=img_off, inst_table_offset=inst_off)
    img, masks, seg, stats = mk(dev)
    with pytest.raises(CggError, match='masks'):
        ops.train_prep_u8(staged.to(dev), img_table, inst_table, img, masks[:-1], seg, stats, MEAN, STD)
    with pytest.raises(CggError, match='HOST'):
        ops.train_prep_u8(staged.to(dev), img_table.to(dev), inst_table, img, masks, seg, stats, MEAN, STD)


# ---- from raw samples to a training step ------------------------------------------------------------------------------------------
PIPELINE = [dict(type='LoadImageFromFile', to_float32=True),
            dict(type='LoadOpenAnnotations', with_bbox=True, with_mask=True, with_caption=True),
            dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Resize', img_scale=(128, 128), ratio_range=(0.1, 2.0), multiscale_mode='range', keep_ratio=True),
            dict(type='RandomCrop', crop_size=(128, 128), crop_type='absolute', recompute_bbox=True, allow_negative_crop=True),
            dict(type='FilterAnnotations', min_gt_bbox_wh=(1e-5, 1e-5), by_mask=True),
            dict(type='Pad', size=(128, 128), pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
            dict(type='Normalize', mean=list(MEAN), std=list(STD), to_rgb=True),
            dict(type='OpenFormatBundle', img_to_float=True),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_caption_ids', 'gt_caption_mask',
                                       'gt_caption_nouns_ids', 'gt_caption_nouns_mask'])]


def _model_cfg():
    return synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                  vocab=500, num_points=256)


def _driver():
    spec = importlib.util.spec_from_file_location('cgg_tools_train_u8', os.path.join(ROOT, 'tools', 'train.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_forward_train_on_prepared_kwargs(dev):
    """`forward_train(**kwargs)` takes TrainPrep's output as it is, and gives the losses it gives on the uploaded host rule's
    output. The two inputs are equal bit for bit (asserted), the random points are drawn from the same seed, so what is left is the
    run-to-run order of the float atomics in the model's own kernels: 1e-4 (1 + |loss|), the bound the training tests use between
    two runs of one step."""
    from util import randomize
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = cgg_amd.registry.build_detector(_model_cfg())
        model.init_weights()
    randomize(model, seed=5)
    model = model.to(dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    spec = tp.parse_train_pipeline(PIPELINE)
    drv = _driver()
    head = _model_cfg()['panoptic_head']
    known = head['num_things_classes'] + head['num_stuff_classes']           # the labels index the head's known classes, as in the driver
    samples = [s for s, _ in zip(drv.synthetic_u8_samples((48, 64), known, seed=3, vocab=500), range(2))]
    assert max(int(s['gt_labels'].max()) for s in samples) < known
    params = [tp.TrainParams(True, (200, 200), (10, 30)), tp.TrainParams(False, (128, 128), (0, 0))]
    host, host_kept = tp.prepare_train_host(samples, params, spec)
    got, kept = tp.TrainPrep(spec, dev).prep(samples, params)
    _assert_equal(got, kept, host, host_kept, dev)
    assert min(kept) >= 1
    losses = []
    for kw in (got, tp.to_device(host, dev)):
        torch.manual_seed(11)
        out = model.forward_train(**kw)
        losses.append({k: float(v.detach()) for k, v in out.items()})
    a, b = losses
    assert a.keys() == b.keys() and len(a) >= 3
    for k in a:
        assert np.isfinite(a[k]) and abs(a[k] - b[k]) <= 1e-4 * (1 + abs(b[k])), (k, a[k], b[k])


def test_train_driver_on_synthetic_raw_samples(tmp_path):
    """tools/train.py CONFIG --synthetic-u8 48x64 --max-iters 2 in a fresh child process: two steps, finite losses in the log"""
    cfg_file = tmp_path / 'tiny_u8_train.py'
    cfg_file.write_text('model = ' + repr(_model_cfg()) + '\n' +
                        "optimizer = dict(type='AdamW', lr=1e-4, weight_decay=0.05)\n" +
                        'data = dict(samples_per_gpu=2, train=dict(pipeline=' + repr(PIPELINE) + '))\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg_file), '--synthetic-u8', '48x64', '--max-iters', '2',
                        '--log-interval', '1', '--work-dir', str(tmp_path / 'work')], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith('{')]
    assert [x['iter'] for x in recs] == [1, 2]
    for x in recs:
        assert np.isfinite(x['loss']) and x['loss'] > 0 and all(np.isfinite(v) for k, v in x.items() if 'loss' in k)


def test_driver_replaces_samples_without_a_surviving_instance(dev):
    drv = _driver()
    spec = _spec((32, 48), (32, 48))
    empty = lambda seed: _raw(37, 53, 0, seed)                     # noqa: E731
    stream = [empty(1), _raw(48, 64, 4, 2), _raw(37, 53, 5, 3), _raw(5, 7, 3, 4), _raw(48, 64, 3, 5)]
    got = list(drv.raw_batches(iter(stream), 2, tp.TrainPrep(spec, dev), np.random.default_rng(9), 'the test stream'))
    assert len(got) == 2
    # the draws, in the driver's order: the batch's samples, then the replacement's; then the second batch
    rng = np.random.default_rng(9)
    p0, p1 = (tp.draw_train_params(rng, s['img'].shape[:2], spec) for s in stream[:2])
    p2 = tp.draw_train_params(rng, stream[2]['img'].shape[:2], spec)
    want, kept = tp.prepare_train_host([stream[2], stream[1]], [p2, p1], spec)
    assert min(kept) >= 1
    _assert_equal(got[0], kept, want, kept, dev)
    p3, p4 = (tp.draw_train_params(rng, s['img'].shape[:2], spec) for s in stream[3:])
    want, kept = tp.prepare_train_host(stream[3:], [p3, p4], spec)
    _assert_equal(got[1], kept, want, kept, dev)
    # 8 x B replacements within one batch, then the stream is named
    with pytest.raises(CggError, match='16 samples of the test stream'):
        list(drv.raw_batches((empty(k) for k in range(100)), 2, tp.TrainPrep(spec, dev), np.random.default_rng(1), 'the test stream'))
