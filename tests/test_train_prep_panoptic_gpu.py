"""cgg_train_prep_panoptic_u8 (csrc/train_prep.hip) against the rule of train_prep.py: every output of `TrainPrep.prep` on raw
panoptic samples EQUALS `prepare_train_host`'s (torch.equal on image, masks, semantic maps, boxes, labels; the kept counts and the
metas), which is by definition the rule on the bitmaps `load_panoptic_host` makes; the C ABI's layout and error codes; the driver.

The kernel works on 16 x 256 tiles with 4 columns per lane (tests/panoptic_cases.py holds the batches, shared with the host test):
  (40, 520): W % 4 == 0, the packed dword stores; 3 tiles each way, so a thing's statistics are reduced from several tiles' atomics.
             Sources 37 x 53 upsampled x 2, 120 x 700 flipped with a window at (138, 520), 64 x 48 flipped that pads the columns,
             30 x 40 shrunk to 6 x 8 (nearly all pad)
  (33, 50):  W % 4 == 2, the byte stores guarded by x < W; one tile
  both id-map forms (int32 dwords; RGB bytes at every byte phase), a sample with zero things, one whose things all lie outside
  the window (kept == 0), one image with 256 records and 200 things (the table's ends and misses of the binary search)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, synthetic, train_prep as tp
from cgg_amd._lib import CggError

import panoptic_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_equal(got, kept, want, want_kept):
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


def _things_on_top(h, w, seed, rgb):
    """three things in the top two source rows, stuff and an unlisted id below: a window at the far margin sees none of them"""
    s = pc.pan_sample(h, w, seed, rgb)
    pan = np.empty((h, w), dtype=np.int32)
    pan[:2, :w // 3], pan[:2, w // 3:2 * w // 3], pan[:2, 2 * w // 3:] = 11, 2**23 + 5, 300
    pan[2:h // 2], pan[h // 2:] = 70000, 9
    s['segments'] = [dict(id=300, category=3, is_thing=True), dict(id=70000, category=90, is_thing=False),
                     dict(id=11, category=1, is_thing=True), dict(id=2**23 + 5, category=2, is_thing=True)]
    s['gt_labels'] = np.array([3, 1, 2], dtype=np.int64)
    s['pan_seg'] = np.stack([pan & 255, (pan >> 8) & 255, (pan >> 16) & 255], axis=2).astype(np.uint8) if rgb else pan
    return s


def _full_batch(case, rgb, seg=True):
    """the shared batch, then a sample with zero things and one whose things all fall outside the window"""
    samples, params, spec = pc.batch(case, rgb, seg)
    form = (lambda i: bool(i % 2)) if rgb == 'mixed' else (lambda i: bool(rgb))
    samples.append(pc.pan_sample(16, 20, 91, form(0), records=5, things=0))
    params.append(pc.far_margin((16, 20), (40, 40), True, spec))
    samples.append(_things_on_top(37, 53, 92, form(1)))
    params.append(pc.far_margin((37, 53), (106, 80), False, spec))
    return samples, params, spec


@pytest.fixture(scope='module')
def host_results():
    """the host rule of every batch here, computed once"""
    out = {}
    for name, case in (('wide', pc.WIDE), ('odd', pc.ODD)):
        for rgb in (False, True, 'mixed'):
            samples, params, spec = _full_batch(case, rgb)
            out[name, rgb] = (samples, params, spec) + tp.prepare_train_host(samples, params, spec)
    return out


@pytest.mark.parametrize('rgb', [False, True, 'mixed'], ids=['int32', 'rgb', 'mixed'])
@pytest.mark.parametrize('name', ['wide', 'odd'])
def test_prep_equals_the_host_rule(dev, host_results, name, rgb):
    samples, params, spec, want, want_kept = host_results[name, rgb]
    got, kept = tp.TrainPrep(spec, dev).prep(samples, params)
    _assert_equal(got, kept, want, want_kept)
    H, W = spec.size
    n = len(samples)
    assert got['gt_semantic_seg'].shape == (n, 1, H, W)
    assert kept[-2] == 0 and kept[-1] == 0 and got['gt_masks'][-2].shape == (0, H, W) and got['gt_masks'][-1].shape == (0, H, W)
    assert len(samples[-1]['gt_labels']) == 3 and len(samples[-2]['gt_labels']) == 0
    assert any(0 < k < 7 for k in kept[:-2]) and max(kept) >= 2


def test_without_a_semantic_plane(dev):
    samples, params, spec = _full_batch(pc.ODD, 'mixed', seg=False)
    want, want_kept = tp.prepare_train_host(samples, params, spec)
    got, kept = tp.TrainPrep(spec, dev).prep(samples, params)
    assert 'gt_semantic_seg' not in got
    _assert_equal(got, kept, want, want_kept)


def _dense_sample(rgb):
    """64 x 48, 16 x 24 blocks of 4 x 2 pixels with ids 10, 20, ..: 256 of them listed (every third id is not, so misses lie BETWEEN
    table entries; the first and the last block's ids are listed, two more blocks carry ids below and above every entry)"""
    h, w = 64, 48
    ids = 10 * (1 + np.arange(16 * 24, dtype=np.int64)) + 2**22
    ids[5], ids[7] = 3, 2**24 - 1                                 # below the smallest and above the largest listed id
    listed = sorted([k for k in range(ids.size) if k % 3 != 1 and k != 5] + [1])
    assert listed[0] == 0 and listed[-1] == ids.size - 1 and 7 not in listed
    assert len(listed) == 256
    r = np.random.default_rng(17)
    place = r.permutation(ids.size)                               # which block of the map carries which id
    pan = np.empty((h, w), dtype=np.int32)
    for k in range(ids.size):
        i, j = divmod(int(place[k]), 24)
        pan[4 * i:4 * i + 4, 2 * j:2 * j + 2] = ids[k]
    order = r.permutation(256).tolist()
    segments = [dict(id=int(ids[listed[k]]), category=int(r.integers(0, 80)) if k < 200 else int(80 + r.integers(0, 53)), is_thing=k < 200)
                for k in order]
    labels = np.array([s['category'] for s in segments if s['is_thing']], dtype=np.int64)
    if rgb:
        pan = np.stack([pan & 255, (pan >> 8) & 255, (pan >> 16) & 255], axis=2).astype(np.uint8)
    lo, hi = min(s['id'] for s in segments), max(s['id'] for s in segments)
    assert lo == ids[0] and hi == ids[-1] and ids[5] < lo and ids[7] > hi
    return dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), pan_seg=pan, segments=segments, gt_labels=labels, filename='dense.jpg')


@pytest.mark.parametrize('rgb', [False, True], ids=['int32', 'rgb'])
def test_256_records_and_200_things(dev, rgb):
    s = _dense_sample(rgb)
    spec = pc.spec_for((64, 48))
    params = [tp.TrainParams(True, (48, 64), (0, 0))]
    assert tp.resized_hw((64, 48), (48, 64)) == (64, 48)
    want, want_kept = tp.prepare_train_host([s], params, spec)
    got, kept = tp.TrainPrep(spec, dev).prep([s], params)
    _assert_equal(got, kept, want, want_kept)
    assert kept == [200] and (want['gt_semantic_seg'] == 255).sum() == 8 * (16 * 24 - 256)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _pitched_layout():
    """two samples (int32, then RGB): image rows of 3 w + 5 bytes from byte 1 on, map rows with a pitch beyond the pixels, the three
    tables LAST, segment table first"""
    a, b = pc.pan_sample(9, 11, 41, False, records=6, things=3, grid=(3, 3)), pc.pan_sample(6, 17, 42, True, records=5, things=2, grid=(2, 4))
    spec = tp.TrainPrepSpec(img_scale=(32, 32), crop_size=(16, 20), size=(16, 24), pad_val=((1.0, 2.0, 3.0), 0, 250), mean=pc.MEAN,
                            std=pc.STD, to_rgb=False, with_seg=True)
    params = [tp.TrainParams(False, (30, 30), (0, 0)), tp.TrainParams(True, (40, 40), (0, 20))]      # 25 x 30 and 14 x 40 resized
    buf = np.full(4096, 0xCC, dtype=np.uint8)
    n, img_rows, pan_rows, seg_rows, first, sfirst = 1, [], [], [], 0, 0
    for s, p in zip((a, b), params):
        h, w = s['img'].shape[:2]
        nh, nw, oy, ox, _, _ = tp.sample_geometry((h, w), p, spec)
        pitch = 3 * w + 5
        off = n
        buf[off:off + h * pitch].reshape(h, pitch)[:, :3 * w] = s['img'].reshape(h, 3 * w)
        n += h * pitch
        pan = s['pan_seg']
        if pan.ndim == 2:
            n = (n + 3) & ~3
            mp = 4 * w + 8
            buf[n:n + h * mp].reshape(h, mp)[:, :4 * w] = pan.view(np.uint8).reshape(h, 4 * w)
        else:
            mp = 3 * w + 2
            buf[n:n + h * mp].reshape(h, mp)[:, :3 * w] = pan.reshape(h, 3 * w)
        slot, rows = 0, []
        for r in s['segments']:
            slot += int(r['is_thing'])
            rows.append((r['id'], ((slot if r['is_thing'] else 0) << 8) | r['category']))
        seg_rows += sorted(rows)
        things = len(s['gt_labels'])
        pan_rows.append((n, mp, int(pan.ndim == 3), sfirst, len(rows)))
        n += h * mp
        img_rows.append((off, h, w, pitch, nh, nw, oy, ox, int(p.flip), first, things, -1))
        first += things
        sfirst += len(rows)
    seg_off = (n + 3) & ~3
    pan_off = seg_off + 8 * len(seg_rows)
    img_off = pan_off + 20 * 2
    end = img_off + 48 * 2
    tables = [torch.tensor(t, dtype=torch.int32) for t in (img_rows, pan_rows, seg_rows)]
    for off, t in zip((img_off, pan_off, seg_off), tables):
        buf[off:off + 4 * t.numel()].view(np.int32)[:] = t.numpy().reshape(-1)
    return (a, b), params, spec, buf[:end].copy(), tables, (img_off, pan_off, seg_off)


def test_entry_with_pitched_rows_into_dirty_outputs(dev):
    """the C-ABI layout in full, into outputs filled with 0xAB: every byte of masks, seg and stats is overwritten and equals the rule"""
    samples, params, spec, buf, (img_table, pan_table, seg_table), (img_off, pan_off, seg_off) = _pitched_layout()
    want, kept = tp.prepare_train_host(list(samples), params, spec)
    N = sum(len(s['gt_labels']) for s in samples)
    img = torch.full((2, 3, 16, 24), float('nan'), device=dev)
    masks = torch.full((N, 16, 24), 0xAB, dtype=torch.uint8, device=dev)
    seg = torch.full((2, 1, 16, 24), 0xAB, dtype=torch.uint8, device=dev)
    stats = torch.full((N, 20), 0xAB, dtype=torch.uint8, device=dev).view(torch.int32)
    assert stats.shape == (N, 5) and stats.is_contiguous()
    assert int(stats[0, 0]) == int(np.array([0xABABABAB], dtype=np.uint32).view(np.int32)[0]) and int(masks[0, 0, 0]) == 0xAB
    ops.train_prep_panoptic_u8(torch.from_numpy(buf).to(dev), img_table, pan_table, seg_table, img, masks, seg, stats, pc.MEAN, pc.STD,
                               (1.0, 2.0, 3.0), to_rgb=False, crop_size=(16, 20), seg_pad=250, img_table_offset=img_off,
                               pan_table_offset=pan_off, seg_table_offset=seg_off)
    assert torch.equal(img.cpu(), torch.from_numpy(want['img'])) and torch.equal(seg.cpu(), torch.from_numpy(want['gt_semantic_seg']))
    st, m = stats.cpu().numpy(), masks.cpu().numpy()
    assert m.max() <= 1
    # every plane, the dropped ones included, is the rule on the loader's bitmap of that thing
    bitmaps = pc.bitmap_samples(list(samples))
    first = 0
    for b, s in enumerate(samples):
        n = len(s['gt_labels'])
        eh, ew = want['img_metas'][b]['img_shape'][:2]
        for i in range(n):
            one = dict(bitmaps[b], gt_masks=bitmaps[b]['gt_masks'][i:i + 1], gt_labels=bitmaps[b]['gt_labels'][i:i + 1])
            w1, k1 = tp.prepare_train_host([one], [params[b]], spec)
            plane = w1['gt_masks'][0][0] if k1[0] else np.zeros((16, 24), dtype=np.uint8)
            assert np.array_equal(m[first + i], plane), (b, i)
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
    samples, _, _, buf, (img_table, pan_table, seg_table), (img_off, pan_off, seg_off) = _pitched_layout()
    N, S = sum(len(s['gt_labels']) for s in samples), seg_table.shape[0]
    staged = np.zeros(8192, dtype=np.uint8)
    staged[:buf.size] = buf
    outs = np.full(1 << 16, 0xAB, dtype=np.uint8)
    f3 = ctypes.c_float * 3
    base = dict(staged=staged.ctypes.data, staged_bytes=buf.size, img_off=img_off, pan_off=pan_off, seg_off=seg_off, it=img_table,
                pt=pan_table, st=seg_table, B=2, N=N, S=S, mean=f3(*pc.MEAN), std=f3(*pc.STD), pad=f3(0, 0, 0), to_rgb=1, seg_pad=255,
                ch=16, cw=20, img=outs.ctypes.data, masks=outs.ctypes.data + 16384, seg=outs.ctypes.data + 32768,
                stats=outs.ctypes.data + 49152, H=16, W=24)
    assert base['staged'] % 16 == 0 and base['img'] % 16 == 0

    def call(**kw):
        a = dict(base, **kw)
        vp = ctypes.c_void_p
        ptr = lambda t: vp(t.data_ptr()) if t is not None else None                                     # noqa: E731
        return lib.cgg_train_prep_panoptic_u8(vp(a['staged']), a['staged_bytes'], a['img_off'], a['pan_off'], a['seg_off'], ptr(a['it']),
                                              ptr(a['pt']), ptr(a['st']), a['B'], a['N'], a['S'], a['mean'], a['std'], a['pad'],
                                              a['to_rgb'], a['seg_pad'], a['ch'], a['cw'], vp(a['img']), vp(a['masks']), vp(a['seg']),
                                              vp(a['stats']), a['H'], a['W'], None)

    def edited(table, row, col, val):
        t = table.clone()
        t[row, col] = val
        return t

    def slot_of(row, slot):
        return (slot << 8) | (int(seg_table[row, 1]) & 255)

    s0 = int(pan_table[0, 4])                                    # image 0 owns segment rows 0 .. s0 - 1, sorted by id
    thing_rows = [i for i in range(s0) if int(seg_table[i, 1]) >> 8]
    other_rows = [i for i in range(s0) if not int(seg_table[i, 1]) >> 8]
    assert len(thing_rows) == 3 and len(other_rows) == 3 and int(pan_table[0, 2]) == 0 and int(pan_table[1, 2]) == 1
    many = torch.stack([torch.arange(257, dtype=torch.int32), torch.full((257,), 7, dtype=torch.int32)], dim=1).contiguous()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    cases = [
        (EINVAL, dict(staged=None)), (EINVAL, dict(it=None)), (EINVAL, dict(pt=None)), (EINVAL, dict(st=None)), (EINVAL, dict(img=None)),
        (EINVAL, dict(masks=None)), (EINVAL, dict(stats=None)), (EINVAL, dict(mean=None)),
        (EINVAL, dict(it=edited(img_table, 1, 0, buf.size - 10))),                       # an image past staged_bytes
        (EINVAL, dict(pt=edited(pan_table, 0, 0, (buf.size - 40) & ~3))),                # an int32 map past staged_bytes
        (EINVAL, dict(pt=edited(pan_table, 1, 0, buf.size - 10))),                       # an RGB map past staged_bytes
        (EINVAL, dict(pt=edited(pan_table, 0, 0, -4))),
        (EINVAL, dict(staged_bytes=img_off + 95)),                                       # the image table past staged_bytes
        (EINVAL, dict(pan_off=buf.size - 36)),                                           # the panoptic table past staged_bytes
        (EINVAL, dict(seg_off=buf.size - 8 * S + 4)),                                    # the segment table past staged_bytes
        (EINVAL, dict(pan_off=pan_off + 2)), (EINVAL, dict(seg_off=seg_off + 1)),        # table offsets that are no multiples of 4
        (EINVAL, dict(pt=edited(pan_table, 0, 0, int(pan_table[0, 0]) + 2))),            # an int32 map off a 4-byte boundary
        (EINVAL, dict(pt=edited(pan_table, 0, 1, 4 * 11 + 2))),                          # ... with a pitch that is no multiple of 4
        (EINVAL, dict(pt=edited(pan_table, 0, 1, 4 * 11 - 4))),                          # int32 pitch < 4 w
        (EINVAL, dict(pt=edited(pan_table, 1, 1, 3 * 17 - 1))),                          # RGB pitch < 3 w
        (EINVAL, dict(pt=edited(pan_table, 1, 2, 2))), (EINVAL, dict(pt=edited(pan_table, 0, 2, -1))),     # an unknown format
        (EINVAL, dict(st=edited(seg_table, 1, 0, int(seg_table[0, 0])))),                # ids equal
        (EINVAL, dict(st=edited(seg_table, 2, 0, int(seg_table[1, 0]) - 1))),            # ids descending
        (EINVAL, dict(st=edited(seg_table, thing_rows[0], 1, slot_of(thing_rows[0], int(seg_table[thing_rows[1], 1]) >> 8)))),  # a slot twice
        (EINVAL, dict(st=edited(seg_table, thing_rows[0], 1, slot_of(thing_rows[0], 4)))),                 # a slot beyond the thing count
        (EINVAL, dict(st=edited(seg_table, thing_rows[0], 1, slot_of(thing_rows[0], 0)))),                 # a slot missing
        (EINVAL, dict(st=edited(seg_table, other_rows[0], 1, -256))),                                       # a negative slot
        (EINVAL, dict(st=edited(seg_table, other_rows[0], 1, 255))),                     # category 255
        (EINVAL, dict(it=edited(img_table, 0, 11, 0))),                                  # a staged semantic map: the offset must be -1
        (EINVAL, dict(pt=edited(pan_table, 1, 3, s0 + 1))),                              # segment ranges that leave a gap
        (EINVAL, dict(S=S - 1)), (EINVAL, dict(S=-1)),
        (EINVAL, dict(N=N - 1)), (EINVAL, dict(it=edited(img_table, 1, 9, 2))),          # thing ranges that do not tile 0 .. N
        (EINVAL, dict(B=0)), (EINVAL, dict(ch=17)), (EINVAL, dict(std=f3(1.0, 0.0, 1.0))), (EINVAL, dict(staged_bytes=0)),
        (EUNSUPPORTED, dict(B=1, N=3, S=257, st=many, pt=edited(pan_table, 0, 4, 257), seg_off=0, staged_bytes=8192)),   # 257 rows
        (EUNSUPPORTED, dict(staged_bytes=2**31 - 8)), (EUNSUPPORTED, dict(H=65536)),
        (EALIGN, dict(staged=base['staged'] + 2)), (EALIGN, dict(img=base['img'] + 4)), (EALIGN, dict(masks=base['masks'] + 1)),
        (EALIGN, dict(seg=base['seg'] + 2)), (EALIGN, dict(stats=base['stats'] + 2)),
    ]
    for i, (code, kw) in enumerate(cases):
        rc = call(**kw)
        assert rc == code, (i, sorted(kw), rc, lib.cgg_last_error_string())
        assert b'cgg_train_prep_panoptic_u8' in lib.cgg_last_error_string(), (i, lib.cgg_last_error_string())
    assert (outs == 0xAB).all(), 'a refused call wrote to its outputs'


def test_wrapper_refuses_host_tensors_and_wrong_shapes(dev):
    samples, _, _, buf, (img_table, pan_table, seg_table), (img_off, pan_off, seg_off) = _pitched_layout()
    N = sum(len(s['gt_labels']) for s in samples)
    mk = lambda d: (torch.empty((2, 3, 16, 24), device=d), torch.empty((N, 16, 24), dtype=torch.uint8, device=d),       # noqa: E731
                    torch.empty((2, 1, 16, 24), dtype=torch.uint8, device=d), torch.empty((N, 5), dtype=torch.int32, device=d))
    staged = torch.from_numpy(buf)
    off = dict(img_table_offset=img_off, pan_table_offset=pan_off, seg_table_offset=seg_off)
    with pytest.raises(CggError, match='ROCm device'):
        ops.train_prep_panoptic_u8(staged, img_table, pan_table, seg_table, *mk('cpu'), pc.MEAN, pc.STD, **off)
    img, masks, seg, stats = mk(dev)
    with pytest.raises(CggError, match='stats'):
        ops.train_prep_panoptic_u8(staged.to(dev), img_table, pan_table, seg_table, img, masks[:-1], seg, stats, pc.MEAN, pc.STD, **off)
    with pytest.raises(CggError, match='HOST'):
        ops.train_prep_panoptic_u8(staged.to(dev), img_table, pan_table.to(dev), seg_table, img, masks, seg, stats, pc.MEAN, pc.STD, **off)
    with pytest.raises(CggError, match='pan_table'):
        ops.train_prep_panoptic_u8(staged.to(dev), img_table, pan_table[:1], seg_table, img, masks, seg, stats, pc.MEAN, pc.STD, **off)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
PIPELINE = [dict(type='LoadImageFromFile', to_float32=True),
            dict(type='LoadOpenPanopticAnnotations', with_bbox=True, with_mask=True, with_seg=True, with_caption=True),
            dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Resize', img_scale=(128, 128), ratio_range=(0.1, 2.0), multiscale_mode='range', keep_ratio=True),
            dict(type='RandomCrop', crop_size=(128, 128), crop_type='absolute', recompute_bbox=True, allow_negative_crop=True),
            dict(type='FilterAnnotations', min_gt_bbox_wh=(1e-5, 1e-5), by_mask=True),
            dict(type='Pad', size=(128, 128), pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
            dict(type='Normalize', mean=list(pc.MEAN), std=list(pc.STD), to_rgb=True),
            dict(type='OpenFormatBundle', img_to_float=True),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_semantic_seg', 'gt_caption_ids', 'gt_caption_mask',
                                       'gt_caption_nouns_ids', 'gt_caption_nouns_mask'])]


def test_train_driver_on_synthetic_panoptic_samples(tmp_path):
    """tools/train.py CONFIG --synthetic-panoptic 48x64 --max-iters 2 in a fresh child process, a panoptic pipeline in the config and
    a head with stuff classes: two steps, finite losses in the log"""
    model = synthetic.model_config(num_things=10, num_stuff=4, num_unknown=3, num_queries=20, depth=50, panoptic=True, enc_layers=2,
                                   dec_layers=3, vocab=500, num_points=256)
    cfg_file = tmp_path / 'tiny_panoptic_train.py'
    cfg_file.write_text('model = ' + repr(model) + '\n' +
                        "optimizer = dict(type='AdamW', lr=1e-4, weight_decay=0.05)\n" +
                        'data = dict(samples_per_gpu=2, train=dict(pipeline=' + repr(PIPELINE) + '))\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg_file), '--synthetic-panoptic', '48x64',
                        '--max-iters', '2', '--log-interval', '1', '--work-dir', str(tmp_path / 'work')], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith('{')]
    assert [x['iter'] for x in recs] == [1, 2]
    for x in recs:
        assert np.isfinite(x['loss']) and x['loss'] > 0 and all(np.isfinite(v) for k, v in x.items() if 'loss' in k)
