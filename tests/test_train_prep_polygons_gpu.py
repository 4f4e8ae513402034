"""The polygon route of csrc/train_prep.hip against rule 6 of train_prep.py, bit for bit: the fill kernel alone
(`ops.polygon_fill_bits`) against `polygon_mask_host` on the seeded cases of tests/poly_cases.py and at the kernel's geometry edges;
`TrainPrep.prep` on polygon samples against the same `TrainPrep` on the bitmaps rule 6 makes of them; the C ABI's error codes; the
driver.

The fill kernel runs one workgroup of 256 threads per instance: a toggle plane of h * w bits (LDS up to ops.POLY_LDS_BITS, else the
workspace), one 32-bit word per thread and scan block, so a block is ops.POLY_SCAN_BITS = 8192 pixels:
  h * w = 31, 32, 33, 63, 64, 65     the last word partly used, exactly used, one bit into the next
  8192, 8193, 8224                   exactly one scan block; one bit and one word more: the carry crosses a block
  601 x 655                          the toggle plane leaves LDS (393655 > 393216 bits); every case again with the route forced
Workspaces and outputs are pre-filled with 0xFF: the kernels clear what they read."""
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

import poly_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fill(dev, images, force=False):
    """every instance's (h, w) uint8 mask from the fill kernel alone, the workspace dirty"""
    buf, it, nt, pt = (torch.from_numpy(a) for a in pc.layout(images))
    N = nt.shape[0]
    nbytes = ops.train_prep_polygons_workspace_bytes(it, N, force_workspace=force)
    ws = torch.full((nbytes // 4 + 3,), -1, dtype=torch.int32, device=dev)
    _, pw = ops.polygon_fill_bits(buf.to(dev), it, nt, pt, buf, ws, force_workspace=force)
    assert nbytes == 4 * N * pw * (2 if force or any(h * w > ops.POLY_LDS_BITS and insts for h, w, insts in images) else 1)
    assert (ws[nbytes // 4:] == -1).all(), 'the kernel wrote past the workspace it asked for'
    out, i = [], 0
    for h, w, insts in images:
        for _ in insts:
            out.append(ops.polygon_bits_to_mask(ws, pw, i, h, w).cpu().numpy())
            i += 1
    return out


def _check(dev, images, force=False):
    got = _fill(dev, images, force)
    i = 0
    for b, (h, w, insts) in enumerate(images):
        for parts in insts:
            want = tp.polygon_mask_host(parts, h, w)
            assert got[i].shape == (h, w) and np.array_equal(got[i], want), (b, h, w, parts, int((got[i] != want).sum()))
            i += 1
    return got


@pytest.mark.parametrize('force', [False, True], ids=['lds', 'workspace'])
def test_fill_equals_the_host_rule_on_the_case_list(dev, force):
    """every case an image of its own with one instance: one launch, planes of five sizes side by side in one workspace"""
    got = _check(dev, [(h, w, [parts]) for _, parts, h, w in pc.CASES], force)
    assert sum(int(g.any()) for g in got) >= len(got) // 3


def _spanning(h, w, seed, k=9):
    """a star-shaped part that reaches over the whole plane, so set runs cross every word and scan-block boundary"""
    r = np.random.default_rng(seed)
    ang = np.sort(r.uniform(0, 2 * np.pi, size=k))
    return np.stack([w / 2 + (w / 2 + 2) * np.cos(ang), h / 2 + (h / 2 + 2) * np.sin(ang)], axis=1).reshape(-1).tolist()


EDGE_PLANES = [(1, 31), (4, 8), (3, 11), (7, 9), (8, 8), (5, 13), (64, 128), (1, 8193), (8193, 1), (32, 257), (257, 32)]


@pytest.mark.parametrize('force', [False, True], ids=['lds', 'workspace'])
def test_word_and_scan_block_edges(dev, force):
    assert [h * w for h, w in EDGE_PLANES[:6]] == [31, 32, 33, 63, 64, 65]
    S = ops.POLY_SCAN_BITS
    assert [h * w for h, w in EDGE_PLANES[6:]] == [S, S + 1, S + 1, S + 32, S + 32]
    images = []
    for j, (h, w) in enumerate(EDGE_PLANES):
        whole = [-1.0, -1.0, w + 1.0, -1.0, w + 1.0, h + 1.0, -1.0, h + 1.0]
        last = [w - 1.0, h - 1.0, float(w), h - 1.0, float(w), float(h), w - 1.0, float(h)]       # the plane's last pixel alone
        images.append((h, w, [[whole], [last], [_spanning(h, w, 10 + j)], [_spanning(h, w, 50 + j, 5), last]]))
    got = _check(dev, images, force)
    for j, (h, w) in enumerate(EDGE_PLANES):
        assert got[4 * j].all() and got[4 * j + 1].sum() == 1 and got[4 * j + 1][h - 1, w - 1] == 1


def test_toggle_plane_past_lds(dev):
    """the smallest route change: 393655 pixels do not fit the LDS toggle plane; next to it an image that does, in the same launch"""
    h, w = pc.OVER_LDS
    assert h * w > ops.POLY_LDS_BITS >= (h - 1) * w
    images = [(h, w, [[pc.circle(w / 2, h / 2, 250.0)], [_spanning(h, w, 3), pc.circle(100.0, 500.0, 80.5, 50)]]),
              (37, 45, [[_spanning(37, 45, 4)]])]
    got = _check(dev, images)
    assert got[0].sum() > 150000 and got[2].any()


def test_many_parts_a_circle_and_no_instance(dev):
    h, w = 48, 64
    r = np.random.default_rng(5)
    many = [pc._random_part(r, h, w, int(r.integers(3, 8)), bool(i % 2)) for i in range(64)]
    images = [(h, w, [many, [pc.circle(30.3, 22.7, 18.4)], []]), (20, 30, []), (6, 7, [[pc.RECT_A[0]], [pc.RECT_B[0]]])]
    got = _check(dev, images)
    assert len(got) == 5 and got[0].any() and not got[2].any()
    assert abs(int(got[1].sum()) - np.pi * 18.4 ** 2) < 60                          # a disc of radius 18.4
    for g, (_, (rows, cols)) in zip(got[3:], (pc.RECT_A, pc.RECT_B)):
        want = np.zeros((6, 7), dtype=np.uint8)
        want[rows, cols] = 1
        assert np.array_equal(g, want)
    # N = 0: nothing is launched, nothing is written
    assert _fill(dev, [(20, 30, [])]) == []


# ---- TrainPrep -----------------------------------------------------------------------------------------------------------------------
def _assert_same(got, kept, want, want_kept):
    assert kept == want_kept and set(got) == set(want)
    for k in want:
        if k == 'img_metas':
            for a, b in zip(got[k], want[k]):
                assert a.keys() == b.keys()
                for f in a:
                    if f == 'scale_factor':
                        assert np.array_equal(a[f], b[f])
                    elif f == 'img_norm_cfg':
                        assert np.array_equal(a[f]['mean'], b[f]['mean']) and np.array_equal(a[f]['std'], b[f]['std'])
                    else:
                        assert a[f] == b[f], f
            continue
        gs, ws = (got[k], want[k]) if isinstance(want[k], list) else ([got[k]], [want[k]])
        assert len(gs) == len(ws), k
        for i, (g, w) in enumerate(zip(gs, ws)):
            assert g.device.type == 'cuda' and g.dtype == w.dtype and g.shape == w.shape, (k, i)
            assert torch.equal(g, w), (k, i)


@pytest.mark.parametrize('flip', [False, True], ids=['noflip', 'flip'])
@pytest.mark.parametrize('scale_up', [False, True], ids=['down', 'up2'])
def test_prep_equals_prep_of_the_bitmaps(dev, flip, scale_up):
    samples, params, spec = pc.prep_batch(flip, scale_up)
    prep = tp.TrainPrep(spec, dev)
    want, want_kept = prep.prep([tp.polygons_to_bitmap_sample(s) for s in samples], params)
    bitmap_bytes = prep.last_staged_bytes
    got, kept = prep.prep(samples, params)
    _assert_same(got, kept, want, want_kept)
    assert prep.last_staged_bytes < bitmap_bytes and bitmap_bytes - prep.last_staged_bytes > 6 * 48 * 64
    assert kept[1] == 0 and kept[2] == 0 and 1 <= kept[0] < 5
    assert got['gt_masks'][1].shape == (0, 64, 64) and got['gt_masks'][0].shape == (kept[0], 64, 64)
    # and the host rule says the same
    host, host_kept = tp.prepare_train_host(samples, params, spec)
    assert host_kept == kept
    for b in range(3):
        assert np.array_equal(got['gt_masks'][b].cpu().numpy(), host['gt_masks'][b])
        assert np.array_equal(got['gt_bboxes'][b].cpu().numpy(), host['gt_bboxes'][b])
    # a second batch through the same object: the workspace is reused, dirty from the first
    got2, kept2 = prep.prep(samples[::-1], params[::-1])
    assert kept2 == kept[::-1] and torch.equal(got2['gt_masks'][2], got['gt_masks'][0])


def _abi_case():
    """two images with pixels, identity geometry into a 16 x 24 plane: (images, pixels, buf, tables)"""
    r = np.random.default_rng(11)
    images = [(12, 20, [[[2.0, 1.0, 15.5, 2.0, 14.0, 10.5, 3.0, 9.0]], [[0.0, 0.0, 5.0, 0.0, 5.0, 4.0], [10.0, 6.0, 19.0, 6.0, 19.0, 11.0]]]),
              (16, 9, [[[1.0, 1.0, 8.0, 2.0, 7.0, 15.0, 2.0, 14.0]]])]
    pixels = [r.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w, _ in images]
    return (images, pixels) + pc.layout(images, pixels)


def test_entry_into_dirty_outputs(dev):
    """the C ABI directly: masks, stats and the workspace filled with 0xFF beforehand; every byte is overwritten and equals the rule"""
    images, pixels, buf, it, nt, pt = _abi_case()
    it, nt, pt, bt = (torch.from_numpy(a) for a in (it, nt, pt, buf))
    N, H, W = 3, 16, 24
    spec = tp.TrainPrepSpec(img_scale=(64, 64), crop_size=(16, 24), size=(16, 24), mean=pc.MEAN, std=pc.STD, to_rgb=True)
    samples = [dict(img=px, gt_masks=np.stack([tp.polygon_mask_host(p, h, w) for p in insts]), gt_labels=np.zeros(len(insts), dtype=np.int64))
               for px, (h, w, insts) in zip(pixels, images)]
    params = [tp.TrainParams(False, (w, h), (0, 0)) for h, w, _ in images]
    assert [tp.resized_hw((h, w), p.scale) for (h, w, _), p in zip(images, params)] == [(12, 20), (16, 9)]
    want, kept = tp.prepare_train_host(samples, params, spec)
    assert kept == [2, 1]
    for force in (False, True):
        img = torch.full((2, 3, H, W), float('nan'), device=dev)
        masks = torch.full((N, H, W), 0xFF, dtype=torch.uint8, device=dev)
        stats = torch.full((N, 20), 0xFF, dtype=torch.uint8, device=dev).view(torch.int32)
        ws = torch.full((ops.train_prep_polygons_workspace_bytes(it, N, force_workspace=force) // 4,), -1, dtype=torch.int32, device=dev)
        ops.train_prep_polygons_u8(bt.to(dev), it, nt, pt, bt, img, masks, stats, ws, pc.MEAN, pc.STD, 0.0, to_rgb=True,
                                   force_workspace=force)
        assert torch.equal(img.cpu(), torch.from_numpy(want['img']))
        m = masks.cpu().numpy()
        assert m.max() == 1 and np.array_equal(m[:2], want['gt_masks'][0]) and np.array_equal(m[2:], want['gt_masks'][1])
        assert np.array_equal(tp.stats_to_boxes(stats.cpu().numpy()), np.concatenate(want['gt_bboxes']))


def test_error_codes_without_a_launch():
    """every refusal is decided on the host, before anything is launched: the buffers here are HOST memory"""
    lib = _lib.load()
    images, pixels, buf, it, nt, pt = _abi_case()
    it, nt, pt = (torch.from_numpy(a) for a in (it, nt, pt))
    staged = np.zeros(buf.size + 64, dtype=np.uint8)
    staged[:buf.size] = buf
    outs = np.full(1 << 16, 0xAB, dtype=np.uint8)
    f3 = ctypes.c_float * 3
    need = ops.train_prep_polygons_workspace_bytes(it, 3)
    assert need == 3 * ((12 * 20 + 31) // 32) * 4
    base = dict(staged=staged.ctypes.data, staged_bytes=buf.size, io=0, no=96, po=96 + 36, it=it, nt=nt, pt=pt, host=staged.ctypes.data,
                B=2, N=3, P=4, mean=f3(*pc.MEAN), std=f3(*pc.STD), pad=f3(0, 0, 0), ch=16, cw=24, img=outs.ctypes.data,
                masks=outs.ctypes.data + 16384, stats=outs.ctypes.data + 32768, H=16, W=24, ws=outs.ctypes.data + 49152, ws_bytes=need,
                force=0)
    assert base['staged'] % 16 == 0 and base['img'] % 16 == 0
    vp = ctypes.c_void_p
    ptr = lambda t: vp(t.data_ptr()) if t is not None else None                                          # noqa: E731

    def prep(**kw):
        a = dict(base, **kw)
        return lib.cgg_train_prep_polygons_u8(vp(a['staged']), a['staged_bytes'], a['io'], a['no'], a['po'], ptr(a['it']), ptr(a['nt']),
                                              ptr(a['pt']), vp(a['host']), a['B'], a['N'], a['P'], a['mean'], a['std'], a['pad'], 1,
                                              a['ch'], a['cw'], vp(a['img']), vp(a['masks']), vp(a['stats']), a['H'], a['W'],
                                              vp(a['ws']), a['ws_bytes'], a['force'], None)

    def fill(**kw):
        a = dict(base, **kw)
        return lib.cgg_polygon_fill_bits(vp(a['staged']), a['staged_bytes'], a['io'], a['no'], a['po'], ptr(a['it']), ptr(a['nt']),
                                         ptr(a['pt']), vp(a['host']), a['B'], a['N'], a['P'], vp(a['ws']), a['ws_bytes'], a['force'], None)

    def edited(table, row, col, val):
        t = table.clone()
        t[row, col] = val
        return t

    def with_coord(part, c, val):
        """a host copy of the staged bytes whose part `part` holds `val` at coordinate c"""
        s = staged.copy()
        s[int(pt[part, 0]) + 8 * c:int(pt[part, 0]) + 8 * c + 8] = np.array([val], dtype=np.float64).view(np.uint8)
        return s

    keep = []                                                    # the edited host copies stay alive while their address is in use

    def host(part, c, val):
        keep.append(with_coord(part, c, val))
        return keep[-1].ctypes.data

    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    bound = float(ops.TRAIN_PREP_MAX_COORD)
    cases = [
        (EINVAL, dict(pt=edited(pt, 1, 0, int(pt[1, 0]) + 4))),                          # coordinates off an 8-byte boundary
        (EINVAL, dict(pt=edited(pt, 3, 0, (buf.size - 40) & ~7))),                       # a part past staged_bytes
        (EINVAL, dict(pt=edited(pt, 3, 1, 5))),                                          # ... by its vertex count (4 -> 5)
        (EINVAL, dict(pt=edited(pt, 2, 1, 0))), (EINVAL, dict(pt=edited(pt, 2, 1, -3))),  # a vertex count below 1
        (EINVAL, dict(pt=edited(pt, 0, 0, -8))),
        (EINVAL, dict(host=host(0, 3, float('nan')))), (EINVAL, dict(host=host(3, 0, float('inf')))),
        (EINVAL, dict(host=host(2, 5, float('-inf')))),
        (EUNSUPPORTED, dict(host=host(1, 2, bound + 1.0))), (EUNSUPPORTED, dict(host=host(3, 5, -bound - 0.5))),
        (EUNSUPPORTED, dict(ws_bytes=need - 1)), (EUNSUPPORTED, dict(ws_bytes=need, force=1)), (EUNSUPPORTED, dict(ws_bytes=0)),
        (EINVAL, dict(staged=None)), (EINVAL, dict(it=None)), (EINVAL, dict(nt=None)), (EINVAL, dict(pt=None)), (EINVAL, dict(host=None)),
        (EINVAL, dict(ws=None)),
        (EINVAL, dict(nt=edited(nt, 1, 0, 1))),                                          # an instance in another image's range
        (EINVAL, dict(nt=edited(nt, 1, 1, 2))), (EINVAL, dict(nt=edited(nt, 1, 2, 1))),  # part ranges that do not tile 0 .. P
        (EINVAL, dict(nt=edited(nt, 2, 2, -1))), (EINVAL, dict(P=3)), (EINVAL, dict(P=5)), (EINVAL, dict(N=2)),
        (EINVAL, dict(no=98)), (EINVAL, dict(po=buf.size - 8)),                          # a table off a 4-byte boundary, past the bytes
        (EINVAL, dict(it=edited(it, 0, 1, 0))), (EUNSUPPORTED, dict(it=edited(it, 0, 1, 65536))),
        (EALIGN, dict(staged=base['staged'] + 4)), (EALIGN, dict(ws=base['ws'] + 2)),
    ]
    for i, (code, kw) in enumerate(cases):
        for fn, name in ((prep, b'cgg_train_prep_polygons_u8'), (fill, b'cgg_polygon_fill_bits')):
            rc = fn(**kw)
            assert rc == code, (i, name, sorted(kw), rc, lib.cgg_last_error_string())
            assert name in lib.cgg_last_error_string(), (i, lib.cgg_last_error_string())
    # the coordinate bound itself passes the coordinate test: the next refusal is the short workspace
    assert fill(host=host(1, 2, bound), ws_bytes=0) == EUNSUPPORTED and b'workspace' in lib.cgg_last_error_string()
    for code, kw in ((EINVAL, dict(img=None)), (EINVAL, dict(masks=None)), (EINVAL, dict(ch=17)), (EALIGN, dict(img=base['img'] + 4)),
                     (EINVAL, dict(it=edited(it, 0, 11, 0)))):
        assert prep(**kw) == code, (sorted(kw), lib.cgg_last_error_string())
    assert (outs == 0xAB).all(), 'a refused call wrote to its outputs'


def test_wrapper_refusals(dev):
    images, pixels, buf, it, nt, pt = _abi_case()
    it, nt, pt, bt = (torch.from_numpy(a) for a in (it, nt, pt, buf))
    ws = torch.empty((1024,), dtype=torch.int32, device=dev)
    with pytest.raises(CggError, match='different devices|ROCm device'):
        ops.polygon_fill_bits(bt, it, nt, pt, bt, ws)
    with pytest.raises(CggError, match='HOST'):
        ops.polygon_fill_bits(bt.to(dev), it, nt.to(dev), pt, bt, ws)
    with pytest.raises(CggError, match='staged_host'):
        ops.polygon_fill_bits(bt.to(dev), it, nt, pt, bt.to(dev), ws)
    with pytest.raises(CggError, match='workspace'):
        ops.polygon_fill_bits(bt.to(dev), it, nt, pt, bt, ws.cpu())
    with pytest.raises(CggError, match='workspace holds'):
        ops.polygon_fill_bits(bt.to(dev), it, nt, pt, bt, ws[:4])
    with pytest.raises(CggError, match='ROCm device'):
        tp.TrainPrep(pc.spec_for((64, 64), (64, 64)), 'cpu')


# ---- the driver --------------------------------------------------------------------------------------------------------------------
PIPELINE = [dict(type='LoadImageFromFile', to_float32=True),
            dict(type='LoadOpenAnnotations', with_bbox=True, with_mask=True, with_caption=True, poly2mask=True),
            dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Resize', img_scale=(128, 128), ratio_range=(0.1, 2.0), multiscale_mode='range', keep_ratio=True),
            dict(type='RandomCrop', crop_size=(128, 128), crop_type='absolute', recompute_bbox=True, allow_negative_crop=True),
            dict(type='FilterAnnotations', min_gt_bbox_wh=(1e-5, 1e-5), by_mask=True),
            dict(type='Pad', size=(128, 128), pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
            dict(type='Normalize', mean=list(pc.MEAN), std=list(pc.STD), to_rgb=True),
            dict(type='OpenFormatBundle', img_to_float=True),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_caption_ids', 'gt_caption_mask',
                                       'gt_caption_nouns_ids', 'gt_caption_nouns_mask'])]


def test_train_driver_on_synthetic_polygon_samples(tmp_path):
    """tools/train.py CONFIG --synthetic-polygons 48x64 --max-iters 2 in a fresh child process: two steps, finite losses in the log"""
    model = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                   vocab=500, num_points=256)
    cfg_file = tmp_path / 'tiny_polygon_train.py'
    cfg_file.write_text('model = ' + repr(model) + '\n' +
                        "optimizer = dict(type='AdamW', lr=1e-4, weight_decay=0.05)\n" +
                        'data = dict(samples_per_gpu=2, train=dict(pipeline=' + repr(PIPELINE) + '))\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg_file), '--synthetic-polygons', '48x64',
                        '--max-iters', '2', '--log-interval', '1', '--work-dir', str(tmp_path / 'work')], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith('{')]
    assert [x['iter'] for x in recs] == [1, 2]
    for x in recs:
        assert np.isfinite(x['loss']) and x['loss'] > 0 and all(np.isfinite(v) for k, v in x.items() if 'loss' in k)
