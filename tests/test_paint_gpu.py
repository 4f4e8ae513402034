"""GPU tests of csrc/paint.hip: the three kernels must EQUAL the numpy rules of paint.py (torch.equal; the arithmetic is integer or
correctly rounded float64, so there is no tolerance), on the shared cases of paint_cases.py; then `show_result` end to end on the
three result forms, and tools/test.py --show-dir."""
import os
import warnings

import numpy as np
import pytest
import torch

import cgg_amd
from cgg_amd import ops, paint, synthetic
from cgg_amd.config import Config

import paint_cases as pc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)             # (a copy: the cases' arrays are shared and may be reversed views)


# ---- instances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('at', pc.ALPHA_THICKNESS)
@pytest.mark.parametrize('n', pc.INSTANCE_COUNTS)
@pytest.mark.parametrize('size', pc.INSTANCE_SIZES)
def test_paint_instances_equals_the_host_rule(dev, size, n, at):
    c = pc.instance_case(size, n, at)
    img, bits, keep, colors = _t(c['img'], dev), _t(c['bits'], dev), _t(c['keep'], dev), _t(c['colors'], dev)
    boxes, box_colors = _t(paint.truncate_boxes(c['boxes']), dev), _t(c['box_colors'], dev)
    flat = torch.full((c['img'].size + 128,), 0xA5, dtype=torch.uint8, device=dev)
    out = flat[64:64 + c['img'].size].view(c['img'].shape)
    got = ops.paint_instances(img, bits, keep, colors, boxes, box_colors, alpha=c['alpha'], thickness=c['thickness'], out=out)
    assert got is out and torch.equal(got.cpu(), torch.from_numpy(c['want']))
    assert bool((flat[:64] == 0xA5).all()) and bool((flat[-64:] == 0xA5).all()), 'wrote outside the image'
    assert torch.equal(img.cpu(), torch.from_numpy(c['img']))                                  # the input is left alone
    fill = ops.paint_instances(img, bits, keep, colors, alpha=c['alpha'], edges=False)
    assert torch.equal(fill.cpu(), torch.from_numpy(c['want_fill_only']))
    # bool planes on the device go through the pack kernel (pad bits zero there) and give the same image, also in place
    packed = ops.pack_bool_masks(_t(c['masks'], dev))
    assert torch.equal(packed.cpu(), torch.from_numpy(pc.pack(c['masks'], (size[1] + 7) // 8)))
    same = ops.paint_instances(img, packed, keep, colors, boxes, box_colors, alpha=c['alpha'], thickness=c['thickness'], out=img)
    assert same is img and torch.equal(img.cpu(), torch.from_numpy(c['want']))


@pytest.mark.parametrize('alpha', [0.8, 0.5, 1.0])
def test_every_value_colour_pair_of_the_blend(dev, alpha):
    c = pc.all_pairs_case(alpha)
    got = ops.paint_instances(_t(c['img'], dev), _t(c['bits'], dev), torch.ones(256, dtype=torch.uint8, device=dev), _t(c['colors'], dev),
                              alpha=alpha, edges=False)
    assert torch.equal(got.cpu(), torch.from_numpy(c['want']))


def test_paint_instances_reads_strided_planes(dev):
    """planes further apart than H * row_bytes, as a slice of a larger buffer has them"""
    c = pc.instance_case((19, 37), 3, (0.8, 2))
    base = torch.full((3, 25, 5), 0xFF, dtype=torch.uint8, device=dev)
    base[:, :19] = _t(c['bits'], dev)
    bits = base[:, :19]
    assert not bits.is_contiguous() and ops.paint_instances_ok(_t(c['img'], dev), bits)
    got = ops.paint_instances(_t(c['img'], dev), bits, _t(c['keep'], dev), _t(c['colors'], dev),
                              _t(paint.truncate_boxes(c['boxes']), dev), _t(c['box_colors'], dev), alpha=0.8, thickness=2)
    assert torch.equal(got.cpu(), torch.from_numpy(c['want']))
    assert not ops.paint_instances_ok(_t(c['img'], dev), torch.zeros(1025, 19, 5, dtype=torch.uint8, device=dev))      # n > 1024
    assert not ops.paint_instances_ok(_t(c['img'], dev), base.transpose(1, 2)[:, :19, :5])                                # rows not contiguous


# ---- components ------------------------------------------------------------------------------------------------------------------
def _records(rec, status):
    status = status.cpu().tolist()
    rec = rec.cpu().numpy()[:min(status[0], rec.shape[0])]
    return rec[np.argsort(rec[:, 0])], status


@pytest.mark.parametrize('kind', pc.COMPONENT_KINDS)
@pytest.mark.parametrize('size', pc.COMPONENT_SIZES)
def test_label_components_equals_the_host_rule(dev, size, kind):
    c = pc.component_case(size, kind)
    rec, status = _records(*ops.label_components(_t(c['pan'], dev), pc.VOID, capacity=4096))
    assert status == [len(c['records']), 0]
    assert rec.dtype == np.int64 and np.array_equal(rec, c['records'])


def test_label_components_overflow_and_fallback(dev):
    c = pc.component_case((65, 129), 'blobs')
    assert len(c['records']) > 4
    rec, status = ops.label_components(_t(c['pan'], dev), pc.VOID, capacity=4)
    rec, status = _records(rec, status)
    assert status == [len(c['records']), 0]                   # the count word is the true count: overflow is count > capacity
    assert rec.shape == (4, 5)
    want = {tuple(r) for r in c['records'].tolist()}
    assert len({tuple(r) for r in rec.tolist()}) == 4 and all(tuple(r) in want for r in rec.tolist())      # any 4 of them, each whole
    # the caller falls back to the host rule: same image as with room for every record, and as the host rule alone
    from types import SimpleNamespace
    p = pc.panoptic_case((65, 129), 'all_but_void')
    model = SimpleNamespace(parameters=lambda: iter(()), num_classes=pc.VOID)
    result = dict(panoptic_all_results=_t(p['pan'], dev))
    small = paint.show_panoptic(model, p['img'], result, show_labels=False, capacity=4)
    roomy = paint.show_panoptic(model, p['img'], result, show_labels=False)
    ids = p['ids']
    colors = paint.instance_colors_host(ids % 1000, paint.get_palette(None, int((ids % 1000).max()) + 1))
    want = paint.paint_panoptic_host(p['img'], p['pan'], ids, colors, pc.VOID)
    assert np.array_equal(small, want) and np.array_equal(roomy, want)


def test_ids_beyond_int32_take_the_host_route(dev):
    """an int64 map with an id the kernels' int32 cannot hold: it must not be truncated and painted under another id"""
    from types import SimpleNamespace
    p = pc.panoptic_case((65, 129), 'all_but_void')
    pan = p['pan'].astype(np.int64)
    pan[pan == 1001] = 2**32 + 1001                           # truncates to 1001
    pan[:8, :8] = 1001                                        # and a real 1001 beside it
    model = SimpleNamespace(parameters=lambda: iter(()), num_classes=pc.VOID)
    ids = np.unique(pan)[::-1]
    ids = ids[ids != pc.VOID]
    colors = paint.instance_colors_host(ids % 1000, paint.get_palette(None, int((ids % 1000).max()) + 1))
    want = paint.paint_panoptic_host(p['img'], pan, ids, colors, pc.VOID)
    for form in (pan, _t(pan, dev)):
        got = paint.show_panoptic(model, _t(p['img'], dev), dict(panoptic_all_results=form), show_labels=False)
        assert np.array_equal(got, want)


def test_label_components_reports_negative_ids(dev):
    pan = pc.id_map('blobs', 7, 300).copy()
    pan[3, 100] = -5
    _, status = ops.label_components(_t(pan, dev), pc.VOID)
    assert status.cpu().tolist()[1] == 2


# ---- panoptic paint --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', pc.PANOPTIC_TABLES)
@pytest.mark.parametrize('size', pc.COMPONENT_SIZES)
def test_paint_panoptic_equals_the_host_rule(dev, size, table):
    c = pc.panoptic_case(size, table)
    asc = np.ascontiguousarray(c['ids'][::-1])
    flat = torch.full((c['img'].size + 128,), 0xA5, dtype=torch.uint8, device=dev)
    out = flat[64:64 + c['img'].size].view(c['img'].shape)
    got = ops.paint_panoptic(_t(c['img'], dev), _t(c['pan'], dev), _t(asc, dev), _t(c['colors'][::-1], dev), out=out)
    assert torch.equal(got.cpu(), torch.from_numpy(c['want']))
    assert bool((flat[:64] == 0xA5).all()) and bool((flat[-64:] == 0xA5).all()), 'wrote outside the image'
    void_px = torch.from_numpy(c['pan'] == pc.VOID)
    assert torch.equal(got.cpu()[void_px], torch.from_numpy(c['img'])[void_px])                 # void untouched
    none = ops.paint_panoptic(_t(c['img'], dev), _t(c['pan'], dev), torch.zeros(0, dtype=torch.int32, device=dev),
                              torch.zeros(0, 3, dtype=torch.uint8, device=dev))
    assert torch.equal(none.cpu(), torch.from_numpy(c['img']))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
PIPELINE = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(96, 64), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Pad', size_divisor=32, pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
                             dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


def _model(dev, panoptic):
    from util import randomize
    kw = dict(num_things=10, num_stuff=4 if panoptic else 0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
              vocab=500, num_points=256, panoptic=panoptic)
    mc = synthetic.model_config(**kw)
    if panoptic:
        mc['test_cfg'].update(object_mask_thr=0.05, iou_thr=0.05, stuff_area_limit=16)      # random weights: let segments through
    cfg = Config(dict(model=mc, data=dict(test=dict(pipeline=PIPELINE))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = cgg_amd.init_detector(cfg, None, device=dev)
    randomize(m, seed=9)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.fill_(1.0)
            mod.running_mean.zero_()
    m.panoptic_fusion_head.test_cfg['max_per_image'] = 20     # k <= Q * n_classes for every type: the path that can bit-pack
    return m


def _image():
    x = synthetic.structured_images(1, 64, 96, seed=4, shapes=8)[0]
    return ((x - x.min()) / (x.max() - x.min()) * 255).round().byte().permute(1, 2, 0).contiguous().numpy()


def test_show_result_instances_end_to_end(dev, tmp_path):
    from PIL import Image
    model, img = _model(dev, panoptic=False), _image()
    assert model.show_result.__func__ is type(model).show_result
    host = cgg_amd.inference_detector(model, img)
    dres = cgg_amd.inference_detector(model, img, device_results=True)
    bres = cgg_amd.inference_detector(model, img, device_results=True, mask_bits=True)
    assert dres['all_results'][2].dtype == torch.bool and bres['all_results'][2].dtype == torch.uint8
    a = model.show_result(img, host, score_thr=0, show_labels=False)
    b = model.show_result(img, dres, score_thr=0, show_labels=False)
    c = model.show_result(torch.from_numpy(img).to(dev), bres, score_thr=0, show_labels=False)
    assert a.shape == img.shape and a.dtype == np.uint8
    assert np.array_equal(a, b) and np.array_equal(a, c)
    bbox_result, mask_result = host['all_results']
    boxes = np.vstack(bbox_result)
    labels = np.concatenate([np.full(len(x), i, np.int64) for i, x in enumerate(bbox_result)])
    masks = [m for per in mask_result for m in per]
    assert len(masks) > 0, 'no detection at all: the comparison is empty'
    want = paint.paint_instances_host(img, np.stack(masks), paint.instance_colors_host(labels, paint.get_palette(None, int(labels.max()) + 1)),
                                      None, boxes, np.tile(np.array([[72, 101, 241]], np.uint8), (len(labels), 1)))
    assert np.array_equal(a, want) and not np.array_equal(a, img)
    # a threshold above every score keeps nothing; one between the scores keeps those above it, as the host rule with `keep`
    assert np.array_equal(model.show_result(img, dres, score_thr=2.0, show_labels=False), img)
    thr = float(np.median(boxes[:, 4]))
    keep = boxes[:, 4] > thr
    colors = np.zeros((len(labels), 3), np.uint8)
    colors[keep] = paint.instance_colors_host(labels[keep], paint.get_palette(None, int(labels.max()) + 1))
    want = paint.paint_instances_host(img, np.stack(masks), colors, keep, boxes, np.tile(np.array([[72, 101, 241]], np.uint8), (len(labels), 1)))
    assert np.array_equal(model.show_result(img, host, score_thr=thr, show_labels=False), want)
    # labels on: shape and dtype hold; out_file is readable and decodes to what was painted
    lab = model.show_result(img, dres, score_thr=0)
    assert lab.shape == img.shape and lab.dtype == np.uint8
    out = tmp_path / 'painted.png'
    assert model.show_result(img, dres, score_thr=0, show_labels=False, out_file=str(out)) is None
    with Image.open(out) as im:
        assert np.array_equal(np.asarray(im.convert('RGB'))[:, :, ::-1], a)
    assert cgg_amd.show_result_pyplot(model, img, dres, score_thr=0, out_file=str(tmp_path / 'pyplot.png')) is None
    assert (tmp_path / 'pyplot.png').exists()


def test_show_result_panoptic_end_to_end(dev, tmp_path):
    from PIL import Image
    model, img = _model(dev, panoptic=True), _image()
    assert model.show_result.__func__ is type(model)._show_pan_result
    host = cgg_amd.inference_detector(model, img)
    dres = cgg_amd.inference_detector(model, img, device_results=True)
    pan = host['panoptic_all_results']
    assert isinstance(pan, np.ndarray) and torch.is_tensor(dres['panoptic_all_results']) and dres['panoptic_all_results'].is_cuda
    a = model.show_result(img, host, score_thr=0, show_labels=False)
    b = model.show_result(img, dres, score_thr=0, show_labels=False)
    assert np.array_equal(a, b) and a.shape == img.shape and a.dtype == np.uint8
    ids = np.unique(pan)[::-1]
    ids = ids[ids != model.num_classes]
    assert len(ids) > 0, 'an all-void map: the comparison is empty'
    colors = paint.instance_colors_host(ids % 1000, paint.get_palette(None, int((ids % 1000).max()) + 1))
    assert np.array_equal(a, paint.paint_panoptic_host(img, pan, ids, colors, model.num_classes))
    lab = model.show_result(img, dres)
    assert lab.shape == img.shape and lab.dtype == np.uint8
    out = tmp_path / 'pan.png'
    assert model.show_result(img, dres, show_labels=False, out_file=str(out)) is None
    with Image.open(out) as im:
        assert np.array_equal(np.asarray(im.convert('RGB'))[:, :, ::-1], a)


def test_test_driver_show_dir(dev, tmp_path):
    import importlib.util
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = cgg_amd.registry.build_detector(cfg)
    randomize(m, seed=21)
    ck = save_checkpoint(m, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny_show.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\ndata = dict(test=dict(pipeline=' + repr(PIPELINE) + '))\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_show', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    show = tmp_path / 'shown'
    res = drv.main([str(cfg_file), ck, '--synthetic-u8', '64x96', '--num-images', '2', '--show-dir', str(show), '--show-score-thr', '0'])
    assert len(res) == 2
    files = sorted(os.listdir(show))
    assert files == ['synthetic_0.png', 'synthetic_1.png']
    from PIL import Image
    for f in files:
        with Image.open(show / f) as im:
            assert im.size == (96, 64)
    # the same base name from two directories, and a frame without a name: three files, none overwritten
    import sys
    sys.path.insert(0, os.path.join(root, 'tests'))
    again = tmp_path / 'again'
    res = drv.main([str(cfg_file), ck, '--data', 'test_paint_gpu:same_names_stream', '--show-dir', str(again), '--show-score-thr', '0'])
    assert len(res) == 3 and sorted(os.listdir(again)) == ['2.png', 'x.png', 'x_1.png']


def same_names_stream(cfg, rank, world):
    """`--data` hook: two frames whose file names share a base name, and a bare frame"""
    frames = [_image(), _image()[::-1].copy(), _image()[:, ::-1].copy()]
    return iter([(frames[0], dict(filename='a/x.jpg', ori_filename='a/x.jpg')), (frames[1], dict(filename='b/x.jpg', ori_filename='b/x.jpg')),
                 frames[2]])
