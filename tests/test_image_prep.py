"""image_prep.py on the host (no GPU): the reference's test pipeline restated -- target sizes and metas, the 8-bit bilinear rule
against known answers and against float64 interpolation, Pad / Normalize in both orders, the collation, the pipeline parser, and the
argument checks of `ops.image_prep_u8` and of the C entry, none of which touches a device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import _lib, data_contract, image_prep as ip, ops
from cgg_amd._lib import CggError

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
IDENT = ip.PrepSpec(img_scale=(1, 1), keep_ratio=False, size_divisor=None)


def _spec(new_hw, **kw):
    """a spec that resizes to exactly (new_h, new_w): keep_ratio=False takes img_scale as (w, h)"""
    d = dict(img_scale=(new_hw[1], new_hw[0]), keep_ratio=False, size_divisor=None)
    d.update(kw)
    return ip.PrepSpec(**d)


def _rand_img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---- rule 1 and the metas ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw, want', [((480, 640), (800, 1067)), ((427, 640), (800, 1199)), ((1024, 1024), (800, 800)),
                                      ((333, 500), (800, 1201)), ((100, 3000), (44, 1333)), ((1, 9), (148, 1333))])
def test_rescale_size(hw, want):
    assert ip.rescale_size(hw, (1333, 800)) == want
    assert ip.rescale_size(hw, (800, 1333)) == want                     # the order of img_scale does not matter when the ratio is kept
    assert ip.rescale_size(hw, (1333, 800), keep_ratio=False) == (800, 1333)


def test_metas_carry_what_collect_carries():
    spec = ip.PrepSpec(img_scale=(1333, 800), size_divisor=32, pad_val=(128, 128, 128), mean=MEAN, std=STD, to_rgb=True)
    batch, metas = ip.prepare_host([_rand_img(12, 16, 0)], ip.PrepSpec(img_scale=(40, 30), size_divisor=32, mean=MEAN, std=STD, to_rgb=True))
    m = metas[0]
    assert set(m) == set(data_contract.META_KEYS)
    assert m['ori_shape'] == (12, 16, 3) and m['img_shape'] == (30, 40, 3) and m['pad_shape'] == (32, 64, 3)
    assert batch.shape == (1, 3, 32, 64) and batch.dtype == np.float32
    assert m['flip'] is False and m['flip_direction'] is None and m['filename'] is None and m['ori_filename'] is None
    assert m['img_norm_cfg']['to_rgb'] is True and m['img_norm_cfg']['mean'].dtype == np.float32
    np.testing.assert_array_equal(m['img_norm_cfg']['std'], np.array(STD, dtype=np.float32))
    m = ip.image_meta((480, 640), spec)
    assert m['img_shape'] == (800, 1067, 3) and m['pad_shape'] == (800, 1088, 3)
    sf = m['scale_factor']
    assert sf.dtype == np.float32 and sf.shape == (4,)
    np.testing.assert_array_equal(sf, np.array([1067 / 640, 800 / 480, 1067 / 640, 800 / 480], dtype=np.float32))


# ---- rules 2 and 3 -----------------------------------------------------------------------------------------------------------------
def test_identity_resize_is_exact():
    img = _rand_img(37, 29, 1)
    np.testing.assert_array_equal(ip.resize_u8(img, 37, 29), img)
    i0, i1, a0, a1 = ip.resize_coefficients(29, 29)
    assert np.array_equal(i0, np.arange(29)) and np.all(a0 == 2048) and np.all(a1 == 0)
    batch, _ = ip.prepare_host([img], _spec((37, 29)))
    np.testing.assert_array_equal(batch[0], img.transpose(2, 0, 1).astype(np.float32))


@pytest.mark.parametrize('value', [0, 1, 127, 254, 255])
def test_constant_image_stays_constant(value):
    img = np.full((9, 14, 3), value, dtype=np.uint8)
    for new in [(23, 31), (4, 5), (9, 40), (30, 14)]:
        assert np.all(ip.resize_u8(img, *new) == value)


def test_known_answers():
    one = lambda rows: np.repeat(np.array(rows, dtype=np.uint8)[:, :, None], 3, axis=2)
    assert ip.resize_u8(one([[0, 255]]), 1, 4)[0, :, 0].tolist() == [0, 64, 191, 255]
    got = ip.resize_u8(one([[10, 20], [30, 40]]), 4, 4)
    assert got[:, :, 1].tolist() == [[10, 13, 18, 20], [15, 17, 22, 25], [25, 27, 32, 35], [30, 33, 38, 40]]
    assert np.array_equal(got[:, :, 0], got[:, :, 2])


def test_coefficients_clamp_at_both_ends():
    i0, i1, a0, a1 = ip.resize_coefficients(1, 7)                      # a single source sample: both taps are sample 0
    assert not i0.any() and not i1.any() and np.all(a0 == 2048) and not a1.any()
    i0, i1, a0, a1 = ip.resize_coefficients(6, 9)
    assert i0[0] == 0 and a1[0] == 0 and i0[-1] == 5 and i1[-1] == 5 and a1[-1] == 0
    assert np.all(a0 + a1 == 2048) and np.all(np.diff(i0) >= 0) and i1.max() <= 5


@pytest.mark.parametrize('src, dst', [((7, 5), (14, 10)), ((13, 9), (29, 21)), ((40, 56), (17, 23)), ((3, 4), (32, 40)),
                                      ((1, 6), (4, 9)), ((33, 31), (64, 61))])
def test_within_one_level_of_float64_interpolation(src, dst):
    """The independent side: |out - rint(exact)| <= 1 EVERYWHERE, exact = F.interpolate(bilinear, align_corners=False) in float64.
    Derivation of the bound on |out - exact| < 1.3: 0.5 for the final rounding, at most 0.5 for the two truncating shifts, about
    0.25 for the 11-bit coefficients; rint(exact) adds at most 0.5, and both sides are integers."""
    img = _rand_img(src[0], src[1], 7 + src[0])
    got = ip.resize_u8(img, *dst).astype(np.int64)
    exact = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None].double(), size=dst, mode='bilinear', align_corners=False)[0]
    want = torch.round(exact).permute(1, 2, 0).numpy().astype(np.int64)
    assert np.abs(got - want).max() <= 1


# ---- rules 4 and 5 -----------------------------------------------------------------------------------------------------------------
def _f64(img_u8_hwc, mean, std, to_rgb):
    x = img_u8_hwc[:, :, ::-1] if to_rgb else img_u8_hwc
    return ((x.astype(np.float64) - np.array(mean)) / np.array(std)).transpose(2, 0, 1)


@pytest.mark.parametrize('to_rgb', [False, True])
def test_pad_before_normalize_scalar_and_tuple(to_rgb):
    img = _rand_img(5, 7, 3)
    for pad_val, src_order in [(128.0, (128, 128, 128)), ((10.0, 20.0, 30.0), (10, 20, 30))]:
        spec = _spec((5, 7), size_divisor=8, pad_val=pad_val, mean=MEAN, std=STD, to_rgb=to_rgb, pad_before_norm=True)
        batch, metas = ip.prepare_host([img], spec)
        assert batch.shape == (1, 3, 8, 8) and metas[0]['pad_shape'] == (8, 8, 3)
        # the reference pads the uint8 BGR image, then normalises the whole padded image
        padded = np.empty((8, 8, 3), dtype=np.uint8)
        padded[:] = np.array(src_order, dtype=np.uint8)
        padded[:5, :7] = img
        np.testing.assert_allclose(batch[0], _f64(padded, MEAN, STD, to_rgb), rtol=0, atol=1e-6)


@pytest.mark.parametrize('to_rgb', [False, True])
def test_normalize_before_pad_holds_pad_val_itself(to_rgb):
    img = _rand_img(6, 3, 4)
    spec = _spec((6, 3), size=(9, 4), pad_val=(1.0, 2.0, 3.0), mean=MEAN, std=STD, to_rgb=to_rgb, pad_before_norm=False)
    batch, _ = ip.prepare_host([img], spec)
    assert batch.shape == (1, 3, 9, 4)
    np.testing.assert_allclose(batch[0, :, :6, :3], _f64(img, MEAN, STD, to_rgb), rtol=0, atol=1e-6)
    for c, v in enumerate((1.0, 2.0, 3.0)):
        assert np.all(batch[0, c, 6:, :] == v) and np.all(batch[0, c, :, 3:] == v)


def test_collate_region_is_zero():
    a, b = _rand_img(10, 30, 5), _rand_img(20, 12, 6)
    spec = ip.PrepSpec(img_scale=(64, 48), keep_ratio=True, size_divisor=16, pad_val=128.0, mean=MEAN, std=STD, to_rgb=True)
    batch, metas = ip.prepare_host([a, b], spec)
    shapes = [m['pad_shape'] for m in metas]
    assert shapes == [(32, 64, 3), (64, 48, 3)] and batch.shape == (2, 3, 64, 64)
    assert [m['img_shape'] for m in metas] == [(21, 64, 3), (64, 38, 3)]
    assert np.all(batch[0, :, 32:, :] == 0) and np.all(batch[1, :, :, 48:] == 0)
    padv = ((np.float32(128) - np.array(MEAN, np.float32)) * (1 / np.array(STD)).astype(np.float32))
    for c in range(3):
        assert np.all(batch[0, c, 21:32, :] == padv[c]) and np.all(batch[1, c, :, 38:48] == padv[c])
    one, _ = ip.prepare_host([a], spec)                                  # each image equals its own single-image preparation
    np.testing.assert_array_equal(batch[0, :, :32, :], one[0])


# ---- the parser --------------------------------------------------------------------------------------------------------------------
def _pipeline(**over):
    norm = dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    transforms = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                  dict(type='Pad', size_divisor=32, pad_val=dict(img=(128, 128, 128), masks=0, seg=255)), norm,
                  dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]
    aug = dict(type='MultiScaleFlipAug', img_scale=(1333, 800), flip=False, transforms=over.pop('transforms', transforms))
    aug.update(over)
    return [dict(type='LoadImageFromFile'), aug]


def test_parse_reference_shaped_pipeline():
    spec = ip.parse_test_pipeline(_pipeline())
    assert spec == ip.PrepSpec(img_scale=(1333, 800), keep_ratio=True, size_divisor=32, size=None, pad_val=(128.0, 128.0, 128.0),
                               mean=MEAN, std=STD, to_rgb=True, pad_before_norm=True)
    p = _pipeline()
    p[0] = dict(type='LoadImageFromWebcam')
    assert ip.parse_test_pipeline(p) == spec
    # mmdet's base configs: Normalize ahead of Pad, scalar pad value 0, DefaultFormatBundle
    base = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Normalize', mean=[1, 2, 3], std=[4, 5, 6], to_rgb=False), dict(type='Pad', size_divisor=32),
            dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]
    got = ip.parse_test_pipeline(_pipeline(transforms=base, img_scale=[(1333, 800)]))
    assert got.pad_before_norm is False and got.pad_val == 0.0 and got.to_rgb is False and got.mean == (1.0, 2.0, 3.0)
    assert ip.parse_test_pipeline(cgg_amd.config.to_config_dict(_pipeline())) == spec       # ConfigDict, as a loaded config gives


def test_parse_refuses_what_is_not_restated():
    with pytest.raises(CggError, match='MultiScaleFlipAug: 2 scales'):
        ip.parse_test_pipeline(_pipeline(img_scale=[(1333, 800), (1000, 600)]))
    with pytest.raises(CggError, match='MultiScaleFlipAug: flip=True'):
        ip.parse_test_pipeline(_pipeline(flip=True))
    t = _pipeline()[1]['transforms']
    with pytest.raises(CggError, match='PhotoMetricDistortion: unknown'):
        ip.parse_test_pipeline(_pipeline(transforms=t[:1] + [dict(type='PhotoMetricDistortion')] + t[1:]))
    with pytest.raises(CggError, match="Resize: interpolation='nearest'"):
        ip.parse_test_pipeline(_pipeline(transforms=[dict(type='Resize', keep_ratio=True, interpolation='nearest')] + t[1:]))
    with pytest.raises(CggError, match='LoadAnnotations: unknown'):
        ip.parse_test_pipeline([dict(type='LoadImageFromFile'), dict(type='LoadAnnotations')] + _pipeline()[1:])
    with pytest.raises(CggError, match='Resize: missing'):
        ip.parse_test_pipeline(_pipeline(transforms=[t[1]] + t[4:]))
    with pytest.raises(CggError, match='Pad: precedes Resize'):
        ip.parse_test_pipeline(_pipeline(transforms=t[1:]))


def test_image_prep_has_no_host_fallback():
    with pytest.raises(CggError, match='ROCm device'):
        ip.ImagePrep(ip.parse_test_pipeline(_pipeline()), 'cpu')
    with pytest.raises(CggError, match='uint8'):
        ip.prepare_host([np.zeros((4, 4, 3), dtype=np.float32)], IDENT)
    with pytest.raises(CggError, match='zero-sized'):
        ip.prepare_host([np.zeros((0, 4, 3), dtype=np.uint8)], IDENT)


# ---- the wrapper and the C entry refuse bad arguments before any device work ---------------------------------------------------------
class _Dev(torch.Tensor):
    """a CPU tensor that claims to live on a ROCm device (the trick of tests/test_mask_feature_head.py)"""

    @property
    def is_cuda(self):
        return True

    def data_ptr(self):
        return 4096


def _wrapper_args():
    staged = torch.zeros(32 + 4 * 5 * 3, dtype=torch.uint8).as_subclass(_Dev)
    table = torch.tensor([[32, 4, 5, 15, 8, 10, 8, 12]], dtype=torch.int32)
    out = torch.zeros(1, 3, 8, 12).as_subclass(_Dev)
    return [staged, table, out, MEAN, STD]


@pytest.mark.parametrize('mutate', ['float source', 'non-contiguous out', 'cpu out', 'table columns', 'int64 table', 'double out',
                                    'batch mismatch', 'device table'])
def test_wrapper_raises_before_any_native_call(monkeypatch, mutate):
    def no_native():
        raise AssertionError('the native library was reached')
    monkeypatch.setattr(ops, '_lib_', no_native)
    a = _wrapper_args()
    if mutate == 'float source':
        a[0] = torch.zeros(92).as_subclass(_Dev)
    elif mutate == 'non-contiguous out':
        a[2] = torch.zeros(1, 3, 12, 8).as_subclass(_Dev).transpose(2, 3)
        assert tuple(a[2].shape) == (1, 3, 8, 12)
    elif mutate == 'cpu out':
        a[2] = torch.zeros(1, 3, 8, 12)
    elif mutate == 'table columns':
        a[1] = torch.zeros(1, 7, dtype=torch.int32)
    elif mutate == 'int64 table':
        a[1] = a[1].long()
    elif mutate == 'double out':
        a[2] = a[2].double()
    elif mutate == 'batch mismatch':
        a[2] = torch.zeros(2, 3, 8, 12).as_subclass(_Dev)
    else:
        a[1] = a[1].as_subclass(_Dev)
    with pytest.raises(CggError):
        ops.image_prep_u8(*a)


@pytest.mark.skipif(torch.cuda.is_available(), reason='hands host pointers to the entry: only where no launch can follow a missed check')
def test_entry_validates_on_the_host():
    """every refusal below returns before the launch: the pointers are host memory and no device exists here"""
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8)                          # host memory, 64-byte aligned
    p = ctypes.c_void_p(buf.data_ptr())
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    mean, std, pad = f3(0, 0, 0), f3(1, 1, 1), f3(0, 0, 0)

    def call(row, B=1, nbytes=4096, Hb=8, Wb=12, table_offset=0, std_=std):
        table = (ctypes.c_int32 * 8)(*row)
        return lib.cgg_image_prep_u8(p, nbytes, table_offset, table, B, mean, std_, pad, 1, 1, p, Hb, Wb, None)

    good = [32, 4, 5, 15, 8, 10, 8, 12]
    EINVAL, EUNSUPPORTED = -1, -2
    assert call(good, B=0) == EINVAL
    assert call([32, 0, 5, 15, 8, 10, 8, 12]) == EINVAL and b'zero-sized' in lib.cgg_last_error_string()
    assert call([32, 4, 0, 15, 8, 10, 8, 12]) == EINVAL
    assert call([32, 4, 5, 15, 9, 10, 8, 12]) == EINVAL                  # new_h > pad_h
    assert call([32, 4, 5, 15, 8, 10, 9, 12]) == EINVAL                  # pad_h > Hb
    assert call([32, 4, 5, 15, 8, 13, 8, 12]) == EINVAL                  # new_w > pad_w
    assert call([32, 4, 5, 15, 8, 10, 8, 13]) == EINVAL                  # pad_w > Wb
    assert call([32, 4, 5, 14, 8, 10, 8, 12]) == EINVAL                  # pitch < 3 w
    assert call(good, nbytes=32 + 59) == EINVAL and b'extends past' in lib.cgg_last_error_string()   # one byte short
    assert call([-1, 4, 5, 15, 8, 10, 8, 12]) == EINVAL
    assert call(good, nbytes=31) == EINVAL                               # the table itself does not fit
    assert call(good, table_offset=2) == EINVAL
    assert call(good, std_=f3(1, 0, 1)) == EINVAL
    assert call([32, 4, 70000, 210000, 8, 10, 8, 12], nbytes=2**30) == EUNSUPPORTED
    assert call(good, nbytes=2**31) == EUNSUPPORTED and call(good, nbytes=2**31 - 8) == EUNSUPPORTED
    assert call(good, Hb=70000) == EUNSUPPORTED
    null = ctypes.c_void_p(None)
    assert lib.cgg_image_prep_u8(null, 64, 0, null, 1, mean, std, pad, 1, 1, p, 8, 12, None) == EINVAL
