"""Raw panoptic samples on the host (train_prep.py, rule 5): `load_panoptic_host` against a literal loop over the records, the
definition of `prepare_train_host` on panoptic samples (= the rule on the bitmap samples that loop makes), and every refusal by the
name of its field. tests/panoptic_cases.py holds the samples and the two batches that the device test shares."""
import copy

import numpy as np
import pytest

import cgg_amd  # noqa: F401
from cgg_amd import synthetic, train_prep as tp
from cgg_amd._lib import CggError

import panoptic_cases as pc


def _ids(pan):
    if pan.ndim == 2:
        return pan.astype(np.int64)
    p = pan.astype(np.int64)
    return p[:, :, 0] + 256 * p[:, :, 1] + 65536 * p[:, :, 2]


def _literal_loader(pan, segments):
    """the loader's loop, loading.py:317-326, as it stands there"""
    pan_png = _ids(pan)
    gt_masks = []
    gt_seg = np.zeros_like(pan_png) + 255
    for mask_info in segments:
        mask = (pan_png == mask_info['id'])
        gt_seg = np.where(mask, mask_info['category'], gt_seg)
        if mask_info.get('is_thing'):
            gt_masks.append(mask.astype(np.uint8))
    return gt_masks, gt_seg


LOADER_CASES = [dict(h=37, w=53, seed=1), dict(h=20, w=31, seed=2, grid=(3, 5), records=9, things=4),
                dict(h=16, w=16, seed=3, things=0, records=5), dict(h=9, w=12, seed=4, things=0, records=0, grid=(2, 3))]


@pytest.mark.parametrize('rgb', [False, True], ids=['int32', 'rgb'])
@pytest.mark.parametrize('case', LOADER_CASES, ids=['12rec-7things', '9rec-4things', 'zero-things', 'zero-records'])
def test_loader_equals_the_literal_loop(case, rgb):
    s = pc.pan_sample(rgb=rgb, **case)
    pan, segments = s['pan_seg'], s['segments']
    assert pan.dtype == (np.uint8 if rgb else np.int32) and pan.shape == (case['h'], case['w']) + ((3,) if rgb else ())
    masks, seg = tp.load_panoptic_host(pan, segments)
    want_masks, want_seg = _literal_loader(pan, segments)
    things = case.get('things', 7)
    assert masks.dtype == np.uint8 and masks.shape == (things, case['h'], case['w'])
    assert seg.dtype == np.uint8 and seg.shape == (case['h'], case['w'])
    assert len(want_masks) == things and all(np.array_equal(a, b) for a, b in zip(masks, want_masks))
    assert np.array_equal(seg, want_seg)
    # what the case is there for
    ids = _ids(pan)
    listed = {r['id'] for r in segments}
    unlisted = ~np.isin(ids, list(listed)) if listed else np.ones(ids.shape, dtype=bool)
    assert unlisted.any() and (seg[unlisted] == 255).all() and (seg[~unlisted] < 255).all()     # an id that no record lists
    if segments:
        assert ids.max() >= 2**23 and max(listed) >= 2**23 and (rgb or max(listed) >= 2**30)
        crowd = [r for r in segments if not r['is_thing'] and r['category'] < pc.NUM_THINGS]
        assert len(crowd) == 1 and (seg[ids == crowd[0]['id']] == crowd[0]['category']).all()      # in the semantic map, no bitmap
        assert all(not (m.astype(bool) & (ids == crowd[0]['id'])).any() for m in masks)
    else:
        assert (seg == 255).all()
    for m, r in zip(masks, [r for r in segments if r['is_thing']]):                                  # record order
        assert m.any() and (ids[m.astype(bool)] == r['id']).all()


def test_the_two_forms_of_one_map_agree():
    s = pc.pan_sample(37, 53, 5, rgb=True)
    a = tp.load_panoptic_host(s['pan_seg'], s['segments'])
    b = tp.load_panoptic_host(_ids(s['pan_seg']).astype(np.int32), s['segments'])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == 'img_metas':
            for x, y in zip(a[k], b[k]):
                assert x.keys() == y.keys()
                for f in x:
                    if f == 'scale_factor':
                        assert np.array_equal(x[f], y[f])
                    elif f == 'img_norm_cfg':
                        assert np.array_equal(x[f]['mean'], y[f]['mean']) and np.array_equal(x[f]['std'], y[f]['std'])
                    else:
                        assert x[f] == y[f], f
        elif isinstance(a[k], list):
            assert len(a[k]) == len(b[k]), k
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                assert x.dtype == y.dtype and np.array_equal(x, y), (k, i)
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('seg', [True, False], ids=['with_seg', 'no_seg'])
@pytest.mark.parametrize('rgb', [False, True, 'mixed'], ids=['int32', 'rgb', 'mixed'])
@pytest.mark.parametrize('case', [pc.WIDE, pc.ODD], ids=['40x520', '33x50'])
def test_host_rule_on_panoptic_samples_is_the_rule_on_the_loaded_bitmaps(case, rgb, seg):
    samples, params, spec = pc.batch(case, rgb, seg)
    got, kept = tp.prepare_train_host(samples, params, spec)
    want, want_kept = tp.prepare_train_host(pc.bitmap_samples(samples), params, spec)
    assert kept == want_kept
    _same(got, want)
    assert ('gt_semantic_seg' in got) == seg
    things = [len(s['gt_labels']) for s in samples]
    assert things == [7] * len(samples)
    assert any(0 < k < n for k, n in zip(kept, things)), 'the case is there to lose things to the crop'
    if seg:                # 255 is the loader's constant, 250 is Pad's value here: the wide case pads, the odd one fills its window
        assert (got['gt_semantic_seg'] == 255).any() and (got['gt_semantic_seg'] == 250).any() == (case is pc.WIDE)


def test_the_wide_case_is_the_geometry_it_claims():
    samples, params, spec = pc.batch(pc.WIDE, False)
    geoms = [tp.sample_geometry(s['img'].shape[:2], p, spec) for s, p in zip(samples, params)]
    assert [g[:2] for g in geoms] == [(74, 106), (178, 1040), (120, 90), (6, 8)]
    assert [g[2:4] for g in geoms] == [(34, 0), (138, 520), (80, 0), (0, 0)]
    assert [p.flip for p in params] == [False, True, True, False]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _base():
    return pc.pan_sample(16, 20, 7, rgb=False)


def _seg_edit(i, **kw):
    def f(s):
        s['segments'] = copy.deepcopy(s['segments'])
        s['segments'][i].update(kw)
    return f


def _set(**kw):
    return lambda s: s.update(kw)


def _rgb_with_wide_id(s):
    s.update(pc.pan_sample(16, 20, 7, rgb=True))
    _seg_edit(0, id=2**24)(s)


def _too_many(s):
    s['segments'] = [dict(id=i, category=1, is_thing=False) for i in range(257)]
    s['gt_labels'] = np.zeros((0,), dtype=np.int64)


REFUSED = [
    ('segments', 'twice', lambda s: _seg_edit(1, id=s['segments'][0]['id'])(s)),
    ('category', 'segments', _seg_edit(2, category=255)),
    ('category', 'segments', _seg_edit(2, category=-1)),
    ('id', 'segments', _seg_edit(0, id=2**31)),
    ('id', 'segments', _seg_edit(0, id=-1)),
    ('id', 'segments', _rgb_with_wide_id),
    ('segments', '257', _too_many),
    ('gt_labels', None, lambda s: s.update(gt_labels=s['gt_labels'][:-1])),
    ('gt_masks', 'pan_seg', _set(gt_masks=np.zeros((7, 16, 20), dtype=np.uint8))),
    ('pan_seg', None, lambda s: s.update(pan_seg=s['pan_seg'].astype(np.int64))),
    ('pan_seg', None, lambda s: s.update(pan_seg=s['pan_seg'].astype(np.uint8))),
    ('pan_seg', None, lambda s: s.update(pan_seg=s['pan_seg'][:-1])),
    ('pan_seg', None, lambda s: s.update(pan_seg=np.zeros((16, 20, 4), dtype=np.uint8))),
    ('pan_seg', None, lambda s: s.update(pan_seg=-s['pan_seg'])),
    ('segments', None, _set(segments=None)),
]


@pytest.mark.parametrize('name, also, edit', REFUSED, ids=[f'{i}-{n}' for i, (n, _, _) in enumerate(REFUSED)])
def test_refusals_name_their_field(name, also, edit):
    s = _base()
    spec = pc.spec_for((16, 20))
    p = [tp.TrainParams(False, (20, 20), (0, 0))]
    tp.prepare_train_host([s], p, spec)                           # the base sample is accepted
    edit(s)
    with pytest.raises(CggError, match=name) as e:
        tp.prepare_train_host([s], p, spec)
    assert also is None or also in str(e.value)


def test_loader_refuses_on_its_own():
    s = _base()
    with pytest.raises(CggError, match='pan_seg'):
        tp.load_panoptic_host(s['pan_seg'].astype(np.float32), s['segments'])
    with pytest.raises(CggError, match='twice'):
        tp.load_panoptic_host(s['pan_seg'], s['segments'] + s['segments'][:1])
    with pytest.raises(CggError, match='category'):
        tp.load_panoptic_host(s['pan_seg'], [dict(id=1, category=300, is_thing=True)])


def test_a_batch_that_mixes_the_two_kinds_is_refused():
    s = _base()
    b = pc.bitmap_samples([s])[0]
    spec = pc.spec_for((16, 20))
    p = [tp.TrainParams(False, (20, 20), (0, 0))] * 2
    for pair in ([s, b], [b, s]):
        with pytest.raises(CggError, match='mixes'):
            tp.prepare_train_host(pair, p, spec)


def pipeline(load):
    return [dict(type='LoadImageFromFile', to_float32=True), load,
            dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Resize', img_scale=(1024, 1024), ratio_range=(0.1, 2.0), multiscale_mode='range', keep_ratio=True),
            dict(type='RandomCrop', crop_size=(1024, 1024), crop_type='absolute', recompute_bbox=True, allow_negative_crop=True),
            dict(type='FilterAnnotations', min_gt_bbox_wh=(1e-5, 1e-5), by_mask=True),
            dict(type='Pad', size=(1024, 1024), pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
            dict(type='Normalize', mean=list(pc.MEAN), std=list(pc.STD), to_rgb=True),
            dict(type='OpenFormatBundle', img_to_float=True), dict(type='Collect', keys=['img', 'gt_masks'])]


def _pan_pipeline(**kw):
    return pipeline(dict(dict(type='LoadOpenPanopticAnnotations', with_bbox=True, with_mask=True, with_seg=True, with_caption=True), **kw))


def test_parser_and_the_panoptic_loader_options():
    """with_mask=False is refused by the loader's name; with_mask_based_bbox (boxes are those of the cropped masks in any case) and
    with_seg=False (only the thing planes) do not make the result differ from the rule and are accepted"""
    for t in ('LoadOpenPanopticAnnotations', 'LoadPanopticAnnotations'):
        with pytest.raises(CggError, match=t + '.*with_mask=False'):
            tp.parse_train_pipeline(_pan_pipeline(type=t, with_mask=False))
        with pytest.raises(CggError, match=t + '.*poly2mask'):
            tp.parse_train_pipeline(_pan_pipeline(type=t, poly2mask=False))
    base = tp.parse_train_pipeline(_pan_pipeline())
    assert base.with_seg
    assert tp.parse_train_pipeline(_pan_pipeline(with_mask_based_bbox=True)) == base
    assert tp.parse_train_pipeline(_pan_pipeline(with_mask_based_bbox=False)) == base
    no_seg = tp.parse_train_pipeline(_pan_pipeline(with_seg=False))
    assert not no_seg.with_seg
    assert no_seg == tp.parse_train_pipeline(pipeline(dict(type='LoadOpenAnnotations', with_bbox=True, with_mask=True, with_caption=True)))


# ---- the synthetic stream ---------------------------------------------------------------------------------------------------------
def test_synthetic_panoptic_stream_is_seeded_and_holds_every_kind():
    a = [s for s, _ in zip(synthetic.panoptic_samples((48, 64), 10, 4, seed=3, vocab=500), range(4))]
    b = [s for s, _ in zip(synthetic.panoptic_samples((48, 64), 10, 4, seed=3, vocab=500), range(4))]
    forms = set()
    for s, t in zip(a, b):
        assert np.array_equal(s['pan_seg'], t['pan_seg']) and s['segments'] == t['segments'] and np.array_equal(s['img'], t['img'])
        forms.add(s['pan_seg'].ndim)
        masks, seg = tp.load_panoptic_host(s['pan_seg'], s['segments'])
        things = [r for r in s['segments'] if r['is_thing']]
        assert len(masks) == len(things) >= 1 and s['gt_labels'].tolist() == [r['category'] for r in things]
        assert int(s['gt_labels'].max()) < 10 and all(m.any() for m in masks)
        kinds = {(r['is_thing'], r['category'] < 10) for r in s['segments']}
        assert kinds == {(True, True), (False, True), (False, False)}          # things, a crowd thing, stuff
        assert (seg == 255).any() and _ids(s['pan_seg']).max() >= 2**23          # ids that no record lists; ids >= 2^23
        assert s['img'].dtype == np.uint8 and s['gt_caption_ids'].max() < 500
    assert forms == {2, 3}
    assert not np.array_equal(a[0]['pan_seg'], a[2]['pan_seg'])
