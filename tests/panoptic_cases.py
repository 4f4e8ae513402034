"""Raw panoptic samples and the batches that tests/test_train_prep_panoptic.py (host) and tests/test_train_prep_panoptic_gpu.py
(device) share: seeded block-structured id maps with their `ann_info['masks']` records.

A map is a grid of rectangles at random cuts, one id per rectangle. The records, in shuffled order, list `things` is_thing segments,
one crowd thing (a thing category with is_thing false: in the semantic map, no bitmap) and stuff up to `records`; the rectangles
left over carry ids that NO record lists (they must come out as 255). Ids are 24-bit so that both map forms can hold them, at least
one of them >= 2^23 (the top bit of the blue byte) and, in the int32 form, one more >= 2^30 where a record lists it.
"""
import numpy as np

from cgg_amd import train_prep as tp

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
NUM_THINGS, NUM_STUFF = 80, 53


def pan_sample(h, w, seed, rgb, records=12, things=7, grid=(4, 4), captions=True):
    r = np.random.default_rng(seed)
    gy, gx = grid
    nb = gy * gx
    assert things + 1 <= records <= nb or records == things == 0
    ycut = np.concatenate([[0], np.sort(r.choice(np.arange(1, h), size=gy - 1, replace=False)), [h]]).astype(int)
    xcut = np.concatenate([[0], np.sort(r.choice(np.arange(1, w), size=gx - 1, replace=False)), [w]]).astype(int)
    ids = r.choice(2**24, size=nb, replace=False).astype(np.int64)
    ids[0] = 2**23 + 12345 + seed                            # ids >= 2^23, in both forms
    if not rgb:
        ids[1] = 2**30 + 77 + seed                           # and beyond 24 bits where the form can hold it
    assert len(set(ids.tolist())) == nb
    pan = np.empty((h, w), dtype=np.int32)
    for k in range(nb):
        i, j = divmod(k, gx)
        pan[ycut[i]:ycut[i + 1], xcut[j]:xcut[j + 1]] = ids[k]
    listed = r.permutation(nb)[:records].tolist()
    if records:                                              # the large ids are listed: blocks 0 and 1 take the first two rows
        listed = [0, 1] + [k for k in listed if k not in (0, 1)][:records - 2]
    kinds = ['thing'] * things + (['crowd'] if records else []) + ['stuff'] * max(records - things - 1, 0)
    segments = []
    for k, kind in zip(listed, kinds):
        cat = int(r.integers(0, NUM_THINGS)) if kind != 'stuff' else int(NUM_THINGS + r.integers(0, NUM_STUFF))
        segments.append(dict(id=int(ids[k]), category=cat, is_thing=kind == 'thing'))
    segments = [segments[i] for i in r.permutation(len(segments)).tolist()]
    labels = np.array([s['category'] for s in segments if s['is_thing']], dtype=np.int64)
    if rgb:
        pan = np.stack([pan & 255, (pan >> 8) & 255, (pan >> 16) & 255], axis=2).astype(np.uint8)
    s = dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), pan_seg=pan, segments=segments, gt_labels=labels,
             filename=f'pan_{seed}.jpg')
    if captions:
        s.update(gt_caption_ids=r.integers(1, 500, size=(8,)), gt_caption_mask=np.ones(8, dtype=np.int64),
                 gt_caption_nouns_ids=r.integers(1, 500, size=(8,)), gt_caption_nouns_mask=np.ones(8, dtype=np.int64))
    return s


def spec_for(size, seg=True):
    return tp.TrainPrepSpec(img_scale=(64, 64), crop_size=size, size=size, pad_val=((128.0, 64.0, 32.0), 0, 250), mean=MEAN, std=STD,
                            to_rgb=True, with_seg=seg)


def far_margin(hw, scale, flip, spec):
    nh, nw = tp.resized_hw(hw, scale)
    return tp.TrainParams(flip, scale, (max(nh - spec.crop_size[0], 0), max(nw - spec.crop_size[1], 0)))


# (size = crop, [(h, w, scale, flip)]): the windows sit at the far margins
WIDE = ((40, 520), [(37, 53, (106, 80), False), (120, 700, (1040, 1040), True), (64, 48, (3000, 90), True), (30, 40, (8, 8), False)])
ODD = ((33, 50), [(37, 53, (106, 80), True), (20, 31, (62, 62), False)])


def batch(case, rgb, seg=True, seed=0):
    """(samples, params, spec) of one of the two cases; rgb: True / False, or 'mixed' for the two forms in turn"""
    size, rows = case
    spec = spec_for(size, seg)
    samples, params = [], []
    for i, (h, w, scale, flip) in enumerate(rows):
        form = bool(i % 2) if rgb == 'mixed' else bool(rgb)
        samples.append(pan_sample(h, w, seed + 10 * i + 1, form))
        params.append(far_margin((h, w), scale, flip, spec))
    return samples, params, spec


def bitmap_samples(samples):
    out = []
    for s in samples:
        b = {k: v for k, v in s.items() if k not in ('pan_seg', 'segments')}
        b['gt_masks'], b['gt_semantic_seg'] = tp.load_panoptic_host(s['pan_seg'], s['segments'])
        out.append(b)
    return out
