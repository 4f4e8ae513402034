"""Synthetic stand-ins for everything the benchmark cannot fetch offline:
class-embedding JSON / known / unknown files with the reference's schema, a model config with the
reference's keys (the `model = dict(type='Mask2FormerOpen', ...)` block of
configs/instance/coco_b48n17.py:16-188 and configs/openset_panoptic/coco_panoptic_p20.py),
COCO-shaped seeded input batches, and raw panoptic samples (an id map and its segment records).
"""
import json
import os
import tempfile

import numpy as np
import torch

_TMP = {}


def write_class_files(num_classes, num_unknown, dim=768, seed=0, root=None):
    """-> dict(class_to_emb_file, known_file, unknown_file). Embeddings ~ N(-0.03, 0.77^2) like the
    measured statistics of datasets/embeddings/*.json; names 'class_i'."""
    key = (num_classes, num_unknown, dim, seed, root)
    if key in _TMP and all(os.path.exists(p) for p in _TMP[key].values()):
        return _TMP[key]
    root = root or tempfile.mkdtemp(prefix='cgg_synth_')
    os.makedirs(root, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    embs = (torch.randn(num_classes, dim, generator=g) * 0.77 - 0.03).tolist()
    names = [f'class_{i}' for i in range(num_classes)]
    # unknown classes: every (num_classes // num_unknown)-th name
    unknown = names[::max(1, num_classes // max(num_unknown, 1))][:num_unknown] if num_unknown else []
    paths = dict(class_to_emb_file=os.path.join(root, f'class_emb_{num_classes}.json'),
                 known_file=os.path.join(root, f'known_{num_classes}.txt'),
                 unknown_file=os.path.join(root, f'unknown_{num_unknown}.txt'))
    with open(paths['class_to_emb_file'], 'w') as f:
        json.dump([dict(id=i, name=n, emb=e) for i, (n, e) in enumerate(zip(names, embs))], f)
    with open(paths['known_file'], 'w') as f:
        f.write('\n'.join(names))
    with open(paths['unknown_file'], 'w') as f:
        f.write('\n'.join(unknown))
    _TMP[key] = paths
    return paths


def model_config(num_things=65, num_stuff=0, num_unknown=17, num_queries=100, depth=50, panoptic=False,
                 num_points=12544, use_caption=True, use_caption_generation=True, files=None,
                 eval_types=None, enc_layers=6, dec_layers=9, vocab=30522, seed=0):
    """A `model` dict with the keys of the reference configs (Mask2FormerOpen / R50 / 100 queries).
    The head is trained on the known classes only (num_things_classes = known), the fusion head scores
    all classes -- as in coco_b48n17.py:30-36 and :154-163."""
    num_classes = num_things + num_stuff
    num_known = num_classes - num_unknown
    files = files or write_class_files(num_classes, num_unknown, seed=seed)
    if eval_types is None:
        eval_types = ['all_results'] if panoptic else ['all_results', 'novel_results', 'base_results']
    head_things = num_known if not panoptic else num_things - num_unknown
    head_classes = head_things + num_stuff
    in_channels = [256, 512, 1024, 2048] if depth >= 50 else [64, 128, 256, 512]
    return dict(
        type='Mask2FormerOpen',
        backbone=dict(type='ResNet', depth=depth, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=3,
                      norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch',
                      init_cfg=None),
        panoptic_head=dict(
            type='Mask2FormerHeadOpen', in_channels=in_channels, strides=[4, 8, 16, 32], feat_channels=256,
            out_channels=256, num_things_classes=head_things, num_stuff_classes=num_stuff,
            num_queries=num_queries, num_transformer_feat_level=3,
            pixel_decoder=dict(
                type='MSDeformAttnPixelDecoder', num_outs=3, norm_cfg=dict(type='GN', num_groups=32),
                act_cfg=dict(type='ReLU'),
                encoder=dict(
                    type='DetrTransformerEncoder', num_layers=enc_layers,
                    transformerlayers=dict(
                        type='BaseTransformerLayer',
                        attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=256, num_heads=8,
                                       num_levels=3, num_points=4, im2col_step=64, dropout=0.0,
                                       batch_first=False, norm_cfg=None, init_cfg=None),
                        ffn_cfgs=dict(type='FFN', embed_dims=256, feedforward_channels=1024, num_fcs=2,
                                      ffn_drop=0.0, act_cfg=dict(type='ReLU', inplace=True)),
                        operation_order=('self_attn', 'norm', 'ffn', 'norm')),
                    init_cfg=None),
                positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
                init_cfg=None),
            enforce_decoder_input_project=False,
            positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
            transformer_decoder=dict(
                type='DetrTransformerDecoder', return_intermediate=True, num_layers=dec_layers,
                transformerlayers=dict(
                    type='DetrTransformerDecoderLayer',
                    attn_cfgs=dict(type='MultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.0,
                                   proj_drop=0.0, dropout_layer=None, batch_first=False),
                    ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048, num_fcs=2,
                                  act_cfg=dict(type='ReLU', inplace=True), ffn_drop=0.0, dropout_layer=None,
                                  add_identity=True),
                    feedforward_channels=2048,
                    operation_order=('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')),
                init_cfg=None),
            caption_generator=dict(type='CaptionTransformer', nb_layers=4, input_dim=768, hidden_dim=768,
                                   ff_dim=512, nb_heads=8, drop_val=0.1, pre_norm=False, seq_length=35,
                                   nb_tokens=vocab),
            loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.0, reduction='mean',
                          class_weight=[1.0] * head_classes + [0.1]),
            loss_cls_emb=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=2.0, reduction='mean',
                              class_weight=[1.0] * head_classes + [0.1]),
            loss_grounding=dict(type='GroundingLoss', loss_weight=2.0),
            loss_caption_generation=dict(type='CrossEntropyLoss', ignore_index=0, loss_weight=2.0),
            loss_mask=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='mean', loss_weight=5.0),
            loss_dice=dict(type='DiceLoss', use_sigmoid=True, activate=True, reduction='mean',
                           naive_dice=True, eps=1.0, loss_weight=5.0),
            class_agnostic=False, use_caption=use_caption, use_class_emb=True,
            use_caption_generation=use_caption_generation,
            class_to_emb_file=files['class_to_emb_file'], known_file=files['known_file'],
            unknown_file=files['unknown_file'], softmax_temperature=10, pred_emb_norm=False,
            text_emb_norm=True, caption_emb_type='bert', caption_gen_emb_type='bert',
            synthetic_text_encoder=True),
        panoptic_fusion_head=dict(
            type='MaskFormerFusionHeadOpen', num_things_classes=num_things if panoptic else num_classes,
            num_stuff_classes=num_stuff if panoptic else 0, panoptic_mode=panoptic, loss_panoptic=None,
            init_cfg=None, use_class_emb=True, class_to_emb_file=files['class_to_emb_file'],
            known_file=files['known_file'], unknown_file=files['unknown_file']),
        train_cfg=dict(
            num_points=num_points, oversample_ratio=3.0, importance_sample_ratio=0.75,
            assigner=dict(type='MaskHungarianAssignerOpen',
                          cls_cost=dict(type='ClassificationCost', weight=0.0),
                          cls_emb_cost=dict(type='ClassificationCost', weight=2.0),
                          mask_cost=dict(type='CrossEntropyLossCost', weight=5.0, use_sigmoid=True),
                          dice_cost=dict(type='DiceCost', weight=5.0, pred_act=True, eps=1.0)),
            sampler=dict(type='MaskPseudoSampler')),
        test_cfg=dict(eval_types=eval_types, max_per_image=100, iou_thr=0.8, filter_low_score=True,
                      use_class_emb=True),
        init_cfg=None)


def backbone_feats(B, H, W, channels=(256, 512, 1024, 2048), seed=0, device='cpu'):
    """N(0,1) feature maps at strides 4/8/16/32 (used when the backbone is bypassed)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, H // s, W // s, generator=g).to(device) for c, s in zip(channels, (4, 8, 16, 32))]


def structured_images(B, H, W, seed=0, shapes=24, noise=0.15):
    """Normalised-image-like batch WITH spatial structure: a smooth background plus `shapes` random rectangles /
    ellipses of random colour per image and a little noise. White-noise images average out in a stride-4 backbone and
    give spatially constant features (every mask all-on or all-off); parity tests need masks with real boundaries."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.linspace(-1, 1, H).view(1, H, 1)
    xs = torch.linspace(-1, 1, W).view(1, 1, W)
    out = torch.empty(B, 3, H, W)
    for b in range(B):
        a = torch.randn(3, 1, 1, generator=g)
        img = a * ys + torch.randn(3, 1, 1, generator=g) * xs + 0.3 * torch.randn(3, 1, 1, generator=g)
        for i in range(shapes):
            cy, cx = (torch.rand(2, generator=g) * 2 - 1).tolist()
            ry, rx = (torch.rand(2, generator=g) * 0.35 + 0.04).tolist()
            col = torch.randn(3, 1, 1, generator=g) * 1.2
            if i % 2 == 0:
                m = ((ys - cy).abs() <= ry) & ((xs - cx).abs() <= rx)
            else:
                m = ((ys - cy) / ry)**2 + ((xs - cx) / rx)**2 <= 1
            img = torch.where(m, col.expand(3, H, W), img)
        out[b] = img + noise * torch.randn(3, H, W, generator=g)
    return out


def img_metas(B, H, W, ori=None):
    ori = ori or (H, W)
    return [dict(img_shape=(H, W, 3), ori_shape=(ori[0], ori[1], 3), pad_shape=(H, W, 3),
                 batch_input_shape=(H, W), scale_factor=1.0, flip=False) for _ in range(B)]


def train_batch(B, H, W, num_classes, max_inst=20, T=35, vocab=30522, seed=0, device='cpu', stuff_range=None):
    """COCO-shaped synthetic training batch: labels, rectangle/ellipse masks at image
    resolution, caption ids [101, tokens..., 102, 0...], noun ids."""
    g = torch.Generator().manual_seed(seed)
    out = dict(gt_bboxes=[], gt_labels=[], gt_masks=[], gt_caption_ids=[], gt_caption_mask=[],
               gt_caption_nouns_ids=[], gt_caption_nouns_mask=[])
    ys = torch.arange(H).view(H, 1).float()
    xs = torch.arange(W).view(1, W).float()
    for _ in range(B):
        n = int(torch.randint(1, max_inst + 1, (1,), generator=g))
        labels = torch.randint(0, num_classes, (n,), generator=g)
        masks = torch.zeros(n, H, W, dtype=torch.uint8)
        boxes = torch.zeros(n, 4)
        for i in range(n):
            cy, cx = (torch.rand(2, generator=g) * torch.tensor([H, W])).tolist()
            hh, ww = (torch.rand(2, generator=g) * torch.tensor([H / 3, W / 3]) + 4).tolist()
            if i % 2 == 0:
                m = ((ys - cy).abs() <= hh / 2) & ((xs - cx).abs() <= ww / 2)
            else:
                m = ((ys - cy) / (hh / 2))**2 + ((xs - cx) / (ww / 2))**2 <= 1
            masks[i] = m.to(torch.uint8)
            boxes[i] = torch.tensor([max(cx - ww / 2, 0), max(cy - hh / 2, 0), min(cx + ww / 2, W), min(cy + hh / 2, H)])
        Ltok = int(torch.randint(5, 21, (1,), generator=g))
        ids = torch.zeros(T, dtype=torch.long)
        ids[0] = 101
        ids[1:1 + Ltok] = torch.randint(min(1000, vocab // 2), vocab, (Ltok,), generator=g)
        ids[1 + Ltok] = 102
        cmask = (ids != 0).long()
        nn_ = int(torch.randint(1, 7, (1,), generator=g))
        nouns = torch.zeros(T, dtype=torch.long)
        nouns[:nn_] = ids[1:1 + nn_]
        out['gt_bboxes'].append(boxes.to(device))
        out['gt_labels'].append(labels.to(device))
        out['gt_masks'].append(masks.to(device))
        out['gt_caption_ids'].append(ids.to(device))
        out['gt_caption_mask'].append(cmask.to(device))
        out['gt_caption_nouns_ids'].append(nouns.to(device))
        out['gt_caption_nouns_mask'].append((nouns != 0).long().to(device))
    return out


def panoptic_sample(hw, num_things, num_stuff, seed=0, vocab=30522, rgb=None, blocks=(4, 5)):
    """One RAW panoptic sample as the dataset holds it before LoadOpenPanopticAnnotations (train_prep.py, rule 5): a uint8 BGR
    image, `pan_seg` = a block-structured id map (blocks[0] x blocks[1] rectangles at random cuts, one 24-bit id each, some >= 2^23;
    (h, w, 3) uint8 RGB when `rgb` -- by default for odd seeds -- else (h, w) int32), `segments` = the records in shuffled order:
    things, stuff (when num_stuff > 0), one crowd thing (a thing category with is_thing false) and two blocks whose ids NO record
    lists (they come out as 255), `gt_labels` = the categories of the is_thing records in record order, and the caption fields."""
    h, w = int(hw[0]), int(hw[1])
    r = np.random.default_rng(seed)
    gy, gx = min(blocks[0], h), min(blocks[1], w)
    ycut = np.concatenate([[0], np.sort(r.choice(np.arange(1, h), size=gy - 1, replace=False)), [h]]).astype(int)
    xcut = np.concatenate([[0], np.sort(r.choice(np.arange(1, w), size=gx - 1, replace=False)), [w]]).astype(int)
    nb = gy * gx
    ids = r.choice(2**24, size=nb, replace=False).astype(np.int64)
    ids[0] |= 2**23                                          # at least one id with the top bit of the blue byte
    ids = np.unique(ids)
    while ids.size < nb:
        ids = np.unique(np.concatenate([ids, r.integers(0, 2**24, size=nb - ids.size)]))
    ids = r.permutation(ids)
    pan = np.empty((h, w), dtype=np.int32)
    for k in range(nb):
        i, j = divmod(k, gx)
        pan[ycut[i]:ycut[i + 1], xcut[j]:xcut[j + 1]] = ids[k]
    order = r.permutation(nb)
    unlisted = set(order[:2].tolist()) if nb > 3 else set()
    crowd = int(order[2]) if nb > 3 else -1
    segments = []
    for k in r.permutation(nb).tolist():
        if k in unlisted:
            continue
        if k == crowd:
            segments.append(dict(id=int(ids[k]), category=int(r.integers(0, num_things)), is_thing=False))
        elif num_stuff > 0 and k % 3 == 0:
            segments.append(dict(id=int(ids[k]), category=int(num_things + r.integers(0, num_stuff)), is_thing=False))
        else:
            segments.append(dict(id=int(ids[k]), category=int(r.integers(0, num_things)), is_thing=True))
    labels = np.array([s['category'] for s in segments if s['is_thing']], dtype=np.int64)
    if rgb is None:
        rgb = bool(seed % 2)
    if rgb:
        pan = np.stack([pan & 255, (pan >> 8) & 255, (pan >> 16) & 255], axis=2).astype(np.uint8)
    cap = train_batch(1, 8, 8, num_classes=max(num_things, 1), max_inst=1, vocab=vocab, seed=seed)
    out = dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), pan_seg=pan, segments=segments, gt_labels=labels,
               filename=f'synthetic_panoptic_{seed}.jpg', ori_filename=f'synthetic_panoptic_{seed}.jpg')
    for k in ('gt_caption_ids', 'gt_caption_mask', 'gt_caption_nouns_ids', 'gt_caption_nouns_mask'):
        out[k] = cap[k][0].numpy()
    return out


def panoptic_samples(hw, num_things, num_stuff, seed=0, vocab=30522, blocks=(4, 5)):
    """Endless seeded stream of `panoptic_sample`s, the two id-map forms in turn."""
    i = 0
    while True:
        yield panoptic_sample(hw, num_things, num_stuff, seed=seed + i, vocab=vocab, blocks=blocks)
        i += 1


def _star_polygon(r, cy, cx, ry, rx, k):
    """a flat x0, y0, x1, y1, ... star-shaped polygon of k vertices around (cx, cy), radii jittered, coordinates with fractions"""
    ang = np.sort(r.uniform(0.0, 2.0 * np.pi, size=k))
    rad = r.uniform(0.55, 1.0, size=k)
    xy = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], axis=1)
    return np.round(xy, 2).reshape(-1).tolist()


def polygon_sample(hw, num_classes, seed=0, vocab=30522, extra=4, vertices=(6, 40)):
    """One RAW polygon sample as the dataset holds it before LoadOpenAnnotations(poly2mask=True) (train_prep.py, rule 6): a uint8 BGR
    image, `gt_polygons` = `ann_info['masks']` (per instance a list of parts, per part a flat x0, y0, x1, y1, ... list), `gt_labels`
    and the caption fields. The instances, in this order (`POLYGON_KINDS` names the first four): one of three parts; one that lies
    partly outside the image; one with a degenerate two-vertex part next to a proper one; one wholly outside the image, which no
    crop keeps; then `extra` star-shaped instances of 1 to 3 parts."""
    h, w = int(hw[0]), int(hw[1])
    r = np.random.default_rng(seed)

    def star(cy, cx, ry, rx):
        return _star_polygon(r, cy, cx, max(ry, 1.0), max(rx, 1.0), int(r.integers(vertices[0], vertices[1] + 1)))

    polys = [
        [star(r.uniform(0.2, 0.8) * h, r.uniform(0.2, 0.8) * w, 0.15 * h, 0.15 * w) for _ in range(3)],
        [star(r.uniform(0.3, 0.7) * h, w - 1.0, 0.3 * h, 0.3 * w)],
        [star(0.5 * h, 0.5 * w, 0.2 * h, 0.2 * w), [round(0.1 * w, 2), round(0.1 * h, 2), round(0.6 * w, 2), round(0.7 * h, 2)]],
        [star(0.5 * h, w + 0.4 * w + 8.0, 0.2 * h, 0.2 * w)],
    ]
    for _ in range(extra):
        polys.append([star(r.uniform(0.0, 1.0) * h, r.uniform(0.0, 1.0) * w, r.uniform(0.03, 0.3) * h, r.uniform(0.03, 0.3) * w)
                      for _ in range(int(r.integers(1, 4)))])
    labels = r.integers(0, max(num_classes, 1), size=len(polys)).astype(np.int64)
    cap = train_batch(1, 8, 8, num_classes=max(num_classes, 1), max_inst=1, vocab=vocab, seed=seed)
    out = dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), gt_polygons=polys, gt_labels=labels,
               filename=f'synthetic_polygons_{seed}.jpg', ori_filename=f'synthetic_polygons_{seed}.jpg')
    for k in ('gt_caption_ids', 'gt_caption_mask', 'gt_caption_nouns_ids', 'gt_caption_nouns_mask'):
        out[k] = cap[k][0].numpy()
    return out


POLYGON_KINDS = ('multi_part', 'partly_outside', 'two_vertex_part', 'never_kept')   # instances 0 .. 3 of every `polygon_sample`


def polygon_samples(hw, num_classes, seed=0, vocab=30522, extra=4, vertices=(6, 40)):
    """Endless seeded stream of `polygon_sample`s."""
    i = 0
    while True:
        yield polygon_sample(hw, num_classes, seed=seed + i, vocab=vocab, extra=extra, vertices=vertices)
        i += 1


def pq_ground_truth(hw, num_things, num_stuff, all_cat_ids=None, seed=0, rgb=None, blocks=(4, 5)):
    """Panoptic ground truth of one image as `pq_eval.PQEvaluator.add` (and `tools/test.py --eval PQ`, as the metas' `gt_pan_seg` /
    `gt_segments`) takes it, from `panoptic_sample`: (id map -- (h, w) int32 or (h, w, 3) uint8 RGB --, records id, category_id,
    iscrowd, area). all_cat_ids: label -> category id (default label + 1); the sample's crowd thing becomes iscrowd = 1, areas are
    pixel counts, two blocks keep ids that no record lists."""
    s = panoptic_sample(hw, num_things, num_stuff, seed=seed, rgb=rgb, blocks=blocks)
    pan = s['pan_seg']
    ids = pan if pan.ndim == 2 else pan[:, :, 0].astype(np.int32) + 256 * pan[:, :, 1].astype(np.int32) + 65536 * pan[:, :, 2].astype(np.int32)
    cats = list(range(1, num_things + num_stuff + 1)) if all_cat_ids is None else list(all_cat_ids)
    segments = [dict(id=r['id'], category_id=int(cats[r['category']]), iscrowd=int(r['category'] < num_things and not r['is_thing']),
                     area=int((ids == r['id']).sum())) for r in s['segments']]
    return pan, segments


CAPTION_WORDS = ('a', 'the', 'man', 'woman', 'dog', 'cat', 'horse', 'bus', 'street', 'beach', 'table', 'plate', 'red', 'white', 'two',
                 'on', 'in', 'near', 'with', 'rides', 'sits', 'stands', 'holds', 'and', 'of', 'food', 'kite', 'hill', 'field', 'snow')


def caption_ground_truth(seed, n, words=CAPTION_WORDS):
    """Caption ground truth of n images as `caption_eval.CaptionEvaluator.add` (and `tools/test.py --eval caption`, as the metas'
    `gt_captions`) takes it: per image a list of 1 .. 5 reference strings of 4 .. 10 words from a small word list, seeded. Every
    image's first reference starts with "a", so that one unigram has idf 0."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        refs = [' '.join(words[int(k)] for k in rs.randint(0, len(words), int(rs.randint(4, 11)))) for _ in range(int(rs.randint(1, 6)))]
        refs[0] = 'a ' + refs[0]
        out.append(refs)
    return out
