#!/usr/bin/env python
"""Minimal inference driver with the command line of the reference's tools/test.py: config + checkpoint -> detector from
the registry -> `simple_test` over a stream of images -> results pickle (`--out`), one process per GPU under
`--launcher pytorch` (images are sharded by rank, results gathered on rank 0). `--eval segm` computes COCO mask AP (and base /
novel / all AP50) on the device when the `--data` stream's metas carry ground truth (`cgg_amd.mask_eval.SegmEvaluator`), `--eval bbox`
(or `proposal`, which the reference runs as the same evaluation) COCO box AP from the results' boxes (`BboxEvaluator`), `--eval PQ`
panoptic quality over All / Known Things / Unknown Things / Stuff from the device maps and segment tables
(`cgg_amd.pq_eval.PQEvaluator`), `--eval caption` BLEU-1..4, CIDEr and ROUGE-L of the generated captions against the metas'
`gt_captions` (`cgg_amd.caption_eval.CaptionEvaluator`, the n-gram work on the device); the other metrics need the dataset classes,
which are out of this build's scope: they are accepted and reported as unavailable.

Both precision modes serve through `pipeline.StagePipeline` (hipGraph per stage, encode of batch k+1 overlapped with decode of
batch k): `--precision fp32` (default) is parity mode -- the reference's f32 semantics on the f32-class x3 kernels --,
`--precision bf16` the faster throughput mode (narrower than the reference's arithmetic).

    python tools/test.py CONFIG CHECKPOINT --out results.pkl --num-images 64 --synthetic 1024
"""
import argparse
import importlib
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

import cgg_amd              # noqa: E402,F401
from cgg_amd import registry, runtime, synthetic                          # noqa: E402
from cgg_amd.checkpoint import load_checkpoint                            # noqa: E402
from cgg_amd.config import Config, parse_option_value                     # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='test (and eval) a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help='checkpoint file ("none": keep the initialisation)')
    p.add_argument('--work-dir', help='the directory to save the metrics file')
    p.add_argument('--out', help='output result file in pickle format')
    p.add_argument('--fuse-conv-bn', action='store_true', help='accepted: the bf16 path always folds BN into the convs')
    p.add_argument('--gpu-id', type=int, default=0)
    p.add_argument('--eval', type=str, nargs='+',
                   help='evaluation metrics. segm: COCO mask AP of every result type the head returns, evaluated on the device from the '
                        'bit-packed masks; needs a --data stream whose metas carry gt_masks (n, h, w) and gt_labels (category ids) at the '
                        'original size (gt_crowd, gt_area optional), and sets --mask-bits. The config may hold segm_eval = dict(all_results='
                        '[category id per label], base_results=[...], novel_results=[...], unknown_cat_ids=[...], all_cat_ids=[...], '
                        'class_agnostic=False, max_dets=(100, 300, 1000)); a type without a list takes label + 1 as the category id. '
                        'bbox: COCO box AP of every result type, evaluated on the device from the results\' (n, 5) boxes; needs metas with '
                        'gt_boxes_xywh (n, 4) float64, the annotations\' own bbox at the original size, and gt_labels (gt_crowd, gt_area '
                        'optional); categories from segm_eval, as for segm; runs alone (no --mask-bits) or next to segm. proposal: the same '
                        'run under that name, as the reference\'s evaluate_det_segm maps it to bbox with unchanged parameters. '
                        'proposal_fast is refused: the reference\'s result files never hold it. '
                        'PQ (or pq): panoptic quality of panoptic_all_results, evaluated on the device from the id maps and segment tables '
                        '(sets with_segments); needs metas with gt_pan_seg ((h, w) int32 ids or (h, w, 3) uint8 RGB) and gt_segments '
                        '(records id, category_id, iscrowd, area) at the original size. The config may hold pq_eval = dict(all_cat_ids=[...], '
                        'isthing=[...], unknown_cat_ids=[...]); by default label + 1 and the first num_things_classes labels are things. '
                        'caption: BLEU-1..4, CIDEr and ROUGE-L (the reference\'s eval_cap_results) of every image\'s caption against the '
                        'reference strings in its meta\'s gt_captions (list of str), on raw whitespace tokens. Captions come from the '
                        'batched beam search, which reads a count on the host and cannot be captured into the staged pipeline: --eval '
                        'caption implies --no-pipeline (the eager route). Token ids are rendered by transformers.BertTokenizer, from '
                        '--caption-vocab or the local cache. Other metrics need the dataset classes: unavailable here')
    p.add_argument('--cfg-options', nargs='+', default=None, help='key=value overrides merged into the config')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none')
    p.add_argument('--local_rank', type=int, default=0)
    # this build's additions
    p.add_argument('--num-images', type=int, default=16)
    p.add_argument('--samples-per-gpu', type=int, default=2)
    p.add_argument('--synthetic', type=int, default=1024, help='synthetic image size (H = W) when --data is not given')
    p.add_argument('--data', default=None,
                   help='pkg.module:function(cfg, rank, world) -> iterable of (img (3,H,W) float tensor, img_meta) -- already resized, '
                        'normalised and padded --, or of raw (h,w,3) uint8 BGR arrays / tensors (alone, or with a dict of extra meta '
                        'keys such as filename): those are prepared on the device by the config\'s data.test.pipeline')
    p.add_argument('--synthetic-u8', default=None, metavar='HxW',
                   help='synthetic raw uint8 frames of this size (e.g. 480x640) instead of --synthetic\'s prepared float tensors: '
                        'exercises the device-side test pipeline without a dataset')
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='fp32 = parity mode: every contraction in f32-class f16 x 3 arithmetic (as accurate as f32 GEMMs; activations '
                        'must satisfy |a| < 4094 -- the run fails loudly otherwise, CGG_X3=0 lifts the limit); bf16 = throughput mode')
    p.add_argument('--no-pipeline', action='store_true', help='plain sequential simple_test (no graphs / overlap)')
    p.add_argument('--rle', action='store_true',
                   help='results in the evaluation format: masks as COCO RLE dicts (what results2json builds with pycocotools from '
                        'the reference\'s arrays), from bit-packed device masks through pinned staging buffers, one asynchronous '
                        'copy per tensor and the C++ host encoder of the extension, overlapped with the next batch')
    p.add_argument('--rle-device', action='store_true',
                   help='--rle with the run boundaries found on the device (RleCollector(device_rle=True)): per mask a few hundred '
                        '4-byte positions cross PCIe instead of its bit plane, and the host only writes the counts strings. Same results')
    p.add_argument('--mask-bits', action='store_true',
                   help='keep the masks bit-packed ((n, H, W / 8) uint8, pixel x = bit x & 7 of byte x >> 3) in the results: '
                        '8x less PCIe traffic and 8x smaller result files; unpacking 315 MB of bool masks per 1024^2 image on '
                        'the host costs more than the copy it saves (28 vs 36 images/s end to end), so it is opt-in')
    p.add_argument('--show', action='store_true', help='paints like --show-dir, into work_dirs/show when no --show-dir is given (no window is opened)')
    p.add_argument('--show-dir', default=None,
                   help='directory where every image of the run is written with its result painted over it (model.show_result on the '
                        'device results the run already holds): DIR/<base name of ori_filename, or index>.png (a base name met before gets _<index> appended). Needs raw uint8 images')
    p.add_argument('--show-score-thr', type=float, default=0.3, help='score threshold of --show-dir (default 0.3)')
    p.add_argument('--caption-vocab', default=None, metavar='VOCAB.TXT',
                   help='--eval caption: the BERT vocabulary file (one token per line) that renders the generated ids; without it the '
                        'locally cached bert-base-uncased tokenizer is used (nothing is downloaded), and the run ends if there is none')
    p.add_argument('--synthetic-captions', action='store_true',
                   help='attach seeded reference captions (synthetic.caption_ground_truth) as gt_captions to the metas of the '
                        'synthetic streams (--synthetic / --synthetic-u8): exercises --eval caption without a dataset')
    args = p.parse_args(argv)
    os.environ.setdefault('LOCAL_RANK', str(args.local_rank))
    return args


def synthetic_images(n, size, seed, pool=4):
    """n images from a pool of `pool` distinct pinned N(0, 1) tensors (drawing 3 x 1024^2 normals on the host costs 20 ms,
    which would make this generator -- not the detector -- the serving bottleneck)."""
    g = torch.Generator().manual_seed(seed)
    meta = synthetic.img_metas(1, size, size)[0]
    imgs = [torch.randn(3, size, size, generator=g) for _ in range(min(pool, n))]
    if torch.cuda.is_available():
        imgs = [t.pin_memory() for t in imgs]
    for i in range(n):
        yield imgs[i % len(imgs)], dict(meta, filename=f'synthetic_{i}.jpg')


def synthetic_u8_images(n, hw, seed, pool=4):
    """n raw (h, w, 3) uint8 frames from a pool of `pool` distinct pinned tensors, as `synthetic_images` does for float batches."""
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randint(0, 256, (hw[0], hw[1], 3), dtype=torch.uint8, generator=g) for _ in range(min(pool, n))]
    if torch.cuda.is_available():
        imgs = [t.pin_memory() for t in imgs]
    for i in range(n):
        yield imgs[i % len(imgs)], dict(filename=f'synthetic_{i}.jpg')


def is_raw_u8(img):
    """a raw (h, w, 3) uint8 image, as opposed to the prepared (3, H, W) float tensor"""
    u8 = img.dtype == torch.uint8 if torch.is_tensor(img) else isinstance(img, np.ndarray) and img.dtype == np.uint8
    return bool(u8) and img.ndim == 3 and img.shape[2] == 3


def to_numpy(result):
    """device results {type: (labels, bboxes (n,5), masks)} -> numpy, one copy per tensor (masks: (n, H, W) bool, or
    (n, H, W / 8) uint8 with --mask-bits)."""
    out = {}
    for key, val in result.items():
        if isinstance(val, dict):          # panoptic_segments: the segment table block {n_kept, table, scores}
            out[key] = {k: v.detach().cpu().numpy() if torch.is_tensor(v) else v for k, v in val.items()}
            continue
        out[key] = tuple(v.detach().cpu().numpy() if torch.is_tensor(v) else v for v in val) \
            if isinstance(val, (tuple, list)) else (val.detach().cpu().numpy() if torch.is_tensor(val) else val)
    return out


def interleave_rank_results(parts):
    """Per-rank result lists (image i was served by rank i % world) -> one list in dataset order: what [3P] mmcv
    `collect_results` does with `zip(*part_list)` (reference tools/test.py -> apis/test.py:79-130), without its
    padding duplicates because the shards here are not padded to equal length."""
    world = len(parts)
    total = sum(len(p) for p in parts)
    out = []
    for i in range(total + world):
        r, j = i % world, i // world
        if j < len(parts[r]):
            out.append(parts[r][j])
    return out[:total]


def coco_evaluator(cls, cfg, model, key, device=None):
    """the SegmEvaluator / BboxEvaluator (`cls`) of result type `key`: categories and options from the config entry segm_eval"""
    opts = dict(cfg.get('segm_eval') or {})
    n_cls = getattr(model.panoptic_fusion_head, key.replace('_results', '_classes'), None) or model.num_classes
    agnostic = bool(opts.get('class_agnostic', False))
    return cls(opts.get(key) or list(range(1, int(n_cls) + 1)), opts.get('unknown_cat_ids'), opts.get('all_cat_ids'),
               max_dets=tuple(opts.get('max_dets', (100, 300, 1000))), class_agnostic=agnostic, device=device,
               skip_images_without_gt=device is not None and not agnostic)


def segm_summary(cfg, model, evaluators, eval_records, device, work_dir, metric='segm'):
    """--eval segm / bbox on rank 0: accumulate every type's image records (this rank's and the gathered ones), print the summary and
    write it to WORK_DIR/segm_eval.json / bbox_eval.json. Without ground truth in the stream nothing was recorded: today's message.
    `metric` is the name the run was asked for (segm, bbox or proposal; proposal writes bbox_eval.json)."""
    from cgg_amd.mask_eval import BboxEvaluator, SegmEvaluator, format_summary
    boxes = metric != 'segm'
    if not eval_records:
        print(f'--eval {metric}: the stream carries no ground truth (metas with {"gt_boxes_xywh" if boxes else "gt_masks"} and gt_labels '
              'come from a --data stream); dataset classes / COCO evaluation are outside this build', flush=True)
        return None
    summary = {}
    for key in sorted(eval_records):
        ev = evaluators.get(key)
        if ev is None:                  # a type only other ranks saw: the same evaluator, without records of its own
            ev = coco_evaluator(BboxEvaluator if boxes else SegmEvaluator, cfg, model, key)
        ev.records = list(eval_records[key])
        res = ev.summarize()
        print(format_summary(key, res, metric), flush=True)
        summary[key] = dict(images=res['images'], stats=res['stats'], base_ap50=res['base_ap50'], novel_ap50=res['novel_ap50'],
                            all_ap50=res['all_ap50'])
    if work_dir:
        os.makedirs(work_dir, exist_ok=True)
        with open(os.path.join(work_dir, 'bbox_eval.json' if boxes else 'segm_eval.json'), 'w') as f:
            json.dump(summary, f, indent=1)
    return summary


def pq_evaluator(cfg, model, device=None):
    """the PQEvaluator of a run: categories from the config entry pq_eval, by default ids 1..n with the first num_things_classes things"""
    from cgg_amd.pq_eval import PQEvaluator
    fh = model.panoptic_fusion_head
    opts = dict(cfg.get('pq_eval') or {})
    n = int(fh.num_classes)
    return PQEvaluator(opts.get('all_cat_ids') or list(range(1, n + 1)),
                       opts.get('isthing') or [int(k < int(fh.num_things_classes)) for k in range(n)],
                       opts.get('unknown_cat_ids'), num_classes=n, device=device)


def pq_summary(cfg, model, records, work_dir):
    """--eval PQ on rank 0: accumulate the image records (of all ranks, in image order), print the table and the twelve numbers and
    write them to WORK_DIR/pq_eval.json. Without ground truth in the stream nothing was recorded: a message."""
    from cgg_amd.pq_eval import format_pq_summary
    if not records:
        print('--eval PQ: the stream carries no ground truth (metas with gt_pan_seg and gt_segments come from a --data stream); dataset '
              'classes / COCO evaluation are outside this build', flush=True)
        return None
    res = pq_evaluator(cfg, model).summarize(extra_records=records)
    print(format_pq_summary(res['pq_results']), flush=True)
    print('PQ_copypaste: ' + res['results']['PQ_copypaste'], flush=True)
    summary = dict(images=res['images'], results=res['results'],
                   splits={k: v for k, v in res['pq_results'].items() if k != 'classwise'},
                   classwise={str(k): v for k, v in res['pq_results']['classwise'].items()},
                   stats={str(k): dict(tp=v['tp'], fp=v['fp'], fn=v['fn'], iou=float(v['iou'])) for k, v in sorted(res['stats'].items())})
    if work_dir:
        os.makedirs(work_dir, exist_ok=True)
        with open(os.path.join(work_dir, 'pq_eval.json'), 'w') as f:
            json.dump(summary, f, indent=1)
    return summary


def caption_tokenizer(vocab=None):
    """--eval caption: the transformers.BertTokenizer that renders token ids, from a vocabulary file or else from the local cache"""
    try:
        import transformers
    except ImportError:
        raise SystemExit('--eval caption: the generated ids are rendered by transformers.BertTokenizer, and transformers is not importable')
    if vocab:
        if not os.path.isfile(vocab):
            raise SystemExit(f'--caption-vocab {vocab}: no such file')
        return transformers.BertTokenizer(vocab)
    try:
        return transformers.BertTokenizer.from_pretrained('bert-base-uncased', local_files_only=True)
    except Exception:
        raise SystemExit('--eval caption: no bert-base-uncased vocabulary in the local cache; give --caption-vocab VOCAB.TXT')


def caption_summary(records, device, work_dir):
    """--eval caption on rank 0: score the (hypothesis, references) records of all ranks, in image order, print the reference's lines
    and write the six numbers to WORK_DIR/caption_eval.json. Without gt_captions in the stream nothing was recorded: a message."""
    from cgg_amd.caption_eval import SCORE_NAMES, CaptionEvaluator, format_caption_summary
    if not records:
        print('--eval caption: the stream carries no ground truth (metas with gt_captions come from a --data stream, or from '
              '--synthetic-captions); dataset classes / COCO evaluation are outside this build', flush=True)
        return None
    res = CaptionEvaluator(device=device).summarize(extra_records=records)
    print(format_caption_summary(res), flush=True)
    summary = dict(images=res['images'], route=res['route'], **{k: res[k] for k in SCORE_NAMES})
    if work_dir:
        os.makedirs(work_dir, exist_ok=True)
        with open(os.path.join(work_dir, 'caption_eval.json'), 'w') as f:
            json.dump(summary, f, indent=1)
    return summary


def _test_stages():
    """CGG_TEST_STAGES (pipeline stage split of the serving loop): validated up front, 2..5 as `pipeline.detector_pipeline` names them
    (4 and 5 add a separate post-processing stage to the 2- / 3-stage split)."""
    v = os.environ.get('CGG_TEST_STAGES', '3')
    if v not in ('2', '3', '4', '5'):
        raise SystemExit(f'CGG_TEST_STAGES={v!r}: expected 2, 3, 4 or 5')
    return int(v)


def main(argv=None):
    args = parse_args(argv)
    if args.eval and 'proposal_fast' in args.eval:
        # the reference's allow-list admits the name, and its evaluate_det_segm then raises KeyError('proposal_fast is not in results')
        raise SystemExit('--eval proposal_fast: the reference\'s result files hold bbox, proposal and segm, never proposal_fast (its '
                         'evaluate_det_segm raises KeyError for it); use bbox or proposal')
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict({k: parse_option_value(v) for k, v in (kv.split('=', 1) for kv in args.cfg_options)})
    distributed = args.launcher == 'pytorch'
    if distributed:
        import torch.distributed as dist
        local = int(os.environ['LOCAL_RANK'])
        torch.cuda.set_device(local)
        dist.init_process_group(backend='nccl')
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        local, rank, world = args.gpu_id, 0, 1
        torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    model = registry.build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
    meta = {}
    if args.checkpoint and args.checkpoint.lower() != 'none':
        meta = load_checkpoint(model, args.checkpoint, map_location='cpu').get('meta', {})
    if 'CLASSES' in meta:
        model.CLASSES = meta['CLASSES']
    model = model.to(device).eval()
    eval_segm = bool(args.eval) and 'segm' in args.eval
    eval_pq = bool(args.eval) and any(m in ('PQ', 'pq') for m in args.eval)        # ('pq' is regarded as 'PQ', as in the reference)
    # --eval bbox / proposal: one box evaluation per name asked for (the reference runs proposal as bbox with unchanged parameters)
    box_metrics = [m for m in ('bbox', 'proposal') if args.eval and m in args.eval]
    eval_caption = bool(args.eval) and 'caption' in args.eval
    if args.eval and [m for m in args.eval if m not in ('segm', 'bbox', 'proposal', 'PQ', 'pq', 'caption')]:
        print('--eval: dataset classes / COCO evaluation are outside this build; results are written with --out', flush=True)
    if eval_segm:
        args.mask_bits = True
    eval_any = eval_segm or eval_pq or bool(box_metrics) or eval_caption
    decode_kwargs = dict(with_segments=True) if eval_pq else {}        # --eval PQ reads the device segment table
    cap_records = []                   # --eval caption: per image of this rank, in order: (hypothesis, references) or None
    if eval_caption:
        if not getattr(model.panoptic_head, 'use_caption_generation', False):
            raise SystemExit('--eval caption: the config\'s head has no caption generator (use_caption_generation)')
        # the batched beam search reads the count of finished images on the host: it cannot be captured, so this is the eager route
        args.no_pipeline = True
        decode_kwargs.update(with_caption=True, caption_batched=True, keep_captions=True,
                             caption_tokenizer=caption_tokenizer(args.caption_vocab))
    pq = [None]                        # --eval PQ: the PQEvaluator, made when the first ground truth arrives
    pq_slots = []                      # per image of this rank, in order: the index of its record in the evaluator, or None
    evaluators = {}                    # --eval segm: result type -> SegmEvaluator, made when the first ground truth arrives
    box_evaluators = {}                # --eval bbox / proposal: result type -> BboxEvaluator, likewise
    eval_metas = []                    # per submitted batch, in submission order: the metas of its images
    evaluated = [None]                 # event after the newest batch's evaluator launches

    def with_captions(samples):
        """--synthetic-captions: seeded reference captions as the metas' gt_captions, by image index"""
        if not args.synthetic_captions:
            return samples
        caps = synthetic.caption_ground_truth(11, args.num_images)
        return ((img, dict(meta, gt_captions=caps[i])) for i, (img, meta) in enumerate(samples))

    if args.data:
        mod, fn = args.data.split(':')
        stream = getattr(importlib.import_module(mod), fn)(cfg, rank, world)
    elif args.synthetic_u8:
        try:
            hw = tuple(int(v) for v in args.synthetic_u8.lower().split('x'))
            assert len(hw) == 2 and min(hw) >= 1
        except (ValueError, AssertionError):
            raise SystemExit(f'--synthetic-u8 {args.synthetic_u8!r}: expected HxW, e.g. 480x640')
        stream = (s for i, s in enumerate(with_captions(synthetic_u8_images(args.num_images, hw, seed=11))) if i % world == rank)
    else:
        stream = (s for i, s in enumerate(with_captions(synthetic_images(args.num_images, args.synthetic, seed=11))) if i % world == rank)

    B = args.samples_per_gpu
    collector, in_copy = None, []
    if args.rle_device:
        args.rle = True
    if args.rle:
        from cgg_amd.host_results import RleCollector, fusion_class_counts
        args.mask_bits = True
        collector = RleCollector(device, fusion_class_counts(model.panoptic_fusion_head), device_rle=args.rle_device)

    show_dir = args.show_dir or (os.path.join('work_dirs', 'show') if args.show else None)
    shown = []                         # per submitted batch, in submission order: its raw images and their file names
    n_shown = 0
    shown_names = set()

    def paint(device_results):
        """--show-dir: the batch's images with their results painted over them, from the device results (masks are not copied)"""
        nonlocal n_shown
        frames = shown.pop(0)
        for (raw, name), res in zip(frames, device_results):
            index = n_shown * world + rank
            stem = os.path.splitext(os.path.basename(name))[0] if name else str(index)
            if stem in shown_names:        # the same base name from another directory (or a repeated name): keep both files
                stem = f'{stem}_{index}'
            shown_names.add(stem)
            model.show_result(raw, res, score_thr=args.show_score_thr, out_file=os.path.join(show_dir, stem + '.png'))
            n_shown += 1

    def evaluate(device_results):
        """--eval segm: every image's result of each type the head returns goes to that type's evaluator (masks stay on the device);
        --eval PQ: its panoptic map and segment table go to the PQEvaluator"""
        from cgg_amd.mask_eval import BboxEvaluator, SegmEvaluator
        for m, res in zip(eval_metas.pop(0), device_results):
            if eval_caption:
                # --eval caption: the image's rendered caption and its reference strings; scored at the end (CIDEr's document
                # frequencies span the corpus)
                refs, cap = m.get('gt_captions'), res.get('cap_results')
                cap_records.append((cap, [str(r) for r in refs]) if refs and isinstance(cap, str) else None)
            if eval_pq:
                # --eval PQ: the image's panoptic map and segment table go to the PQEvaluator (both stay on the device)
                pan = res.get('panoptic_all_results', res.get('pan_results'))
                if m.get('gt_pan_seg') is None or m.get('gt_segments') is None or pan is None or res.get('panoptic_segments') is None:
                    pq_slots.append(None)
                else:
                    if pq[0] is None:
                        pq[0] = pq_evaluator(cfg, model, device)
                    pq_slots.append(len(pq[0].records))
                    pq[0].add(pan, res['panoptic_segments'], m['gt_pan_seg'], m['gt_segments'])
            with_masks = eval_segm and m.get('gt_masks') is not None and m.get('gt_labels') is not None
            with_boxes = bool(box_metrics) and m.get('gt_boxes_xywh') is not None and m.get('gt_labels') is not None
            if not (with_masks or with_boxes):
                continue
            for key, val in res.items():
                if not (key.endswith('_results') and isinstance(val, (tuple, list)) and len(val) == 3):
                    continue
                if with_masks:
                    if key not in evaluators:
                        evaluators[key] = coco_evaluator(SegmEvaluator, cfg, model, key, device)
                    evaluators[key].add(val[0], val[1], val[2], m['gt_masks'], m['gt_labels'], m.get('gt_crowd'), m.get('gt_area'))
                if with_boxes:
                    # (gt_area is the annotation's own area: the masks' for a dataset that has them, the box's w * h when None)
                    if key not in box_evaluators:
                        box_evaluators[key] = coco_evaluator(BboxEvaluator, cfg, model, key, device)
                    box_evaluators[key].add(val[0], val[1], m['gt_boxes_xywh'], m['gt_labels'], m.get('gt_crowd'), m.get('gt_area'))

    def emit(device_results):
        """device results of one batch -> `results` (numpy now, or a future of the RLE collector)"""
        if eval_any:
            evaluate(device_results)
            # the evaluator's kernels read the result buffers on THIS stream: the pipeline's last stage waits for them before it
            # writes a slot again (a wait on the GPU; without the RLE collector the copies below end in a host wait anyway)
            evaluated[0] = torch.cuda.Event()
            evaluated[0].record()
        if show_dir is not None:
            paint(device_results)
        if collector is None:
            results.extend(to_numpy(r) for r in device_results)
        else:
            fut = collector.submit(device_results)
            results.append(fut)
            in_copy.append(fut)

    def copies_done(keep=0):
        """host-side wait until all but the `keep` newest batches have been copied out of their device buffers"""
        while len(in_copy) > keep:
            RleCollector.wait_copied(in_copy.pop(0))

    prep = None                        # device-side test pipeline, built when the stream yields its first raw uint8 image

    def image_prep():
        nonlocal prep
        if prep is None:
            from cgg_amd.image_prep import ImagePrep, parse_test_pipeline
            try:
                pipeline = cfg.data.test.pipeline
            except (AttributeError, KeyError):
                raise SystemExit('tools/test.py: raw uint8 images need the config\'s data.test.pipeline (Resize / Pad / Normalize)')
            prep = ImagePrep(parse_test_pipeline(pipeline), device)
        return prep

    results, pending = [], []          # pending: (pipeline, slot) pairs -- a slot is only meaningful for ITS pipeline
    slot_copied = {}                   # (pipeline, slot) -> event: that slot's last results have been copied to the host
    n_img, t0 = 0, None
    pipe = None
    with torch.no_grad(), runtime.precision_scope(args.precision):
        group = []

        def drain():
            """copy out every batch still in flight, in submission order, from the pipeline that produced it"""
            while pending:
                owner, slot = pending.pop(0)
                emit(owner.wait(slot))

        def run(group):
            nonlocal pipe, t0, n_img
            raw = [g[0] for g in group] if is_raw_u8(group[0][0]) else None
            if show_dir is not None:
                if raw is None:
                    raise SystemExit('tools/test.py: --show-dir paints over the raw uint8 images (--synthetic-u8, or a --data stream of '
                                     'them); prepared float tensors cannot be shown')
                shown.append([(g[0], (g[1] or {}).get('ori_filename', (g[1] or {}).get('filename'))) for g in group])
            if raw is not None:
                # raw uint8 images: resized, padded, normalised and collated by ONE kernel (cgg_amd.image_prep), which is launched
                # below -- into the pipeline's own input buffer when a captured pipeline serves this batch
                shape, metas = image_prep().describe(raw)
                metas = [dict(m, **(g[1] or {}), batch_input_shape=tuple(shape[-2:])) for m, g in zip(metas, group)]
                imgs = None
            else:
                # straight into a device batch (pinned sources copy asynchronously; torch.stack would build a pageable staging tensor)
                imgs = torch.empty((len(group),) + tuple(group[0][0].shape), dtype=group[0][0].dtype, device=device)
                for k, g in enumerate(group):
                    imgs[k].copy_(g[0], non_blocking=True)
                metas = [dict(g[1], batch_input_shape=tuple(imgs.shape[-2:])) for g in group]
                shape = tuple(imgs.shape)
            if eval_any:
                eval_metas.append(metas)
            use_pipe = (not args.no_pipeline and len(group) == B
                        and all(m['img_shape'] == metas[0]['img_shape'] and m['ori_shape'] == metas[0]['ori_shape'] for m in metas))
            if use_pipe:
                key = (tuple(shape), metas[0]['img_shape'], metas[0]['ori_shape'])
                if pipe is None or pipe.meta_key != key:
                    drain()            # the old pipeline's results leave before its buffers are dropped
                    pipe = pipes.get(key)
                    if pipe is None:
                        from cgg_amd.pipeline import detector_pipeline
                        if imgs is None:
                            imgs = image_prep()(raw)[0]        # the example batch the graphs are captured on
                        pipe = detector_pipeline(model, imgs, metas, stages=_test_stages(), defer_tail=False, rescale=True, device_results=True, mask_bits=args.mask_bits, **decode_kwargs)
                        pipe.meta_key = key
                        pipes[key] = pipe
                        torch.cuda.synchronize()
                    if t0 is None:
                        t0, n_img = time.perf_counter(), 0
                depth = len(pipe.stages) - 1       # batches that may stay in flight behind the one being submitted
                if collector is not None:
                    copies_done(keep=depth + 1)    # bounds the pinned staging in use; ordering is enforced on the GPU below
                    # the slot this submit reuses: its previous batch's device->host copies must have left before the LAST stage
                    # overwrites the result buffers -- a GPU-side wait on that stage's stream, not a host wait
                    ev = slot_copied.pop((id(pipe), pipe._n % pipe.slots), None)
                    if ev is not None:
                        pipe.streams[-1].wait_event(ev)
                if evaluated[0] is not None:
                    pipe.streams[-1].wait_event(evaluated[0])
                if imgs is None:
                    # the kernel writes the static input of the slot this submit takes, once stage 0 of the slot's previous batch
                    # has read it (a wait on the GPU; an event that was never recorded does not wait)
                    s_in = pipe._n % pipe.slots
                    torch.cuda.current_stream(device).wait_event(pipe.done[0][s_in])
                    imgs = image_prep()(raw, out=pipe.inputs[s_in])[0]
                slot = pipe.submit(imgs)
                # `imgs` was filled on this stream but is READ by stage 0 on the pipeline's first stream, after `run` has dropped
                # its reference: without this the caching allocator may hand the block to the next batch's host->device copy
                # while stage 0 has not copied the previous batch yet (batch k served with batch k + 1's pixels)
                if imgs is not pipe.inputs[slot]:      # (a raw batch was written into the pipeline's own persistent input)
                    imgs.record_stream(pipe.streams[0])
                pending.append((pipe, slot))
                # results of the batch `depth` submits back are copied out while the newer ones run
                while len(pending) > depth:
                    owner, old_slot = pending.pop(0)
                    emit(owner.wait(old_slot))
                    if collector is not None:
                        slot_copied[(id(owner), old_slot)] = in_copy[-1].copied
            else:
                drain()                # keep dataset order: earlier batches first
                if t0 is None:
                    t0 = time.perf_counter()
                if imgs is None:
                    imgs = image_prep()(raw)[0]
                emit(model.simple_test(imgs, metas, rescale=True, device_results=True, mask_bits=args.mask_bits, **decode_kwargs))
                if collector is not None:
                    copies_done()
            n_img += len(group)

        pipes = {}                     # one captured pipeline per (batch shape, img_shape, ori_shape)

        def shape_key(sample):
            """what the images of one batch share: the prepared tensor's shape, or a raw image's padded shape"""
            if is_raw_u8(sample[0]):
                from cgg_amd.image_prep import image_geometry
                return ('u8',) + image_geometry(sample[0].shape[:2], image_prep().spec)[2:]
            return tuple(sample[0].shape)

        for sample in stream:
            if is_raw_u8(sample):
                sample = (sample, None)        # a raw image without extra meta keys
            # a batch holds images of ONE padded shape (the reference pads a batch to its largest image through the
            # dataset's collate; this driver takes pre-sized tensors and starts a new batch when the shape changes)
            if group and shape_key(sample) != shape_key(group[0]):
                run(group)
                group = []
            group.append(sample)
            if len(group) == B:
                run(group)
                group = []
        if group:
            run(group)                 # trailing short batch: sequential path (len(group) != B)
        drain()
        torch.cuda.synchronize()
        # parity mode stores its GEMM-consumed activations as f16 x 3 pieces of 16 a: a value with |a| >= 4094 (an un-normalised
        # input, a checkpoint with one huge BN-folded scale) becomes inf / NaN. Every producer raises a device flag; ONE read at
        # the end of the run turns it into an error instead of silently wrong masks (the f32 reference has no such limit)
        if args.precision == 'fp32' and runtime.x3a_enabled():
            from cgg_amd import ops
            if ops.x3_overflow_check(device):
                raise SystemExit('tools/test.py: an activation left the f16 x 3 range of parity mode (|a| >= 4094): results may hold '
                                 'inf / NaN. Re-run with CGG_X3=0 (f32 library path, no range limit).')
        if collector is not None:          # futures -> host results, in submission (= dataset) order
            flat = []
            for r in results:
                flat.extend(r.result())
            results = flat
            collector.close()
    dt = time.perf_counter() - (t0 or time.perf_counter())
    eval_records = {key: ev.image_records() for key, ev in evaluators.items()}     # per image a few KB of match records, no masks
    box_records = {key: ev.image_records() for key, ev in box_evaluators.items()}
    pq_records = []                    # --eval PQ: per image of this rank its record (a few hundred bytes) or None
    if eval_pq:
        recs = pq[0].image_records() if pq[0] is not None else []
        pq_records = [None if k is None else recs[k] for k in pq_slots]
    if distributed:
        import torch.distributed as dist
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(results, gathered, dst=0)
        if rank == 0:
            results = interleave_rank_results(gathered)
        if eval_segm:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(eval_records, parts, dst=0)
            if rank == 0:
                for part in parts[1:]:
                    for key, recs in part.items():
                        eval_records.setdefault(key, []).extend(recs)
        if box_metrics:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(box_records, parts, dst=0)
            if rank == 0:
                for part in parts[1:]:
                    for key, recs in part.items():
                        box_records.setdefault(key, []).extend(recs)
        if eval_pq:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(pq_records, parts, dst=0)
            if rank == 0:
                pq_records = interleave_rank_results(parts)        # image order: the float sums do not depend on the number of ranks
        if eval_caption:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(cap_records, parts, dst=0)
            if rank == 0:
                cap_records = interleave_rank_results(parts)       # image order, as for PQ
        dist.destroy_process_group()
    if eval_segm and rank == 0:
        segm_summary(cfg, model, evaluators, eval_records, device, args.work_dir)
    if rank == 0:
        for metric in box_metrics:
            segm_summary(cfg, model, box_evaluators, box_records, device, args.work_dir, metric=metric)
    if eval_pq and rank == 0:
        pq_summary(cfg, model, [r for r in pq_records if r is not None], args.work_dir)
    if eval_caption and rank == 0:
        caption_summary([r for r in cap_records if r is not None], device, args.work_dir)
    if rank == 0:
        print(json.dumps(dict(images=len(results), images_per_sec_this_rank=round(n_img / max(dt, 1e-9), 1),
                              precision=args.precision, pipeline=pipe is not None,
                              results='coco-rle' if args.rle else ('bit-packed' if args.mask_bits else 'bool arrays'))), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'wb') as f:
                pickle.dump(results, f)
    return results


if __name__ == '__main__':
    main()
