"""The reference's demo entry points ([3P] mmdet.apis.init_detector / inference_detector, which the headline call
`inference_detector(model, img, with_caption=True)` goes through), with the test pipeline run on the device (image_prep.py).

    model = init_detector('configs/instance/coco_b48n17.py', 'cgg.pth', device='cuda:0')
    result = inference_detector(model, bgr_uint8_image, with_caption=True)
    show_result_pyplot(model, bgr_uint8_image, result, score_thr=0.95)
"""
import numpy as np
import torch

from ._lib import CggError
from .checkpoint import load_checkpoint
from .config import Config, parse_option_value
from .image_prep import ImagePrep, parse_test_pipeline
from .registry import build_detector


def init_detector(config, checkpoint=None, device='cuda:0', cfg_options=None):
    """config: a `Config` or the path of a reference-style config file; checkpoint: a path (or a loaded checkpoint dict), None keeps
    the initialisation. Returns the detector in eval mode on `device`, with `.cfg` (read by `inference_detector`) and, when the
    checkpoint's meta has them, `.CLASSES`."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError(f'config must be a filename or Config object, but got {type(config)}')
    if cfg_options is not None:
        config.merge_from_dict({k: parse_option_value(v) if isinstance(v, str) else v for k, v in cfg_options.items()})
    model_cfg = config.model
    if 'pretrained' in model_cfg:
        model_cfg['pretrained'] = None
    model = build_detector(model_cfg, test_cfg=config.get('test_cfg'))
    if checkpoint is not None:
        meta = load_checkpoint(model, checkpoint, map_location='cpu').get('meta', {})
        if 'CLASSES' in meta:
            model.CLASSES = meta['CLASSES']
    model.cfg = config
    return model.to(device).eval()


def _read_image(path):
    """file -> (h, w, 3) uint8 BGR. JPEG decoders differ in their last bit, so decoding is outside the parity claim."""
    try:
        from PIL import Image
    except ImportError:
        raise CggError(f'inference_detector: reading {path!r} needs PIL, which is not importable here; pass the decoded image '
                       '((h, w, 3) uint8, BGR) instead')
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _prep_of(model):
    """the model's cached ImagePrep; rebuilt when the model has moved or its cfg's test pipeline no longer parses to the same spec"""
    cfg = getattr(model, 'cfg', None)
    if cfg is None:
        raise CggError('inference_detector: the model has no .cfg (build it with init_detector, or set model.cfg to a Config with '
                       'data.test.pipeline)')
    spec = parse_test_pipeline(cfg.data.test.pipeline)
    prep = getattr(model, '_image_prep', None)
    device = next(model.parameters()).device
    if prep is None or prep.device != device or prep.spec != spec:
        prep = model._image_prep = ImagePrep(spec, device)
    return prep


def inference_detector(model, imgs, **kwargs):
    """One image or a list / tuple of them -> one result or a list, as the reference. An image is an (h, w, 3) uint8 array or tensor
    (CPU or device) in BGR channel order -- what cv2.imread and the reference's loaders produce -- or a file name, which is decoded
    with PIL and flipped to BGR (file decoding is outside the parity claim: JPEG decoders differ). The images are resized, padded,
    normalised and collated on the device by the config's test pipeline (`ImagePrep`), then
    `model(img=[batch], img_metas=[metas], return_loss=False, rescale=True, **kwargs)` runs under `torch.no_grad()`;
    `with_caption=True`, `device_results`, `mask_bits` and any other keyword reach `simple_test` untouched."""
    is_batch = isinstance(imgs, (list, tuple))
    if not is_batch:
        imgs = [imgs]
    names = [i if isinstance(i, str) else None for i in imgs]
    arrays = [_read_image(i) if isinstance(i, str) else i for i in imgs]
    batch, metas = _prep_of(model)(arrays)
    for m, name in zip(metas, names):
        if name is not None:
            m['filename'] = m['ori_filename'] = name
    with torch.no_grad():
        results = model(img=[batch], img_metas=[metas], return_loss=False, rescale=True, **kwargs)
    return results if is_batch else results[0]


def show_result_pyplot(model, img, result, score_thr=0.3, title='result', wait_time=0, palette=None, out_file=None):
    """[3P] mmdet.apis.show_result_pyplot, the last line of the reference's demo: `model.show_result` with one `palette` for boxes,
    text and masks, shown in a matplotlib window titled `title` -- or written to `out_file` (then no window is opened)."""
    if hasattr(model, 'module'):
        model = model.module
    return model.show_result(img, result, score_thr=score_thr, show=True, wait_time=wait_time, win_name=title, bbox_color=palette,
                             text_color=(200, 200, 200), mask_color=palette, out_file=out_file)
