#!/usr/bin/env python
"""Generate tests/golden/g12_paint.npz by EXECUTING THE REFERENCE'S OWN open_set/core/visualization/image.py.

Runs only where the reference tree is at hand; the fixture (inputs + expected outputs, no reference source) is committed and is
what travels. Usage:  python tests/golden/make_golden_paint.py REFERENCE_ROOT

image.py imports cv2, mmcv, pycocotools and four mmdet modules at its top, none of which is installed: they are stub modules
here (nothing of them is reached by the two functions that run). matplotlib is imported for real where it is installed and
stubbed otherwise; the axes object handed to `draw_masks` is a stub that records what is added to it.

  draw_masks(ax, img, masks, color, with_edge=False, alpha)   the fill rule, `img[mask] = img[mask] * (1 - alpha) + color * alpha`,
                                                               mask after mask, on a seeded 24 x 40 x 3 image with 6 overlapping
                                                               masks (three cover one common region) and colours with 0 and 255;
                                                               at alpha 0.8 (the value imshow_det_bboxes uses), 0.5 and 1.0
  _get_adaptive_scales(areas)                                  the text scale, below, between and above its two area bounds
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, child = name.rpartition('.')
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], child, m)
    return m


class _Axes:
    def __init__(self):
        self.collections = []

    def add_collection(self, p):
        self.collections.append(p)


def load_reference_image_module(ref_root):
    _stub('cv2')
    _stub('mmcv')
    _stub('pycocotools')
    _stub('pycocotools.mask')
    for name in ('mmdet', 'mmdet.core', 'mmdet.core.evaluation', 'mmdet.core.mask', 'mmdet.core.visualization'):
        _stub(name)
    _stub('mmdet.core.evaluation.panoptic_utils', INSTANCE_OFFSET=1000)
    _stub('mmdet.core.mask.structures', bitmap_to_polygon=None)
    _stub('mmdet.core.utils', mask2ndarray=None)
    _stub('mmdet.core.visualization.palette', get_palette=None, palette_val=None)
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        _stub('matplotlib')
        _stub('matplotlib.pyplot')
        _stub('matplotlib.collections', PatchCollection=lambda *a, **k: ('PatchCollection', a, k))
        _stub('matplotlib.patches', Polygon=None)
    path = os.path.join(ref_root, 'open_set', 'core', 'visualization', 'image.py')
    spec = importlib.util.spec_from_file_location('ref_visualization_image', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    rs = np.random.RandomState(12)
    H, W = 24, 40
    img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    img[0, :8] = 0
    img[0, 8:16] = 255
    masks = np.zeros((6, H, W), bool)
    masks[0, 2:14, 3:20] = True
    masks[1, 8:20, 10:30] = True
    masks[2, 5:12, 15:38] = True            # 0, 1 and 2 share rows 8..11, columns 15..19
    masks[3] = rs.rand(H, W) < 0.3          # scattered pixels over everything
    masks[4, 0, :] = True                   # the row of zeros and 255s
    masks[4, :, 0] = True
    masks[5, 18:24, 30:40] = True
    colors = np.array([[0, 255, 17], [255, 255, 255], [0, 0, 0], [200, 1, 254], [128, 127, 126], [3, 250, 99]], np.uint8)
    return img, masks, colors


def main(ref_root):
    ref = load_reference_image_module(ref_root)
    img, masks, colors = inputs()
    out = dict(img=img, masks=masks, colors=colors)
    for alpha, tag in ((0.8, 'a08'), (0.5, 'a05'), (1.0, 'a10')):
        ax = _Axes()
        _, painted = ref.draw_masks(ax, img.copy(), masks.copy(), color=colors.copy(), with_edge=False, alpha=alpha)
        assert painted.dtype == np.uint8 and painted.shape == img.shape and len(ax.collections) == 1
        out['painted_' + tag] = painted
    areas = np.array([0, 1, 799, 800, 801, 4321.5, 15400, 29999, 30000, 30001, 1e6], np.float64)
    out['areas'] = areas
    out['scales'] = ref._get_adaptive_scales(areas)
    path = os.path.join(HERE, 'g12_paint.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
