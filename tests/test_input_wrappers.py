"""The staged-batch contract of the input-side wrappers in ops.py, on CPU tensors: `image_prep_u8`, `train_prep_u8`,
`train_prep_panoptic_u8`, `train_prep_polygons_workspace_bytes`, `polygon_fill_bits`, `train_prep_polygons_u8`. No GPU, no library.

Every wrapper checks types and shapes, then `staged_bytes`, and only then asks for a device address, so a CPU tensor reaches the
first `dev_ptr` exactly when nothing was refused earlier. Each case below starts from a valid argument list of the smallest layout
with every table non-empty (B = 2 images of 16 x 24, N = 3 instances, a semantic map, S = 3 segment rows, P = 3 parts), injects ONE
fault, and expects a `CggError` whose message starts with the wrapper's name and names the faulty argument. Three kinds of case
state less, because the wrappers have always said less there:
  * an empty batch is refused as `<wrapper>: an empty batch`: it names no argument;
  * `train_prep_polygons_workspace_bytes` with a non-contiguous table is refused by `host_ptr`, whose message names the argument only
    (the case asserts the argument name alone); its empty batch is refused by the library, not the wrapper, and has no case here;
  * `mean` is read after the device addresses are taken, so its cases stand `dev_ptr` in for a device.
"""
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops
from cgg_amd._lib import CggError

B, H, W, N, S, P = 2, 16, 24, 3, 3, 3
NBYTES = 4096
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

# argument names per call, in the wrapper's positional order; the keyword `staged_bytes` is passed by name
CALLS = {
    'image_prep_u8': ('staged', 'table', 'out', 'mean', 'std'),
    'train_prep_u8': ('staged', 'img_table', 'inst_table', 'img', 'masks', 'seg', 'stats', 'mean', 'std'),
    'train_prep_panoptic_u8': ('staged', 'img_table', 'pan_table', 'seg_table', 'img', 'masks', 'seg', 'stats', 'mean', 'std'),
    'train_prep_polygons_workspace_bytes': ('img_table', 'N'),
    'polygon_fill_bits': ('staged', 'img_table', 'inst_table', 'part_table', 'staged_host', 'workspace'),
    'train_prep_polygons_u8': ('staged', 'img_table', 'inst_table', 'part_table', 'staged_host', 'img', 'masks', 'stats', 'workspace',
                               'mean', 'std'),
}
# (rows, cols) of every table a call takes
TABLES = {
    'image_prep_u8': {'table': (B, 8)},
    'train_prep_u8': {'img_table': (B, 12), 'inst_table': (N, 3)},
    'train_prep_panoptic_u8': {'img_table': (B, 12), 'pan_table': (B, 5), 'seg_table': (S, 2)},
    'train_prep_polygons_workspace_bytes': {'img_table': (B, 12)},
    'polygon_fill_bits': {'img_table': (B, 12), 'inst_table': (N, 3), 'part_table': (P, 2)},
    'train_prep_polygons_u8': {'img_table': (B, 12), 'inst_table': (N, 3), 'part_table': (P, 2)},
}
IMG = {'image_prep_u8': 'out', 'train_prep_u8': 'img', 'train_prep_panoptic_u8': 'img', 'train_prep_polygons_u8': 'img'}
POLY = ('polygon_fill_bits', 'train_prep_polygons_u8')


def valid(call):
    """a fresh, valid argument dict of `call` (CPU tensors)"""
    a = {name: torch.zeros(shape, dtype=torch.int32) for name, shape in TABLES[call].items()}
    a.update(staged=torch.zeros(NBYTES, dtype=torch.uint8), staged_host=torch.zeros(NBYTES, dtype=torch.uint8),
             img=torch.zeros((B, 3, H, W)), out=torch.zeros((B, 3, H, W)), masks=torch.zeros((N, H, W), dtype=torch.uint8),
             seg=torch.zeros((B, 1, H, W), dtype=torch.uint8), stats=torch.zeros((N, 5), dtype=torch.int32),
             workspace=torch.zeros(64, dtype=torch.int32), mean=MEAN, std=STD, N=N)
    return {k: a[k] for k in CALLS[call]}


def invoke(call, a, **kw):
    return getattr(ops, call)(*[a[k] for k in CALLS[call]], **kw)


def _cases():
    """(call, argument the message must name, whether the message must start with the wrapper's name, edit of the argument dict ->
    keywords, needs a stand-in for dev_ptr)"""
    out = []

    def add(call, arg, edit, prefix=True, fake_dev=False, tag=None):
        out.append(pytest.param(call, arg, prefix, edit, fake_dev, id=f'{call}-{arg}-{tag}'))

    def put(name, value):
        return lambda a: a.__setitem__(name, value) or {}

    for call in CALLS:
        has = CALLS[call]
        if 'staged' in has:
            add(call, 'staged', put('staged', torch.zeros(NBYTES, dtype=torch.int8)), tag='dtype')
            add(call, 'staged', put('staged', torch.zeros((2, NBYTES // 2), dtype=torch.uint8)), tag='2d')
            add(call, 'staged_bytes', lambda a: {'staged_bytes': NBYTES + 1}, tag='past-staged')
        for name, (rows, cols) in TABLES[call].items():
            add(call, name, put(name, torch.zeros((rows, cols + 1), dtype=torch.int32)), tag='cols')
            add(call, name, put(name, torch.zeros((rows, cols), dtype=torch.int64)), tag='dtype')
            add(call, name, put(name, torch.zeros((rows, 2 * cols), dtype=torch.int32)[:, ::2]),
                prefix=call != 'train_prep_polygons_workspace_bytes', tag='strided')
        if call in IMG:
            img = IMG[call]
            add(call, img, put(img, torch.zeros((B + 1, 3, H, W))), tag='batch')
            add(call, img, put(img, torch.zeros((B, 4, H, W))), tag='channels')
            add(call, img, put(img, torch.zeros((B, 3, H, W), dtype=torch.float64)), tag='dtype')
            add(call, 'mean', put('mean', (1.0, 2.0)), fake_dev=True, tag='two')
        if 'masks' in has:
            add(call, 'masks', put('masks', torch.zeros((N, H, W + 1), dtype=torch.uint8)), tag='shape')
            add(call, 'masks', put('masks', torch.zeros((N, H, W), dtype=torch.int32)), tag='dtype')
            add(call, 'stats', put('stats', torch.zeros((N, 4), dtype=torch.int32)), tag='shape')
            add(call, 'stats', put('stats', torch.zeros((N, 5), dtype=torch.int64)), tag='dtype')
        if 'seg' in has:
            add(call, 'seg', put('seg', torch.zeros((B, H, W), dtype=torch.uint8)), tag='shape')
            add(call, 'seg', put('seg', torch.zeros((B, 1, H, W), dtype=torch.float32)), tag='dtype')
        if 'pan_table' in has:
            add(call, 'pan_table', put('pan_table', torch.zeros((B + 1, 5), dtype=torch.int32)), tag='rows')
        if call in POLY:
            add(call, 'staged_host', lambda a: a.__setitem__('staged_host', torch.zeros(NBYTES // 2, dtype=torch.uint8))
                or {'staged_bytes': NBYTES // 2 + 1}, tag='bytes-past')
            add(call, 'staged_host', put('staged_host', torch.zeros(NBYTES, dtype=torch.int8)), tag='dtype')
            add(call, 'staged_host', put('staged_host', torch.zeros((2, NBYTES // 2), dtype=torch.uint8)), tag='2d')
            add(call, 'workspace', put('workspace', torch.zeros(64, dtype=torch.float32)), tag='dtype')
            add(call, 'workspace', put('workspace', torch.zeros((8, 8), dtype=torch.int32)), tag='2d')
        if call != 'train_prep_polygons_workspace_bytes':

            def empty(a, call=call):
                first = next(iter(TABLES[call]))
                for name, (rows, cols) in TABLES[call].items():
                    if rows == B:
                        a[name] = torch.zeros((0, cols), dtype=torch.int32)
                if call in IMG:
                    a[IMG[call]] = torch.zeros((0, 3, H, W))
                if 'seg' in a:
                    a['seg'] = torch.zeros((0, 1, H, W), dtype=torch.uint8)
                assert a[first].shape[0] == 0
                return {}
            add(call, 'empty batch', empty, tag='B0')
    return out


@pytest.mark.parametrize('call, arg, prefix, edit, fake_dev', _cases())
def test_one_fault_is_refused_by_name(call, arg, prefix, edit, fake_dev, monkeypatch):
    a = valid(call)
    kw = edit(a)
    if fake_dev:
        monkeypatch.setattr(ops, 'dev_ptr', lambda t, *rest, **k: None)
    with pytest.raises(CggError) as e:
        invoke(call, a, **kw)
    msg = str(e.value)
    assert arg in msg, msg
    if prefix:
        assert msg.startswith(call + ': '), msg


@pytest.mark.parametrize('call', [c for c in CALLS if 'staged' in CALLS[c]])
def test_fault_free_call_reaches_the_device_test(call):
    """nothing is refused before the first device address: a valid CPU argument list fails on `staged`, and only there"""
    with pytest.raises(CggError, match='must live on a ROCm device') as e:
        invoke(call, valid(call))
    assert str(e.value).startswith(f'{call}: staged'), str(e.value)
    with pytest.raises(CggError, match='must live on a ROCm device') as e:
        invoke(call, valid(call), staged_bytes=NBYTES)
    assert str(e.value).startswith(f'{call}: staged'), str(e.value)
