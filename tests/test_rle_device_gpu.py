"""GPU tests of the device-side RLE (csrc/rle_device.hip): the kernels against the numpy rule on every shared case (offsets,
positions, the column-major planes of the workspace, guard words), the overflow contract, the collector's device mode against
the default collector (fallback from the column planes included, inputs overwritten after `wait_copied`) and the driver flag.
Everything is integer / byte equality."""
import os
import warnings

import numpy as np
import pytest
import torch

import rle_cases as RC
from cgg_amd import ops, registry, synthetic
from cgg_amd.host_results import RleCollector, rle_transitions_host

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0x5A5A5A5A


def run_kernels(c, dev, capacity):
    """-> (positions with GUARD words past `capacity`, offsets, cols) as numpy"""
    n = len(c['names'])
    bits = torch.from_numpy(c['base']).to(dev)[:, :c['H']]          # the strided case keeps its plane stride on the device
    assert bits.stride(0) == c['base'].shape[1] * c['row_bytes']
    pos = torch.full((capacity + GUARD,), PATTERN, dtype=torch.int32, device=dev)
    _, offs, ws = ops.rle_transitions(bits, c['W'], capacity=capacity, positions=pos)
    torch.cuda.synchronize()
    Wp, Hb = ops.rle_cols_shape(c['H'], c['W'])
    cols = ws[:n * Wp * Hb * 8].view(torch.int64).view(n, Wp, Hb).cpu().numpy().view(np.uint64)
    return pos.cpu().numpy().view(np.uint32), offs.cpu().numpy(), cols


@pytest.mark.parametrize('idx', RC.CASE_IDS, ids=RC.case_name)
def test_kernels_equal_the_rule(dev, idx):
    c = RC.case(idx)
    want_pos, want_offs = rle_transitions_host(c['bits'], c['W'])
    total = int(want_offs[-1])
    pos, offs, cols = run_kernels(c, dev, capacity=total)             # exactly enough: the last mask ends at `capacity`
    assert np.array_equal(offs, want_offs)
    assert np.array_equal(pos[:total], want_pos)
    assert (pos[total:] == PATTERN).all() and pos[total:].size == GUARD
    assert np.array_equal(cols, RC.cols_host(c['px']))                # zeros in the padding columns and rows included
    got = ops.rle_strings_from_transitions(pos[:total].copy(), offs, c['H'], c['W'])
    assert got == RC.expected_rles(idx)
    assert ops.rle_encode_colmajor(cols, c['H'], c['W']) == RC.expected_rles(idx)


@pytest.mark.parametrize('idx', [3, 5], ids=RC.case_name)
def test_overflow_keeps_offsets_complete_and_the_earlier_masks_exact(dev, idx):
    c = RC.case(idx)
    want_pos, want_offs = rle_transitions_host(c['bits'], c['W'])
    k = c['names'].index('checkerboard')
    capacity = int(want_offs[k + 1]) - 1                              # one short of the checkerboard, enough for the masks before
    assert capacity >= want_offs[k] > 0
    pos, offs, cols = run_kernels(c, dev, capacity)
    assert np.array_equal(offs, want_offs)
    fit = int(want_offs[k])
    assert np.array_equal(pos[:fit], want_pos[:fit])
    assert (pos[fit:] == PATTERN).all()                               # no part of a mask that does not fit, nothing past capacity
    assert np.array_equal(cols, RC.cols_host(c['px']))
    pos0, offs0, _ = run_kernels(c, dev, 0)                           # capacity 0: offsets only
    assert np.array_equal(offs0, want_offs) and (pos0 == PATTERN).all()


def test_no_masks_on_the_device(dev):
    pos, offs, _ = ops.rle_transitions(torch.zeros(0, 8, 2, dtype=torch.uint8, device=dev), 16, capacity=4)
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == [0]


def synthetic_results(dev):
    """2 images x 2 eval types, 5 masks of 96 x 128 each: disks plus one checkerboard (index 2: masks 0 and 1 fit a small
    run_capacity, the checkerboard and the disks after it take the fallback)"""
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(5)
    out = []
    for i in range(2):
        per = {}
        for key in ('all_results', 'novel_results'):
            px = np.zeros((5, H, W), bool)
            for j in range(5):
                cy, cx, r = rng.uniform(10, H - 10), rng.uniform(10, W - 10), rng.uniform(8, 30)
                px[j] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            px[2] = (yy + xx) % 2 == 0
            labels = torch.from_numpy(rng.integers(0, 3, 5)).to(dev)
            bboxes = torch.from_numpy(rng.random((5, 5)).astype(np.float32)).to(dev)
            per[key] = (labels, bboxes, torch.from_numpy(RC.pack(px, W // 8)).to(dev))
        out.append(per)
    return out


def assert_same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for key in ra:
            (bbox_a, segm_a), (bbox_b, segm_b) = ra[key], rb[key]
            assert len(bbox_a) == len(bbox_b) and all(np.array_equal(x, y) for x, y in zip(bbox_a, bbox_b))
            assert segm_a == segm_b, key                              # dict for dict, counts bytes included


@pytest.mark.parametrize('run_capacity', [600, 1 << 16, 0], ids=['small', 'ample', 'zero'])
def test_collector_device_mode_equals_the_default_collector(dev, run_capacity):
    results = synthetic_results(dev)
    ncls = dict(all_results=3, novel_results=3)
    plain = RleCollector(dev, ncls)
    want = plain.submit(results).result()
    plain.close()
    assert sum(len(c) for im in want for key in im for c in im[key][1]) == 20
    col = RleCollector(dev, ncls, device_rle=True, run_capacity=run_capacity)
    work = [{k: tuple(t.clone() for t in v) for k, v in im.items()} for im in results]
    fut = col.submit(work)
    RleCollector.wait_copied(fut)
    for im in work:                                                   # nothing reads the caller's tensors any more
        for v in im.values():
            for t in v:
                t.zero_()
    torch.cuda.synchronize()
    got = fut.result()
    again = col.submit(results).result()                              # the slot buffers are reused
    col.close()
    assert_same_results(got, want)
    assert_same_results(again, want)
    # 600 holds the two disks (at most 2 transitions per column: <= 122 each) but not the checkerboard's 12287: per submit and
    # tensor the checkerboard and the two masks after it take the fallback; 2^16 holds everything, 0 nothing
    fallback = {600: 2 * 4 * 3, 1 << 16: 0, 0: 2 * 4 * 5}[run_capacity]
    assert col.stats['masks'] == 40 and col.stats['fallback_masks'] == fallback


def test_test_driver_rle_device_results_equal_rle(dev, tmp_path):
    """tools/test.py --rle-device returns what --rle returns (set-up of test_test_driver_rle_results_equal_bool_masks)"""
    import importlib.util
    import sys
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2,
                                 dec_layers=3, vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=21)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    ck = save_checkpoint(model, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_rle_device', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    a = drv.main([str(cfg_file), ck, '--num-images', '7', '--synthetic', '128', '--rle-device'])
    b = drv.main([str(cfg_file), ck, '--num-images', '7', '--synthetic', '128', '--rle'])
    assert len(a) == 7 and len(b) == 7
    assert_same_results(a, b)
    assert sum(len(c) for im in a for key in im for c in im[key][1]) > 0
