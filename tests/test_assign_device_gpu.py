"""GPU tests of the device Hungarian solver (csrc/lsap_device.hip, `ops.linear_sum_assignment_device`) and of the training
targets built on it (`Mask2FormerHeadOpen._targets_device`): scipy's and the host solver's INDICES on identical bits, the status
words, and `_targets_batched` / `loss` equal element for element (to the bit) with `DEVICE_ASSIGN` on and off."""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import cgg_amd  # noqa: F401
from cgg_amd import mask2former_head as M2F
from cgg_amd import ops, synthetic
from test_assign_device import problem_set
from util import Bank, build_heads, small_cfg

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def stride_set():
    """Widths that cross the 64-lane stride of the column scan against a few heights, both ways round and square; half random,
    half {0, 1} ties. -> tuple of (matrix, scipy rows, scipy cols)."""
    rng = np.random.RandomState(5)
    shapes = []
    for nc in (1, 2, 63, 64, 65, 127, 128, 129):
        for nr in (1, 7, 64, 65):
            shapes += [(nr, nc), (nc, nr)]
        shapes.append((nc, nc))
    out = []
    for k, (nr, nc) in enumerate(shapes):
        x = rng.rand(nr, nc).astype(np.float32) if k % 2 == 0 else rng.randint(0, 2, (nr, nc)).astype(np.float32)
        x.setflags(write=False)
        r, c = linear_sum_assignment(x)
        out.append((x, r.astype(np.int64), c.astype(np.int64)))
    return tuple(out)


def solve_on_device(dev, mats):
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(dev)
    rows, cols, status = ops.linear_sum_assignment_device(flat, [m.shape[0] for m in mats], [m.shape[1] for m in mats])
    rows, cols, status = rows.cpu().numpy(), cols.cpu().numpy(), status.cpu().tolist()
    out, o = [], 0
    for m in mats:
        k = min(m.shape)
        out.append((rows[o:o + k], cols[o:o + k]))
        o += k
    assert o == rows.size == cols.size
    return out, status


def test_indices_equal_scipy_and_the_host_solver(dev):
    """Every matrix of the CPU file and the lane-stride set in ONE launch: rows and cols equal scipy's and
    `ops.linear_sum_assignment_batch`'s exactly -- identical input bits, so no tie allowance."""
    cases = problem_set() + stride_set()
    mats = [c[0] for c in cases]
    got, status = solve_on_device(dev, mats)
    host = ops.linear_sum_assignment_batch([torch.from_numpy(np.array(m)) for m in mats])
    assert status == [0, 0]
    for p, ((x, wr, wc), (r, c), (hr, hc)) in enumerate(zip(cases, got, host)):
        assert r.tolist() == wr.tolist() and c.tolist() == wc.tolist(), ('scipy', p, x.shape)
        assert r.tolist() == hr.tolist() and c.tolist() == hc.tolist(), ('host solver', p, x.shape)


def test_status_words_identity_pairing_and_untouched_neighbours(dev):
    """One launch mixes good problems with a NaN, a -inf and an infeasible one: the status words name the first bad problem, the
    check raises with the host solver's message, the bad problems pair k with k, the good ones are still exact."""
    good = [c for c in problem_set()[:40:4]] + [c for c in stride_set()[5:45:8]]
    rng = np.random.RandomState(9)
    nan = rng.rand(9, 14).astype(np.float32)
    nan[4, 3] = np.nan
    ninf = rng.rand(70, 6).astype(np.float32)
    ninf[69, 5] = -np.inf
    infeasible = np.full((2, 2), np.inf, np.float32)
    wide = rng.rand(5, 66).astype(np.float32)              # rows 1 and 3 can only take column 65
    wide[1, :65] = np.inf
    wide[3, :65] = np.inf
    mats = [c[0] for c in good]
    bad_at = {3: ninf, 7: nan, 11: infeasible, 12: wide}
    for at in sorted(bad_at):
        mats.insert(at, bad_at[at])
    got, status = solve_on_device(dev, mats)
    assert status == [1, 3 + 1]
    with pytest.raises(ops.CggError, match=r'problem 3: .*invalid numeric entries'):
        ops.lsap_status_check(torch.tensor(status, dtype=torch.int32, device=dev))
    gi = iter(good)
    for p, (m, (r, c)) in enumerate(zip(mats, got)):
        if p in bad_at:
            ident = list(range(min(m.shape)))
            assert r.tolist() == ident and c.tolist() == ident, p
        else:
            _, wr, wc = next(gi)
            assert r.tolist() == wr.tolist() and c.tolist() == wc.tolist(), p
    # an infeasible problem alone reports its own code
    _, status = solve_on_device(dev, [mats[0], wide, infeasible])
    assert status == [2, 1 + 1]
    with pytest.raises(ops.CggError, match=r'problem 1: .*infeasible'):
        ops.lsap_status_check(status)


# ---- the head: Q = 20, 112 points, 32 x 32 logits, 3 layers, B = 4 images with G = 0, 1, 5 and 25 (> Q) ----------------------
GS = (0, 1, 5, 25)


def _ground_truth(H, W, num_classes, seed):
    g = torch.Generator().manual_seed(seed)
    labels, masks = [], []
    for G in GS:
        labels.append(torch.randint(0, num_classes, (G,), generator=g))
        m = torch.zeros(G, H, W, dtype=torch.uint8)
        for i in range(G):
            y0, x0 = int(torch.randint(0, H - 8, (1,), generator=g)), int(torch.randint(0, W - 8, (1,), generator=g))
            hh, ww = int(torch.randint(4, H // 2, (1,), generator=g)), int(torch.randint(4, W // 2, (1,), generator=g))
            m[i, y0:y0 + hh, x0:x0 + ww] = 1
        masks.append(m)
    return labels, masks


class DevicePoints:
    """`Bank`'s pinned draws, uploaded BEFORE the call under test: handing them out waits for nothing."""

    def __init__(self, seed, calls, shape, dev):
        bank = Bank(seed)
        self.draws = [bank('target', shape, dev) for _ in range(calls)]
        self.at = 0

    def __call__(self, kind, shape, device):
        assert kind == 'target' and tuple(shape) == tuple(self.draws[self.at].shape)
        self.at += 1
        return self.draws[self.at - 1]


@pytest.fixture(scope='module')
def small_head(dev):
    cfg = small_cfg(num_queries=20, num_points=112)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prod, _ = build_heads(cfg)
    prod = prod.to(dev).train()
    for m in prod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return cfg, prod


@pytest.fixture(scope='module')
def target_inputs(dev, small_head):
    cfg, prod = small_head
    n, B, Q, h, H = 3, len(GS), 20, 32, 128
    K1 = prod.class_embs.shape[0]
    g = torch.Generator().manual_seed(44)
    labels, masks = _ground_truth(H, H, cfg['panoptic_head']['num_things_classes'], 45)
    cls = [torch.randn(B, Q, K1, generator=g).to(dev) for _ in range(n)]
    emb = [(torch.randn(B, Q, K1, generator=g) * 2).to(dev) for _ in range(n)]
    preds = [(torch.randn(B, Q, h, h, generator=g) * 2).to(dev) for _ in range(n)]
    return cls, emb, preds, [l.to(dev) for l in labels], [m.to(dev).float() for m in masks]


def _targets(prod, inputs, device_assign, overlap, point_hook=None):
    cls, emb, preds, labels, gt_f = inputs
    old = M2F.DEVICE_ASSIGN
    M2F.DEVICE_ASSIGN = device_assign
    prod.point_hook = point_hook if point_hook is not None else Bank(21)
    prod._overlap_result = None
    try:
        out = prod._targets_batched(cls, emb, preds, labels, gt_f, overlap=overlap)
        return out, prod._overlap_result
    finally:
        M2F.DEVICE_ASSIGN = old
        prod.point_hook = None
        prod._overlap_result = None


def _same_targets(a, b, n, Q):
    assert len(a) == len(b) == n
    m = [min(Q, G) for G in GS]
    for ta, tb in zip(a, b):
        la, wa, pba, _, ka, da = ta
        lb, wb, pbb, _, kb, db = tb
        assert ka == kb == sum(m) and da['pm'] == db['pm'] == max(m)
        assert list(pba) == list(pbb)
        assert la.dtype == lb.dtype == torch.int64 and wa.dtype == wb.dtype == torch.float32
        assert torch.equal(la, lb) and torch.equal(wa, wb)
        for key in 'bqgr':
            assert da[key].dtype == db[key].dtype == torch.int64 and da[key].shape == db[key].shape == (ka,), key
            assert torch.equal(da[key], db[key]), key


@pytest.mark.parametrize('with_overlap', [False, True])
def test_targets_equal_the_host_path(dev, small_head, target_inputs, with_overlap):
    _, prod = small_head
    calls = []

    def overlap():
        calls.append(1)
        return ('overlapped', len(calls))

    fn = overlap if with_overlap else None
    prod.assign_status = None
    on, res_on = _targets(prod, target_inputs, True, fn)
    off, res_off = _targets(prod, target_inputs, False, fn)
    _same_targets(on, off, 3, 20)
    if with_overlap:
        assert res_on == ('overlapped', 1) and res_off == ('overlapped', 2)
    else:
        assert res_on is None and res_off is None and not calls
    assert all(torch.is_tensor(t[3]) and t[3].is_cuda and torch.equal(t[3], t[5]['g']) for t in on)     # the `pos_g` slot
    assert prod.assign_status.tolist() == [0, 0]
    ops.lsap_status_check(prod.assign_status)


def test_no_host_round_trip(dev, small_head, target_inputs, monkeypatch):
    """With `DEVICE_ASSIGN` on the host solver is never called, and nothing in the call waits for the device (torch's sync debug
    mode raises on `.cpu()`, `.item()`, boolean indexing, pageable copies, ...); the random points are uploaded beforehand."""
    _, prod = small_head

    def refuse(costs):
        raise AssertionError('the host solver was called on the device path')

    monkeypatch.setattr(ops, 'linear_sum_assignment_batch', refuse)
    hook = DevicePoints(21, 3 * len(GS), (1, 112, 2), dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        on, res = _targets(prod, target_inputs, True, lambda: 'overlapped', point_hook=hook)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert res == 'overlapped' and hook.at == 3 * len(GS)
    monkeypatch.undo()
    off, _ = _targets(prod, target_inputs, False, None)
    _same_targets(on, off, 3, 20)


def test_loss_equal_to_the_bit(dev, small_head, monkeypatch):
    """`head.loss` on the same predictions, ground truth and pinned points with the flag on and off: every entry of the loss
    dict has the same bits. `ops.topk_select` returns the SET of the most uncertain points in an order that varies from launch
    to launch (the mask losses then sum the same terms in another order: 1-2 ulp between two runs of ONE path), so its indices
    are sorted here, for both runs alike."""
    cfg, prod = small_head
    select = ops.topk_select
    monkeypatch.setattr(ops, 'topk_select', lambda u, k: select(u, k).sort(1).values)
    B, H = len(GS), 128
    feats = [f.to(dev) for f in synthetic.backbone_feats(B, H, H, channels=(64, 128, 256, 512), seed=31)]
    metas = synthetic.img_metas(B, H, H)
    batch = synthetic.train_batch(B, H, H, num_classes=cfg['panoptic_head']['num_things_classes'], max_inst=4, vocab=500, seed=32,
                                  device=dev)
    labels, masks = _ground_truth(H, H, cfg['panoptic_head']['num_things_classes'], 46)
    prod._lazy_masks = True
    try:
        cls, emb, preds = prod(feats, metas)
    finally:
        prod._lazy_masks = False
    gt_labels, gt_masks = prod.preprocess_gt([l.to(dev) for l in labels], [m.to(dev) for m in masks], None, metas)
    cap_embs, cap_mask, noun_embs, noun_mask = None, batch['gt_caption_mask'], None, batch['gt_caption_nouns_mask']
    if prod.use_caption_generation:
        cap_embs, cap_mask = prod.extract_word_embeddings(batch['gt_caption_ids'], cap_mask, prod.caption_gen_emb_type)
    if prod.use_caption:
        noun_embs, noun_mask = prod.extract_word_embeddings(batch['gt_caption_nouns_ids'], noun_mask, prod.caption_emb_type)

    def run(flag):
        old = M2F.DEVICE_ASSIGN
        M2F.DEVICE_ASSIGN = flag
        prod.point_hook = Bank(5)
        try:
            losses = prod.loss(cls, emb, preds, gt_labels, gt_masks, batch['gt_caption_ids'], cap_embs, cap_mask,
                               batch['gt_caption_nouns_ids'], noun_embs, noun_mask, metas)
            return {k: v.detach().float().cpu() for k, v in losses.items()}
        finally:
            M2F.DEVICE_ASSIGN = old
            prod.point_hook = None

    on, off = run(True), run(False)
    assert set(on) == set(off) and len(on) >= 7
    for k in sorted(on):
        assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), (k, float(on[k]), float(off[k]))
        assert bool(torch.isfinite(on[k]).all()), k
    ops.lsap_status_check(prod.assign_status)


def test_assign_hook_keeps_the_host_path(dev, small_head, target_inputs):
    """With `assign_hook` set the host path runs whatever the flag says, and the hook sees every problem once."""
    _, prod = small_head
    seen = []

    def hook(li, b, rows, cols, cost):
        seen.append((li, b, tuple(cost.shape)))
        return rows, cols

    prod.assign_hook = hook
    prod.assign_status = None
    try:
        hooked, _ = _targets(prod, target_inputs, True, None)
    finally:
        prod.assign_hook = None
    assert prod.assign_status is None                      # the device path was not taken
    assert sorted(seen) == sorted((li, b, (20, G)) for li in range(3) for b, G in enumerate(GS) if G)
    off, _ = _targets(prod, target_inputs, False, None)
    _same_targets(hooked, off, 3, 20)


def test_bad_costs_do_not_stop_the_step_and_are_reported(dev, small_head, target_inputs):
    """A NaN mask logit makes one problem's costs invalid: the call returns in-range targets of the usual sizes, the head's
    status words name that problem (problems are image-major: images 1, 2, 3 hold 0-2, 3-5, 6-8) and keep it over a later
    clean step until they are zeroed, and `ops.lsap_status_check` raises the host solver's message."""
    _, prod = small_head
    cls, emb, preds, labels, gt_f = target_inputs
    bad = [p.clone() for p in preds]
    bad[1][2, 0] = float('nan')                            # layer 1, image 2 (G = 5), query 0
    prod.assign_status = None
    out, _ = _targets(prod, (cls, emb, bad, labels, gt_f), True, None)
    assert prod.assign_status.tolist() == [ops.LSAP_INVALID, 4 + 1]
    m = [min(20, G) for G in GS]
    for lab, w, pos_b, g, k, devi in out:
        assert k == sum(m) and len(pos_b) == k and devi['q'].shape == devi['g'].shape == (k,)
        assert int(lab.min()) >= 0 and int(lab.max()) <= prod.num_classes and float(w.sum()) == k
        assert int(devi['q'].min()) >= 0 and int(devi['q'].max()) < 20
        assert bool((devi['g'] < torch.tensor(GS, device=dev)[devi['b']]).all()) and int(devi['g'].min()) >= 0
    assert out[1][5]['q'][1:6].tolist() == out[1][5]['g'][1:6].tolist() == [0, 1, 2, 3, 4]      # the identity pairing
    _targets(prod, target_inputs, True, None)
    assert prod.assign_status.tolist() == [ops.LSAP_INVALID, 4 + 1]
    with pytest.raises(ops.CggError, match=r'problem 4: .*invalid numeric entries'):
        ops.lsap_status_check(prod.assign_status)
    prod.assign_status.zero_()
    _targets(prod, target_inputs, True, None)
    ops.lsap_status_check(prod.assign_status)
