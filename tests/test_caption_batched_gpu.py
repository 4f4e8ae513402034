"""-m gpu: csrc/beam_step.hip against the rule of caption_search.py (`beam_step_host` in float64), the batched caption search end to
end on the device against the single-image search, and `inference_detector` on a list of images with captions.

Decisions are compared exactly, so every compared step asserts the margin condition first: in the float64 run of the rule the
smallest gap in `weighted` between consecutive selected candidates, and between the last selected and the first rejected one,
exceeds 1e-4 (the seeds were picked on the host so that it holds with room). The kernel's f32 `weighted` is within ~1e-5 of the
float64 value, so a mismatch under that condition is a bug and not a tie.

Float fields: |kernel - float64| <= 1e-5 + 4 spacing_f32(|value|). The weights are sums of at most 35 f32 log-probabilities of
magnitude up to ~15, so a few spacings of f32 at the weight's own magnitude is what f32 accumulation gives; the 1e-5 covers the
log-sum-exp over 30 522 terms.

Shapes of the step test: V = 30 (one ragged chunk, fewer columns than a workgroup has threads), 1003 (odd: rows are only 4-byte
aligned, the scalar-load path) and 30 522 (30 chunks, the last ragged; rows 8-byte and not 16-byte aligned: the 8-byte-load
path); L = 1 and 4; B = 1 and 3; beam = 2, 7 and 8 (the slot limit); nlive = 1, 3 and beam mixed in a batch; one done image."""
import warnings

import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops, synthetic
from cgg_amd.caption_search import beam_search, beam_search_batched
from cgg_amd.config import Config

from caption_batched_util import ALPHA, EOS, INT_KEYS, MARGIN, SCENARIOS, make_case, run_host64, spacing_f32
from util import build_heads, randomize, small_cfg

pytestmark = pytest.mark.gpu

# cases whose first seed leaves a gap below 1e-3 somewhere take a later one: case -> how many times 100 is added to the seed
SEED_BUMP = {10: 1, 12: 1, 27: 1, 29: 1, 30: 1, 31: 1, 35: 3, 42: 1, 44: 1, 46: 2, 47: 2, 51: 1, 52: 1, 57: 3, 59: 5, 60: 2,
             65: 1, 66: 1, 71: 1, 72: 15}


def _grid():
    case, out = 0, []
    for V in (30, 1003, 30522):
        for L in (1, 4):
            for B in (1, 3):
                for beam in (2, 7, 8):
                    for first in (False, True):
                        case += 1
                        scen = ('first', 'first_eos')[(case // 2) % 2] if first else SCENARIOS[(case // 2) % 4]
                        out.append((case, V, L, B, beam, first, scen, 2))
    # rows that are only 4-byte aligned although V is even: the scalar-load path at the full vocabulary
    out.append((case + 1, 30522, 4, 3, 7, False, 'eos', 1))
    return out


GRID = _grid()


def build_case(case, V, L, B, beam, first, scen):
    seed = 5000 + case + 100 * SEED_BUMP.get(case, 0)
    return make_case(seed, B, beam, V, L, scen, first, case % 3 if (B == 3 and not first) else None)


def _offset_logits(lg, dev, offset):
    """the logits on the device, `offset` floats past an allocation boundary: 2 -> row 0 is 8-byte and not 16-byte aligned"""
    flat = torch.empty(lg.numel() + 4, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + lg.numel()].view(lg.shape)
    view.copy_(lg)
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def _compare(case, step, got, want, before, was_done):
    for k in INT_KEYS:
        assert torch.equal(getattr(got, k).cpu(), getattr(want, k)), (case, step, k, getattr(got, k).cpu(), getattr(want, k))
    for k in ops.BeamState.FLOAT_FIELDS:
        g, w = getattr(got, k).cpu().double(), getattr(want, k)
        assert bool(((g - w).abs() <= 1e-5 + 4 * spacing_f32(w)).all()), (case, step, k, g, w)
    for b, d in enumerate(was_done):
        if d:                                                         # bit-identical to the values before the call
            for k in ops.BeamState.FIELDS:
                if k != 'ndone':
                    assert torch.equal(getattr(got, k)[b].cpu(), getattr(before, k)[b]), (case, step, k, b)


@pytest.mark.parametrize('case,V,L,B,beam,first,scen,offset', GRID, ids=[f'{g[0]}-V{g[1]}-L{g[2]}-B{g[3]}-beam{g[4]}-{g[6]}-off{g[7]}' for g in GRID])
def test_beam_step_kernel_equals_the_rule(dev, case, V, L, B, beam, first, scen, offset):
    """`ops.beam_step` == `beam_step_host` in float64 on the same logits and state, over two consecutive steps (the biased step of
    the scenario, then a plain one that finishes nothing: the best_idx reset)."""
    st, logits, length, max_len = build_case(case, V, L, B, beam, first, scen)
    snaps, margins = run_host64(st, logits, length, max_len, first)
    d = st.clone(device=dev)
    before = st
    for i in range(2):
        assert float(margins[i].min()) > MARGIN, (case, i, margins[i])
        was_done = before.done.tolist()
        ops.beam_step(_offset_logits(logits[i], dev, offset), d, length + i, ALPHA, max_len, first=first and i == 0)
        _compare(case, i, d, snaps[i], before, was_done)
        before = d.clone(device='cpu')


def test_scenarios_of_the_step_test_occur():
    """what the grid above claims to cover happens in it (float64 rule on the host): an EOS among the candidates, the break in the
    middle of the walk, no continued sequence, a best_idx reset, a done image beside a running one, EOS at the BOS step"""
    seen = dict(eos=0, brk=0, nocont=0, reset=0, done_beside=0, first_eos=0)
    for case, V, L, B, beam, first, scen, _ in GRID:
        if V == 30522 and case % 5:
            continue                                                   # the full vocabulary adds nothing to this count
        st, logits, length, max_len = build_case(case, V, L, B, beam, first, scen)
        snaps, _ = run_host64(st, logits, length, max_len, first)
        a, b = snaps
        for i in range(B):
            if st.done[i]:
                seen['done_beside'] += int(B > 1)
                continue
            grew = int(a.nfin[i]) - int(st.nfin[i])
            if first:
                seen['first_eos'] += int(EOS in a.seqs[i, :int(a.nlive[i]), 1].tolist())
                continue
            seen['eos'] += int(grew > 0)
            # candidates the walk consumed before it stopped: sequences it continued (a token at position `length`) + finished
            consumed = int((a.seqs[i, :, length] != 0).sum()) + grew
            seen['brk'] += int(scen == 'break' and bool(a.done[i]) and int(a.nfin[i]) == beam and consumed < beam)
            seen['nocont'] += int(bool(a.done[i]) and int(a.nfin[i]) < beam)
            seen['reset'] += int(int(a.best_idx[i]) != 0 and not a.done[i] and int(b.best_idx[i]) == 0)
    assert all(v > 0 for v in seen.values()), seen


# ---- the search end to end ---------------------------------------------------------------------------------------------------------
FEATURE_SEED = 17


@pytest.fixture(scope='module')
def prod(dev):
    """the head of tests/test_head_gpu.py (same builder, same seed) with EOS made likely enough that the searches finish sentences"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        head, _ = build_heads(small_cfg())
    with torch.no_grad():
        head.caption_generator.generator.bias[102] += 1.5
    return head.to(dev).eval()


def _margin_report(head, emb, i):
    margins = []
    beam_search_batched(head, emb[i:i + 1], 101, 102, max_len=35, beam_width=7, return_ids=True, rule='host64', margins=margins)
    return [float(m[0]) for m in margins]


def test_batched_search_on_the_device_equals_the_single_image_search(dev, prod):
    """`simple_test(..., with_caption=True)` on B = 3 returns a list of 3 captions; element i is what `beam_search` decodes from
    image i's embeddings alone (the search of the parent commit). The float64 rule keeps every step of all three searches more
    than the margin from a tie (asserted); if ids differ anyway, the per-step margins of that image are printed."""
    B, H, W = 3, 64, 96
    feats = synthetic.backbone_feats(B, H, W, channels=(64, 128, 256, 512), seed=FEATURE_SEED)
    metas = synthetic.img_metas(B, H, W)
    with torch.no_grad():
        out = prod.simple_test([f.to(dev) for f in feats], metas, with_caption=True)
        emb = out[1]
        assert isinstance(out[3], list) and len(out[3]) == 3
        margins = []
        ids64 = beam_search_batched(prod, emb, 101, 102, max_len=35, beam_width=7, return_ids=True, rule='host64', margins=margins)
        worst = torch.stack(margins).min(0).values
        print('smallest margin per image:', worst.tolist(), 'steps:', len(margins))
        assert float(worst.min()) > MARGIN, worst
        ids = beam_search_batched(prod, emb, 101, 102, max_len=35, beam_width=7, return_ids=True)
        assert any(len(s) for s in ids), 'no search finished a sentence: the comparison is empty'
        for i in range(B):
            want = beam_search(prod, emb[i:i + 1], 101, 102, max_len=35, beam_width=7, return_ids=True)
            if ids[i] != want:
                print(f'image {i}: batched {ids[i]} single {want} float64 rule {ids64[i]}; per-step margins {_margin_report(prod, emb, i)}')
            assert ids[i] == want, i
            assert beam_search_batched(prod, emb[i:i + 1], 101, 102, max_len=35, beam_width=7, return_ids=True) == [want]
        # what simple_test returned is the same search rendered as beam_search renders it
        assert out[3] == beam_search_batched(prod, emb, 101, 102, max_len=35, beam_width=7)
        # caption_batched=True forces the batched search at B = 1: a one-element list with the ids of the existing path
        one = [f[:1].to(dev) for f in feats]
        single = prod.simple_test(one, metas[:1], with_caption=True)
        forced = prod.simple_test(one, metas[:1], with_caption=True, caption_batched=True)
        assert isinstance(forced[3], list) and len(forced[3]) == 1 and forced[3][0] == single[3]


# ---- the public entry ----------------------------------------------------------------------------------------------------------------
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PIPELINE = [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=(192, 128), flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Pad', size_divisor=32, pad_val=dict(img=(128, 128, 128), masks=0, seg=255)),
                             dict(type='Normalize', mean=list(MEAN), std=list(STD), to_rgb=True),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


@pytest.fixture(scope='module')
def model(dev):
    """the small synthetic detector of tests/test_image_prep_gpu.py with 'cap_results' among its eval_types"""
    cfg = Config(dict(model=synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2,
                                                   dec_layers=3, vocab=500, num_points=256,
                                                   eval_types=['all_results', 'cap_results']),
                      data=dict(test=dict(pipeline=PIPELINE))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = cgg_amd.init_detector(cfg, None, device=dev)
    randomize(m, seed=9)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.fill_(1.0)
            mod.running_mean.zero_()
    with torch.no_grad():
        m.panoptic_head.caption_generator.generator.bias[102] += 3.0
    return m


def _structured_u8(h, w, seed):
    x = synthetic.structured_images(1, h, w, seed=seed, shapes=8)[0]
    return ((x - x.min()) / (x.max() - x.min()) * 255).round().byte().permute(1, 2, 0).contiguous().numpy()


def test_inference_detector_captions_a_list_of_images(dev, model, monkeypatch):
    """`inference_detector(model, [img0, img1], with_caption=True)` -- the README's example, a ValueError before the batched search --
    returns two results whose `cap_results` are what the single-image call gives for each image. Both images have the padded
    shape of the batch (128 x 192), so each sees the same input alone as in the batch. The tokenizer is made unavailable, so both
    searches return token ids (what they do offline without a cached vocabulary) and not a rendering that may hide them. The
    float64 rule keeps every step of both searches more than the margin from a tie (asserted on the batch's embeddings)."""
    try:
        import transformers

        def unavailable(*a, **k):
            raise OSError('no cached vocabulary')
        monkeypatch.setattr(transformers.BertTokenizer, 'from_pretrained', unavailable)
    except ImportError:
        pass
    embs = []
    real = model.panoptic_head.simple_test
    monkeypatch.setattr(model.panoptic_head, 'simple_test', lambda *a, **k: (lambda out: (embs.append(out[1]), out)[1])(real(*a, **k)))
    imgs = [_structured_u8(128, 192, 5), _structured_u8(128, 192, 6)]
    got = cgg_amd.inference_detector(model, imgs, with_caption=True)
    assert isinstance(got, list) and len(got) == 2
    margins = []
    with torch.no_grad():
        beam_search_batched(model.panoptic_head, embs[0], 101, 102, max_len=35, beam_width=7, return_ids=True, rule='host64',
                            margins=margins)
    worst = torch.stack(margins).min(0).values
    print('smallest margin per image:', worst.tolist(), 'steps:', len(margins))
    assert float(worst.min()) > MARGIN, worst
    caps = [g['cap_results'] for g in got]
    assert all(isinstance(c, list) and c and c[0] == 101 and c[-1] == 102 for c in caps), caps
    for i, img in enumerate(imgs):
        alone = cgg_amd.inference_detector(model, img, with_caption=True)
        assert 'all_results' in alone and alone['cap_results'] == caps[i], (i, alone['cap_results'], caps[i])
