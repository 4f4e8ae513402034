"""GPU tests of the device side of the caption metrics (csrc/caption_eval.hip): `ops.caption_bleu_lcs`, `ops.caption_ngram_keys` and
`ops.cider_sums` equal the rules of `cgg_amd.caption_eval` exactly -- integers as arrays, doubles by their bit patterns, so there is no
tolerance -- on the reference-made fixture G16, a hand-made edge set and seeded corpora at the edges of the kernels' geometry; the two
routes of `CaptionEvaluator` agree in every array; corpora outside the gate take the numpy route; `tools/test.py --eval caption` end
to end."""
import functools
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import caption_eval as CE
from cgg_amd import ops, registry, synthetic
from cgg_amd._lib import CggError

import caption_cases as C

pytestmark = pytest.mark.gpu

CAP_L, CAP_R = ops.CAPTION_MAX_LEN, ops.CAPTION_MAX_REFS

# (seed, N, R, Lmin, Lmax, V, spaces, dense): images 1, 2, 3, 65, 130 (one wave per image: more than one workgroup per CU at 65, more
# than the CUs' first round at 130 is not needed for correctness, the grid is the image count); references 1, 5, 7; sentence lengths
# 0, 1, 3, 4 (the n-gram orders run out), 63, 64, 65 (the lane stride of a wave) and the cap, 128; 4 tokens (heavy repetition: counts
# above 1, clipping, ties) and about 300. `dense` corpora must satisfy the conditions below on their own.
SEEDED = [(11, 1, 1, 0, 1, 4, True, False), (12, 2, 5, 3, 4, 4, True, False), (13, 3, 7, 0, 4, 300, True, False),
          (14, 65, 5, 1, 12, 300, True, True), (15, 130, 1, 0, 9, 4, True, False), (16, 3, 5, 63, 65, 300, True, False),
          (17, 2, 7, CAP_L, CAP_L, 4, False, False), (18, 65, 7, 3, 14, 4, True, True)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (hyps, refs, corpus, host components), computed once per corpus and shared"""
    if name in ('a', 'b'):
        hyps, refs = C.fixture_corpus(name)
    elif name == 'edge':
        hyps, refs = C.edge_corpus()
    else:
        hyps, refs = C.random_corpus(*SEEDED[name][:7])
    corpus = CE.intern_corpus_host(hyps, refs)
    return hyps, refs, corpus, CE.CaptionEvaluator.components_host(corpus)


CASES = ['a', 'b', 'edge'] + list(range(len(SEEDED)))


@pytest.mark.parametrize('name', CASES)
def test_the_kernels_equal_the_rules(dev, name):
    hyps, refs, corpus, want = _case(name)
    assert ops.caption_eval_ok(*CE.corpus_limits(corpus))
    ev = CE.CaptionEvaluator(device=dev)
    got = ev.components_device(corpus)
    C.assert_components_equal(got, want, f'case {name}')
    C.assert_components_equal(ev.components_device(corpus), got, f'case {name}, second run')
    if name == 6:
        assert CE.corpus_limits(corpus)[1] == CAP_L and (np.diff(corpus['sent_off']) == CAP_L).sum() >= 8


def test_the_seeded_corpora_are_not_empty_cases():
    """with the host rule: at least a third of the images have correct[3] > 0, an image has CIDEr exactly 0, a sentence with tokens
    has norm 0, at least 10 % of the hypothesis n-grams are absent from all references -- in each dense corpus and over all of them"""
    tot = np.zeros(6)
    for i, spec in enumerate(SEEDED):
        hyps, refs, corpus, c = _case(i)
        _, cider = CE.cider_finish_host(c['norm2'], c['num'], corpus)
        hyp_pos = np.zeros(len(corpus['words']), bool)
        for n in range(corpus['N']):
            s = corpus['img_off'][n]
            hyp_pos[corpus['sent_off'][s]:corpus['sent_off'][s + 1]] = True
        d = c['df_pos'][hyp_pos]
        row = np.array([(c['correct'][:, 3] > 0).sum(), corpus['N'], (cider == 0).sum(),
                        ((c['norm2'][:, 0] == 0) & (np.diff(corpus['sent_off']) > 0)).sum(), (d == 0).sum(), (d >= 0).sum()], np.float64)
        tot += row
        print(spec, row.tolist())
        for r in ([row] if spec[7] else []) + ([tot] if i == len(SEEDED) - 1 else []):
            assert 3 * r[0] >= r[1] and r[2] >= 1 and r[3] >= 1 and 10 * r[4] >= r[5], (spec, r)
    # the lengths the kernels change path at all occur, in one stream or the other
    lens = set()
    for i in range(len(SEEDED)):
        corpus = _case(i)[2]
        lens |= set(np.diff(corpus['sent_off']).tolist()) | set(np.diff(corpus['sent_off_sp']).tolist())
    assert lens >= {0, 1, 3, 4, 63, 64, 65, CAP_L}


def test_keys_flags_and_marks_at_the_ops_level(dev):
    """the key packing and the first-occurrence flags against a direct statement; an image beyond a cap is marked, not evaluated"""
    hyps, refs, corpus, want = _case('edge')
    d = {k: torch.from_numpy(corpus[k]).to(dev) for k in ('words', 'sent_off', 'words_sp', 'sent_off_sp', 'img_off')}
    keys, flags = ops.caption_ngram_keys(d['words'], d['sent_off'], d['img_off'])
    keys, flags = keys.cpu().numpy(), flags.cpu().numpy()
    sents = CE.corpus_sentences(corpus)
    w = 0
    for image in sents:
        seen = set()
        for j, s in enumerate(image):
            for i in range(len(s)):
                for k in range(4):
                    g = tuple(s[i:i + k + 1]) if i + k < len(s) else None
                    assert keys[w, k] == (0 if g is None else sum(t << (16 * q) for q, t in enumerate(g)))
                    assert flags[w, k] == (1 if g is not None and j > 0 and g not in seen else 0)
                    if g is not None and j > 0:
                        seen.add(g)
                w += 1
    assert w == len(corpus['words'])
    # one image of CAP_R + 1 references between two ordinary ones: marked in every output, its neighbours evaluated
    hyps, refs = ['x y', 'x y z', 'x'], [['x y'], ['x %d' % i for i in range(CAP_R + 1)], ['x', 'y x']]
    corpus = CE.intern_corpus_host(hyps, refs)
    assert not ops.caption_eval_ok(*CE.corpus_limits(corpus))
    host = CE.CaptionEvaluator.components_host(corpus)
    d = {k: torch.from_numpy(corpus[k]).to(dev) for k in ('words', 'sent_off', 'words_sp', 'sent_off_sp', 'img_off')}
    bleu, lcs = ops.caption_bleu_lcs(d['words'], d['sent_off'], d['words_sp'], d['sent_off_sp'], d['img_off'])
    bleu, lcs = bleu.cpu().numpy(), lcs.cpu().numpy()
    assert (bleu[1] == -1).all() and (lcs[1:CAP_R + 2] == -1).all()
    for n in (0, 2):
        assert bleu[n].tolist() == [host['testlen'][n], host['reflen'][n]] + host['guess'][n].tolist() + host['correct'][n].tolist()
    assert lcs[0] == host['lcs'][0] and lcs[-2:].tolist() == host['lcs'][-2:].tolist()
    keys, flags = ops.caption_ngram_keys(d['words'], d['sent_off'], d['img_off'])
    lo, hi = corpus['sent_off'][corpus['img_off'][1]], corpus['sent_off'][corpus['img_off'][2]]
    assert (keys[lo:hi] == 0).all() and (flags[lo:hi] == 0).all() and (keys[:lo, 0] != 0).all() and (keys[hi:, 0] != 0).all()
    # empty corpora are legal and launch nothing; a CPU tensor is refused
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    bleu, lcs = ops.caption_bleu_lcs(e, z, e, z, z)
    assert tuple(bleu.shape) == (0, 10) and lcs.numel() == 0
    assert ops.caption_ngram_keys(e, z, z)[0].shape == (0, 4)
    with pytest.raises(CggError):
        ops.caption_ngram_keys(torch.zeros(3, dtype=torch.int32), z, z)


@pytest.mark.parametrize('name', ['a', 'b', 'edge', 3, 7])
def test_the_two_routes_of_the_evaluator_agree(dev, name):
    hyps, refs = _case(name)[:2]
    on_dev, on_host = CE.CaptionEvaluator(device=dev), CE.CaptionEvaluator()
    on_dev.add_batch(hyps, refs)
    on_host.add_batch(hyps, refs)
    a, b = on_dev.summarize(), on_host.summarize()
    assert (a['route'], b['route']) == ('device', 'host')
    C.assert_summaries_equal(a, b, f'case {name}')
    if name == 'a':
        z = C.fixture()
        assert np.array_equal(a['correct'], z['a_correct']) and np.array_equal(a['lcs'], z['a_lcs'])
        np.testing.assert_allclose(a['cider'], z['a_cider_img'], rtol=1e-12, atol=0)


def test_corpora_outside_the_gate_take_the_numpy_route(dev):
    assert ops.caption_eval_ok(65535, CAP_L, CAP_R)
    assert not ops.caption_eval_ok(65536, 1, 1) and not ops.caption_eval_ok(10, CAP_L + 1, 1) and not ops.caption_eval_ok(10, 1, CAP_R + 1)

    def both(hyps, refs):
        on_dev, on_host = CE.CaptionEvaluator(device=dev), CE.CaptionEvaluator()
        on_dev.add_batch(hyps, refs)
        on_host.add_batch(hyps, refs)
        a, b = on_dev.summarize(), on_host.summarize()
        C.assert_summaries_equal(a, b)
        return a

    # 65536 distinct tokens: 32 images x 16 references x 128 tokens. One token fewer, and the corpus is inside: token id 65535 packs
    toks = ['t%d' % i for i in range(65536)]
    refs = [[' '.join(toks[(n * 16 + r) * 128:(n * 16 + r + 1) * 128]) for r in range(16)] for n in range(32)]
    hyps = [' '.join(toks[n * 2048 + 5:n * 2048 + 12]) for n in range(32)]
    res = both(hyps, refs)
    assert res['route'] == 'host' and (res['correct'][:, 3] == 4).all()
    refs[-1][-1] = ' '.join(toks[-128:-1])
    res = both(hyps, refs)
    assert res['route'] == 'device' and (res['correct'][:, 3] == 4).all()
    # a sentence one past the length cap, in a reference and in a hypothesis; only in the split(" ") stream; one reference too many
    long = ' '.join('w%d' % (i % 7) for i in range(CAP_L + 1))
    assert both(['w1 w2 w3', 'w0'], [[long, 'w1 w2'], ['w0 w1']])['route'] == 'host'
    assert both([long, 'w0'], [['w1 w2'], ['w0 w1']])['route'] == 'host'
    spaced = long[:-len(' w%d' % (CAP_L % 7))].replace(' w3 ', ' w3  ', 1)
    assert len(spaced.split()) == CAP_L and len(spaced.split(' ')) == CAP_L + 1
    assert both([spaced, 'w0'], [['w1 w2'], ['w0 w1']])['route'] == 'host'
    assert both(['w1'], [['w%d' % i for i in range(CAP_R + 1)]])['route'] == 'host'
    assert both(['w1'], [['w%d' % i for i in range(CAP_R)]])['route'] == 'device'


def _tiny_caption_model(tmp_path, seed):
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    with torch.no_grad():
        model.panoptic_head.caption_generator.generator.bias[102] += 3.0      # sentences end
    ck = save_checkpoint(model, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\n')
    special = {0: '[PAD]', 100: '[UNK]', 101: '[CLS]', 102: '[SEP]', 103: '[MASK]'}
    vocab = tmp_path / 'vocab.txt'
    vocab.write_text(''.join(special.get(i, 'w%d' % i) + '\n' for i in range(500)))
    return str(cfg_file), ck, str(vocab)


def test_tools_test_eval_caption(dev, tmp_path, capsys):
    """tools/test.py --eval caption --synthetic-captions on a small synthetic model, the ids rendered through a vocabulary file written
    here: caption_eval.json holds the six numbers, and they are those of a host evaluator fed the captions the driver returns and the
    same synthetic references; a stream without gt_captions gets a message"""
    cfg_file, ck, vocab = _tiny_caption_model(tmp_path, seed=9)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_caption', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    common = [cfg_file, ck, '--num-images', '3', '--synthetic', '64', '--eval', 'caption', '--precision', 'bf16', '--caption-vocab', vocab]
    results = drv.main(common + ['--synthetic-captions', '--work-dir', str(tmp_path / 'a')])
    out = capsys.readouterr().out
    assert 'BLUE-1 = ' in out and 'CIDEr = ' in out and 'Rouge = ' in out and '"pipeline": false' in out
    got = json.loads((tmp_path / 'a' / 'caption_eval.json').read_text())
    assert got['images'] == 3 and got['route'] == 'device' and set(got) == set(CE.SCORE_NAMES) | {'images', 'route'}
    caps = [r['cap_results'] for r in results]
    print('captions:', caps)
    assert len(caps) == 3 and all(isinstance(c, str) for c in caps) and any(c.split() for c in caps)
    ev = CE.CaptionEvaluator()
    ev.add_batch(caps, synthetic.caption_ground_truth(11, 3))
    want = ev.summarize()
    for k in CE.SCORE_NAMES:
        assert np.float64(got[k]).view(np.int64) == np.float64(want[k]).view(np.int64), (k, got[k], want[k])
    drv.main(common[:2] + ['--num-images', '1'] + common[4:])
    assert '--eval caption: the stream carries no ground truth' in capsys.readouterr().out
