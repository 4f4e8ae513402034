"""CPU tests of the caption-metric rules (`cgg_amd.caption_eval`): they reproduce fixture G16, which the reference's own bleu.py,
cider.py and rouge.py computed; their integer parts equal an independent `collections.Counter` statement on seeded corpora; the two
token streams round-trip; records split over two ranks merge to the same summary; and tools/test.py parses `--eval caption`."""
import importlib.util
import os

import numpy as np
import pytest

import cgg_amd  # noqa: F401
from cgg_amd import caption_eval as CE

import caption_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want)
    assert (err <= RTOL * np.abs(want)).all(), (what, got, want)


def _summary(hyps, refs):
    ev = CE.CaptionEvaluator()
    ev.add_batch(hyps, refs)
    return ev.summarize()


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_the_rules_reproduce_the_reference_on_the_fixture(tag):
    """Integers exactly (BLEU components, lengths, LCS, document frequencies), every float within relative 1e-12: the only sources of
    difference are libm (pow, exp, log: a few ulp each) and `v * v` against the reference's `pow(v, 2)` (at most 1 ulp per positive
    term, about 8 * 2^-53 on a score), both far below 1e-12; an error of the rule itself shows at 1e-3 or more.

    Observed where the fixture was made: every score of both runs is BIT-EQUAL to the reference's -- BLEU-1..4, ROUGE-L and CIDEr, per
    image and per corpus (the test prints the count of unequal values; it asserts only the tolerance, since libm may differ elsewhere)."""
    z = C.fixture()
    hyps, refs = C.fixture_corpus(tag)
    res = _summary(hyps, refs)
    assert res['route'] == 'host' and res['images'] == len(hyps) == (12 if tag == 'a' else 1)
    for k in ('testlen', 'reflen', 'guess', 'correct', 'lcs'):
        assert np.array_equal(res[k], z[f'{tag}_{k}']), k
    assert (res['total_testlen'], res['total_reflen']) == (int(z[tag + '_total_testlen']), int(z[tag + '_total_reflen']))
    # the closest length really is one of the lengths, and the components cover what the issue lists
    corpus = CE.intern_corpus_host(hyps, refs)
    assert np.array_equal(np.concatenate([np.diff(corpus['sent_off'])[a + 1:b] for a, b in zip(corpus['img_off'][:-1], corpus['img_off'][1:])]),
                          z[tag + '_reflens'])
    # document frequencies: n-gram for n-gram. (The reference's defaultdict also holds, with 0.0, the hypothesis n-grams it looked up.)
    df, df_pos = CE.ngram_df_host(corpus)
    vocab = corpus['vocab']
    got = {'\t'.join(vocab[t - 1] for t in g): v for g, v in df.items()}
    want = {str(g): int(v) for g, v in zip(z[tag + '_df_ngrams'], z[tag + '_df']) if v > 0}
    assert got == want
    assert np.array_equal(df_pos, C.df_pos_from({tuple(g.split('\t')): v for g, v in want.items()}, hyps, refs))
    assert np.array_equal(res['df_pos'], df_pos)
    _close([res[f'Bleu_{k}'] for k in range(1, 5)], z[tag + '_bleu'], 'bleu')
    _close(res['bleu'], z[tag + '_bleu_img'], 'bleu per image')
    _close(res['CIDEr'], z[tag + '_cider'], 'cider')
    _close(res['cider'], z[tag + '_cider_img'], 'cider per image')
    _close(res['ROUGE_L'], z[tag + '_rouge'], 'rouge')
    _close(res['rouge'], z[tag + '_rouge_img'], 'rouge per image')
    unequal = sum(int((np.asarray(a, np.float64).view(np.int64) != np.asarray(b, np.float64).view(np.int64)).sum()) for a, b in (
        (res['bleu'], z[tag + '_bleu_img']), (res['cider'], z[tag + '_cider_img']), (res['rouge'], z[tag + '_rouge_img']),
        (res['CIDEr'], z[tag + '_cider']), (res['ROUGE_L'], z[tag + '_rouge'])))
    print(f'run {tag}: {unequal} scores differ from the reference in their bits')


def test_the_fixture_holds_the_cases_it_was_made_for():
    z = C.fixture()
    hyps, refs = C.fixture_corpus('a')
    res = _summary(hyps, refs)
    assert '' in hyps and sorted(set(z['a_testlen'].tolist()))[:4] == [0, 1, 2, 3] and (z['a_guess'] == 0).any()
    i = hyps.index('a a a a a cat cat')
    assert refs[i] == ['a cat'] and z['a_correct'][i].tolist() == [2, 1, 0, 0] and z['a_guess'][i].tolist() == [7, 6, 5, 4]
    i = hyps.index('two dogs play in snow')                                       # |6 - 5| = |4 - 5|: the shorter, though it comes second
    assert [len(r.split()) for r in refs[i]] == [6, 4] and z['a_reflen'][i] == 4
    assert {len(r) for r in refs} >= {1, 7}
    corpus = CE.intern_corpus_host(hyps, refs)
    assert len(corpus['words_sp']) > len(corpus['words'])                         # double and trailing spaces
    assert z['a_df'].max() == 12 and z['a_df_ngrams'][np.argmax(z['a_df'])] == 'a'      # in every image: idf = 0
    s = corpus['img_off'][hyps.index('a')]
    assert (res['norm2'][s] == 0).all() and (res['norm2'] == 0).all(axis=1).sum() >= 2      # and a reference "a" as well
    i = hyps.index('zebra crossing nowhere fast')
    assert z['a_cider_img'][i] == 0.0 and res['cider'][i] == 0.0
    assert 'A horse.' in hyps and z['a_cider'] > 0 and z['a_bleu'][3] > 0 and z['a_rouge'] > 0


@pytest.mark.parametrize('seed,N,R,Lmin,Lmax,V', [(1, 1, 1, 0, 5, 4), (2, 9, 5, 0, 12, 4), (3, 20, 7, 3, 9, 300), (4, 7, 2, 1, 40, 30)])
def test_the_rules_equal_a_counter_statement_on_seeded_corpora(seed, N, R, Lmin, Lmax, V):
    hyps, refs = C.random_corpus(seed, N, R, Lmin, Lmax, V)
    hyps, refs = hyps + C.edge_corpus()[0], refs + C.edge_corpus()[1]
    corpus = CE.intern_corpus_host(hyps, refs)
    want = C.counter_components(hyps, refs)
    got = CE.bleu_components_host(corpus)
    for k in ('testlen', 'reflen', 'guess', 'correct'):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert np.array_equal(CE.lcs_host(corpus), want['lcs'])
    df, df_pos = CE.ngram_df_host(corpus)
    vocab = corpus['vocab']
    assert {tuple(vocab[t - 1] for t in g): v for g, v in df.items()} == dict(want['df'])
    assert np.array_equal(df_pos, C.df_pos_from(want['df'], hyps, refs))
    # the sums, once more with Counter and plain floats; `length` is the bigram count
    idf = CE.idf_table_host(len(hyps))
    sums = CE.cider_sums_host(corpus, df, idf)
    s = p = 0
    for hyp, rr in zip(hyps, refs):
        hv = [{g: float(c) * float(idf[want['df'].get(g, 0)]) for g, c in C._ngrams(hyp.split(), k).items()} for k in range(1, 5)]
        for j, sent in enumerate([hyp] + rr):
            vec = [{g: float(c) * float(idf[want['df'].get(g, 0)]) for g, c in C._ngrams(sent.split(), k).items()} for k in range(1, 5)]
            for k in range(4):
                acc = 0.0
                for v in vec[k].values():           # a Counter keeps first-occurrence order
                    acc += v * v
                assert acc == sums['norm2'][s, k]
                if j:
                    acc = 0.0
                    for g, v in hv[k].items():
                        acc += min(v, vec[k].get(g, 0.0)) * vec[k].get(g, 0.0)
                    assert acc == sums['num'][p, k]
            s += 1
            p += 1 if j else 0
    assert s == corpus['S'] and p == corpus['S'] - corpus['N']
    res = _summary(hyps, refs)
    assert np.isfinite(res['cider']).all() and 0 <= res['ROUGE_L'] <= 1 and (res['bleu'] >= 0).all()


def test_idf_table():
    t = CE.idf_table_host(12)
    assert t.shape == (13,) and t[0] == t[1] == np.log(12.0) and t[12] == 0.0 and t[3] == np.log(12.0) - np.log(3.0)
    one = CE.idf_table_host(1)
    assert one.tolist() == [1.0, 1.0]                    # ref_len = 1, the reference's branch for a single image


def test_the_token_streams_round_trip():
    hyps, refs = C.fixture_corpus('a')
    hyps, refs = hyps + C.edge_corpus()[0], refs + C.edge_corpus()[1]
    corpus = CE.intern_corpus_host(hyps, refs)
    assert corpus['N'] == len(hyps) and corpus['S'] == len(hyps) + sum(len(r) for r in refs) == len(corpus['sent_off']) - 1
    assert corpus['words'].dtype == corpus['sent_off'].dtype == corpus['img_off'].dtype == np.int32
    assert corpus['words'].min() >= 1 and max(corpus['words'].max(), corpus['words_sp'].max()) == corpus['V'] == len(corpus['vocab'])
    # split(" ") loses nothing; split() gives the strings with single spaces
    assert CE.corpus_strings(corpus, '_sp') == list(zip(hyps, refs))
    assert CE.corpus_strings(corpus, '') == [(' '.join(h.split()), [' '.join(r.split()) for r in rr]) for h, rr in zip(hyps, refs)]
    i = hyps.index('a  man on a horse ')
    s = corpus['img_off'][i]
    assert corpus['sent_off'][s + 1] - corpus['sent_off'][s] == 5 and corpus['sent_off_sp'][s + 1] - corpus['sent_off_sp'][s] == 7
    i = hyps.index('')
    s = corpus['img_off'][i]
    assert corpus['sent_off'][s + 1] == corpus['sent_off'][s] and corpus['sent_off_sp'][s + 1] - corpus['sent_off_sp'][s] == 1
    # case and punctuation are kept apart
    assert len({corpus['vocab'].index(t) for t in ('A', 'a', 'horse', 'horse.')}) == 4
    assert CE.corpus_limits(corpus) == (corpus['V'], 11, 7)
    with pytest.raises(ValueError):
        CE.intern_corpus_host(['a'], [])
    with pytest.raises(ValueError, match='at least one reference'):
        CE.CaptionEvaluator().add('a', [])


def test_records_of_two_ranks_merge_to_the_summary_of_one_evaluator():
    hyps, refs = C.random_corpus(5, 11, 3, 2, 10, 12)
    whole = _summary(hyps, refs)
    rank0, rank1 = CE.CaptionEvaluator(), CE.CaptionEvaluator()
    rank0.add_batch(hyps[:6], refs[:6])
    for h, r in zip(hyps[6:], refs[6:]):
        rank1.add(h, r)
    assert rank1.records() == list(zip(hyps[6:], refs[6:]))
    C.assert_summaries_equal(rank0.summarize(extra_records=rank1.records()), whole)
    C.assert_summaries_equal(CE.CaptionEvaluator().summarize(extra_records=rank0.records() + rank1.records()), whole)
    assert rank0.summarize()['images'] == 6                 # the evaluator's own records are untouched
    text = CE.format_caption_summary(whole).splitlines()
    assert [t.split(' = ')[0] for t in text] == ['BLUE-1', 'BLUE-2', 'BLUE-3', 'BLUE-4', 'CIDEr', 'Rouge']
    assert text[4] == f'CIDEr = {whole["CIDEr"]:0.3f}'
    with pytest.raises(ValueError, match='no image'):
        CE.CaptionEvaluator().summarize()


def test_the_entry_points_validate_without_a_device():
    """the header's conventions: CGG_EINVAL = -1, CGG_EUNSUPPORTED = -2, an empty corpus is legal and launches nothing"""
    import ctypes
    from cgg_amd import _lib, ops
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cgg_caption_bleu_lcs_i32(null, null, 0, null, null, 0, null, 0, 0, null, null, null) == 0           # N = 0
    assert lib.cgg_caption_ngram_keys_i64(null, null, 0, null, 0, 0, null, null, null) == 0
    assert lib.cgg_cider_sums_f64(null, null, 0, null, null, 0, null, 0, 0, null, null, null) == 0
    assert lib.cgg_caption_bleu_lcs_i32(p, p, 4, p, p, 4, p, 2, 1, p, p, null) == -1                               # S < N
    assert lib.cgg_caption_bleu_lcs_i32(p, null, 4, p, p, 4, p, 1, 2, p, p, null) == -1 and b'null' in lib.cgg_last_error_string()
    assert lib.cgg_caption_ngram_keys_i64(p, p, (1 << 28) + 1, p, 1, 2, p, p, null) == -2                          # too many words
    odd = ctypes.c_void_p(((p.value + 7) & ~7) + 4)
    assert lib.cgg_caption_ngram_keys_i64(p, p, 4, p, 1, 2, odd, p, null) == -1                                    # keys misaligned
    assert lib.cgg_cider_sums_f64(p, p, -1, p, p, 4, p, 1, 2, p, p, null) == -1
    assert lib.cgg_cider_sums_f64(p, p, 0, p, p, 4, p, 1, 2, p, p, null) == -1                                     # words without ids
    assert (ops.CAPTION_MAX_LEN, ops.CAPTION_MAX_REFS, ops.CAPTION_MAX_VOCAB) == (128, 32, 65535)
    assert ops.caption_eval_ok(65535, 128, 32) and not ops.caption_eval_ok(65536, 128, 32)
    assert not ops.caption_eval_ok(1, 129, 1) and not ops.caption_eval_ok(1, 1, 33)


def _driver():
    spec = importlib.util.spec_from_file_location('cgg_tools_test_caption_args', os.path.join(ROOT, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_the_driver_parses_eval_caption(tmp_path):
    drv = _driver()
    a = drv.parse_args(['cfg.py', 'none', '--eval', 'caption', '--caption-vocab', 'vocab.txt', '--synthetic-captions'])
    assert a.eval == ['caption'] and a.caption_vocab == 'vocab.txt' and a.synthetic_captions is True
    a = drv.parse_args(['cfg.py', 'none', '--eval', 'segm', 'caption'])
    assert a.eval == ['segm', 'caption'] and a.caption_vocab is None and a.synthetic_captions is False
    # without a vocabulary file or a cached tokenizer the run ends by naming the option
    with pytest.raises(SystemExit, match='--caption-vocab'):
        drv.caption_tokenizer(str(tmp_path / 'missing_vocab.txt'))
    from cgg_amd import synthetic
    gt = synthetic.caption_ground_truth(3, 4)
    assert gt == synthetic.caption_ground_truth(3, 4) and gt != synthetic.caption_ground_truth(4, 4)
    assert len(gt) == 4 and all(isinstance(r, str) and r for refs in gt for r in refs) and all(len(refs) >= 1 for refs in gt)
