#!/usr/bin/env python
"""Generate tests/golden/g16_caption_eval.npz by EXECUTING THE REFERENCE'S OWN caption scorers: open_set/utils/eval/caption/bleu/bleu.py
(+ bleu_scorer.py), cider/cider.py (+ cider_scorer.py) and rouge/rouge.py, as `eval_cap_results` (open_set/datasets/coco_open.py:
745-781) calls them: Bleu(n=4), Cider(), Rouge() on gts = {image: [references]}, res = {image: [hypothesis]}.

Runs only where the reference tree is at hand; the fixture (inputs + recorded outputs, no reference source) is committed and is
what travels. Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_caption.py REFERENCE_ROOT
(the variable keeps Python from writing __pycache__ into the reference tree; the script sets it for itself as well).

NOTHING IS STUBBED: the three directories are loaded as packages with importlib, so that their relative imports resolve, and they
need numpy only. Recorded: the inputs; per image the BLEU components of `ctest` (testlen, guess, correct, the list of reference
lengths) and the closest length by the scorer's own `_single_reflen`; `_testlen` / `_reflen`; BLEU-1..4, CIDEr and ROUGE-L per image
and per corpus; CIDEr's document frequencies; `my_lcs` of every pair on the split(" ") tokens.

Run 'a', 12 images:
  0   an ordinary image, 5 references                          1   an EMPTY hypothesis
  2   a hypothesis of 1 word, "a": the unigram occurs in the references of EVERY image (idf = 0), so every norm of this
      sentence is 0 and the division is skipped; one of its references is "a" as well (a reference of norm 0)
  3   a hypothesis of 2 words                                  4   a hypothesis of 3 words  (guess holds zeros in 1 .. 4)
  5   "a a a a a cat cat" against the single reference "a cat": clipping (correct < count), an image with 1 reference
  6   a hypothesis of 5 words against references of 6 and 4 words, the longer one first: the tie takes the shorter
  7   7 references                                             8   double spaces and a trailing space: split() and split(" ") differ
  9   hypothesis n-grams that no reference holds (its CIDEr is 0)
  10  case and punctuation variants: A / a, horse / horse.     11  a hypothesis equal to one of its references
Run 'b', 1 image: the `ref_len = 1` branch of compute_cider.
"""
import importlib
import importlib.util
import os
import sys

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True

import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

RUN_A = [
    ('a man riding a horse on a beach', ['a man rides a horse along the beach', 'a person riding a horse on a beach', 'man on a horse near the sea',
                                         'a man is riding a brown horse on the sand', 'the rider and a horse on a beach']),
    ('', ['a cat sits on a mat', 'there is a cat']),
    ('a', ['a', 'a dog', 'one dog in a park']),
    ('a dog', ['a dog runs', 'the dog and a ball']),
    ('a red bus', ['a red bus on a street', 'a bus that is red']),
    ('a a a a a cat cat', ['a cat']),
    ('two dogs play in snow', ['two dogs play in a field', 'dogs in a field']),
    ('a plate of food on a table', ['a plate of food', 'food on a table', 'a table with a plate of food on it', 'a white plate with food',
                                    'some food sits on a plate on a table', 'a plate on a table', 'a meal']),
    ('a  man on a horse ', ['a man  rides a horse', 'a man on  a horse ', ' a man on a horse']),
    ('zebra crossing nowhere fast', ['a street with a sign', 'a sign on a pole']),
    ('A horse.', ['a horse', 'A horse', 'a horse. A horse.']),
    ('a kite flies over a hill', ['a kite flies over a hill', 'a kite in the sky over a hill']),
]
RUN_B = [('a man riding a horse', ['a man rides a horse', 'the man on a horse'])]


def load_reference_scorers(ref_root):
    base = os.path.join(ref_root, 'open_set', 'utils', 'eval', 'caption')
    mods = {}
    for pkg, leaf in (('bleu', 'bleu'), ('cider', 'cider'), ('rouge', 'rouge')):
        name = 'ref_caption_' + pkg
        d = os.path.join(base, pkg)
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, '__init__.py'), submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[pkg] = importlib.import_module(f'{name}.{leaf}')
    mods['bleu_scorer'] = sys.modules['ref_caption_bleu.bleu_scorer']
    mods['cider_scorer'] = sys.modules['ref_caption_cider.cider_scorer']
    return mods


def run(mods, images, tag):
    gts = {i: list(refs) for i, (_, refs) in enumerate(images)}
    res = {i: [hyp] for i, (hyp, _) in enumerate(images)}
    out = {tag + '_hyps': np.array([h for h, _ in images], dtype=np.str_),
           tag + '_refs': np.array([r for _, refs in images for r in refs], dtype=np.str_),
           tag + '_ref_img': np.array([i for i, (_, refs) in enumerate(images) for _ in refs], np.int64)}
    # BLEU: `Bleu.compute_score`, then the same scorer class again for its internals (Bleu keeps its scorer to itself)
    score, scores = mods['bleu'].Bleu(n=4).compute_score(gts, res)
    out[tag + '_bleu'] = np.array(score, np.float64)
    out[tag + '_bleu_img'] = np.array(scores, np.float64).T
    scorer = mods['bleu_scorer'].BleuScorer(n=4)
    for i in gts:
        scorer += (res[i][0], gts[i])
    again, _ = scorer.compute_score(option='closest')
    assert list(again) == list(score)
    out[tag + '_testlen'] = np.array([c['testlen'] for c in scorer.ctest], np.int64)
    out[tag + '_guess'] = np.array([c['guess'] for c in scorer.ctest], np.int64)
    out[tag + '_correct'] = np.array([c['correct'] for c in scorer.ctest], np.int64)
    out[tag + '_reflens'] = np.array([l for c in scorer.ctest for l in c['reflen']], np.int64)
    out[tag + '_reflen'] = np.array([scorer._single_reflen(c['reflen'], 'closest', c['testlen']) for c in scorer.ctest], np.int64)
    out[tag + '_total_testlen'] = np.int64(scorer._testlen)
    out[tag + '_total_reflen'] = np.int64(scorer._reflen)
    # CIDEr
    score, scores = mods['cider'].Cider().compute_score(gts, res)
    out[tag + '_cider'] = np.float64(score)
    out[tag + '_cider_img'] = np.array(scores, np.float64)
    cs = mods['cider_scorer'].CiderScorer(n=4, sigma=6.0)
    for i in gts:
        cs += (res[i][0], gts[i])
    cs.compute_doc_freq()
    grams = sorted(cs.document_frequency)
    out[tag + '_df_ngrams'] = np.array(['\t'.join(g) for g in grams], dtype=np.str_)
    out[tag + '_df'] = np.array([cs.document_frequency[g] for g in grams], np.float64)
    # ROUGE-L
    rouge = mods['rouge']
    score, scores = rouge.Rouge().compute_score(gts, res)
    out[tag + '_rouge'] = np.float64(score)
    out[tag + '_rouge_img'] = np.array(scores, np.float64)
    out[tag + '_lcs'] = np.array([rouge.my_lcs(r.split(' '), h.split(' ')) for h, refs in images for r in refs], np.int64)
    return out


def main(ref_root):
    mods = load_reference_scorers(ref_root)
    out = {}
    out.update(run(mods, RUN_A, 'a'))
    out.update(run(mods, RUN_B, 'b'))
    path = os.path.join(HERE, 'g16_caption_eval.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')
    for tag in ('a', 'b'):
        print(tag, 'bleu', out[tag + '_bleu'], 'cider', out[tag + '_cider'], 'rouge', out[tag + '_rouge'])
        print(tag, 'cider per image', out[tag + '_cider_img'])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
