"""Shared inputs of the caption-metric tests: fixture G16 (made by tests/golden/make_golden_caption.py, which executes the reference's
bleu.py, cider.py and rouge.py), a hand-made edge set, seeded corpora, and an independent statement of the integer parts with
`collections.Counter` on the strings themselves."""
import collections
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_caption_eval.npz')
INT_KEYS = ('testlen', 'reflen', 'guess', 'correct', 'lcs', 'df_pos')
F64_KEYS = ('norm2', 'num')
SCORES = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'CIDEr', 'ROUGE_L')


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_corpus(tag='a'):
    """-> (hyps, refs) of run 'a' (12 images) or 'b' (1 image)"""
    z = fixture()
    hyps = [str(h) for h in z[tag + '_hyps']]
    refs = [[] for _ in hyps]
    for r, i in zip(z[tag + '_refs'], z[tag + '_ref_img']):
        refs[int(i)].append(str(r))
    return hyps, refs


def edge_corpus():
    """Hand-made, each image one edge of the kernels (every image's references hold "x", so its idf is 0):
    0  hypothesis and reference equal               1  no common token                   2  the empty hypothesis
    3  an empty REFERENCE next to a real one        4  one token against one token       5  n-grams that repeat with a period of 2
    6  the same reference three times               7  only spaces: split() is empty, split(" ") holds empty tokens
    8  a 4-gram that matches at the very end of both sentences                           9  hypothesis longer than every reference"""
    return (['x y z w', 'p q r', '', 'x y', 'x', 'x y x y x y x', 'x y z', '   ', 'k l x y z w', 'x y z w v u t s r q p'],
            [['x y z w'], ['x s t'], ['x y'], ['', 'x y z'], ['x'], ['y x y x', 'x y x'], ['x y z', 'x y z', 'x y z'], ['x', ' x '],
             ['m x y z w'], ['x y', 'z w x']])


def random_corpus(seed, N, R, Lmin, Lmax, V, spaces=True):
    """Seeded corpus: N images of R references each, sentences of Lmin .. Lmax tokens from w0 .. w{V-1} (drawn with a skew towards the
    low indices, so that n-grams repeat), the hypothesis a corrupted copy of one reference: tokens replaced, dropped or doubled, cut
    to Lmax. Every fourth image's hypothesis is made of tokens no reference of the corpus uses (CIDEr exactly 0), every seventh is
    empty; with `spaces`, now and then a double space or a trailing space (they lengthen the split(" ") stream). The last token of
    one reference of every image is "w0", and reference 0 of image 0 is "w0" alone: the unigram has idf 0, that sentence norm 0."""
    rs = np.random.RandomState(seed)

    def sentence(L):
        idx = np.minimum(rs.randint(0, V, L), rs.randint(0, V, L))
        return ['w%d' % i for i in idx]

    hyps, refs = [], []
    for n in range(N):
        rr = [sentence(int(rs.randint(Lmin, Lmax + 1))) for _ in range(R)]
        k = int(rs.randint(R))
        rr[k] = rr[k][:-1] + ['w0']
        if n == 0:
            rr[0] = ['w0']
        src = list(rr[int(rs.randint(R))])
        hyp = []
        for t in src:
            u = rs.rand()
            if u < 0.08:
                hyp.append('w%d' % rs.randint(V))
            elif u < 0.12:
                continue
            elif u < 0.17:
                hyp += [t, t]
            else:
                hyp.append(t)
        hyp = hyp[:Lmax]
        if n % 4 == 1:
            hyp = ['u%d' % rs.randint(5) for _ in range(int(rs.randint(max(Lmin, 1), Lmax + 1)))]
        if n % 7 == 6:
            hyp = []
        sep = ['  ' if spaces and rs.rand() < 0.1 else ' ' for _ in hyp]
        h = ''.join(t + s for t, s in zip(hyp, sep))
        hyps.append(h if spaces and rs.rand() < 0.2 else h.rstrip(' '))
        refs.append([' '.join(r) for r in rr])
    return hyps, refs


# ---- the integer parts once more, on strings, with collections.Counter --------------------------------
def _ngrams(tokens, k):
    return collections.Counter(tuple(tokens[i:i + k]) for i in range(len(tokens) - k + 1))


def counter_components(hyps, refs):
    """testlen, reflen, guess, correct, lcs, df (n-gram of strings -> images) stated independently of caption_eval"""
    testlen, reflen, guess, correct, lcs = [], [], [], [], []
    df = collections.Counter()
    for hyp, rr in zip(hyps, refs):
        h = hyp.split()
        testlen.append(len(h))
        lens = [len(r.split()) for r in rr]
        best = min(abs(l - len(h)) for l in lens)
        reflen.append(min(l for l in lens if abs(l - len(h)) == best))
        guess.append([max(0, len(h) - k) for k in range(4)])
        row = []
        for k in range(1, 5):
            hc = _ngrams(h, k)
            clip = collections.Counter()
            for r in rr:
                clip |= _ngrams(r.split(), k)        # the maximum of the counts
            row.append(sum((hc & clip).values()))      # the minimum of the counts
        correct.append(row)
        seen = set()
        for r in rr:
            for k in range(1, 5):
                seen |= set(_ngrams(r.split(), k))
        df.update(seen)
        a = hyp.split(' ')
        for r in rr:
            b = r.split(' ')
            prev = [0] * (len(b) + 1)
            for x in a:                                 # row by row over the hypothesis, the other way round than my_lcs
                cur = [0]
                for j, y in enumerate(b):
                    cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
                prev = cur
            lcs.append(prev[-1])
    return dict(testlen=np.array(testlen, np.int32), reflen=np.array(reflen, np.int32), guess=np.array(guess, np.int32).reshape(-1, 4),
                correct=np.array(correct, np.int32).reshape(-1, 4), lcs=np.array(lcs, np.int32), df=df)


def df_pos_from(df, hyps, refs):
    """the (W, 4) table of `caption_eval.ngram_df_host` from a df over n-grams of strings"""
    rows = []
    for hyp, rr in zip(hyps, refs):
        for s in [hyp] + list(rr):
            t = s.split()
            for i in range(len(t)):
                rows.append([df.get(tuple(t[i:i + k]), 0) if i + k <= len(t) else -1 for k in range(1, 5)])
    return np.array(rows, np.int32).reshape(-1, 4)


def assert_components_equal(a, b, where=''):
    """the integer arrays as arrays, the double sums by their bit patterns"""
    for k in INT_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), (where, k, x, y)
    for k in F64_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype == np.float64 and x.shape == y.shape, (where, k)
        bad = np.nonzero(x.view(np.int64).reshape(-1) != y.view(np.int64).reshape(-1))[0]
        assert bad.size == 0, (where, k, bad[:5], x.reshape(-1)[bad[:5]], y.reshape(-1)[bad[:5]])


def assert_summaries_equal(a, b, where=''):
    assert_components_equal(a, b, where)
    for k in SCORES:
        assert np.float64(a[k]).view(np.int64) == np.float64(b[k]).view(np.int64), (where, k, a[k], b[k])
    for k in ('bleu', 'cider', 'rouge'):
        assert a[k].shape == b[k].shape and a[k].view(np.int64).tolist() == b[k].view(np.int64).tolist(), (where, k)
    assert (a['total_testlen'], a['total_reflen'], a['images']) == (b['total_testlen'], b['total_reflen'], b['images']), where
