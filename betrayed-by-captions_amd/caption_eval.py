"""Caption metrics (`--eval caption`): BLEU-1..4, CIDEr and ROUGE-L of one hypothesis per image against its references. The rules in
plain Python / numpy, and `CaptionEvaluator`, which runs them on the host or hands every per-n-gram step to the device
(csrc/caption_eval.hip through `ops.caption_bleu_lcs` / `ops.caption_ngram_keys` / `ops.cider_sums`).

The rules restate the scorers that the reference's `eval_cap_results` (open_set/datasets/coco_open.py:745-781) calls, under
open_set/utils/eval/caption/, without importing them. Each scorer is split where integers or ordered IEEE sums end and libm begins:

  intern_corpus_host     the two tokenisations: `s.split()` (BLEU, CIDEr) and `s.split(" ")` (ROUGE-L), as int32 ids
  bleu_components_host   `cook_refs` / `cook_test` (bleu_scorer.py:35-84) with option 'closest': integers
  bleu_finish_host       `BleuScorer.compute_score` from bleu_scorer.py:199 on, literally
  lcs_host               `my_lcs` (rouge.py:13-34): integers;   rouge_finish_host   `Rouge.calc_score` / `compute_score` (:45-102)
  ngram_df_host          `compute_doc_freq` (cider_scorer.py:93-104): integers;   idf_table_host   ref_len - np.log(max(1.0, df))
  cider_sums_host        the sums of `counts2vec` and `sim` (cider_scorer.py:107-151): ordered double sums
  cider_finish_host      the rest of `sim` and `compute_cider` (:130, :153-182) and the corpus mean (:193)

Nothing is lower-cased or stripped: the reference scores the raw annotation strings against the decoded hypothesis, and so does
this. Nothing is claimed about pycocoevalcap's PTB tokenizer, which the reference does not call either.

ONE DELIBERATE DEVIATION: the reference squares a tf-idf weight with `pow(v, 2)`, libm's pow, which differs from `v * v` in the last
bit for about one value in a thousand; the rule here is `v * v`, and no equality with a particular libm is claimed.
"""
import math

import numpy as np

N_ORDERS = 4
SCORE_NAMES = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'CIDEr', 'ROUGE_L')      # the six numbers of a summary
SIGMA = 6.0
BETA = 1.2


# ------------------------------------------------------------------------------------------------
# tokens
# ------------------------------------------------------------------------------------------------
def intern_corpus_host(hyps, refs):
    """hyps: N strings; refs: N lists of strings. -> dict(words, sent_off, words_sp, sent_off_sp, img_off, vocab, N, S, V).

    Sentences in order: per image its hypothesis, then its references; img_off int32 (N + 1,) = the first sentence of every image.
    words / sent_off: the `s.split()` stream -- token ids int32 and the first word of every sentence (S + 1,); words_sp /
    sent_off_sp: the `s.split(" ")` stream of the same sentences, where "a  b" has three tokens and "" has one, the empty token.
    ids are 1 .. V in order of first appearance, shared by both streams (0 is padding and never appears); vocab[id - 1] = the token."""
    if len(hyps) != len(refs):
        raise ValueError(f'intern_corpus_host: {len(hyps)} hypotheses, {len(refs)} reference lists')
    ids = {}
    words, words_sp, sent_off, sent_off_sp, img_off = [], [], [0], [0], [0]
    for hyp, rs in zip(hyps, refs):
        rs = list(rs)
        for s in [hyp] + rs:
            if not isinstance(s, str):
                raise TypeError(f'intern_corpus_host: a sentence must be a str (got {type(s).__name__})')
            for tok in s.split():
                words.append(ids.setdefault(tok, len(ids) + 1))
            sent_off.append(len(words))
            for tok in s.split(' '):
                words_sp.append(ids.setdefault(tok, len(ids) + 1))
            sent_off_sp.append(len(words_sp))
        img_off.append(len(sent_off) - 1)
    return dict(words=np.array(words, np.int32).reshape(-1), sent_off=np.array(sent_off, np.int32),
                words_sp=np.array(words_sp, np.int32).reshape(-1), sent_off_sp=np.array(sent_off_sp, np.int32),
                img_off=np.array(img_off, np.int32), vocab=list(ids), N=len(hyps), S=len(sent_off) - 1, V=len(ids))


def corpus_sentences(corpus, stream=''):
    """-> per image the list of its sentences (hypothesis first) as lists of ids; stream '' = split(), '_sp' = split(" ")"""
    words, off, img = corpus['words' + stream].tolist(), corpus['sent_off' + stream].tolist(), corpus['img_off'].tolist()
    return [[words[off[s]:off[s + 1]] for s in range(img[n], img[n + 1])] for n in range(len(img) - 1)]


def corpus_strings(corpus, stream='_sp'):
    """the sentences back as strings, per image (hypothesis, [references]): ' '.join of the tokens. The split(" ") stream gives the
    original strings back exactly; the split() stream gives them with every run of whitespace as one space"""
    vocab = corpus['vocab']
    return [(' '.join(vocab[t - 1] for t in sents[0]), [' '.join(vocab[t - 1] for t in s) for s in sents[1:]])
            for sents in corpus_sentences(corpus, stream)]


def _precook(words, n=N_ORDERS):
    """`precook` (bleu_scorer.py:23-33, cider_scorer.py:11-26): n-gram -> count, a dict in insertion order: by order k, then position"""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            ngram = tuple(words[i:i + k])
            counts[ngram] = counts.get(ngram, 0) + 1
    return counts


# ------------------------------------------------------------------------------------------------
# BLEU
# ------------------------------------------------------------------------------------------------
def bleu_components_host(corpus):
    """`cook_refs` + `cook_test` with the reference length of option 'closest' (bleu_scorer.py:35-84, :189), per image, integers:
    dict(testlen (N,), reflen (N,), guess (N, 4), correct (N, 4)) int32."""
    N = corpus['N']
    out = dict(testlen=np.zeros(N, np.int32), reflen=np.zeros(N, np.int32), guess=np.zeros((N, 4), np.int32),
               correct=np.zeros((N, 4), np.int32))
    for i, sents in enumerate(corpus_sentences(corpus)):
        reflen, maxcounts = [], {}
        for ref in sents[1:]:
            counts = _precook(ref)
            reflen.append(len(ref))
            for ngram, count in counts.items():
                maxcounts[ngram] = max(maxcounts.get(ngram, 0), count)
        testlen, counts = len(sents[0]), _precook(sents[0])
        out['testlen'][i] = testlen
        out['reflen'][i] = min((abs(l - testlen), l) for l in reflen)[1]
        out['guess'][i] = [max(0, testlen - k + 1) for k in range(1, N_ORDERS + 1)]
        correct = [0] * N_ORDERS
        for ngram, count in counts.items():
            correct[len(ngram) - 1] += min(maxcounts.get(ngram, 0), count)
        out['correct'][i] = correct
    return out


def bleu_finish_host(comp):
    """`BleuScorer.compute_score` from bleu_scorer.py:199 on (option 'closest', so `_single_reflen` has been applied already):
    -> (bleus: 4 floats, bleu_list: 4 lists of N floats, total testlen, total reflen)."""
    n = N_ORDERS
    small = 1e-9
    tiny = 1e-15  # so that if guess is 0 still return 0
    bleu_list = [[] for _ in range(n)]
    _testlen = 0
    _reflen = 0
    totalcomps = {'testlen': 0, 'reflen': 0, 'guess': [0] * n, 'correct': [0] * n}
    for i in range(len(comp['testlen'])):
        comps = dict(testlen=int(comp['testlen'][i]), reflen=int(comp['reflen'][i]), guess=[int(v) for v in comp['guess'][i]],
                     correct=[int(v) for v in comp['correct'][i]])
        testlen = comps['testlen']
        _testlen += testlen
        reflen = comps['reflen']
        _reflen += reflen
        for key in ['guess', 'correct']:
            for k in range(n):
                totalcomps[key][k] += comps[key][k]
        bleu = 1.
        for k in range(n):
            bleu *= (float(comps['correct'][k]) + tiny) / (float(comps['guess'][k]) + small)
            bleu_list[k].append(bleu ** (1. / (k + 1)))
        ratio = (testlen + tiny) / (reflen + small)  # N.B.: avoid zero division
        if ratio < 1:
            for k in range(n):
                bleu_list[k][-1] *= math.exp(1 - 1 / ratio)
    totalcomps['reflen'] = _reflen
    totalcomps['testlen'] = _testlen
    bleus = []
    bleu = 1.
    for k in range(n):
        bleu *= float(totalcomps['correct'][k] + tiny) / (totalcomps['guess'][k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (_testlen + tiny) / (_reflen + small)  # N.B.: avoid zero division
    if ratio < 1:
        for k in range(n):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus, bleu_list, _testlen, _reflen


# ------------------------------------------------------------------------------------------------
# ROUGE-L
# ------------------------------------------------------------------------------------------------
def _my_lcs(string, sub):
    """`my_lcs` (rouge.py:13-34)"""
    if len(string) < len(sub):
        sub, string = string, sub
    lengths = [[0 for i in range(0, len(sub) + 1)] for j in range(0, len(string) + 1)]
    for j in range(1, len(sub) + 1):
        for i in range(1, len(string) + 1):
            if string[i - 1] == sub[j - 1]:
                lengths[i][j] = lengths[i - 1][j - 1] + 1
            else:
                lengths[i][j] = max(lengths[i - 1][j], lengths[i][j - 1])
    return lengths[len(string)][len(sub)]


def lcs_host(corpus):
    """LCS length of every (hypothesis, reference) pair in the split(" ") stream: int32 (P,), pairs in sentence order"""
    out = []
    for sents in corpus_sentences(corpus, '_sp'):
        out.extend(_my_lcs(ref, sents[0]) for ref in sents[1:])
    return np.array(out, np.int32).reshape(-1)


def rouge_finish_host(lcs, corpus, beta=BETA):
    """`Rouge.calc_score` per image and the mean of `compute_score` (rouge.py:45-102) -> (mean, scores (N,) float64)"""
    off, img = corpus['sent_off_sp'].tolist(), corpus['img_off'].tolist()
    score, p = [], 0
    for n in range(corpus['N']):
        len_c = off[img[n] + 1] - off[img[n]]
        prec, rec = [], []
        for s in range(img[n] + 1, img[n + 1]):
            len_r = off[s + 1] - off[s]
            l = int(lcs[p])
            p += 1
            prec.append(l / float(len_c))
            rec.append(l / float(len_r))
        prec_max = max(prec)
        rec_max = max(rec)
        if prec_max != 0 and rec_max != 0:
            score.append(((1 + beta ** 2) * prec_max * rec_max) / float(rec_max + beta ** 2 * prec_max))
        else:
            score.append(0.0)
    return np.mean(np.array(score)), np.array(score)


# ------------------------------------------------------------------------------------------------
# CIDEr
# ------------------------------------------------------------------------------------------------
def ngram_df_host(corpus):
    """`compute_doc_freq` (cider_scorer.py:93-104): df[g] = the number of images whose references contain n-gram g.
    -> (df: dict n-gram (tuple of ids) -> int, df_pos int32 (W, 4): the df of the n-gram of order k + 1 that starts at every word of
    the split() stream -- 0 for a hypothesis n-gram that no reference holds --, -1 where the sentence ends before it does)"""
    df = {}
    sents = corpus_sentences(corpus)
    for image in sents:
        for ngram in set(ngram for ref in image[1:] for ngram in _precook(ref)):
            df[ngram] = df.get(ngram, 0) + 1
    df_pos = np.full((len(corpus['words']), N_ORDERS), -1, np.int32)
    w = 0
    for image in sents:
        for s in image:
            for i in range(len(s)):
                for k in range(min(N_ORDERS, len(s) - i)):
                    df_pos[w + i, k] = df.get(tuple(s[i:i + k + 1]), 0)
            w += len(s)
    return df, df_pos


def idf_table_host(N):
    """float64 (N + 1,): idf of a document frequency 0 .. N, as cider_scorer.py:120-124, :162-164 compute it, one scalar numpy call per
    entry: `ref_len - np.log(max(1.0, df))` with ref_len = np.log(float(N)), and the integer 1 when N == 1. Made on the host in both
    routes; the device only looks it up."""
    ref_len = np.log(float(N)) if N > 0 else 0.0
    if N == 1:
        ref_len = 1
    return np.array([ref_len - np.log(max(1.0, float(d))) for d in range(N + 1)], np.float64)


def cider_sums_host(corpus, df=None, idf_table=None):
    """The ordered sums of `counts2vec` and `sim` (cider_scorer.py:107-151). With v = float(tf) * idf for an n-gram of a sentence:
    norm2 float64 (S, 4) = sum of v * v over the sentence's distinct n-grams of each order, in the insertion order of `precook`'s
    dict (within an order: by first position); num float64 (P, 4) = sum over the hypothesis' distinct n-grams, in that order, of
    min(v_hyp, v_ref) * v_ref, v_ref = 0.0 for an n-gram the reference lacks. Every product and add is one double operation."""
    if df is None:
        df = ngram_df_host(corpus)[0]
    if idf_table is None:
        idf_table = idf_table_host(corpus['N'])
    norm2, num = [], []

    def counts2vec(cnts):
        vec = [{} for _ in range(N_ORDERS)]
        norm = [0.0 for _ in range(N_ORDERS)]
        for ngram, term_freq in cnts.items():
            n = len(ngram) - 1
            v = float(term_freq) * float(idf_table[df.get(ngram, 0)])
            vec[n][ngram] = v
            norm[n] += v * v
        return vec, norm

    for image in corpus_sentences(corpus):
        vec, norm = counts2vec(_precook(image[0]))
        norm2.append(norm)
        for ref in image[1:]:
            vec_ref, norm_ref = counts2vec(_precook(ref))
            norm2.append(norm_ref)
            val = [0.0 for _ in range(N_ORDERS)]
            for n in range(N_ORDERS):
                for ngram in vec[n]:
                    v_ref = vec_ref[n].get(ngram, 0.0)
                    val[n] += min(vec[n][ngram], v_ref) * v_ref
            num.append(val)
    return dict(norm2=np.array(norm2, np.float64).reshape(-1, N_ORDERS), num=np.array(num, np.float64).reshape(-1, N_ORDERS))


def cider_finish_host(norm2, num, corpus, sigma=SIGMA):
    """The rest of `counts2vec` / `sim` / `compute_cider` / `compute_score` (cider_scorer.py:128-131, :144, :153-182, :193) ->
    (mean, scores (N,) float64). `length` is the reference's own: it sums tf where len(ngram) - 1 == 1, the bigrams, so it is
    max(0, L - 1) of the split() stream."""
    off, img = corpus['sent_off'].tolist(), corpus['img_off'].tolist()
    scores, p = [], 0
    for i in range(corpus['N']):
        h = img[i]
        norm = [np.sqrt(v) for v in norm2[h]]
        length = max(0, off[h + 1] - off[h] - 1)
        score = np.array([0.0 for _ in range(N_ORDERS)])
        refs = range(h + 1, img[i + 1])
        for s in refs:
            norm_ref = [np.sqrt(v) for v in norm2[s]]
            length_ref = max(0, off[s + 1] - off[s] - 1)
            delta = float(length - length_ref)
            val = np.array([float(v) for v in num[p]])
            p += 1
            for n in range(N_ORDERS):
                if (norm[n] != 0) and (norm_ref[n] != 0):
                    val[n] /= (norm[n] * norm_ref[n])
                assert not math.isnan(val[n])
                val[n] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
            score += val
        score_avg = np.mean(score)
        score_avg /= len(refs)
        score_avg *= 10.0
        scores.append(score_avg)
    return np.mean(np.array(scores)), np.array(scores)


# ------------------------------------------------------------------------------------------------
# the evaluator
# ------------------------------------------------------------------------------------------------
def corpus_limits(corpus):
    """(V, the longest sentence of either stream, the most references of an image): what `ops.caption_eval_ok` decides on"""
    longest = max([0] + np.diff(corpus['sent_off']).tolist() + np.diff(corpus['sent_off_sp']).tolist())
    return corpus['V'], int(longest), int(max([0] + (np.diff(corpus['img_off']) - 1).tolist()))


def format_caption_summary(res):
    """the lines `eval_cap_results` prints (coco_open.py:766-781), without its timings"""
    lines = [f'BLUE-{k} = {res["Bleu_%d" % k]:0.3f}' for k in range(1, N_ORDERS + 1)]
    lines.append(f'CIDEr = {res["CIDEr"]:0.3f}')
    lines.append(f'Rouge = {res["ROUGE_L"]:0.3f}')
    return '\n'.join(lines)


class CaptionEvaluator:
    """BLEU-1..4, CIDEr and ROUGE-L of a stream of images, each one hypothesis string against its reference strings.

    add(hyp, refs) takes one image, add_batch(hyps, refs_list) a batch; an image needs at least one reference. records() gives the
    strings back, [(hyp, [refs])] in `add` order: what a distributed run gathers. summarize(extra_records=None) scores this
    evaluator's records followed by `extra_records` (those of other ranks), so that rank 0 scores all images in image order.

    CIDEr's document frequencies span the corpus, so nothing is scored before `summarize`. device=None: the numpy rules of this
    module. With a device, `summarize` interns the strings on the host, makes ONE upload of the id streams and the idf table, runs
    the three kernels (`ops.caption_bleu_lcs`, `ops.caption_ngram_keys` with torch.unique / torch.bincount for the n-gram ids and
    their df, `ops.cider_sums`), makes ONE copy back of the integer and double arrays and hands them to the same `*_finish_host`
    functions. A corpus outside `ops.caption_eval_ok` takes the numpy rules, as a whole. Both routes return equal arrays, bit for bit."""

    def __init__(self, device=None):
        self.device = None
        self._records = []
        self.route = None          # 'device' or 'host': the route of the last summarize()
        if device is not None:
            import torch
            self.device = torch.device(device)

    def add(self, hyp, refs):
        refs = list(refs)
        if not isinstance(hyp, str) or not refs or not all(isinstance(r, str) for r in refs):
            raise ValueError('CaptionEvaluator.add: a hypothesis string and at least one reference string per image '
                             f'(got {type(hyp).__name__} and {len(refs)} references)')
        self._records.append((hyp, refs))

    def add_batch(self, hyps, refs_list):
        hyps, refs_list = list(hyps), list(refs_list)
        if len(hyps) != len(refs_list):
            raise ValueError(f'CaptionEvaluator.add_batch: {len(hyps)} hypotheses, {len(refs_list)} reference lists')
        for hyp, refs in zip(hyps, refs_list):
            self.add(hyp, refs)

    def records(self):
        return list(self._records)

    # -- the integer and ordered-sum parts, by either route --------------------------------------
    @staticmethod
    def components_host(corpus):
        comp = bleu_components_host(corpus)
        df, df_pos = ngram_df_host(corpus)
        sums = cider_sums_host(corpus, df)
        return dict(comp, lcs=lcs_host(corpus), df_pos=df_pos, norm2=sums['norm2'], num=sums['num'])

    def components_device(self, corpus):
        import torch
        from . import ops
        dev = self.device
        N, S = corpus['N'], corpus['S']
        W, Wsp, P = len(corpus['words']), len(corpus['words_sp']), corpus['S'] - corpus['N']
        idf = idf_table_host(N)
        # one pinned buffer, one upload: the idf table first (8-byte aligned), then the int32 streams
        ints = [corpus[k] for k in ('words', 'sent_off', 'words_sp', 'sent_off_sp', 'img_off')]
        n_int = sum(len(a) for a in ints)
        stage = torch.empty(8 * (N + 1) + 4 * n_int, dtype=torch.uint8, pin_memory=True)
        raw = stage.numpy()
        raw[:8 * (N + 1)] = idf.view(np.uint8)
        raw[8 * (N + 1):] = np.concatenate(ints).astype(np.int32).view(np.uint8)
        dbuf = stage.to(dev, non_blocking=True)
        d_idf = dbuf[:8 * (N + 1)].view(torch.float64)
        d_int = dbuf[8 * (N + 1):].view(torch.int32)
        parts, o = [], 0
        for a in ints:
            parts.append(d_int[o:o + len(a)])
            o += len(a)
        words, sent_off, words_sp, sent_off_sp, img_off = parts
        # one output buffer, one copy back: doubles first
        sizes = (('norm2', 8, S * 4), ('num', 8, P * 4), ('bleu', 4, N * 10), ('lcs', 4, P), ('df_pos', 4, W * 4))
        out = torch.empty(sum(b * n for _, b, n in sizes), dtype=torch.uint8, device=dev)
        view, o = {}, 0
        for name, b, n in sizes:
            view[name] = out[o:o + b * n].view(torch.float64 if b == 8 else torch.int32)
            o += b * n
        ops.caption_bleu_lcs(words, sent_off, words_sp, sent_off_sp, img_off, bleu=view['bleu'].view(N, 10), lcs=view['lcs'])
        keys, flags = ops.caption_ngram_keys(words, sent_off, img_off)
        if W:
            # n-gram ids and document frequencies: integer plumbing. Key 0 (no n-gram) gets an id of its own, which nothing reads
            uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
            df = torch.bincount(inv[flags.reshape(-1) != 0], minlength=int(uniq.numel())).to(torch.int32)
            gids = inv.to(torch.int32).view(W, 4)
            view['df_pos'].copy_(torch.where(keys.reshape(-1) != 0, df[inv], torch.full_like(df[inv], -1)))
        else:
            df, gids = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev)
        ops.cider_sums(gids, df, d_idf, sent_off, img_off, norm2=view['norm2'].view(S, 4), num=view['num'].view(P, 4))
        host = out.cpu().numpy()
        res, o = {}, 0
        for name, b, n in sizes:
            res[name] = host[o:o + b * n].view(np.float64 if b == 8 else np.int32).copy()
            o += b * n
        bleu = res['bleu'].reshape(N, 10)
        return dict(testlen=bleu[:, 0].copy(), reflen=bleu[:, 1].copy(), guess=bleu[:, 2:6].copy(), correct=bleu[:, 6:10].copy(),
                    lcs=res['lcs'], df_pos=res['df_pos'].reshape(W, 4), norm2=res['norm2'].reshape(S, 4), num=res['num'].reshape(P, 4))

    # -- the whole run -----------------------------------------------------------------------------
    def summarize(self, extra_records=None):
        """-> dict(Bleu_1 .. Bleu_4, CIDEr, ROUGE_L (floats); bleu (N, 4), cider (N,), rouge (N,) per image; the integer components
        testlen, reflen, guess, correct, lcs, df_pos and the sums norm2, num; total_testlen, total_reflen, images, route)."""
        records = self.records() + [(h, list(r)) for h, r in (extra_records or ())]
        if not records:
            raise ValueError('CaptionEvaluator.summarize: no image was added')
        corpus = intern_corpus_host([h for h, _ in records], [r for _, r in records])
        on_device = False
        if self.device is not None:
            from . import ops
            on_device = ops.caption_eval_ok(*corpus_limits(corpus))
        c = self.components_device(corpus) if on_device else self.components_host(corpus)
        self.route = 'device' if on_device else 'host'
        bleus, bleu_list, total_testlen, total_reflen = bleu_finish_host(c)
        cider, cider_scores = cider_finish_host(c['norm2'], c['num'], corpus)
        rouge, rouge_scores = rouge_finish_host(c['lcs'], corpus)
        res = {f'Bleu_{k + 1}': float(bleus[k]) for k in range(N_ORDERS)}
        res.update(CIDEr=float(cider), ROUGE_L=float(rouge), bleu=np.array(bleu_list, np.float64).T.reshape(-1, N_ORDERS),
                   cider=np.asarray(cider_scores, np.float64), rouge=np.asarray(rouge_scores, np.float64),
                   total_testlen=int(total_testlen), total_reflen=int(total_reflen), images=len(records), route=self.route, **c)
        return res
