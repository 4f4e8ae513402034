"""A/B of the two routes of `caption_eval.CaptionEvaluator` on a corpus of a user's size, in ONE process, alternating: the device route
(one upload, the three kernels of csrc/caption_eval.hip with torch.unique / torch.bincount between them, one copy back) against the
numpy / plain-Python rules. The corpus: --images images x --refs references of 8 .. 14 words from a Zipf vocabulary of about 8000
tokens, the hypothesis a corrupted copy of one reference. Interning (strings -> ids) and the shared `*_finish_host` functions are the
same code in both routes and are reported on their own. Median [min .. max] over --reps alternating repetitions after a warm-up.

    python scratch/caption_eval_ab.py [--reps 10] [--images 5000] [--refs 5] [--out profiles/caption_eval_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cgg_amd  # noqa: E402,F401
from cgg_amd import caption_eval as CE  # noqa: E402
from cgg_amd import ops  # noqa: E402


def med(v):
    return f'{statistics.median(v):10.2f} [{min(v):.2f} .. {max(v):.2f}] ms'


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def zipf_corpus(seed, N, R, vocab=8000):
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    hyps, refs = [], []
    for _ in range(N):
        rr = [['w%d' % t for t in rs.choice(vocab, size=int(rs.randint(8, 15)), p=p)] for _ in range(R)]
        hyp = [t if rs.rand() < 0.8 else 'w%d' % rs.choice(vocab, p=p) for t in rr[int(rs.randint(R))]]
        hyps.append(' '.join(hyp))
        refs.append([' '.join(r) for r in rr])
    return hyps, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--refs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    hyps, refs = zipf_corpus(7, a.images, a.refs)
    corpus = CE.intern_corpus_host(hyps, refs)
    V, longest, most = CE.corpus_limits(corpus)
    assert ops.caption_eval_ok(V, longest, most)
    ev = CE.CaptionEvaluator(device=dev)
    t_intern, t_dev, t_host, t_finish = [], [], [], []
    parts = {k: [] for k in ('upload', 'bleu_lcs', 'keys', 'unique+bincount+df_pos', 'cider_sums')}
    for rep in range(a.reps + 1):
        dt, corpus = timed(lambda: CE.intern_corpus_host(hyps, refs))
        d1, got = timed(lambda: ev.components_device(corpus))
        d2, want = timed(lambda: CE.CaptionEvaluator.components_host(corpus))
        t0 = time.perf_counter()
        CE.bleu_finish_host(got)
        CE.cider_finish_host(got['norm2'], got['num'], corpus)
        CE.rouge_finish_host(got['lcs'], corpus)
        d3 = (time.perf_counter() - t0) * 1e3
        for k in ('testlen', 'reflen', 'guess', 'correct', 'lcs', 'df_pos'):
            assert np.array_equal(got[k], want[k]), k
        for k in ('norm2', 'num'):
            assert got[k].view(np.int64).tolist() == want[k].view(np.int64).tolist(), k
        # the device route's parts on their own
        dp = {}
        dp['upload'], d = timed(lambda: {k: torch.from_numpy(corpus[k]).to(dev) for k in ('words', 'sent_off', 'words_sp', 'sent_off_sp', 'img_off')})
        dp['bleu_lcs'], _ = timed(lambda: ops.caption_bleu_lcs(d['words'], d['sent_off'], d['words_sp'], d['sent_off_sp'], d['img_off']))
        dp['keys'], (keys, flags) = timed(lambda: ops.caption_ngram_keys(d['words'], d['sent_off'], d['img_off']))

        def ids():
            uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
            df = torch.bincount(inv[flags.reshape(-1) != 0], minlength=int(uniq.numel())).to(torch.int32)
            return inv.to(torch.int32).view(-1, 4), df, torch.where(keys.reshape(-1) != 0, df[inv], torch.full_like(df[inv], -1))

        dp['unique+bincount+df_pos'], (gids, df, _) = timed(ids)
        idf = torch.from_numpy(CE.idf_table_host(corpus['N'])).to(dev)
        dp['cider_sums'], _ = timed(lambda: ops.cider_sums(gids, df, idf, d['sent_off'], d['img_off']))
        print(f'round {rep}: device {d1:.1f} ms, host {d2:.1f} ms', flush=True)
        if rep:
            t_intern.append(dt)
            t_dev.append(d1)
            t_host.append(d2)
            t_finish.append(d3)
            for k, v in dp.items():
                parts[k].append(v)
    lines = [f'caption_eval_ab: device route (CaptionEvaluator.components_device: one upload, three kernels, torch.unique / bincount, one copy '
             f'back) vs host route (components_host: the plain-Python rules), {a.reps} alternating repetitions after 1 warm-up round, one '
             'process; median [min .. max]; both routes return equal arrays (integers as arrays, doubles bit for bit, asserted every round)',
             f'{a.images} images x {a.refs} references of 8 .. 14 words, Zipf vocabulary: V = {V} tokens, {len(corpus["words"])} words, '
             f'{corpus["S"]} sentences, longest {longest}',
             f'  intern_corpus_host (strings -> ids, both routes)   {med(t_intern)}',
             f'  device route, integers and sums                    {med(t_dev)}',
             f'  host route, integers and sums                      {med(t_host)}',
             f'  *_finish_host (libm part, both routes)             {med(t_finish)}',
             f'  end to end = intern + route + finish: device {statistics.median(t_intern) + statistics.median(t_dev) + statistics.median(t_finish):.1f} ms, '
             f'host {statistics.median(t_intern) + statistics.median(t_host) + statistics.median(t_finish):.1f} ms',
             '  the device route\'s parts, each waited for on its own (wall clock around the call):']
    lines += [f'    {k:<48s} {med(v)}' for k, v in parts.items()]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
