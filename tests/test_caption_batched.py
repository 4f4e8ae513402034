"""CPU tests of the batched caption search (caption_search.beam_search_batched): the step rule `beam_step_host` against a literal
per-image transcription of `beam_search`'s loop body, the G8 goldens through the batched search, `decode_step_batched` against
`decode_step`, and the argument checks of the C entry `cgg_beam_step` (no launch is reached)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, registry
from cgg_amd import caption_transformer as P_ct
from cgg_amd.bert_embeddings import BertEmbeddings as P_Bert
from cgg_amd.caption_search import beam_search, beam_search_batched, beam_step_host

from caption_batched_util import ALPHA, BOS, EOS, MARGIN, SCENARIOS, make_case, run_host64
from util import randomize

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- 1. the rule against the loop body of beam_search ------------------------------------------------------------------------
def transcribed_first(logits, beam_width):
    """caption_search.py lines 43-48 for one image: logits (L, V) = the stacked generator outputs of the BOS position."""
    logits = logits.mean(0)
    logp = torch.log_softmax(logits[None, :].float(), dim=1)[0]
    w, cand = torch.topk(logp, k=beam_width, largest=True)
    weights, cand = w.cpu(), cand.cpu().tolist()
    seqs = [[BOS, c] for c in cand]
    parents = [0] * len(seqs)
    return seqs, weights, parents


def transcribed_step(seqs, weights, finished, logits, max_len, beam_width, alpha):
    """caption_search.py lines 55-89 for one image, on Python lists: logits (L, nb, V) = the stacked generator outputs.
    -> (seqs, weights, parents, best_idx, keep, (where the walk broke off, number of candidates)); `finished` is appended to."""
    keep = True
    best_score, best_idx = -100.0, 0
    nb, length = len(seqs), len(seqs[0])
    logits = logits.mean(0)
    logp = torch.log_softmax(logits.float(), dim=1)                     # (nb, V)
    V = logp.shape[1]
    weighted = (logp + weights[:, None]) / length ** alpha
    w, pos = torch.topk(weighted.flatten(), k=min(beam_width, weighted.numel()), largest=True)
    w = (w * length ** alpha).cpu()                                     # de-normalised
    pos = pos.cpu().tolist()
    new_w, new_seqs, parents = [], [], []
    stopped_at = None
    for idx, p in enumerate(pos):
        row, col = p // V, p % V
        seq = seqs[row] + [col]
        if col == EOS:
            score = float(w[idx]) / len(seq) ** alpha
            finished.append((seq, score))
            if score > best_score:
                best_score, best_idx = score, len(finished) - 1
            if len(finished) == beam_width:
                keep = False
                stopped_at = idx          # (the test's own note of where the walk stopped)
                break
        elif len(seq) < max_len - 1:
            new_w.append(w[row])          # (sic) reference :141 indexes the new weights by the parent row
            new_seqs.append(seq)
            parents.append(row)
    if not new_seqs:
        keep = False
    else:
        weights = torch.stack(new_w) if new_w else weights
        seqs = new_seqs
    return seqs, weights, parents, best_idx, keep, (stopped_at, len(pos))


def image_lists(st, b, length):
    n = int(st.nlive[b])
    seqs = st.seqs[b, :n, :length].tolist()
    finished = [(st.fin_seqs[b, i, :int(st.fin_len[b, i])].tolist(), float(st.fin_score[b, i])) for i in range(int(st.nfin[b]))]
    return seqs, st.weights[b, :n].clone(), finished


def check_image(st, b, seqs, weights, finished, best_idx, keep, parents):
    """the state of image b equals the transcription's lists field by field"""
    S = st.beam
    n, length = len(seqs), len(seqs[0])
    assert int(st.nlive[b]) == n
    assert st.seqs[b, :n, :length].tolist() == seqs
    assert torch.equal(st.weights[b, :n], weights)                     # the same torch f32 operations: exactly equal
    assert int(st.nfin[b]) == len(finished)
    for i, (s, sc) in enumerate(finished):
        assert st.fin_seqs[b, i, :int(st.fin_len[b, i])].tolist() == s
        assert float(st.fin_score[b, i]) == float(torch.tensor(sc, dtype=torch.float32))
    assert int(st.best_idx[b]) == best_idx
    assert bool(st.done[b]) == (not keep)
    own = list(range(b * S, (b + 1) * S))
    if keep:
        assert st.tokens[b * S:b * S + n].tolist() == [s[-1] for s in seqs]
        assert st.parents[b * S:b * S + n].tolist() == [b * S + p for p in parents]
        assert st.tokens[b * S + n:(b + 1) * S].tolist() == [EOS] * (S - n) and st.parents[b * S + n:(b + 1) * S].tolist() == own[n:]
    else:
        assert st.tokens[b * S:(b + 1) * S].tolist() == [EOS] * S and st.parents[b * S:(b + 1) * S].tolist() == own


def snapshot(st, b):
    return {k: getattr(st, k)[b].clone() for k in ops.BeamState.FIELDS if k != 'ndone'}


def test_beam_step_host_equals_the_transcribed_loop_body():
    """`beam_step_host` == lines 43-48 / 55-89 of caption_search.py run per image on Python lists, on random states, for
    beam in {2, 5, 7}, nlive in {1, beam} (and 3), V = 30, L in {1, 3}; every branch of the walk is seen at least once."""
    V = 30
    seen = dict(eos=0, brk=0, nocont=0, reset=0, done_beside=0, first_eos=0)
    case = 0
    for beam in (2, 5, 7):
        for L in (1, 3):
            for B in (1, 3):
                for scen in SCENARIOS + ('first', 'first_eos'):
                    case += 1
                    first = scen.startswith('first')
                    done_image = case % 3 if B == 3 and not first else None
                    st, logits, length, max_len = make_case(1000 + case, B, beam, V, L, scen, first, done_image)
                    _, margins = run_host64(st, logits, length, max_len, first)
                    for i in range(2):
                        # the margin condition: no decision compared below rests on a near-tie
                        assert float(margins[i].min()) > MARGIN, (case, scen, i, margins[i])
                        ln = length + i
                        before = [image_lists(st, b, ln) for b in range(B)]
                        frozen = [snapshot(st, b) for b in range(B)]
                        was_done = st.done.tolist()
                        ndone0, best0 = int(st.ndone), st.best_idx.tolist()
                        beam_step_host(logits[i], st, ln, ALPHA, EOS, max_len, first=first and i == 0)
                        for b in range(B):
                            if was_done[b]:
                                after = snapshot(st, b)
                                assert all(torch.equal(frozen[b][k], after[k]) for k in after), (case, b)
                                assert st.tokens[b * beam:(b + 1) * beam].tolist() == [EOS] * beam
                                seen['done_beside'] += int(any(not d for d in was_done))
                                continue
                            seqs, weights, finished = before[b]
                            lg = logits[i][:, b * beam:b * beam + len(seqs)]
                            if first and i == 0:
                                s2, w2, par = transcribed_first(lg[:, 0], beam)
                                keep, bi = True, best0[b]
                                seen['first_eos'] += int(any(s[-1] == EOS for s in s2))
                            else:
                                nf0 = len(finished)
                                s2, w2, par, bi, keep, (stop, ncand) = transcribed_step(seqs, weights, finished, lg, max_len, beam,
                                                                                        ALPHA)
                                seen['eos'] += int(len(finished) > nf0)
                                seen['brk'] += int(stop is not None and stop < ncand - 1)
                                seen['nocont'] += int(len(finished) < beam and not keep)
                                seen['reset'] += int(best0[b] != 0 and bi == 0 and len(finished) == nf0 and nf0 > 0)
                            check_image(st, b, s2, w2, finished, bi, keep, par)
                        assert int(st.ndone) == int(st.done.sum()) >= ndone0
    assert all(v > 0 for v in seen.values()), seen


# ---- 2. the G8 goldens through the batched search ------------------------------------------------------------------------------
class _StubTokenizer:
    def decode(self, ids):
        return ' '.join(str(int(i)) for i in ids)


def gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) if z[k].dtype.kind in 'fiub' and z[k].shape != () else z[k] for k in z.files}


def g8_head(cfg, seed, c):
    gen = P_ct.CaptionTransformer(**cfg).eval()
    randomize(gen, seed=seed)
    with torch.no_grad():
        gen.generator.bias[2] += 1.0 + 0.5 * c
    be = P_Bert(None, vocab_size=30, hidden_size=32)
    randomize(be.word_embeddings, seed=seed + 100)
    randomize(be.LayerNorm, seed=seed + 200)
    return types.SimpleNamespace(bert_embeddings=be, caption_generator=gen)


def test_g8_goldens_through_the_batched_search():
    """Every G8 case as image 0 of a batch of 3 (the golden memory and two seeded perturbations of it): element 0 is the
    reference's sentence, every element is what `beam_search` gives for that memory alone (ids and the tokenizer stub), and the
    float64 run of the rule keeps every decision of the search more than the margin away from a tie. One B = 1 case."""
    z = gold('g8_beam_search.npz')
    cfg = json.loads(str(z['cfg']))
    for case in range(int(z['n_cases'])):
        seed, beam, max_len, c = [int(v) for v in z[f'params{case}']]
        head = g8_head(cfg, seed, c)
        mem0 = z[f'mem{case}']
        g = torch.Generator().manual_seed(7000 + case)
        mem = torch.cat([mem0, mem0 + 0.3 * torch.randn(mem0.shape, generator=g), mem0 + 0.3 * torch.randn(mem0.shape, generator=g)], 0)
        margins = []
        beam_search_batched(head, mem, 1, 2, max_len=max_len, beam_width=beam, return_ids=True, rule='host64', margins=margins)
        assert min(float(m.min()) for m in margins) > MARGIN, (case, margins)
        ids = beam_search_batched(head, mem, 1, 2, max_len=max_len, beam_width=beam, return_ids=True)
        sent = beam_search_batched(head, mem, 1, 2, max_len=max_len, beam_width=beam, tokenizer=_StubTokenizer())
        assert isinstance(ids, list) and len(ids) == 3 and len(sent) == 3
        assert sent[0] == str(z[f'sentence{case}']), (case, sent[0], str(z[f'sentence{case}']))
        for i in range(3):
            assert ids[i] == beam_search(head, mem[i:i + 1], 1, 2, max_len=max_len, beam_width=beam, return_ids=True), (case, i)
            assert sent[i] == beam_search(head, mem[i:i + 1], 1, 2, max_len=max_len, beam_width=beam, tokenizer=_StubTokenizer())
        if case == 0:
            one = beam_search_batched(head, mem0, 1, 2, max_len=max_len, beam_width=beam, tokenizer=_StubTokenizer())
            assert one == [str(z['sentence0'])]


# ---- 3. the batched incremental decode -------------------------------------------------------------------------------------------
def test_decode_step_batched_equals_decode_step():
    """`decode_step_batched` == `decode_step` row for row over 5 steps: two images whose slots follow different parent
    permutations and one image with dead slots (their rows are not compared: nobody reads them). Both run the same operations
    per row in the same order, but the CPU library's GEMM does not promise that a row's result is independent of the number of
    rows M it is computed with (15 here against 5 or 3; a one-row product takes another routine altogether, which is why the
    single-image side starts with all its rows at step 0), so `torch.equal` is not asserted: the rows agree to 1e-6 absolute
    (8.3e-7 at most on the build this was written on, the two five-slot images bit-identical; outputs are O(1) LayerNorm rows)."""
    torch.manual_seed(5)
    gen = registry.build_head(dict(type='CaptionTransformer', nb_layers=3, input_dim=48, hidden_dim=48, ff_dim=96, nb_heads=4,
                                   drop_val=0.1, pre_norm=False, seq_length=12, nb_tokens=50)).eval()
    B, S, T = 3, 5, 5
    mem = torch.randn(B, 9, 48)
    toks = torch.randn(T, B * S, 1, 48)
    live = [5, 5, 3]                                       # image 2 keeps two dead slots
    perms = [[None, [0, 0, 0, 0, 0], [0, 1, 2, 3, 4], [4, 3, 3, 0, 1], [2, 2, 1, 0, 4]],
             [None, [0, 0, 0, 0, 0], [4, 4, 1, 0, 2], [1, 0, 2, 2, 3], [3, 1, 4, 0, 0]],
             [None, [0, 0, 0], [2, 1, 0], [0, 0, 2], [1, 2, 2]]]
    with torch.no_grad():
        bstate = gen.begin_decode_batched(mem, S, T)
        single = [gen.begin_decode(mem[b:b + 1]) for b in range(B)]
        exact = True
        for t in range(T):
            parents = torch.arange(B * S)
            for b in range(B):
                if t > 0:
                    parents[b * S:b * S + live[b]] = torch.tensor(perms[b][t]) + b * S
            got = gen.decode_step_batched(toks[t], bstate, parents)
            for b in range(B):
                n = live[b]
                want = gen.decode_step(toks[t, b * S:b * S + n], single[b], None if t == 0 else torch.tensor(perms[b][t]))
                for a, w in zip(got, want):
                    exact = exact and torch.equal(a[b * S:b * S + n], w)
                    assert (a[b * S:b * S + n] - w).abs().max().item() <= 1e-6, (t, b)
    assert bstate['length'] == T and bstate['k'][0].shape == (B * S, T, 4, 12)
    print('decode_step_batched bit-identical to decode_step on this build:', exact)


# ---- 4. the C entry's argument checks ----------------------------------------------------------------------------------------------
def test_cgg_beam_step_argument_checks_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(logits=p, L=4, B=1, beam=7, V=30522, ndone=p, length=2, max_len=35, state_max_len=35):
        return lib.cgg_beam_step(logits, L, B, beam, V, p, p, p, p, p, p, p, p, p, ndone, p, p, p, length, 0.7, 102, max_len,
                                 state_max_len, 0, None)
    EINVAL = -1
    for kw, word in ((dict(logits=null), b'null'), (dict(ndone=null), b'null'), (dict(beam=9), b'beam'), (dict(beam=0), b'beam'),
                     (dict(V=5), b'smaller than beam'), (dict(L=0), b'L and B'), (dict(max_len=36), b'sized for'),
                     (dict(length=35), b'length')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.cgg_last_error_string(), (kw, lib.cgg_last_error_string())
    assert call(max_len=300, state_max_len=300) == -2                  # CGG_EUNSUPPORTED: rows longer than the kernel's LDS copy
    assert lib.cgg_beam_step_workspace_bytes(2, 7, 30522) == 2 * 7 * 30 * 18 * 4
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.beam_step(torch.zeros(4, 7, 30), ops.BeamState(1, 7, 35, 101, 102), 1, 0.7, 35, first=True)
