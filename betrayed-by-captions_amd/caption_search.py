"""Caption inference: beam search over the caption generator (open_set/utils/eval/inference.py:84-159, called from
open_set/models/mask2former_head.py:966-972 when `with_caption` / 'cap_results' is requested).

Same search as the reference, including its scoring quirks (they decide which sentence is returned):
  * the step logits are the MEAN over the decoder blocks of `generator(block_output)` (:92-93, :113);
  * candidates are ranked by (log p + parent weight) / length**alpha, the kept weight is de-normalised again (:118-120);
  * a continued sequence inherits `weights[row]` -- the new top-k array indexed by the PARENT's position (:141), not
    the candidate's own weight;
  * finished sequences are scored weight / len**alpha; the running maximum is reset at every step (:123-124), so the
    winner is the best sequence finished in the last step (else the first finished one); the search stops after
    `beam_width` finished sequences or when no live sequence is shorter than max_len - 1.
What differs is where it runs and how much of it: embeddings, transformer, generator, log-softmax and top-k stay on the
device and ONE small device->host copy per step (2 * beam_width numbers) drives the host bookkeeping (the reference moves
the full (beams, vocab) log-probabilities to the host every step); and the decoder runs INCREMENTALLY -- only the newest
position of every beam, against per-block key / value prefixes re-gathered by parent beam and cross-attention keys / values
computed once per image (`CaptionTransformer.begin_decode / decode_step`) -- where the reference re-runs every whole
sequence, the (beams, len, vocab) generator output included, at every step (:108-113). `kv_cache=False` keeps that
full re-run (the tests hold the two against each other).

`beam_search_batched` decodes a whole batch of images at once: 7 B rows through the decoder and the generator per step, and
the step's decision and bookkeeping in one place for all images -- `ops.beam_step` (csrc/beam_step.hip) on a ROCm device, where
the host reads nothing but a 4-byte counter every fourth step, or `beam_step_host`, the same rule in plain torch. The rule is
the loop body above with two things pinned down that the single-image search leaves to torch: the live sequences of an image
occupy slots 0 .. nlive - 1 in the order their candidates were accepted, and equal candidates are ordered by the smaller
row * V + col (`torch.topk` leaves the order of ties open, so any order conforms to the reference).
"""
import torch


def _embed(head, ids):
    be = head.bert_embeddings
    return be.LayerNorm(be.word_embeddings(ids))


def beam_search(head, memory, BOS, EOS, max_len, beam_width=7, alpha=0.7, logging=False, tokenizer=None,
                return_ids=False, kv_cache=True):
    """memory (1, Q, d) = the image's query embeddings. Returns the decoded sentence (reference behaviour) or, with
    `return_ids` / when no tokenizer is available offline, the best token-id sequence (BOS ... EOS)."""
    if memory.shape[0] != 1:
        raise ValueError('beam_search decodes one image at a time (memory batch must be 1), as the reference does')
    dev = memory.device
    gen = head.caption_generator
    with torch.no_grad():
        tgt = _embed(head, torch.tensor([[BOS]], device=dev))                   # (1, 1, d)
        if kv_cache:
            state = gen.begin_decode(memory)
            outs = [o[0] for o in gen.decode_step(tgt, state)]
        else:
            outs = [o[0, 0, :] for o in gen(tgt=tgt, memory=memory)[0]]
        logits = torch.stack([gen.generator(o) for o in outs], 0).mean(0)
        logp = torch.log_softmax(logits[None, :].float(), dim=1)[0]
        w, cand = torch.topk(logp, k=beam_width, largest=True)
        weights, cand = w.cpu(), cand.cpu().tolist()
        seqs = [[BOS, c] for c in cand]
        parents = [0] * len(seqs)
        finished = []
        best_idx = 0
        keep = True
        while keep:
            # (sic) the reference re-initialises its running maximum at EVERY step (:123-124): the returned sentence is
            # the best one finished in the LAST step that finished any, or the first finished one overall
            best_score, best_idx = -100.0, 0
            ids = torch.tensor(seqs, dtype=torch.long, device=dev)             # (nb, len)
            nb, length = ids.shape
            if kv_cache:
                outs = gen.decode_step(_embed(head, ids[:, -1:]), state, torch.tensor(parents, dtype=torch.long, device=dev))
            else:
                outs = [o[:, -1, :] for o in gen(_embed(head, ids), memory.expand(nb, -1, -1).contiguous())[0]]
            logits = torch.stack([gen.generator(o) for o in outs], 0).mean(0)
            logp = torch.log_softmax(logits.float(), dim=1)                     # (nb, V)
            V = logp.shape[1]
            weighted = (logp + weights.to(dev)[:, None]) / length ** alpha
            w, pos = torch.topk(weighted.flatten(), k=min(beam_width, weighted.numel()), largest=True)
            w = (w * length ** alpha).cpu()                                     # de-normalised
            pos = pos.cpu().tolist()
            new_w, new_seqs, parents = [], [], []
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
    if logging:
        for s, sc in finished:
            print(s, sc)
    best = finished[best_idx][0] if finished else []
    if return_ids:
        return best
    if tokenizer is None:
        try:
            import transformers
            tokenizer = transformers.BertTokenizer.from_pretrained('bert-base-uncased', local_files_only=True)
        except Exception:
            return best
    res = ''
    for i, (s, _) in enumerate(finished):
        sentence = tokenizer.decode(s)
        if i == best_idx:
            res = sentence[1:-1]
    return res


# ---- the batched search ---------------------------------------------------------------------------------------------------
def beam_step_host(logits, state, length, alpha, EOS, max_len, first=False, margins=None):
    """THE RULE of one step of the batched search, for every image of the batch, in plain torch (CPU or device tensors; float64
    logits and a float64 state give the comparison form). `ops.beam_step` follows it on the device.

    logits (L, B * S, V): the generator output of each decoder block at the newest position, row b * S + s = slot s of image b
    (S = state.beam); `state` an `ops.BeamState`, updated in place; `length` = the current length of every live sequence. For each
    image that is not done: mean over L, log-softmax per live row, weighted = (log p + weight[row]) / length**alpha, the
    k = min(S, nlive V) largest over the live rows in descending order (equal values by the smaller row * V + col), de-normalised
    again, then the walk of `beam_search`: EOS appends to the finished list with score w / len**alpha (the running best is reset at
    every step the image runs; S finished sequences stop the walk and the image), any other token continues the sequence while
    len < max_len - 1 and inherits w[parent row] (sic); no continued sequence ends the image. `first`: the BOS step (one live row,
    weight 0, length 1) -- every candidate becomes a live sequence with its own weight, EOS included. A done image is left
    untouched. state.tokens / state.parents receive the newest token and the global parent row of every slot for the next decoder
    step; dead slots (and all slots of a done image) get EOS and their own row.

    `margins` (a list) receives one (B,) float64 tensor: per image the smallest gap in `weighted` between consecutive selected
    candidates and between the last selected and the first rejected one (inf for a done image) -- how far the step's decision
    is from a tie."""
    L, rows, V = logits.shape
    B, S = state.B, state.beam
    if rows != B * S:
        raise ValueError(f'beam_step_host: logits has {rows} rows, the state {B} x {S} slots')
    length = int(length)
    norm = length ** alpha
    gaps = torch.full((B,), float('inf'), dtype=torch.float64)
    nlive, done = state.nlive.tolist(), state.done.tolist()
    for b in range(B):
        own = torch.arange(b * S, (b + 1) * S, dtype=torch.int64, device=state.parents.device)
        state.tokens[b * S:(b + 1) * S] = EOS
        state.parents[b * S:(b + 1) * S] = own
        if done[b]:
            continue
        nl = nlive[b]
        lg = logits[:, b * S:b * S + nl].mean(0)
        logp = torch.log_softmax(lg if lg.dtype == torch.float64 else lg.float(), dim=1)               # (nl, V)
        weighted = ((logp + state.weights[b, :nl].to(logp.dtype)[:, None]) / norm).flatten()
        k = min(S, weighted.numel())
        top = torch.topk(weighted, min(k + 1, weighted.numel())).values
        idx = torch.nonzero(weighted >= top[k - 1]).flatten()            # ascending position: a stable sort keeps ties in that order
        vals, order = torch.sort(weighted[idx], descending=True, stable=True)
        pos = idx[order][:k].cpu().tolist()
        sel = vals[:k]
        g = torch.cat([sel, top[k:k + 1]]).double()
        if g.numel() > 1:
            gaps[b] = float((g[:-1] - g[1:]).min())
        w = (sel * norm).cpu()                                          # de-normalised
        old = state.seqs[b, :nl, :length].cpu().tolist()
        nfin = int(state.nfin[b])
        best_score, best_idx = -100.0, 0
        new_w, new_seqs, parents = [], [], []
        finished_all = False
        for i, p in enumerate(pos):
            row, col = p // V, p % V
            seq = old[row] + [col]
            if first:
                new_w.append(w[i])
                new_seqs.append(seq)
                parents.append(row)
            elif col == EOS:
                score = float(w[i]) / len(seq) ** alpha
                state.fin_seqs[b, nfin, :len(seq)] = torch.tensor(seq, dtype=torch.int32)
                state.fin_len[b, nfin] = len(seq)
                state.fin_score[b, nfin] = score
                if score > best_score:
                    best_score, best_idx = score, nfin
                nfin += 1
                if nfin == S:
                    finished_all = True
                    break
            elif len(seq) < max_len - 1:
                new_w.append(w[row])             # (sic) reference :141 indexes the new weights by the parent row
                new_seqs.append(seq)
                parents.append(row)
        state.nfin[b] = nfin
        if not first:
            state.best_idx[b] = best_idx
        if new_seqs:
            n = len(new_seqs)
            state.seqs[b, :n, :length + 1] = torch.tensor(new_seqs, dtype=torch.int32)
            state.weights[b, :n] = torch.stack(new_w).to(state.weights.dtype)
            state.nlive[b] = n
        if finished_all or not new_seqs:
            state.done[b] = 1
            state.ndone += 1
        else:
            state.tokens[b * S:b * S + n] = torch.tensor([s[-1] for s in new_seqs], dtype=torch.int64)
            state.parents[b * S:b * S + n] = torch.tensor(parents, dtype=torch.int64) + b * S
    if margins is not None:
        margins.append(gaps)
    return state


def _render(finished, best_idx, return_ids, tokenizer):
    """What `beam_search` returns for its list of finished sequences (its lines after the loop)."""
    best = finished[best_idx] if finished else []
    if return_ids:
        return best
    if tokenizer is None:
        try:
            import transformers
            tokenizer = transformers.BertTokenizer.from_pretrained('bert-base-uncased', local_files_only=True)
        except Exception:
            return best
    res = ''
    for i, s in enumerate(finished):
        sentence = tokenizer.decode(s)
        if i == best_idx:
            res = sentence[1:-1]
    return res


def beam_search_batched(head, memory, BOS, EOS, max_len, beam_width=7, alpha=0.7, return_ids=False, tokenizer=None, rule='auto',
                        margins=None):
    """`beam_search` for memory (B, Q, d): a list of B results, each what `beam_search` returns for that image alone ([] / '' when
    nothing finished). Every step embeds the slots' newest tokens, runs `decode_step_batched` over all B * beam_width rows, writes
    the L generator outputs into one (L, B * beam_width, V) buffer and advances every image with one `ops.beam_step` (ROCm tensors)
    or `beam_step_host` (CPU tensors; `rule='host'` forces it anywhere, `rule='host64'` evaluates it in float64 on the f32 logits).
    On the device the host never reads a candidate: it reads the 4-byte count of finished images at every fourth step and the
    finished sequences once at the end. `margins` (a list) receives `beam_step_host`'s per-step margins (host rules only)."""
    from . import ops
    if rule not in ('auto', 'host', 'host64'):
        raise ValueError(f"beam_search_batched: rule must be 'auto', 'host' or 'host64' (got {rule!r})")
    if memory.is_cuda and torch.cuda.is_current_stream_capturing():
        raise ValueError('beam_search_batched reads the count of finished images on the host and cannot be captured into a hipGraph '
                         '(captions are outside the staged pipeline; tools/test.py: --no-pipeline)')
    dev = memory.device
    B, S = memory.shape[0], int(beam_width)
    gen = head.caption_generator
    kernel = rule == 'auto' and memory.is_cuda
    state = ops.BeamState(B, S, max_len, BOS, EOS, device=dev, float_dtype=torch.float64 if rule == 'host64' else torch.float32)
    # A step at sequence length l makes candidates of l + 1 tokens, and one is continued only while l + 1 < max_len - 1. The BOS
    # step runs at l = 1 and continues everything; the steps after it run at l = 2, 3, ... and the one at l = max_len - 2 can
    # continue nothing, which ends every image still running: at most max_len - 3 steps past the first (one, where max_len < 4,
    # because the step at l = 2 runs whatever max_len says -- `beam_search` enters its loop before it tests anything).
    steps = 1 + max(1, max_len - 3)
    with torch.no_grad():
        dstate = gen.begin_decode_batched(memory, S, steps)
        W, bias = gen.generator.weight, gen.generator.bias
        L = len(gen.transformer_decoder.decoders)
        buf = torch.empty((L, B * S, W.shape[0]), dtype=torch.float32, device=dev)
        for it in range(steps):
            outs = gen.decode_step_batched(_embed(head, state.tokens[:, None]), dstate, state.parents)
            for l, o in enumerate(outs):
                if o.dtype == torch.float32 and W.dtype == torch.float32 and bias is not None:
                    torch.addmm(bias, o, W.t(), out=buf[l])              # what F.linear computes, written in place
                else:
                    buf[l].copy_(gen.generator(o))
            if kernel:
                ops.beam_step(buf, state, it + 1, alpha, max_len, first=it == 0)
                if it % 4 == 0 and it and int(state.ndone.item()) == B:
                    break
            else:
                beam_step_host(buf.double() if rule == 'host64' else buf, state, it + 1, alpha, EOS, max_len, first=it == 0,
                               margins=margins)
                if int(state.ndone) == B:
                    break
    fin_seqs, fin_len = state.fin_seqs.cpu().tolist(), state.fin_len.cpu().tolist()
    nfin, best_idx = state.nfin.cpu().tolist(), state.best_idx.cpu().tolist()
    out = []
    for b in range(B):
        finished = [fin_seqs[b][i][:fin_len[b][i]] for i in range(nfin[b])]
        out.append(_render(finished, best_idx[b], return_ids, tokenizer))
    return out
