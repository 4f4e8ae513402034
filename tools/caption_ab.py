"""Caption search, per-image loop against the batched search (caption_search.beam_search / beam_search_batched), on the device.

    python tools/caption_ab.py [out.txt]

The caption head of configs/instance/coco_b48n17.py by size -- 4 decoder blocks, 768 channels, 100 queries, V = 30 522 -- with
synthetic weights (N(0, 1 / fan_in), so that a row of logits is about unit normal) and the EOS bias of the G8 recipe, scaled to
this vocabulary, so that the searches end. For B = 1, 2, 8 images: `beam_search` in a loop over the images (the search of the
commit before the batched one, which stays the B = 1 path) against one `beam_search_batched`, HIP events around whole searches
after a warm-up, median of 5, the two alternating. The results of the two are compared. Then the step kernels of csrc/beam_step.hip
alone at B = 2 and 8: device events around 200 launches of each pass on a state that keeps 7 live rows per image, and the byte
floor of pass 1, L * rows * V * 4 bytes, against the HBM bandwidth."""
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cgg_amd  # noqa: E402,F401
from cgg_amd import ops  # noqa: E402
from cgg_amd.bert_embeddings import BertEmbeddings  # noqa: E402
from cgg_amd.caption_search import beam_search, beam_search_batched  # noqa: E402
from cgg_amd.caption_transformer import CaptionTransformer  # noqa: E402

BOS, EOS, MAX_LEN, BEAM, V, HIDDEN, BLOCKS = 101, 102, 35, 7, 30522, 768, 4
EOS_BIAS = 2.5
HBM_BYTES_PER_S = 8.0e12          # MI355X peak HBM3E bandwidth


def build_head(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    gen = CaptionTransformer(nb_layers=BLOCKS, input_dim=HIDDEN, hidden_dim=HIDDEN, ff_dim=512, nb_heads=8, drop_val=0.1,
                             pre_norm=False, seq_length=MAX_LEN, nb_tokens=V).eval()
    be = BertEmbeddings(None, vocab_size=V, hidden_size=HIDDEN)
    with torch.no_grad():
        for m in (gen, be):
            for name, p in sorted(m.named_parameters()):
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=g) / (1.0 if 'word_embeddings' in name else p.shape[1] ** 0.5))
                elif name.endswith('bias'):
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
        gen.generator.bias[EOS] += EOS_BIAS
    return types.SimpleNamespace(bert_embeddings=be.to(dev), caption_generator=gen.to(dev))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def searches(head, dev, say):
    say(f'{"B":>2} {"loop of beam_search ms":>24} {"beam_search_batched ms":>24} {"speed-up":>9}  tokens of the returned sentences')
    for B in (1, 2, 8):
        mem = torch.randn((B, 100, HIDDEN), generator=torch.Generator().manual_seed(10 + B)).to(dev)

        def loop():
            return [beam_search(head, mem[i:i + 1], BOS, EOS, MAX_LEN, beam_width=BEAM, return_ids=True) for i in range(B)]

        def batched():
            return beam_search_batched(head, mem, BOS, EOS, MAX_LEN, beam_width=BEAM, return_ids=True)
        a, b = loop(), batched()                       # warm-up of every shape both use
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(loop)[0])
            tb.append(timed(batched)[0])
        ma, mb = statistics.median(ta), statistics.median(tb)
        say(f'{B:>2} {ma:>17.2f} ({min(ta):.2f}-{max(ta):.2f}) {mb:>11.2f} ({min(tb):.2f}-{max(tb):.2f}) {ma / mb:>8.2f}x  '
            f'{[len(s) for s in b]}' + ('' if a == b else f'   DIFFERENT from the loop: {[len(s) for s in a]}'))


def step_kernels(dev, say):
    say('')
    say(f'{"B":>2} {"rows":>5} {"pass 1 us":>10} {"pass 2 us":>10} {"pass 1 bytes":>13} {"floor us":>9} {"of floor":>9}')
    N = 200
    for B in (2, 8):
        g = torch.Generator().manual_seed(3)
        logits = torch.randn((BLOCKS, B * BEAM, V), generator=g).to(dev)
        logits[:, :, EOS] -= 30.0                      # nobody finishes: the state keeps 7 live rows per image from call to call
        st = ops.BeamState(B, BEAM, MAX_LEN, BOS, EOS, device=dev)
        ops.beam_step(logits, st, 1, 0.7, MAX_LEN, first=True)
        ops.beam_step(logits, st, 2, 0.7, MAX_LEN)
        assert st.nlive.tolist() == [BEAM] * B and int(st.ndone) == 0
        us = {}
        for passes in (1, 2):
            for _ in range(10):
                ops.beam_step(logits, st, 3, 0.7, MAX_LEN, passes=passes)
            torch.cuda.synchronize()
            reps = []
            for _ in range(5):
                reps.append(timed(lambda: [ops.beam_step(logits, st, 3, 0.7, MAX_LEN, passes=passes) for _ in range(N)])[0])
            us[passes] = statistics.median(reps) * 1e3 / N
        assert st.nlive.tolist() == [BEAM] * B and int(st.ndone) == 0
        nbytes = BLOCKS * B * BEAM * V * 4
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        say(f'{B:>2} {B * BEAM:>5} {us[1]:>10.1f} {us[2]:>10.1f} {nbytes:>13d} {floor:>9.1f} {floor / us[1]:>8.0%}')
    say('(per launch, from device events around 200 back-to-back launches, so launch gaps are inside; the logits of one step stay in')
    say(' the 256 MiB last-level cache between launches, which a search step shares: the generator GEMMs have just written them)')


def main(argv):
    if not torch.cuda.is_available():
        raise SystemExit('caption_ab.py measures on a ROCm device; none is available')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'caption search A/B on {torch.cuda.get_device_name(0)}: {BLOCKS} blocks, {HIDDEN} channels, V = {V}, beam {BEAM}, '
        f'max_len {MAX_LEN}, EOS bias {EOS_BIAS}; ms per whole search of all B images, median of 5 (min-max)')
    with torch.no_grad():
        searches(build_head(dev), dev, say)
        step_kernels(dev, say)
    if len(argv) > 1:
        with open(argv[1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv)
