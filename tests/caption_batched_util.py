"""Seeded states and logits for the batched caption search's step rule (tests/test_caption_batched.py on the host,
tests/test_caption_batched_gpu.py on the device): random fixed-slot states with the logits biased so that the branches of
the walk are taken -- an EOS among the candidates, the `len(finished) == beam` break in the middle of the walk, no continued
sequence, a step that finishes nothing after one that did, a done image beside a running one, the BOS step with EOS as a
candidate."""
import torch

from cgg_amd import ops
from cgg_amd.caption_search import beam_step_host

BOS, EOS, ALPHA = 1, 2, 0.7
MARGIN = 1e-4          # the smallest gap in `weighted` a compared decision may rest on (float64 run of the rule)
SCENARIOS = ('plain', 'eos', 'break', 'nocont')
INT_KEYS = ('seqs', 'nlive', 'fin_seqs', 'fin_len', 'nfin', 'best_idx', 'done', 'ndone', 'tokens', 'parents')


def nlives_for(B, beam, case):
    """nlive of each image: 1, 3 and beam mixed inside a batch of 3, cycled over the cases for a single image"""
    opts = [1, min(3, beam), beam]
    return opts if B == 3 else [opts[(case + i) % 3] for i in range(B)]


def make_case(seed, B, beam, V, L, scenario, first=False, done_image=None, max_len=12):
    """-> (state, [logits of step A, logits of step B], length of step A, max_len). Step B is a plain step with EOS pushed
    down, so an image that finished something in step A and still runs has its best_idx reset there."""
    g = torch.Generator().manual_seed(seed)
    S = beam
    st = ops.BeamState(B, S, max_len, BOS, EOS)
    length = 1 if first else (max_len - 2 if scenario == 'nocont' else 4)
    logits = [torch.randn((L, B * S, V), generator=g) * 2.0 for _ in range(2)]
    logits[1][:, :, EOS] -= 30.0
    nl = [1] * B if first else nlives_for(B, beam, seed)
    for b in range(B):
        n = nl[b]
        if not first:
            st.nlive[b] = n
            st.seqs[b, :n, :length] = torch.randint(3, V, (n, length), generator=g).int()
            st.seqs[b, :n, 0] = BOS
            st.weights[b, :n] = -5.0 * torch.rand(n, generator=g) - 0.5 * length
            nf = S - 1 if scenario == 'break' else int(torch.randint(0, S - 1, (1,), generator=g)) if S > 1 else 0
            nf = min(nf, S - 1)
            st.nfin[b] = nf
            for i in range(nf):
                ln = int(torch.randint(3, length + 1, (1,), generator=g))
                st.fin_seqs[b, i, :ln] = torch.randint(3, V, (ln,), generator=g).int()
                st.fin_len[b, i] = ln
                st.fin_score[b, i] = -float(torch.rand(1, generator=g)) - 1.0
            st.best_idx[b] = int(torch.randint(0, max(nf, 1), (1,), generator=g))
        rows = slice(b * S, b * S + n)
        if scenario == 'eos' or (first and scenario == 'first_eos'):
            logits[0][:, rows, EOS] += 6.0           # EOS lands among the candidates, not necessarily first
        elif scenario == 'break':
            logits[0][:, b * S, EOS] += 12.0         # ... first of them, with beam - 1 finished already: the walk stops at once
        elif scenario in ('plain', 'first'):
            logits[0][:, :, EOS] -= 30.0
    if done_image is not None and not first:
        st.done[done_image] = 1
        st.ndone += 1
    return st, logits, length, max_len


def run_host64(st, logits_steps, length, max_len, first):
    """The rule in float64 over the steps of a case -> (state after each step, margins of each step)."""
    h = st.clone(float_dtype=torch.float64)
    snaps, margins = [], []
    for i, lg in enumerate(logits_steps):
        beam_step_host(lg.double(), h, length + i, ALPHA, EOS, max_len, first=first and i == 0, margins=margins)
        snaps.append(h.clone())
    return snaps, margins


def spacing_f32(x):
    """distance from |x| to the next larger float32"""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()
