"""A/B of one Swin block's window attention at the four BASELINE configs[3] stage shapes (Swin-B at 1024^2, batch 4): the fused
kernels (csrc/window_attn.hip) against the roll / partition / SDPA path (`swin.WINATTN = False`, what CGG_SWIN_WINATTN=0 selects).

Timed: `ShiftWindowMSA` from the normed rows to the input of `proj` (the module with `proj` replaced by the identity: pad, qkv linear,
attention, crop), forward alone (no_grad) and forward + backward, parity mode. Every (shape, path) is warmed first; the two paths then
alternate, each window is `--iters` calls between device-synchronised events; reported are the median and the min .. max of the
`--rounds` windows (the run-to-run spread of this very call). A second pass collects the kernels' own times through
`ops.KERNEL_EVENTS` and states them against the roofs they could hit: HBM bytes (qkv + out + lse forward; qkv + lse + grad_out +
grad_qkv + the grad_table partials backward) at 6.3 TB/s achievable, and the f32 MFMA issued (144 / 504 v_mfma_f32_16x16x4_f32 per
wavefront of 16 tokens) at 157.3 TFLOP/s.

    python scratch/window_attn_probe.py [--batch 4] [--iters 10] [--rounds 5] [--out profiles/window_attn_probe.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cgg_amd  # noqa: E402,F401
from cgg_amd import ops, runtime, swin  # noqa: E402

STAGES = ((128, 4, 256), (256, 8, 128), (512, 16, 64), (1024, 32, 32))      # (C, heads, map side) of Swin-B at 1024^2
HBM, MFMA_F32 = 6.3e12, 157.3e12


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# window attention A/B, batch {args.batch}, ws 12, parity mode; ms per call: median (min .. max) of {args.rounds} windows of '
        f'{args.iters} calls, paths alternating')
    say('# C heads map shift | fwd native | fwd sdpa | fwd+bwd native | fwd+bwd sdpa | speedup fwd, fwd+bwd')
    runtime.set_precision('fp32')
    for C, heads, side in STAGES:
        for shift in (0, 6):
            g = torch.Generator().manual_seed(C + shift)
            m = swin.ShiftWindowMSA(C, heads, 12, shift)
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(torch.randn(p.shape, generator=g) * (C ** -0.5 if p.dim() > 1 and p.shape[-1] == C else 1.0))
            m.w_msa.proj = torch.nn.Identity()
            m = m.to(dev).train()
            x = torch.randn(args.batch, side * side, C, generator=g).to(dev).requires_grad_(True)
            go = torch.randn(args.batch, side * side, C, generator=g).to(dev)

            def fwd():
                with torch.no_grad():
                    m(x, (side, side))

            def fwdbwd():
                for p in m.parameters():
                    p.grad = None
                x.grad = None
                m(x, (side, side)).backward(go)

            res = {}
            for name, fn in (('fwd', fwd), ('fwdbwd', fwdbwd)):
                for flag in (True, False):
                    swin.WINATTN = flag
                    window(fn, 3)                                    # warm this (shape, path)
                t = {True: [], False: []}
                for _ in range(args.rounds):
                    for flag in (True, False):
                        swin.WINATTN = flag
                        t[flag].append(window(fn, args.iters))
                res[name] = t
            swin.WINATTN = True

            def fmt(v):
                return f'{statistics.median(v):7.3f} ({min(v):.3f} .. {max(v):.3f})'
            sp = [statistics.median(res[k][False]) / statistics.median(res[k][True]) for k in ('fwd', 'fwdbwd')]
            say(f'{C:5d} {heads:2d} {side:3d} {shift} | {fmt(res["fwd"][True])} | {fmt(res["fwd"][False])} | '
                f'{fmt(res["fwdbwd"][True])} | {fmt(res["fwdbwd"][False])} | {sp[0]:.2f}x {sp[1]:.2f}x')

            # the kernels alone, against their roofs
            ops.KERNEL_EVENTS = {}
            for _ in range(5):
                fwdbwd()
            torch.cuda.synchronize()
            ev, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
            Hp = (side + 11) // 12 * 12
            tok = args.batch * Hp * Hp
            waves = tok // 16 * heads
            nchunk = ops._lib_().cgg_window_attn_backward_workspace_bytes(args.batch, Hp, Hp, heads, 12)
            for key, nbytes, mfma in (('window_attn_fwd', tok * 4 * C * 4 + tok * heads * 4, 144),
                                      ('window_attn_bwd', tok * 7 * C * 4 + tok * heads * 4 + nchunk, 504)):
                ms = statistics.median(a.elapsed_time(b) for a, b in ev[key])
                fl = waves * mfma * 2048
                say(f'      {key}: {ms:.3f} ms; {nbytes / 1e6:.0f} MB -> {nbytes / ms / 1e9 / HBM * 1e12 * 100:.0f} % of 6.3 TB/s; '
                    f'{fl / 1e9:.1f} GFLOP of f32 MFMA -> {fl / ms / 1e9 / MFMA_F32 * 1e12 * 100:.0f} % of 157.3 TFLOP/s')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
