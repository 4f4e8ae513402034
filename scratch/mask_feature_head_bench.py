"""cgg_mask_feature_head_x3 (GroupNorm apply + ReLU, mask_feature 1 x 1, packed x3 images in one launch) vs the three calls it
replaces, at the configs[1] and configs[4] mask-feature maps. HIP events, 20 launches each, the two paths alternated over 5 rounds.
Both sides include the GroupNorm statistics passes (the three-call side's GroupNorm entry point runs them itself); `stats` alone is
timed too, so the apply pass's share can be read off. The inputs rotate over 4 copies of z (the 134 MB map would otherwise sit in the
Infinity Cache from launch to launch, which it does not inside the step).

    python scratch/mask_feature_head_bench.py [out.txt]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cgg_amd  # noqa: F401
from cgg_amd import ops, runtime

dev = torch.device('cuda')
C, G, EPS, N_LAUNCH, ROUNDS, COPIES = 256, 32, 1e-5, 20, 5, 4
POOLS = [1, 2, 4, 8]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(fn, n=N_LAUNCH):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def run(B, H, W):
    g = torch.Generator().manual_seed(H)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
    zs = [r(B, H * W, C) for _ in range(COPIES)]
    gamma, beta, wt, bias = 1 + 0.1 * r(C), 0.1 * r(C), r(C, C, k=1 / 16), 0.1 * r(C)
    wk = ops.pack_linear_weight_x3(wt)
    ws = ops.group_norm_nhwc_workspace(B, H * W, G, dev)
    a = torch.empty_like(zs[0])
    gn = (gamma, beta, EPS, G)

    def stats(i):
        ops.group_norm_nhwc_stats(zs[i % COPIES], G, ws)

    def gn_full(i):
        ops.group_norm_nhwc_x3a(zs[i % COPIES], gamma, beta, G, EPS, ws, out=(a, 0, H * W * C), relu=True)

    def gemm(i):
        return runtime.linear_x3s(a.view(B * H * W, C), wt, bias)

    mf = gemm(0)

    def pack(i):
        return ops.pack_mask_feature_nhwc_x3(mf.view(B, H, W, C), POOLS)

    def three(i):
        gn_full(i)
        return ops.pack_mask_feature_nhwc_x3(gemm(i).view(B, H, W, C), POOLS)

    def fused_cfg(cfg):
        def f(i):
            z = zs[i % COPIES]
            ops.group_norm_nhwc_stats(z, G, ws)
            return ops.mask_feature_head_x3(z.view(B, H, W, C), ws, gn, wk, bias, POOLS, cfg=cfg)
        return f

    def head_only(cfg):
        return lambda i: ops.mask_feature_head_x3(zs[i % COPIES].view(B, H, W, C), ws, gn, wk, bias, POOLS, cfg=cfg)

    # same bits first
    old = three(0)
    new = fused_cfg(-1)(0)
    same = all(torch.equal(new[p].hi.view(torch.int16), o.hi.view(torch.int16)) and
               torch.equal(new[p].lo.view(torch.int16), o.lo.view(torch.int16)) for p, o in zip(POOLS, old))
    fns = dict(three=three, fused_4w=fused_cfg(0), fused_8w=fused_cfg(1), stats=stats, gn_full=gn_full, gemm=gemm, pack=pack,
               head_4w=head_only(0), head_8w=head_only(1))
    for f in fns.values():
        for i in range(3):
            f(i)
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            t[k].append(timeit(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    say(f'(B, H, W) = ({B}, {H}, {W}): {B * H * W} rows, pools {POOLS}; images bit-identical: {same}')
    for k in fns:
        say(f'  {k:9s} median {med[k]:7.1f} us   runs ' + ' '.join(f'{x:.1f}' for x in t[k]))
    byts = B * H * W * C * 4 * (1 + 1 + sum(1.0 / (p * p) for p in POOLS[1:]))
    for k in ('fused_4w', 'fused_8w'):
        say(f'  {k} saves {med["three"] - med[k]:.1f} us = {100 * (1 - med[k] / med["three"]):.1f} % of the three-call sum '
            f'(slowest fused run {max(t[k]):.1f} vs fastest three-call run {min(t["three"]):.1f})')
    for k in ('head_4w', 'head_8w'):
        say(f'  {k}: {byts / med[k] / 1e6:.2f} TB/s of the {byts / 1e6:.0f} MB it must move, '
            f'{2.0 * 3 * B * H * W * C * C / med[k] / 1e6:.0f} TF/s f16')
    rep = med['gn_full'] - med['stats'] + med['gemm'] + med['pack']
    say(f'  apply pass = gn_full - stats = {med["gn_full"] - med["stats"]:.1f} us; the three replaced kernels, timed apart = {rep:.1f} us')
    for k in ('head_4w', 'head_8w'):
        say(f'  {k} alone vs the three replaced kernels: saves {rep - med[k]:.1f} us = {100 * (1 - med[k] / rep):.1f} %')
    return same


ok = True
for shape in ((2, 256, 256), (2, 200, 336)):
    ok = run(*shape) and ok
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
