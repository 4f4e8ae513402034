"""Every entry point around the 256-wide row LayerNorm (the kernels on csrc/row_norm.h and the two that still write the rule out), through
ONE given build of libcgg_hip.so: a SHA-256 per output tensor on seeded off-centre rows at the row-block edges ("hashes"), then device-event
timings at bench.py's configs[1] shapes (43 008 x 256 encoder rows, 200 query rows), 10 warm-up calls, median / min / p90 of 60
("times"). Run it once per library, each in a fresh process under its own time limit, alternating (before, after, before, after): the
two runs of one library give the spread that a difference between the libraries has to exceed. -> profiles/row_norm_refactor_ab.txt
usage: row_norm_refactor_ab.py <path of libcgg_hip.so> <result .json>"""
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
assert _lib._lib is None
from cgg_amd import ops

dev = torch.device('cuda:0')
C = 256
HASH, TIME = {}, {}
g = torch.Generator().manual_seed(7)
F32, BF16 = torch.float32, torch.bfloat16


def put(name, *outs):
    for i, t in enumerate(outs):
        if t is not None:
            assert f'{name} #{i}' not in HASH, name
            HASH[f'{name} #{i}'] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def rows(M, scale=1.0, dt=F32):
    """off-centre rows: mean 3 .. 9 by row, spread 0.02 (a changed summation order shows in the variance)"""
    mean = 3.0 + (torch.arange(M) % 7).float().view(M, 1)
    return ((mean + 0.02 * torch.randn(M, C, generator=g)) * scale).to(dt).to(dev)


def rnd(*shape, s=1.0):
    return (torch.randn(*shape, generator=g) * s).to(dev)


def norm(eps=1e-5):
    return 1.0 + rnd(C, s=0.1), rnd(C, s=0.1), eps


def poses(M):
    return [('nopos', None), ('pos=M', rnd(M, C)), ('pos=48', rnd(48, C))]


LEVELS = (3, [(4, 4), (2, 3), (1, 2)])            # 72 rows: across a 64-row block edge, level boundaries inside a block
KV_B, KV_S, KV_STARTS = 3, 24, [0, 16, 22]

# ---- hashes ---------------------------------------------------------------------------------------------------------------------
# one wave per row, four rows per workgroup: cgg_add_layernorm_ex, cgg_add_layernorm_kv
gam, bet, _ = norm()
for M in (1, 3, 4, 5, 63, 64, 65, 129):
    for adt in (F32, BF16):
        for bdt in (F32, BF16):
            a, b = rows(M, dt=adt), rows(M, 0.5, dt=bdt)
            for pn, pos in poses(M):
                for f32 in (True, False):           # bf16 + bf16 without y32 is the half-wave kernel
                    put(f'add_layernorm_ex M={M} {adt} {bdt} {pn} f32={f32}',
                        *ops.add_layernorm_stream(a, b, gam, bet, 1e-5, pos=pos, want_f32=f32, want_bf16=True, want_pos=pos is not None))
            if bdt is F32:
                put(f'add_layernorm_ex M={M} {adt} b=None', *ops.add_layernorm_stream(a, None, gam, bet, 1e-5))
shift, kpos = rnd(KV_S, C), rnd(KV_S, C)
for adt in (F32, BF16):
    for bdt in (F32, BF16):
        a, b = rows(KV_B * KV_S, dt=adt).view(KV_B, KV_S, C), rows(KV_B * KV_S, 0.5, dt=bdt).view(KV_B, KV_S, C)
        put(f'add_layernorm_kv {adt} {bdt}', *ops.add_layernorm_kv(a, b, gam, bet, 1e-5, shift, kpos, KV_STARTS))

# 64-row blocks, 16 lanes per row: the encoder kernels
for FF in (256, 1024):
    W1, b1, W2, b2 = rnd(FF, C, s=1 / 16), rnd(FF, s=0.1), rnd(C, FF, s=1 / 32), rnd(C, s=0.1)
    Wo, bo = rnd(C, C, s=1 / 16), rnd(C, s=0.1)
    n0, n1 = norm(), norm()
    p16 = [ops.pack_linear_weight(w.contiguous()) for w in (W1, W2, Wo)]
    p3 = [ops.pack_linear_weight_x3(w.contiguous()) for w in (W1, W2, Wo)]
    for M in (1, 63, 64, 65, 129):
        x, a = rows(M, 0.5), rnd(M, C)
        x16, a16 = x.bfloat16(), a.bfloat16()
        for pn, pos in poses(M):
            kw = dict(pos=pos, want_f32=True, want_bf16=True, want_pos=pos is not None)
            put(f'encoder_ffn_ln M={M} F={FF} {pn}', *ops.encoder_ffn_ln(x16, p16[0], b1, p16[1], b2, *n1, **kw))
            put(f'encoder_layer_tail M={M} F={FF} {pn}', *ops.encoder_layer_tail(a16, x16, p16[2], bo, n0, p16[0], b1, p16[1], b2, n1, **kw))
            for x3a in (False, True):
                xin = ops.x3a_encode(x) if x3a else x
                put(f'encoder_layer_tail_x3 x3a={x3a} M={M} F={FF} {pn}',
                    *ops.encoder_layer_tail_x3(a, xin, p3[2], bo, n0, p3[0], b1, p3[1], b2, n1, pos=pos, want_pos=pos is not None, x3a=x3a))
    x16 = rows(KV_B * KV_S, 0.5).bfloat16().view(KV_B, KV_S, C)
    a16 = rnd(KV_B * KV_S, C).bfloat16().view(KV_B, KV_S, C)
    put(f'encoder_ffn_ln_kv F={FF}', *ops.encoder_ffn_ln_kv(x16, p16[0], b1, p16[1], b2, *n1, shift, kpos, KV_STARTS))
    put(f'encoder_layer_tail kv F={FF}',
        *ops.encoder_layer_tail(a16, x16, p16[2], bo, n0, p16[0], b1, p16[1], b2, n1, kv=(shift, kpos, KV_STARTS), want_f32=True))
assert ops.x3_overflow_check(dev, reset=True) is False

# 32-row blocks, one wave per row, four rows per wave: the decoder kernels
Wm = [rnd(C, C, s=1 / 16) for _ in range(5)]
bm = [rnd(C, s=0.1) for _ in range(5)]
Wqkv, bqkv = rnd(3 * C, C, s=1 / 16), rnd(3 * C, s=0.1)
na, nb = norm(), norm(1e-3)
for kind, pack in (('bf16', ops.pack_linear_weight), ('x3', ops.pack_linear_weight_x3)):
    pw = [pack(w.contiguous()) for w in Wm]
    pqkv = pack(Wqkv.contiguous())
    mlp = (pw[0], bm[0], pw[1], bm[1], pw[2], bm[2])
    for M in (1, 3, 4, 5, 63, 64, 65, 129):
        for nsum in (1, 3):
            planes = torch.stack([rows(M, 1.0 / nsum) for _ in range(nsum)])
            for pn, pos in poses(M)[1:]:
                put(f'decoder_tail_{kind} M={M} nsum={nsum} {pn} q', *ops.decoder_tail(planes, na, pos, nb, mlp, (pw[3], bm[3]), want_pos=True))
                put(f'decoder_tail_{kind} M={M} nsum={nsum} {pn}', *ops.decoder_tail(planes, na, pos, nb, mlp))
        core, res = rnd(M, C), rows(M)
        for pn, pos in poses(M)[1:]:
            put(f'decoder_mid_{kind} M={M} {pn} qkv', *ops.decoder_mid(core, pw[4], bm[4], res, na, pos, (pqkv, bqkv)))
        put(f'decoder_mid_{kind} M={M}', *ops.decoder_mid(core, pw[4], bm[4], res, na))
assert ops.x3_overflow_check(dev, reset=True) is False

# 256-row blocks: the backward (per-workgroup partials and an atomic maximum: both reproducible)
for M in (1, 3, 4, 5, 255, 256, 257):
    a, dy = rows(M), rnd(M, C)
    dya, dyb = rnd(M, C).bfloat16(), rnd(M, C).bfloat16()
    for bn, b in (('b=None', None), ('b=f32', rows(M, 0.5)), ('b=bf16', rows(M, 0.5, dt=BF16))):
        put(f'add_layernorm_backward M={M} {bn}', *ops.add_layernorm_backward(dy, a, b, gam, 1e-5, want_bf16=True))
        put(f'add_layernorm_backward M={M} {bn} dy16', *ops.add_layernorm_backward(dy, a, b, gam, 1e-5, dy16a=dya, dy16b=dyb))
        put(f'add_layernorm_backward M={M} {bn} only dy16a', *ops.add_layernorm_backward(None, a, b, gam, 1e-5, dy16a=dya))
        put(f'add_layernorm_backward_amax M={M} {bn}', *ops.add_layernorm_backward(dy, a, b, gam, 1e-5, want_bf16=True, want_amax=True))
torch.cuda.synchronize()
print(f'{len(HASH)} outputs hashed', flush=True)

# ---- times ----------------------------------------------------------------------------------------------------------------------
WARM, REPS = 10, 60


def timed(name, fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    TIME[name] = dict(median_us=statistics.median(ts), min_us=ts[0], p90_us=ts[int(0.9 * len(ts))])
    print(f'{name:52s} median {TIME[name]["median_us"]:9.1f} us   min {ts[0]:9.1f}   p90 {TIME[name]["p90_us"]:9.1f}', flush=True)


B, S, FF, Q = 2, 21504, 1024, 100                       # configs[1]: 128^2 + 64^2 + 32^2 rows per image, 100 queries
M = B * S
starts = [0, 16384, 20480]
a32, b32 = rows(M), rows(M, 0.5)
b16 = b32.bfloat16()
pos, shift = rnd(S, C), rnd(S, C)
timed('add_layernorm_ex f32 + bf16 -> y32, y16, yp16', lambda: ops.add_layernorm_stream(a32, b16, gam, bet, 1e-5, pos=pos, want_pos=True))
timed('add_layernorm_ex f32 + f32 -> y32', lambda: ops.add_layernorm_stream(a32, b32, gam, bet, 1e-5, want_bf16=False))
a16 = a32.bfloat16()
timed('add_layernorm_ex bf16 + bf16 -> y16, yp16 (half-wave)',
      lambda: ops.add_layernorm_stream(a16, b16, gam, bet, 1e-5, pos=pos, want_f32=False, want_pos=True))
timed('add_layernorm_kv f32 + bf16', lambda: ops.add_layernorm_kv(a32.view(B, S, C), b16.view(B, S, C), gam, bet, 1e-5, shift, pos, starts))
dy = rnd(M, C)
timed('add_layernorm_backward f32 + bf16, dx16', lambda: ops.add_layernorm_backward(dy, a32, b16, gam, 1e-5, want_bf16=True))
timed('add_layernorm_backward_amax f32 + f32', lambda: ops.add_layernorm_backward(dy, a32, b32, gam, 1e-5, want_amax=True))
del b32, a16, dy
W1, b1, W2, b2 = rnd(FF, C, s=1 / 16), rnd(FF, s=0.1), rnd(C, FF, s=1 / 32), rnd(C, s=0.1)
Wo, bo = rnd(C, C, s=1 / 16), rnd(C, s=0.1)
n0, n1 = norm(), norm()
p16 = [ops.pack_linear_weight(w.contiguous()) for w in (W1, W2, Wo)]
p3 = [ops.pack_linear_weight_x3(w.contiguous()) for w in (W1, W2, Wo)]
x32, at32 = rows(M, 0.5), rnd(M, C)
x16, at16 = x32.bfloat16().view(B, S, C), at32.bfloat16().view(B, S, C)
timed('encoder_ffn_ln -> y16, yp16', lambda: ops.encoder_ffn_ln(x16, p16[0], b1, p16[1], b2, *n1, pos=pos, want_pos=True))
timed('encoder_ffn_ln_kv', lambda: ops.encoder_ffn_ln_kv(x16, p16[0], b1, p16[1], b2, *n1, shift, pos, starts, want_f32=False))
timed('encoder_layer_tail -> y16, yp16',
      lambda: ops.encoder_layer_tail(at16, x16, p16[2], bo, n0, p16[0], b1, p16[1], b2, n1, pos=pos, want_pos=True))
timed('encoder_layer_tail kv',
      lambda: ops.encoder_layer_tail(at16, x16, p16[2], bo, n0, p16[0], b1, p16[1], b2, n1, kv=(shift, pos, starts)))
timed('encoder_layer_tail_x3 -> y, yp',
      lambda: ops.encoder_layer_tail_x3(at32, x32, p3[2], bo, n0, p3[0], b1, p3[1], b2, n1, pos=pos, want_pos=True))
x3a = ops.x3a_encode(x32)
timed('encoder_layer_tail_x3a -> y, yp',
      lambda: ops.encoder_layer_tail_x3(at32, x3a, p3[2], bo, n0, p3[0], b1, p3[1], b2, n1, pos=pos, want_pos=True, x3a=True))
MQ = B * Q
qpos = rnd(Q, C)
planes, core, res = torch.stack([rows(MQ, 0.125) for _ in range(8)]), rnd(MQ, C), rows(MQ)
for kind, pack in (('bf16', ops.pack_linear_weight), ('x3', ops.pack_linear_weight_x3)):
    pw = [pack(w.contiguous()) for w in Wm]
    pqkv = pack(Wqkv.contiguous())
    mlp = (pw[0], bm[0], pw[1], bm[1], pw[2], bm[2])
    timed(f'decoder_tail_{kind} 200 rows, 8 planes, q', lambda: ops.decoder_tail(planes, na, qpos, nb, mlp, (pw[3], bm[3]), want_pos=True))
    timed(f'decoder_mid_{kind} 200 rows, qkv', lambda: ops.decoder_mid(core, pw[4], bm[4], res, na, qpos, (pqkv, bqkv)))

torch.cuda.synchronize()
assert os.path.abspath(_lib.LIB_PATH) == os.path.abspath(sys.argv[1]) and _lib._lib is not None
with open(sys.argv[2], 'w') as f:
    json.dump(dict(hashes=HASH, times=TIME), f, indent=1)
