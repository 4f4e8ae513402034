"""A/B of the MSDeformAttn family (csrc/msda.hip, msda_bwd.hip, msda_common.h) between two builds. -> profiles/msda_refactor_ab.txt

  msda_refactor_ab.py isa <dir of before *.s> <dir of after *.s>
      hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S output of the same sources, both sides: per kernel the resources, whether the
      instruction text is the same once labels and register numbers are normalised ("ord": the same lines in another order), and the per-opcode counts of every floating-point,
      conversion, DPP / lane, LDS and memory instruction. No GPU needed.
  msda_refactor_ab.py run <path of libcgg_hip.so> <result .json>
      through ONE build, in a fresh process: a SHA-256 per output of every cgg_msda_* entry that ops.py reaches on five pyramids whose
      expected fast-path gates are computed here from the rule and printed, one non-stream shape on the generic kernels, the two
      geometry queries, the (code, text) of invalid calls, then device-event timings at the encoder's shape (10 warm-up calls, median
      of 60). Run it alternating (before, after, before, after): the two runs of one library say which outputs reproduce themselves
      and give the spread that a difference between the libraries has to exceed.
  msda_refactor_ab.py report <before 1> <after 1> <before 2> <after 2>     (the four .json)"""
import collections
import ctypes
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- isa ------------------------------------------------------------------------------------------------------------------------
CHECKED = re.compile(r'^(v_\w*(f16|f32|f64|bf16)\w*|v_cvt\w*|v_mfma\w*|\w+_dpp|v_permlane\w*|v_readlane\w*|v_readfirstlane\w*|ds_\w+|'
                     r'global_\w+|buffer_\w+|flat_\w+|scratch_\w+|s_load\w*|s_buffer_load\w*)$')


def kernels_of(path):
    """{demangled kernel: dict(res=..., text=[normalised instruction lines], ops=Counter)} of one .s file"""
    out, name, body = {}, None, []
    res_keys = {'NumVgprs': 'vgpr', 'TotalNumSgprs': 'sgpr', 'ScratchSize': 'scratch', 'Occupancy': 'occ', 'LDSByteSize': 'lds'}
    for line in open(path):
        m = re.match(r'^(_Z\w+|cgg_\w+):', line)
        if m and name is None:
            name, body, res = m.group(1), [], {}
            continue
        if name is None:
            continue
        m = re.match(r'^; (\w+): (\d+)', line)
        if m and m.group(1) in res_keys:
            res[res_keys[m.group(1)]] = int(m.group(2))
            if m.group(1) == 'Occupancy':                    # the last of these lines in the resource comment block
                if 'vgpr' in res and body:                  # (device functions that are not kernels have no such block)
                    out[name] = dict(res=res, text=body, ops=collections.Counter(t.split()[0] for t in body))
                name = None
            continue
        code = line.split(';')[0].strip()
        if not code or code.startswith('.') or code.endswith(':'):
            continue
        code = re.sub(r'\.LBB\d+_\d+', 'L', code)
        code = re.sub(r'\b([vsa])\[\d+:\d+\]', r'\1[]', code)
        code = re.sub(r'\b([vsa])\d+\b', r'\1', code)
        body.append(code)
    names = list(out)
    dem = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n') if names else []
    return {re.sub(r'^void |\(.*$', '', d): out[n] for n, d in zip(names, dem)}


def isa(before_dir, after_dir):
    print('# file / kernel | VGPRs before -> after | SGPRs | scratch | LDS | occupancy | instruction lines | same ISA | checked counts '
          '[other opcodes that differ]')
    n = same = 0
    for f in sorted(os.listdir(after_dir)):
        kb, ka = kernels_of(os.path.join(before_dir, f)), kernels_of(os.path.join(after_dir, f))
        assert set(kb) == set(ka), (f, set(kb) ^ set(ka))
        for k in ka:
            b, a = kb[k], ka[k]
            diff = {o: (b['ops'][o], a['ops'][o]) for o in set(b['ops']) | set(a['ops']) if b['ops'][o] != a['ops'][o]}
            bad = {o: v for o, v in diff.items() if CHECKED.match(o)}
            other = ', '.join(f'{o} {v[0]}->{v[1]}' for o, v in sorted(diff.items()) if o not in bad)
            eq = b['text'] == a['text']
            n, same = n + 1, same + eq
            r = ' | '.join(f'{b["res"][x]:>5} -> {a["res"][x]:>5}' for x in ('vgpr', 'sgpr', 'scratch', 'lds', 'occ'))
            print(f'  {f.replace(".s", ".hip"):14s} {k:62s} | {r} | {len(b["text"]):5d} -> {len(a["text"]):5d} | {"yes" if eq else "ord" if sorted(b["text"]) == sorted(a["text"]) else "NO "} | '
                  f'{"equal" if not bad else "DIFFER " + str(bad)}{"   [" + other + "]" if other else ""}')
    print(f'{same} of {n} kernels have the same ISA')


# ---- report ---------------------------------------------------------------------------------------------------------------------
def report(paths):
    b1, a1, b2, a2 = (json.load(open(p)) for p in paths)
    for key in ('gates', 'queries', 'errors'):
        assert b1[key] == b2[key] and a1[key] == a2[key]
        bad = [k for k in b1[key] if b1[key][k] != a1[key].get(k)]
        print(f'{key}: {len(b1[key])} entries, {"all equal between the libraries" if not bad and b1[key].keys() == a1[key].keys() else "DIFFER: " + str(bad)}')
    for k, v in b1['gates'].items():
        print(f'  {k}: {v}')
    for k, v in b1['queries'].items():
        print(f'  {k}: before {v} after {a1["queries"][k]}')
    for k, v in b1['errors'].items():
        print(f'  {k}: {v}')
    hb, ha = b1['hashes'], a1['hashes']
    assert hb.keys() == ha.keys() == b2['hashes'].keys() == a2['hashes'].keys()
    exempt = sorted(k for k in hb if hb[k] != b2['hashes'][k])
    unstable_after = sorted(k for k in ha if ha[k] != a2['hashes'][k] and k not in exempt)
    differ = sorted(k for k in hb if k not in exempt and (hb[k] != ha[k] or hb[k] != a2['hashes'][k]))
    print(f'hashes: {len(hb)} outputs; {len(exempt)} do not reproduce themselves within the before library (exempt): {exempt}')
    print(f'  after does not reproduce itself: {unstable_after}')
    print(f'  differ between the libraries: {differ}')
    print('# call | before 1 | before 2 | spread | after 1 | after 2 | mean after - mean before')
    for k in b1['times']:
        t = [x['times'][k]['median_us'] for x in (b1, b2, a1, a2)]
        print(f'  {k:44s} | {t[0]:8.2f} | {t[1]:8.2f} | {abs(t[0] - t[1]):6.2f} | {t[2]:8.2f} | {t[3]:8.2f} | {(t[2] + t[3] - t[0] - t[1]) / 2:+6.2f}')


if sys.argv[1] == 'isa':
    isa(sys.argv[2], sys.argv[3])
    sys.exit(0)
if sys.argv[1] == 'report':
    report(sys.argv[2:6])
    sys.exit(0)
assert sys.argv[1] == 'run'

# ---- run ------------------------------------------------------------------------------------------------------------------------
sys.path.insert(0, ROOT)
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib

_lib.LIB_PATH = os.path.abspath(sys.argv[2])
assert _lib._lib is None
from cgg_amd import ops
from cgg_amd._lib import dev_ptr, stream_ptr

dev = torch.device('cuda:0')
LIB = _lib.load()
HASH, TIME, GATES, QUERIES, ERRORS = {}, {}, {}, {}, {}
g = torch.Generator().manual_seed(11)


def put(name, *outs):
    for i, t in enumerate(outs):
        assert f'{name} #{i}' not in HASH, name
        HASH[f'{name} #{i}'] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def rnd(*shape, s=1.0):
    return (torch.randn(*shape, generator=g) * s).to(dev)


def tiles(hw, start, N, wm, hm, sm):
    """the rule of msda_levels_tile: ascending, gapless, sum == N, every w / h / start a multiple of (wm, hm, sm)"""
    expect = 0
    for (h, w), s in zip(hw, start):
        if s != expect or w % wm or h % hm or s % sm:
            return False
        expect += h * w
    return expect == N


def sorted_rule(hw, N, Nv, D, P):
    """the condition of msda_sort_plan as far as these pyramids exercise it: queries == pixels, areas sum to Nv, D == 32, P == 4, an
    integer scale between every level and the coarsest one (reordered tables allowed)"""
    hc, wc = min(hw, key=lambda x: x[1])
    return N == Nv and D == 32 and P == 4 and sum(h * w for h, w in hw) == Nv and \
        all(w % wc == 0 and h % hc == 0 and w // wc == h // hc for h, w in hw)


def problem(hw, start, B, H, D, P, Nq=None):
    """value, raw [offsets | logits] rows with offsets of +-2 px, reference points = the pixel centres when queries == pixels"""
    L = len(hw)
    Nv = sum(h * w for h, w in hw)
    pix = Nq is None
    Nq = Nv if pix else Nq
    value = rnd(B, Nv, H, D)
    offs = (torch.rand(B, Nq, H * L * P * 2, generator=g) * 4 - 2).to(dev)
    rows = torch.cat([offs, rnd(B, Nq, H * L * P)], -1).contiguous()
    ref = torch.rand(Nq, 2, generator=g)
    if pix:
        for (h, w), s in zip(hw, start):
            ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
            ref[s:s + h * w] = torch.stack([(xs.flatten() + 0.5) / w, (ys.flatten() + 0.5) / h], -1)
    return value, rows, ref.to(dev), rnd(B, Nq, H * D), Nv, Nq


def prologue(rows, ref, hw, B, Nq, H, L, P):
    hwa, _ = ops._levels(hw, [0] * L)
    loc = torch.empty((B, Nq, H, L, P, 2), dtype=torch.float32, device=dev)
    aw = torch.empty((B, Nq, H, L, P), dtype=torch.float32, device=dev)
    ops._call('cgg_msda_prologue', dev_ptr(rows), rows.shape[-1], dev_ptr(ref), hwa, dev_ptr(loc), dev_ptr(aw), B, Nq, H, L, P, stream_ptr(dev))
    return loc, aw


def every_entry(tag, hw, start, B, H, D, P, Nq=None, stream_shape=True):
    L = len(hw)
    value, rows, ref, gout, Nv, Nq = problem(hw, start, B, H, D, P, Nq)
    hwa, sta = ops._levels(hw, start)
    QUERIES[tag] = dict(overwrites=int(LIB.cgg_msda_backward_overwrites(hwa, sta, B, Nv, H, D, L, Nq, P)),
                        workspace_bytes=int(LIB.cgg_msda_backward_workspace_bytes(hwa, sta, B, Nv, H, D, L, Nq, P)))
    put(f'{tag} forward_fused f32 packed', ops.msda_forward_fused(value, hw, start, rows, ref, P))
    if stream_shape:
        buf, vpad = ops.padded_value_rows(B, Nv, H, D, dev)
        buf.zero_()
        vpad.copy_(value)
        put(f'{tag} forward_fused_vld padded rows', ops.msda_forward_fused(vpad, hw, start, rows, ref, P))
        if Nq == Nv:
            merged = torch.cat([value.flatten(2), rows], -1).contiguous()
            put(f'{tag} forward_fused_vld merged rows', ops.msda_forward_fused_rows(merged, hw, start, ref, P, H, D))
    v16, r16 = value.bfloat16(), rows.bfloat16()
    put(f'{tag} forward_fused_bf16', ops.msda_forward_fused_bf16(v16, hw, start, r16, ref, P))
    if stream_shape:
        put(f'{tag} forward_fused_bf16_hm', ops.msda_forward_fused_bf16(v16.permute(0, 2, 1, 3).contiguous(), hw, start, r16, ref, P, head_major=True))
    put(f'{tag} forward_hostlevels bf16 value fused', ops.msda_forward_fused(v16, hw, start, rows, ref, P))
    loc, aw = prologue(rows, ref, hw, B, Nq, H, L, P)
    put(f'{tag} prologue', loc, aw)
    put(f'{tag} forward_hostlevels', ops.msda_forward_hostlevels(value, hw, start, loc, aw))
    put(f'{tag} forward_hostlevels bf16 value', ops.msda_forward_hostlevels(v16, hw, start, loc, aw))
    shapes = torch.tensor(hw, dtype=torch.int64, device=dev)
    starts = torch.tensor(start, dtype=torch.int64, device=dev)
    put(f'{tag} forward (device table)', ops.msda_forward(value, shapes, starts, loc, aw))
    put(f'{tag} backward (device table)', *ops.msda_backward(value, shapes, starts, loc, aw, gout))
    vr, lr, ar = value.clone().requires_grad_(), loc.clone().requires_grad_(), aw.clone().requires_grad_()
    out = ops.MultiScaleDeformableAttnFunction.apply(vr, shapes, starts, lr, ar, 64)
    out.backward(gout)
    put(f'{tag} mmcv function', out.detach(), vr.grad, lr.grad, ar.grad)
    for two_pass in (True, False):
        for side in (True, False):
            ops.MSDA_BWD_2P, ops.MSDA_BWD_2S = two_pass, side
            gv, gl, gw = ops.msda_backward_hostlevels(value, hw, start, loc, aw, gout)
            put(f'{tag} backward_hostlevels_ws workspace={two_pass} side={side}', gv, gl, gw)
    ops.MSDA_BWD_2P = ops.MSDA_BWD_2S = True
    gv, grows = ops.msda_rows_backward(value, rows, ref, hw, start, P, gout)
    put(f'{tag} rows backward (prologue, backward, prologue backward)', gv, grows)
    return value, rows, ref, gout, Nv, Nq


PYRAMIDS = [
    ('pyramid 1', [(32, 32), (16, 16), (8, 8)], [0, 1024, 1280]),
    ('pyramid 2', [(16, 16), (8, 8), (4, 4)], [0, 256, 320]),
    ('pyramid 3', [(8, 16), (4, 8), (4, 8)], [0, 128, 160]),
    ('pyramid 4', [(4, 6), (2, 3), (1, 2)], [0, 24, 30]),
    ('pyramid 5 (1 listed 1, 0, 2)', [(16, 16), (32, 32), (8, 8)], [1024, 0, 1280]),
]
B, H, D, P = 2, 8, 32, 4
for tag, hw, start in PYRAMIDS:
    N = sum(h * w for h, w in hw)
    GATES[tag] = dict(Nq=N, t2d=N % 16 == 0 and tiles(hw, start, N, 4, 4, 16), t8=N % 64 == 0 and tiles(hw, start, N, 8, 8, 64),
                      patch=N % 32 == 0 and tiles(hw, start, N, 8, 4, 32), sorted=sorted_rule(hw, N, N, D, P),
                      fits=all(s >= 0 and s + h * w <= N for (h, w), s in zip(hw, start)))
    print(tag, hw, start, GATES[tag], flush=True)
    every_entry(tag, hw, start, B, H, D, P)
    assert QUERIES[tag]['overwrites'] == int(GATES[tag]['sorted']), (tag, QUERIES[tag])
    print('  ', QUERIES[tag], flush=True)
every_entry('generic H=4 D=16 L=2 P=2', [(6, 5), (3, 2)], [0, 30], 2, 4, 16, 2, Nq=37, stream_shape=False)
torch.cuda.synchronize()
print(f'{len(HASH)} outputs hashed', flush=True)

# ---- invalid calls: (code, text) of every entry, all refused on the host before a launch ----------------------------------------
tag, hw, start = PYRAMIDS[0]
L = 3
value, rows, ref, gout, Nv, Nq = problem(hw, start, B, H, D, P)
loc, aw = prologue(rows, ref, hw, B, Nq, H, L, P)
v16, r16 = value.bfloat16(), rows.bfloat16()
out = torch.empty(B, Nq, H * D, device=dev)
out16 = out.bfloat16()
gv, gl, gw = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(aw)
LD = 3 * H * L * P
hw4, start4 = PYRAMIDS[3][1], PYRAMIDS[3][2]
N4 = 32
S = stream_ptr(dev)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def calls(hwl, stl, Lc=L, ld=LD, vld=H * D, table=True, ow=0, Nvc=None, small=False):
    """every cgg_msda_* entry with a level table, as (symbol, args)"""
    n = Nvc or Nv
    hwa, sta = ops._levels(hwl, stl)
    dhw = torch.tensor(hwl, dtype=torch.int64, device=dev)
    dst = torch.tensor(stl, dtype=torch.int64, device=dev)
    keep.extend([dhw, dst])
    th, ts = (hwa, sta) if table else (None, None)
    dh, ds = (p(dhw), p(dst)) if table else (None, None)
    dims = (B, n, H, D, Lc, n, P)
    return [
        ('cgg_msda_forward', (p(value), dh, ds, p(loc), p(aw), p(out)) + dims + (0, S)),
        ('cgg_msda_forward_fused', (p(value), dh, ds, p(rows), ld, p(ref), p(out)) + dims + (0, S)),
        ('cgg_msda_forward_hostlevels', (p(value), th, ts, p(loc), p(aw), None, 0, p(out)) + dims + (0, 0, S)),
        ('cgg_msda_forward_hostlevels', (p(value), th, ts, p(rows), None, p(ref), ld, p(out)) + dims + (0, 1, S)),
        ('cgg_msda_forward_fused_vld', (p(value), vld, th, ts, p(rows), ld, p(ref), p(out)) + dims + (S,)),
        ('cgg_msda_forward_fused_bf16', (p(v16), th, ts, p(r16), ld, p(ref), p(out16)) + dims + (S,)),
        ('cgg_msda_forward_fused_bf16_hm', (p(v16), th, ts, p(r16), ld, p(ref), p(out16)) + dims + (S,)),
        ('cgg_msda_backward', (p(value), dh, ds, p(loc), p(aw), p(gout), p(gv), p(gl), p(gw)) + dims + (S,)),
        ('cgg_msda_backward_hostlevels', (p(value), th, ts, p(loc), p(aw), p(gout), p(gv), p(gl), p(gw)) + dims + (ow, S)),
        ('cgg_msda_backward_hostlevels_2s', (p(value), th, ts, p(loc), p(aw), p(gout), p(gv), p(gl), p(gw)) + dims + (ow, S, None)),
        ('cgg_msda_backward_hostlevels_ws', (p(value), vld, th, ts, p(loc), p(aw), p(gout), p(gv), p(gl), p(gw)) + dims + (ow, None, 0, S, None)),
    ]


keep = []
over = list(start[:-1]) + [start[-1] + 1]
INVALID = [
    ('null table', calls(hw, start, table=False), None),
    ('L = 9', calls(hw * 3, start * 3, Lc=9), None),
    ('last level overruns Nv by one pixel', calls(hw, over), None),
    ('ld = 3 H L P - 1', calls(hw, start, ld=LD - 1), ('forward_fused', 'forward_hostlevels')),
    ('vld = H D - 4', calls(hw, start, vld=H * D - 4), ('_vld', '_ws')),
    ('overwrite_loc_attn = 1 on pyramid 4', calls(hw4, start4, ow=1, Nvc=N4), ('backward_hostlevels',)),
]
for what, cs, only in INVALID:
    for i, (sym, args) in enumerate(cs):
        if only and not any(o in sym for o in only) or (what.startswith('ld') and i == 2):
            continue
        rc = getattr(LIB, sym)(*args)
        assert rc != 0, (what, sym)
        ERRORS[f'{what}: {sym}{" fused" if i == 3 else ""}'] = [rc, LIB.cgg_last_error_string().decode()]
torch.cuda.synchronize()
for k, v in ERRORS.items():
    print(f'{k}: {v}', flush=True)

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
    print(f'{name:44s} median {TIME[name]["median_us"]:9.1f} us   min {ts[0]:9.1f}   p90 {TIME[name]["p90_us"]:9.1f}', flush=True)


hw, start = [(128, 128), (64, 64), (32, 32)], [0, 16384, 20480]              # the encoder: 2 images of 128^2 + 64^2 + 32^2 queries
value, rows, ref, gout, Nv, Nq = problem(hw, start, B, H, D, P)
loc, aw = prologue(rows, ref, hw, B, Nq, H, 3, P)
merged = torch.cat([value.flatten(2), rows], -1).contiguous()
v16, r16 = value.bfloat16(), rows.bfloat16()
vhm = v16.permute(0, 2, 1, 3).contiguous()
timed('forward_fused f32 packed', lambda: ops.msda_forward_fused(value, hw, start, rows, ref, P))
timed('forward_fused_vld f32 merged rows', lambda: ops.msda_forward_fused_rows(merged, hw, start, ref, P, H, D))
timed('forward_fused_bf16 row-major', lambda: ops.msda_forward_fused_bf16(v16, hw, start, r16, ref, P))
timed('forward_fused_bf16_hm head-major', lambda: ops.msda_forward_fused_bf16(vhm, hw, start, r16, ref, P, head_major=True))
timed('backward_hostlevels_ws (incl. zero-fills)', lambda: ops.msda_backward_hostlevels(value, hw, start, loc, aw, gout))

torch.cuda.synchronize()
assert os.path.abspath(_lib.LIB_PATH) == os.path.abspath(sys.argv[2]) and _lib._lib is not None
with open(sys.argv[3], 'w') as f:
    json.dump(dict(hashes=HASH, times=TIME, gates=GATES, queries=QUERIES, errors=ERRORS), f, indent=1)
