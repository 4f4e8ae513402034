"""The fused layer kernels at their row, plane and LayerNorm edges: decoder_tail, decoder_mid, decoder_ffn, layernorm_chain, the
LayerNorm epilogue of linear_rows (32 rows per workgroup) and encoder_ffn_ln, encoder_layer_tail, encoder_layer_tail_x3 / x3a (64 rows
per workgroup). Operands, float64 references and the bound: tests/layer_cases.py; its room and teeth: tests/test_layer_cases.py.

Every kernel goes through its `ops` wrapper, the decoder kernels with both weight kinds (`pack_linear_weight`: bf16 operands,
`pack_linear_weight_x3`: f16 x 3). Every output is compared with float64 over every element,

    |got - want| <= FACTOR * max(e_ref, T) + extra          (layer_cases: T = u S of the stage that forms the output)

and every call is made twice and must be bit-identical.
Decoder rows: (M, pos rows) = (1, 1) one row; (31, 100) one short of the workgroup and pos rows > M; (32, 20) exactly full; (33, 100)
one row into a second workgroup; (77, 20) a position wrap that is not aligned to the workgroup, M % pos rows != 0. Planes: 1, 3, 8 (the
decoder tail's cap) and, for `layernorm_chain`, 9 and 16. FFN widths 256 .. 4096 = 1 .. 16 planes. Row-strided (260) views of x, core
and res. Encoder rows: M = 1, 63, 64, 65, 130; FFN widths 256, 512, 1024; pos rows 1 and 50; the K / V variants with B = 2 and levels
2 x 3, 4 x 5, 8 x 9 (level boundaries inside the 64-row blocks).
Conditioning: 43 rows of tests/norm_cases.py (row r is of kind r % 11, so the ragged last workgroup of the decoder kernels, rows 32 ..
42, holds every kind) as the SUM the kernel forms in front of its LayerNorm -- the plane sum, proj + bias + res, x + a Wo^T -- with an
exactly computable GEMM part, held per family to norm_cases' f32-class bound (linear_rows: rows of N = 32, 49 and 256 elements);
cond='second' hands the SECOND LayerNorm of a kernel off-centre, tight rows through a first one with gamma 2^-10, beta 64; the 'round' case of `layer_cases.tail_case` makes the
mask MLP's result depend on where the hidden blocks are rounded.

Each test prints worst error / bound per output. Measured on an MI355X, worst over the parametrisation (*/fam: the worst family of
the per-family conditioning bound; a bf16 output spends up to the whole of `extra`, one bf16 rounding, on its own rounding):

  decoder_tail      bf16    y 0.14  yp 0.16  me 0.061  qn 0.0016        cond: y 0.12  y/fam 0.19  me 0.051  qn 0.0088
                                                                        round: me 1.6e-06  qn 3.7e-06
                    x3      y 0.14  yp 0.16  me 0.08   qn 0.046         cond: y 0.12  y/fam 0.19  me 0.15   qn 0.12
                                                                        round: me 0.12  qn 0.036
  decoder_mid       bf16    x1 0.18   q 0.01   kv 0.012                 cond: x1 0.068  x1/fam 0.12  q 0.0067  kv 0.0089
                    x3      x1 0.089  q 0.06   kv 0.051                 cond: x1 0.034  x1/fam 0.12  q 0.12    kv 0.12
  decoder_ffn       bf16    planes 0.023  sum 0.0062
                    x3      planes 0.1    sum 0.065
  linear_rows + LN  bf16    y 0.19   yp 0.19                                    cond (N = 32, 49, 256): y 0.1   y/fam 0.19
                    x3      y 0.1    yp 0.11                                    cond (N = 32, 49, 256): y 0.081 y/fam 0.19
  layernorm_chain           y 0.16  yp 0.17  z 0.18                     cond: y 0.13  y/fam 0.19  z 0.14  z/fam 0.22
  encoder_ffn_ln    bf16    y32 0.048   y16 0.64  yp16 0.9              cond: y32/fam 0.17  y16 0.92  yp16 0.98
                                                                        kv: y32 0.018  m16 0.72  mp16 0.85
  encoder_layer_tail bf16   y32 0.0077  y16 0.15  yp16 0.51             cond: y16 0.051  yp16 0.21
                                                                        kv: y32 0.0019  m16 0.086  mp16 0.1
                    x3      y 0.12  yp 0.13                             cond: y 0.2  y/fam 0.21
                    x3a     y 0.15  yp 0.14                             cond: y 0.1  y/fam 0.16

  second LayerNorm on rows of mean 64 / 32, spread 1e-3 / 5e-4 (cond='second'):
    decoder_tail (through me)  bf16 me 0.075  x3 me 0.093       layernorm_chain  z 0.15  z/fam 0.22
    encoder_layer_tail         x3, x3a y 0.066  y/fam 0.21      bf16: x1 is stored as bf16 = 64 exactly, y = beta_1 (y16 2.6e-06)

cgg_encoder_layer_tail_bf16 is the one kernel NOT held to the per-family f32-class bound: it rounds x1 to bf16 before anything reads
it, so its LN0 is pinned only to bf16 class (layer_cases' docstring says what that leaves open).
No kernel is above 1, FACTOR = 8 unchanged. The bf16 GEMM outputs sit far below their bound (u = 2^-9 on the whole of S allows every
operand on the wrong bf16 neighbour at once; the kernels and float64 disagree on a handful per case), which is why the 'round' case
exists: there a misplaced rounding point is an O(1) error of the result.
"""
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops

import layer_cases as LC

pytestmark = pytest.mark.gpu

C = LC.C
_PACKED = {}


def _pack(kind, dev, W):
    """the packed device image of weight W (cached by the CPU tensor: the cases are)"""
    key = (kind, id(W))
    if key not in _PACKED:
        fn = ops.pack_linear_weight if kind == 'bf16' else ops.pack_linear_weight_x3
        _PACKED[key] = (W, fn(W.to(dev).contiguous()))
    return _PACKED[key][1]


def _norm(n, dev):
    return n[0].to(dev), n[1].to(dev), n[2]


def _twice(fn):
    """fn() twice: the outputs (tensors or None) must be bit-identical; -> the first"""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for i, (s, t) in enumerate(zip(a, b)):
        assert (s is None) == (t is None) and (s is None or torch.equal(s, t)), f'output {i} differs between two calls'
    return a


def _strided(t, dev):
    """t (M, 256) as a column view with row stride 260 of a wider buffer whose other columns are NaN"""
    buf = torch.full((t.shape[0], 260), float('nan'), device=dev)
    buf[:, :C] = t.to(dev)
    v = buf[:, :C]
    assert v.stride(0) == 260
    return v


# ------------------------------------------------------------------------------------------------
# decoder_tail
# ------------------------------------------------------------------------------------------------
def _run_tail(dev, case, label):
    o, kind = case.o, case.kind
    planes, pos = o.planes.to(dev), o.pos.to(dev)
    na, nb = _norm(o.norm_a, dev), _norm(o.norm_b, dev)
    mlp = tuple(_pack(kind, dev, t) if i % 2 == 0 else t.to(dev) for i, t in enumerate(o.mlp))
    qp = (_pack(kind, dev, o.qproj[0]), o.qproj[1].to(dev))
    full = None
    for with_q in (True, False):
        for want_pos in (True, False):
            y, yp, me, qn = _twice(lambda: ops.decoder_tail(planes, na, pos, nb, mlp, qp if with_q else None, want_pos=want_pos))
            assert (yp is None) == (not want_pos) and (qn is None) == (not with_q)
            LC.assert_all(f'{label} q={with_q} pos={want_pos}', case, dict(y=y, yp=yp, me=me, qn=qn))
            if full is None:
                full = (y, yp, me, qn)
            else:                       # an output does not depend on which others were asked for
                assert torch.equal(y, full[0]) and torch.equal(me, full[2])
                assert (yp is None or torch.equal(yp, full[1])) and (qn is None or torch.equal(qn, full[3]))


@pytest.mark.parametrize('nsum', [1, 3, 8])
@pytest.mark.parametrize('M,pos_rows', LC.M_POS)
@pytest.mark.parametrize('kind', LC.KINDS)
def test_decoder_tail(dev, kind, M, pos_rows, nsum):
    _run_tail(dev, LC.tail_case(kind, M, pos_rows, nsum), f'decoder_tail {kind} M={M} pos={pos_rows} nsum={nsum}')


@pytest.mark.parametrize('cond', [True, 'second', 'round'], ids=['cond', 'second', 'round'])
@pytest.mark.parametrize('kind', LC.KINDS)
def test_decoder_tail_conditioning(dev, kind, cond):
    """LN_a on norm_cases rows formed as the sum of three planes, LN_b on its output (eps_b = 1e-3), per family; the same with
    gamma_a = 2^-10, beta_a = 64, so that LN_b (seen through the mask MLP) gets rows of mean 64 and spread 1e-3; and the case whose
    mask MLP is decided by the rounding point of the hidden blocks"""
    M = 33 if cond == 'round' else 43
    _run_tail(dev, LC.tail_case(kind, M, 20, 3, cond=cond), f'decoder_tail {kind} {cond}')


# ------------------------------------------------------------------------------------------------
# layernorm_chain
# ------------------------------------------------------------------------------------------------
def _run_chain(dev, case, label):
    o = case.o
    planes = o.planes.to(dev)
    args = (_norm(o.norm_a, dev), o.pos.to(dev), _norm(o.norm_b, dev))
    y, yp, z = _twice(lambda: ops.layernorm_chain(planes, *args))
    LC.assert_all(label, case, dict(y=y, yp=yp, z=z))
    if planes.shape[0] == 1:            # the 2-D form is the one-plane form
        y2, yp2, z2 = ops.layernorm_chain(planes[0], *args)
        assert torch.equal(y2, y) and torch.equal(yp2, yp) and torch.equal(z2, z)
    y1, yp1, z1 = ops.layernorm_chain(planes, args[0])
    assert yp1 is None and z1 is None and torch.equal(y1, y)


@pytest.mark.parametrize('nsum', [1, 3, 8, 9, 16])
@pytest.mark.parametrize('M,pos_rows', LC.M_POS)
def test_layernorm_chain_planes(dev, M, pos_rows, nsum):
    """3-D input: the float64 sum of ALL planes, past the 8 the decoder tail holds"""
    _run_chain(dev, LC.tail_case('f32', M, pos_rows, nsum), f'layernorm_chain M={M} pos={pos_rows} nsum={nsum}')


@pytest.mark.parametrize('nsum', [3, 9])
def test_layernorm_chain_conditioning(dev, nsum):
    _run_chain(dev, LC.tail_case('f32', 43, 20, nsum, cond=True), f'layernorm_chain cond nsum={nsum}')


def test_layernorm_chain_second_norm_conditioning(dev):
    """gamma_a = 2^-10, beta_a = 64: z = LN_b(y) on rows of mean 64 and spread 1e-3, per family"""
    _run_chain(dev, LC.tail_case('f32', 43, 20, 3, cond='second'), 'layernorm_chain second')


# ------------------------------------------------------------------------------------------------
# decoder_mid
# ------------------------------------------------------------------------------------------------
def _run_mid(dev, case, label):
    o, kind = case.o, case.kind
    core, res, pos = o.core.to(dev), o.res.to(dev), o.pos.to(dev)
    wo, bo, norm = _pack(kind, dev, o.wo), o.bo.to(dev), _norm(o.norm, dev)
    qkv = (_pack(kind, dev, o.qkv[0]), o.qkv[1].to(dev))
    x1, q, kv = _twice(lambda: ops.decoder_mid(core, wo, bo, res, norm, pos, qkv))
    LC.assert_all(f'{label} qkv', case, dict(x1=x1, q=q, kv=kv))
    only = _twice(lambda: ops.decoder_mid(core, wo, bo, res, norm))
    assert only[1] is None and only[2] is None and torch.equal(only[0], x1)
    sv = ops.decoder_mid(_strided(o.core, dev), wo, bo, _strided(o.res, dev), norm, pos, qkv)
    assert torch.equal(sv[0], x1) and torch.equal(sv[1], q) and torch.equal(sv[2], kv), 'row-strided core / res'


@pytest.mark.parametrize('M,pos_rows', LC.M_POS)
@pytest.mark.parametrize('kind', LC.KINDS)
def test_decoder_mid(dev, kind, M, pos_rows):
    _run_mid(dev, LC.mid_case(kind, M, pos_rows), f'decoder_mid {kind} M={M} pos={pos_rows}')


@pytest.mark.parametrize('kind', LC.KINDS)
def test_decoder_mid_conditioning(dev, kind):
    """the LayerNorm on norm_cases rows formed as core Wo^T + bo + res with an exact projection, per family"""
    _run_mid(dev, LC.mid_case(kind, 43, 20, cond=True), f'decoder_mid {kind} cond')


# ------------------------------------------------------------------------------------------------
# decoder_ffn
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Fw', [256, 768, 2048, 4096])
@pytest.mark.parametrize('M', [m for m, _ in LC.M_POS])
@pytest.mark.parametrize('kind', LC.KINDS)
def test_decoder_ffn(dev, kind, M, Fw):
    """every plane against its own float64 value (plane 0 alone carries b2 and the residual), their float64 sum, and x as a
    row-strided view"""
    case = LC.ffn_case(kind, M, Fw)
    o = case.o
    w1, w2 = _pack(kind, dev, o.w1), _pack(kind, dev, o.w2)
    b1, b2, x = o.b1.to(dev), o.b2.to(dev), o.x.to(dev)
    planes, = _twice(lambda: ops.decoder_ffn(x, w1, b1, w2, b2, Fw))
    assert planes.shape == (Fw // C, M, C)
    LC.assert_all(f'decoder_ffn {kind} M={M} F={Fw}', case, dict(planes=planes, sum=planes.double().sum(0)))
    assert torch.equal(ops.decoder_ffn(_strided(o.x, dev), w1, b1, w2, b2, Fw), planes), 'row-strided x'


# ------------------------------------------------------------------------------------------------
# linear_rows_bf16 with the LayerNorm epilogue
# ------------------------------------------------------------------------------------------------
def _run_linear(dev, case, N, label):
    o, kind = case.o, case.kind
    w = _pack(kind, dev, o.w)
    x, b, res, pos, norm = o.x.to(dev), o.b.to(dev), o.res.to(dev), o.pos.to(dev), _norm(o.norm, dev)
    y, yp = _twice(lambda: ops.linear_rows_bf16(x, w, N, b, res=res, ln=norm, pos=pos, want_pos=True))
    LC.assert_all(label, case, dict(y=y, yp=yp))
    assert torch.equal(ops.linear_rows_bf16(x, w, N, b, res=res, ln=norm), y)


@pytest.mark.parametrize('K', [16, 256])
@pytest.mark.parametrize('N', [32, 49, 256])
@pytest.mark.parametrize('M,pos_rows', LC.M_POS)
@pytest.mark.parametrize('kind', LC.KINDS)
def test_linear_rows_layernorm(dev, kind, M, pos_rows, N, K):
    _run_linear(dev, LC.linear_ln_case(kind, M, N, K, pos_rows), N, f'linear_rows+ln {kind} M={M} pos={pos_rows} N={N} K={K}')


@pytest.mark.parametrize('N', [32, 49, 256])
@pytest.mark.parametrize('kind', LC.KINDS)
def test_linear_rows_layernorm_conditioning(dev, kind, N):
    """the epilogue's own LayerNorm (two passes across the waves over LDS, csrc/linear_rows2.hip) on norm_cases rows of N elements
    formed as x W^T + b + res with an exact projection, per family"""
    _run_linear(dev, LC.linear_ln_case(kind, 43, N, 256, 20, cond=True), N, f'linear_rows+ln {kind} cond N={N}')


# ------------------------------------------------------------------------------------------------
# encoder kernels: encoder_ffn_ln, encoder_layer_tail (bf16), encoder_layer_tail_x3 (x3 / x3a)
# ------------------------------------------------------------------------------------------------
def _run_enc(dev, case, variant, kind, label):
    """the plain call of the case's kernel, twice -> its outputs under the spec's names (x3a rows decoded), checked"""
    o = case.o
    wk = 'bf16' if kind == 'bf16' else 'x3'
    w1, w2 = _pack(wk, dev, o.w1), _pack(wk, dev, o.w2)
    b1, b2, n1, pos = o.b1.to(dev), o.b2.to(dev), _norm(o.norm1, dev), o.pos.to(dev)
    x = o.x.to(dev)
    if variant == 'tail':
        a, wo, bo, n0 = o.a.to(dev), _pack(wk, dev, o.wo), o.bo.to(dev), _norm(o.norm0, dev)
    if kind == 'bf16':
        x16 = x.bfloat16()
        assert torch.equal(x16.float(), x)
        if variant == 'ffn':
            call = lambda **kw: ops.encoder_ffn_ln(x16, w1, b1, w2, b2, *n1, pos=pos, **kw)                      # noqa: E731
        else:
            a16 = a.bfloat16()
            assert torch.equal(a16.float(), a)
            call = lambda **kw: ops.encoder_layer_tail(a16, x16, wo, bo, n0, w1, b1, w2, b2, n1, pos=pos, **kw)   # noqa: E731
        y32, y16, yp16 = _twice(lambda: call(want_f32=True, want_bf16=True, want_pos=True))
        LC.assert_all(label, case, LC.enc_outs(case, y32, y16.float(), yp16.float()))
        p = pos[LC.pos_index(x.shape[0], pos.shape[0]).to(dev)]
        assert torch.equal(y16, y32.bfloat16()) and torch.equal(yp16, (y32 + p).bfloat16()), 'bf16 outputs are not the roundings'
        only = call(want_f32=False, want_bf16=True, want_pos=False)
        assert only[0] is None and only[2] is None and torch.equal(only[1], y16)
        return y32
    if kind == 'x3a':
        x = ops.x3a_encode(x)
        assert torch.equal(ops.x3a_decode(x), o.x.to(dev)), 'the case starts from the values the x3a rows hold'
    ops.x3_overflow_check(dev, reset=True)
    y, yp = _twice(lambda: ops.encoder_layer_tail_x3(a, x, wo, bo, n0, w1, b1, w2, b2, n1, pos=pos, want_pos=True, x3a=kind == 'x3a'))
    assert ops.x3_overflow_check(dev, reset=True) is False
    only = ops.encoder_layer_tail_x3(a, x, wo, bo, n0, w1, b1, w2, b2, n1, x3a=kind == 'x3a')
    assert only[1] is None and torch.equal(only[0], y)
    if kind == 'x3a':
        y, yp = ops.x3a_decode(y), ops.x3a_decode(yp)
    LC.assert_all(label, case, LC.enc_outs(case, y, None, yp))
    return y


@pytest.mark.parametrize('pos_rows', [1, 50])
@pytest.mark.parametrize('FF', [256, 512, 1024])
@pytest.mark.parametrize('M', LC.ENC_M)
@pytest.mark.parametrize('kind,variant', LC.ENC_KERNELS, ids=[f'{v}_{k}' for k, v in LC.ENC_KERNELS])
def test_encoder_kernels(dev, kind, variant, M, FF, pos_rows):
    """one row, one short of / exactly / one past the 64-row workgroup, two workgroups and a ragged third; 1, 2 and 4 hidden chunks"""
    _run_enc(dev, LC.enc_case(kind, variant, M, FF, pos_rows), variant, kind, f'encoder {variant} {kind} M={M} FF={FF} pos={pos_rows}')


@pytest.mark.parametrize('kind,variant', LC.ENC_KERNELS, ids=[f'{v}_{k}' for k, v in LC.ENC_KERNELS])
def test_encoder_kernels_conditioning(dev, kind, variant):
    """norm_cases rows (bf16 kinds for the bf16 kernels) as the sum in front of the kernel's first LayerNorm, exact GEMMs"""
    _run_enc(dev, LC.enc_case(kind, variant, 43, 512, 50, cond=True), variant, kind, f'encoder {variant} {kind} cond')


@pytest.mark.parametrize('kind', ['bf16', 'x3', 'x3a'])
def test_encoder_layer_tail_second_norm_conditioning(dev, kind):
    """gamma_0 = 2^-10, beta_0 = 64: x1 = 64 + O(1e-3), and with FFN(x1) = -relu(x1) / 2 LayerNorm 1 normalises rows of mean 32 and
    spread 5e-4 (x3, x3a: per family; bf16: x1 is stored as bf16, i.e. exactly 64, and y = beta_1 must come out)"""
    _run_enc(dev, LC.enc_case(kind, 'tail', 43, 512, 50, cond='second'), 'tail', kind, f'encoder tail {kind} second')


@pytest.mark.parametrize('variant', ['ffn', 'tail'])
def test_encoder_kernels_kv(dev, variant):
    """`encoder_ffn_ln_kv` / `encoder_layer_tail(kv=...)`: B = 2, levels 2 x 3, 4 x 5, 8 x 9 (S = 98, M = 196: level boundaries inside
    the 64-row blocks). y32 bit-identical to the plain variant; m16 / mp16 = bf16(y + shift), bf16(y + shift + pos), level-major,
    against float64 of the remapped rows"""
    B, level_hw = LC.ENC_LEVELS
    S = sum(h * w for h, w in level_hw)
    case = LC.enc_case('bf16', variant, B * S, 512, S, levels=LC.ENC_LEVELS)
    y32_plain = _run_enc(dev, case, variant, 'bf16', f'encoder {variant} kv (plain call)')
    o = case.o
    w1, w2 = _pack('bf16', dev, o.w1), _pack('bf16', dev, o.w2)
    b1, b2, n1, pos, shift = o.b1.to(dev), o.b2.to(dev), _norm(o.norm1, dev), o.pos.to(dev), o.shift.to(dev)
    x16 = o.x.to(dev).bfloat16().view(B, S, C)
    starts = [0]
    for h, w in level_hw[:-1]:
        starts.append(starts[-1] + h * w)
    if variant == 'ffn':
        run = lambda: ops.encoder_ffn_ln_kv(x16, w1, b1, w2, b2, *n1, shift, pos, starts, want_f32=True)          # noqa: E731
    else:
        a16, wo, bo, n0 = o.a.to(dev).bfloat16().view(B, S, C), _pack('bf16', dev, o.wo), o.bo.to(dev), _norm(o.norm0, dev)
        run = lambda: ops.encoder_layer_tail(a16, x16, wo, bo, n0, w1, b1, w2, b2, n1, kv=(shift, pos, starts), want_f32=True)  # noqa: E731
    y32, m16, mp16 = _twice(run)
    assert torch.equal(y32.view(B * S, C), y32_plain)
    # level-major -> image order: invert the permutation that layer_cases.level_major applies to the row index
    order = LC.level_major(torch.arange(B * S, dtype=torch.float32).view(-1, 1), B, level_hw).view(-1).long()
    back = torch.empty_like(order)
    back[order] = torch.arange(B * S)
    back = back.to(dev)
    LC.assert_all(f'encoder {variant} kv', case, LC.enc_outs(case, y32.view(B * S, C), None, None, m16[back].float(), mp16[back].float()))
