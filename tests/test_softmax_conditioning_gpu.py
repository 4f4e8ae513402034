"""The kernels that contain a softmax on the rows of tests/softmax_cases.py: scores of +-30 and more, one dominant key (first,
interior, in the ragged tail), a common offset of +-100, two equal maxima in different tiles, the largest score on a blocked key,
a single visible key, ramps whose running maximum changes at every tile and whose low end underflows.

Every output is compared with float64, per family, and no element is left out:

    |got - want| <= FACTOR * max(e_ref, u * S)          (softmax_cases.ratios)

e_ref = the largest error over the family of torch's own f32 formulation on the CPU (masked_fill(-inf) -> softmax -> matmul,
logsumexp, F.cross_entropy, autograd of these; with P rounded to bf16 before the PV product for the bf16-operand kernels),
FACTOR = 8, u = 2^-24 (f32 kernels), 2^-22 (f16 x 3), 2^-9 (bf16 operands, fed bf16-representable q, k, v, grad_out), and S by
kind of output as tabulated in softmax_cases. tests/test_softmax_cases.py shows on the CPU that a correct kernel of this design
has room under the bound (worst 0.25; 0.56 for bf16 operands). Each test prints its worst error / bound per family.

`masked_xattn_bf16` takes key counts that are a multiple of 4 only, so its ragged shape is (1, 37, 332) in place of (1, 37, 333):
five 64-key chunks and a tail of 12 keys.

Measured on an MI355X, worst error / bound over the shapes of each test (sh+- = shift_pos / shift_neg, sp0 / spM / spL = spike_first /
_mid / _last, mmax = masked_max, 1vis = single_visible, undf = underflow; 0 = below 0.005, - = the family is not part of the case):

                                    unit large   sh+   sh-   sp0   spM   spL  ramp   tie  mmax  1vis  undf   other
masked_xattn f32 / strided out      0.12  0.21  0.13  0.13     0     0     0  0.12  0.11  0.33     0  0.14
masked_xattn x3 out                 0.10  0.12  0.10  0.13  0.05  0.04  0.05  0.10  0.05  0.12  0.04  0.10
masked_xattn train f32 out          0.12  0.21  0.13  0.13     0     0     0  0.12  0.11  0.33     0  0.14
masked_xattn train f32 lse          0.10  0.12  0.08  0.07  0.12  0.12  0.12  0.14  0.12  0.01  0.16  0.13
masked_xattn train f32 grad_q       0.02  0.04  0.08  0.07  0.02  0.02  0.02  0.12  0.01     0  0.02  0.24
masked_xattn train f32 grad_kv         -     -     -     -     -     -     -     -     -     -     -     -   all 0.12
masked_xattn train x3 out           0.10  0.12  0.10  0.13  0.05  0.04  0.05  0.10  0.05  0.12  0.04  0.10
masked_xattn train x3 lse           0.02  0.02  0.04  0.03  0.05  0.04  0.04  0.05  0.05     0  0.08  0.05
masked_xattn train x3 grad_q        0.01  0.03  0.03  0.02     0     0     0  0.07  0.01     0     0  0.06
masked_xattn train x3 grad_kv          -     -     -     -     -     -     -     -     -     -     -     -   all 0.03
masked_xattn train bf16 out         0.22  0.55  0.14  0.20     0     0     0  0.21     0  0.13     0  0.11
masked_xattn train bf16 lse         0.01  0.05  0.06  0.07  0.04  0.04  0.04  0.05  0.05     0  0.06  0.02
masked_xattn train bf16 grad_q      0.01  0.01     0     0     0     0     0     0     0     0     0     0
masked_xattn train bf16 grad_kv        -     -     -     -     -     -     -     -     -     -     -     -   all 0.00
masked_xattn_bf16 out               0.22  0.53  0.12  0.25     0     0     0  0.17     0  0.18     0  0.14
window_attention out                0.22  0.15  0.12  0.13  0.11  0.20  0.15  0.13  0.13     -     -  0.14   table_large 0.13  beats_the_mask 0.00
window_attention lse                0.09  0.11  0.12  0.13  0.12  0.12  0.15  0.12  0.08     -     -  0.11   table_large 0.06  beats_the_mask 0.12
window_attention grad_q             0.04  0.09  0.09  0.09     0     0     0  0.16  0.07     -     -  0.17   table_large 0.09  beats_the_mask 0.00
window_attention grad_k                -     -     -     -     -     -     -     -     -     -     -     -   all 0.14
window_attention grad_v                -     -     -     -     -     -     -     -     -     -     -     -   all 0.06
window_attention grad_table            -     -     -     -     -     -     -     -     -     -     -     -   all 0.21
ce_rows f32 loss                    0.09  0.09  0.07  0.07  0.04  0.05  0.02  0.05  0.05     -     -  0.04
ce_rows f32 lse                     0.13  0.03  0.04  0.04     0     0     0  0.05  0.02     -     -  0.04
ce_rows f32 grad                    0.03  0.02  0.01  0.01     0     0     0  0.02  0.02     -     -  0.01
ce_rows bf16 loss                   0.08  0.05  0.07  0.07     0     0     0  0.02  0.05     -     -  0.05
ce_rows bf16 lse                    0.09  0.04  0.04  0.04     0     0     0  0.02  0.02     -     -  0.05
ce_rows bf16 grad                   1.00*  0.98  0.94  0.93  0.89  0.90  0.76  0.85  0.93     -     -  0.80
ce_rows -inf loss                   0.09  0.03  0.05  0.07  0.13  0.05     0  0.05  0.02     -     -  0.10
ce_rows -inf lse                    0.09  0.02  0.03  0.04  0.10     0     0  0.03  0.02     -     -  0.05
rowwise_softmax_argmax prob         0.13  0.12  0.12  0.17     0     0     0  0.32     0     -     -  0.04
rowwise_softmax_argmax max          0.13  0.12  0.10  0.17     0     0     0  0.25     0     -     -  0.04
grounding cost                         -  0.04  0.14     -     -     -     -     -     -     -     -     -
grounding dsim                         -  0.05  0.04     -     -     -     -     -     -     -     -     -
msda_forward_fused out                 -     -  0.12  0.13     -     -     -     -     -     -     -     -   spike 0.12  flat 0.13
msda_rows_backward grad_value          -     -     -     -     -     -     -     -     -     -     -     -   all 0.02
msda_rows_backward grad_logits         -     -  0.03  0.04     -     -     -     -     -     -     -     -   spike 0.00  flat 0.03

* 0.997: the bound of a bf16 gradient is one bf16 rounding of `want` plus the f32 term, and the kernel's output is a rounding.
Everything else stands at or below 0.55 (bf16 operands) and 0.33 (f32, f16 x 3), next to 0.56 and 0.27 for the emulated kernels of
tests/test_softmax_cases.py, so FACTOR and u stand. Two findings:
  * `ce_rows_forward` on a row whose first vector is all -inf, read by a thread with a second pass (N = 2056): loss and lse were NaN
    on all ten rows before the fix in csrc/ce_rows.hip (ratio inf); 0.13 and 0.10 after.
  * grad_k of `window_attention_backward` at ws = 7, shift 0 stood at 1.36 of the bound as first stated,
    S = (1 + max A) max |want|. A correct emulation of the lse-recompute design stands at 1.34 of it (test_softmax_cases.py): the
    bound lacked the term S_rows that softmax_cases.ratios now states, and with it kernel and emulation are both at 0.14.
The f32 backward of `masked_xattn` is linear in a 2^-20 grad_out to 8e-40 (products of the `underflow` rows that fall below 2^-126);
the f16 x 3 backward to the bit.
"""
import pytest
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import ops, runtime
from cgg_amd.query_decoder import pack_bool_mask
from oracle import ops as ref

import softmax_cases as SC
from test_norm_conditioning_gpu import _bf16_rounding
from test_window_attn_gpu import _coords, dense_ref

pytestmark = pytest.mark.gpu

H = 4
E = H * SC.D_HEAD
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _report(results):
    """results: [(label, ratios)] -> prints every one, then asserts every one"""
    bad = {}
    for label, r in results:
        print(f'{label}: ' + '  '.join(f'{k}={v[2]:.3g}' for k, v in r.items()))
        bad.update({f'{label} {k}': v for k, v in r.items() if not v[2] <= 1.0})
    assert not bad, f'(error, bound, error / bound) {bad}'


# ------------------------------------------------------------------------------------------------
# A. masked cross-attention
# ------------------------------------------------------------------------------------------------
XATTN_SHAPES = [(1, 37, 333, True), (2, 130, 200, True), (1, 100, 100, False)]
_ids = lambda s: f'B{s[0]}Q{s[1]}S{s[2]}{"" if s[3] else "unmasked"}'         # noqa: E731


def _attn_case(shape, bf16=False):
    """(case, grad_out, float64 references, torch's f32 references) of one shape, computed once"""
    def make():
        B, Q, S, masked = shape
        c = SC.attention(B, Q, S, H, seed=S, masked=masked, bf16=bf16)
        go = torch.randn(B, Q, E, generator=torch.Generator().manual_seed(S + 1))
        if bf16:
            go = go.bfloat16().float()
        return c, go, SC.attention_refs(c, go), SC.attention_refs(c, go, torch.float32, p_dtype=torch.bfloat16 if bf16 else None)
    return _cached(('attn', shape, bf16), make)


def _bits(c, dev):
    return None if c.mask is None else pack_bool_mask(c.mask).contiguous().to(dev)


@pytest.mark.parametrize('form', ['f32', 'x3', 'strided'])
@pytest.mark.parametrize('shape', XATTN_SHAPES, ids=_ids)
def test_masked_xattn_forward(dev, shape, form, monkeypatch):
    """`ops.masked_xattn`: the f32-MFMA kernel, the f16 x 3 kernel, and the f32 kernel on kv as a column slice of a wider tensor"""
    c, _, want, ref32 = _attn_case(shape)
    monkeypatch.setattr(ops, 'XATTN_X3', form == 'x3')
    kv = c.kv.to(dev)
    if form == 'strided':
        wide = torch.randn(c.B, c.S, 2 * E + 64, device=dev)
        wide[..., 32:32 + 2 * E] = kv
        kv = wide[..., 32:32 + 2 * E]
        assert not kv.is_contiguous()
    with runtime.precision_scope('fp32'):
        assert runtime.x3_enabled()
        out = ops.masked_xattn(c.q.to(dev), kv, _bits(c, dev), H)
    r = SC.attention_ratios(c, dict(out=out.cpu()), want, ref32, SC.U_X3 if form == 'x3' else SC.U_F32)
    _report([(f'masked_xattn {form} {_ids(shape)} out', r['out'])])


def _train(dev, c, go, scope, scale_go=1.0):
    with runtime.precision_scope(scope):
        q, kv, bits = c.q.to(dev), c.kv.to(dev), _bits(c, dev)
        out, lse = ops.masked_xattn(q, kv, bits, H, return_lse=True)
        gq, gkv = ops.masked_xattn_backward(q, kv, bits, out, lse, (go * scale_go).to(dev), H)
    return dict(out=out, lse=lse, grad_q=gq, grad_kv=gkv)


@pytest.mark.parametrize('form', ['f32', 'x3'])
@pytest.mark.parametrize('shape', XATTN_SHAPES, ids=_ids)
def test_masked_xattn_train(dev, shape, form, monkeypatch):
    """`return_lse=True` forward in the CGG_F32 / CGG_F32_X3 mode (out and lse) and the backward in f32 / f16 x 3 mode, fed the out
    and lse of its own forward: grad_q per family, grad_kv globally. A 2^-20 grad_out gives the f16 x 3 backward's gradients times
    2^-20 to the bit (its operands take their pre-scale from max |grad_out|). The f32 backward is linear to the bit only while no
    product underflows: on the `underflow` rows P dS falls below 2^-126 with the small grad_out, so there the two agree to
    S products of less than 2^-126 each, scaled back by 2^20, times an operand below 4094."""
    c, go, want, ref32 = _attn_case(shape)
    x3 = form == 'x3'
    monkeypatch.setattr(ops, 'XATTN_X3', True)
    monkeypatch.setattr(ops, 'XATTN_X3_TRAIN', x3)
    monkeypatch.setattr(ops, 'XATTN_X3_BWD', x3)
    with runtime.precision_scope('fp32'):
        assert ops._xattn_train_dtype(forward=True) == (ops.CGG_F32_X3 if x3 else 0) and ops._xattn_train_dtype() == 0
    got = _train(dev, c, go, 'fp32')
    small = _train(dev, c, go, 'fp32', 2.0 ** -20)
    r = SC.attention_ratios(c, {k: v.cpu() for k, v in got.items()}, want, ref32, SC.U_X3 if x3 else SC.U_F32)
    _report([(f'masked_xattn train {form} {_ids(shape)} {k}', v) for k, v in r.items()])
    for name in ('grad_q', 'grad_kv'):
        diff = (small[name] * 2.0 ** 20 - got[name]).abs().max().item()
        print(f'masked_xattn train {form} {_ids(shape)} {name}: 2^-20 grad_out off by {diff:.3g}')
        assert diff <= (0.0 if x3 else max(c.S, c.Q) * SC.X3_RANGE * 2.0 ** -106), (name, diff)


@pytest.mark.parametrize('shape', XATTN_SHAPES, ids=_ids)
def test_masked_xattn_train_bf16_mfma(dev, shape):
    """throughput-mode training (CGG_F32_BF16MFMA): f32 rows in memory, products on bf16 MFMA operands"""
    c, go, want, ref32 = _attn_case(shape, bf16=True)
    with runtime.precision_scope('bf16'):
        assert ops._xattn_train_dtype(forward=True) == ops.CGG_F32_BF16MFMA
    got = _train(dev, c, go, 'bf16')
    r = SC.attention_ratios(c, {k: v.cpu() for k, v in got.items()}, want, ref32, SC.U_BF16)
    _report([(f'masked_xattn train bf16 {_ids(shape)} {k}', v) for k, v in r.items()])


@pytest.mark.parametrize('shape', [(1, 37, 332, True), (2, 130, 200, True), (1, 100, 100, False)], ids=_ids)
def test_masked_xattn_bf16(dev, shape):
    """`ops.masked_xattn_bf16`: bf16 K and transposed V"""
    c, _, want, ref32 = _attn_case(shape, bf16=True)
    out = ops.masked_xattn_bf16(c.q.to(dev), c.k.bfloat16().to(dev), c.v.bfloat16().transpose(1, 2).contiguous().to(dev),
                                _bits(c, dev), H)
    r = SC.attention_ratios(c, dict(out=out.cpu()), want, ref32, SC.U_BF16)
    _report([(f'masked_xattn_bf16 {_ids(shape)} out', r['out'])])


# ------------------------------------------------------------------------------------------------
# B. window attention
# ------------------------------------------------------------------------------------------------
WINDOW_CASES = [(7, (14, 21), 0), (7, (14, 21), 3), (12, (24, 36), 6)]
W_HEADS = 2


def _window_case(ws, hw, shift, table_large):
    """qkv of softmax_cases.window_qkv on the token geometry of test_window_attn_gpu._coords, a randn table (N(0, 20^2) for the
    family `table_large`), dense_ref with its autograd in float64 and f32, and softmax_cases.window_scales (A, S_rows)."""
    def make():
        B, L, C = 2, hw[0] * hw[1], W_HEADS * 32
        win, reg, ly, lx = _coords(hw[0], hw[1], ws, shift)
        qkv, fams, fam = SC.window_qkv(B, W_HEADS, win, reg, ly * ws + lx, ws * ws, seed=100 * ws + shift, shifted=shift > 0,
                                       table_large=table_large)
        g = torch.Generator().manual_seed(ws + shift)
        table = torch.randn((2 * ws - 1) ** 2, W_HEADS, generator=g) * (SC.TABLE_LARGE if table_large else 1.0)
        go = torch.randn(B, L, C, generator=g)

        def run(dt):
            qd, td = qkv.to(dt).requires_grad_(), table.to(dt).requires_grad_()
            out, lse = dense_ref(qd, td, hw, ws, shift, W_HEADS)
            gq, gt = torch.autograd.grad(out, (qd, td), go.to(dt))
            return dict(out=out.detach(), lse=lse.detach(), grad_qkv=gq, grad_table=gt)
        A, (S_k, S_v, S_t) = SC.window_scales(qkv, table, go, win, reg, ly, lx, ws, W_HEADS)
        if shift > 0 and not table_large:                                     # beats_the_mask is what it claims
            logits = SC.window_logits(qkv.double(), table.double(), win, reg, ly, lx, ws, W_HEADS)[0]
            rows = (fam == fams.index('beats_the_mask'))[:, None, :, None] & SC._multi_region(win, reg)[None, None, :, None]
            other = (reg[:, None] != reg[None, :])[None, None]
            best_other = logits.masked_fill(~other, float('-inf')).amax(-1, keepdim=True)
            best_same = logits.masked_fill(other, float('-inf')).amax(-1, keepdim=True)
            assert bool(rows.any()) and bool(((best_other - best_same > 30.0) | ~rows).all())      # it wins after the -100
        return dict(qkv=qkv, table=table, go=go, fams=fams, fam=fam, A=A, S_rows=(S_k, S_v, S_t), want=run(torch.float64),
                    ref32=run(torch.float32))
    return _cached(('window', ws, hw, shift, table_large), make)


@pytest.mark.parametrize('table_large', [False, True], ids=['table_unit', 'table_large'])
@pytest.mark.parametrize('ws,hw,shift', WINDOW_CASES)
def test_window_attention(dev, ws, hw, shift, table_large):
    """`ops.window_attention` / `window_attention_backward` (fed the forward's own lse) against the dense float64 formulation of
    tests/test_window_attn_gpu.py: out, lse and the q-part of grad_qkv per family; its k-part, its v-part and grad_table globally.
    In a shifted case the -100 between regions comes on top of the family's scores, and the rows of `beats_the_mask` put 150 on a
    key of another region, which therefore still wins: the kernel has to follow the reference, not treat -100 as blocked."""
    k = _window_case(ws, hw, shift, table_large)
    qkv, table, fams, fam, A = k['qkv'].to(dev), k['table'].to(dev), k['fams'], k['fam'], k['A']
    B, L, C = 2, hw[0] * hw[1], W_HEADS * 32
    out, lse = ops.window_attention(qkv, table, hw, ws, shift, W_HEADS, return_lse=True)
    gqkv, gtab = ops.window_attention_backward(qkv, table, lse, k['go'].to(dev), hw, ws, shift, W_HEADS)
    out, lse, gqkv, gtab = out.cpu(), lse.cpu(), gqkv.cpu(), gtab.cpu()
    w, r = k['want'], k['ref32']
    fam_rows, fam_lse = fam[:, :, None].expand(B, L, C), fam[:, None, :].expand(B, W_HEADS, L)
    tag = f'window_attention ws={ws} hw={hw} shift={shift}'
    part = lambda t, i: t[..., i * C:(i + 1) * C]                             # noqa: E731
    _report([(f'{tag} out', SC.ratios('out', out, w['out'], r['out'], fam_rows, fams, None, SC.U_F32)),
             (f'{tag} lse', SC.ratios('lse', lse, w['lse'], r['lse'], fam_lse, fams, A, SC.U_F32)),
             (f'{tag} grad_q', SC.ratios('grad_rows', part(gqkv, 0), part(w['grad_qkv'], 0), part(r['grad_qkv'], 0), fam_rows, fams,
                                         (A, fam_lse), SC.U_F32)),
             (f'{tag} grad_k', SC.ratios('grad_sum', part(gqkv, 1), part(w['grad_qkv'], 1), part(r['grad_qkv'], 1), None, fams, A,
                                         SC.U_F32, S_rows=k['S_rows'][0])),
             (f'{tag} grad_v', SC.ratios('grad_sum', part(gqkv, 2), part(w['grad_qkv'], 2), part(r['grad_qkv'], 2), None, fams, A,
                                         SC.U_F32, S_rows=k['S_rows'][1])),
             (f'{tag} grad_table', SC.ratios('grad_sum', gtab, w['grad_table'], r['grad_table'], None, fams, A, SC.U_F32,
                                             S_rows=k['S_rows'][2]))])


# ------------------------------------------------------------------------------------------------
# C. row kernels on given logits
# ------------------------------------------------------------------------------------------------
CE_PAD = 8                # columns of -1e30 behind the vocabulary, as `generator_ce_rows` pads it
IGNORE = -100


def _ce_case(N, bf16):
    """40 rows: family r % 10, target placement (r // 10) % 4 -- on the row maximum, on the row minimum, in the last column of
    the vocabulary, ignored; N >= 1000 ends in CE_PAD columns of -1e30"""
    def make():
        pad = CE_PAD if N >= 1000 else 0
        M = 4 * len(SC.families(False))
        lg = SC.logit_rows(M, N - pad, seed=N + bf16, bf16=bf16)
        x = torch.cat([lg.x, torch.full((M, pad), -1e30)], 1)
        if bf16:
            x = x.bfloat16().float()
        real = lg.x.double()
        place = (torch.arange(M) // len(lg.fams)) % 4
        target = torch.where(place == 0, real.argmax(1), torch.where(place == 1, real.argmin(1), torch.full((M,), N - pad - 1)))
        target = torch.where(place == 3, torch.full((M,), IGNORE), target)
        g = torch.randn(M, generator=torch.Generator().manual_seed(N))

        def run(dt):
            xs = x.to(dt).requires_grad_()
            loss = F.cross_entropy(xs, target, ignore_index=IGNORE, reduction='none')
            grad, = torch.autograd.grad(loss, xs, g.to(dt))
            return loss.detach(), xs.detach().logsumexp(1), grad
        return dict(lg=lg, x=x, target=target, g=g, want=run(torch.float64), ref32=run(torch.float32))
    return _cached(('ce', N, bf16), make)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('N', [8, 1000, 1032, 4104])
def test_ce_rows(dev, N, bf16):
    """`ops.ce_rows_forward` / `ce_rows_backward_`: a thread with nothing to read (8), the idle-lane combine (1000), a second pass by
    a few threads (1032), several passes (4104). loss and lse against F.cross_entropy / logsumexp, the in-place gradient (fed the
    kernel's own lse) against autograd; a bf16 gradient adds one bf16 rounding of `want`."""
    k = _ce_case(N, bf16)
    lg, tag = k['lg'], f'ce_rows N={N} {"bf16" if bf16 else "f32"}'
    x = k['x'].to(dev).bfloat16() if bf16 else k['x'].to(dev)
    assert torch.equal(x.float().cpu(), k['x'])
    loss, lse = ops.ce_rows_forward(x, k['target'].to(dev), IGNORE)
    (wl, wlse, wg), (rl, rlse, rg) = k['want'], k['ref32']
    res = [(f'{tag} loss', SC.ratios('lse', loss.cpu(), wl, rl, lg.fam, lg.fams, lg.A, SC.U_F32)),
           (f'{tag} lse', SC.ratios('lse', lse.cpu(), wlse, rlse, lg.fam, lg.fams, lg.A, SC.U_F32))]
    assert bool((loss.cpu()[k['target'] == IGNORE] == 0).all())
    grad = ops.ce_rows_backward_(x.clone(), k['target'].to(dev), lse, k['g'].to(dev), IGNORE)
    fam2 = lg.fam[:, None].expand(-1, N)
    res.append((f'{tag} grad', SC.ratios('grad_rows', grad.float().cpu(), wg, rg, fam2, lg.fams, (lg.A, lg.fam), SC.U_F32,
                                         extra=_bf16_rounding(wg) if bf16 else None)))
    _report(res)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_ce_rows_minus_inf_columns(dev, bf16):
    """rows of N = 2056 whose first vector (4 f32 / 8 bf16 columns) is all -inf, read by a thread that has a second pass: the row's
    lse and loss are torch's finite values (the kernel once kept exp(-inf - -inf) = NaN through the second pass)"""
    N, V = 2056, 8 if bf16 else 4
    lg = SC.logit_rows(len(SC.families(False)), N, seed=7, bf16=bf16)
    x = lg.x.clone()
    x[:, :V] = float('-inf')
    target = torch.full((x.shape[0],), N - 1)
    want = F.cross_entropy(x.double(), target, reduction='none')
    ref32 = F.cross_entropy(x, target, reduction='none')
    assert torch.isfinite(want).all()
    A = x[:, V:].double().abs().amax(1)
    xd = x.to(dev).bfloat16() if bf16 else x.to(dev)
    loss, lse = ops.ce_rows_forward(xd, target.to(dev), IGNORE)
    _report([('ce_rows -inf loss', SC.ratios('lse', loss.cpu(), want, ref32, lg.fam, lg.fams, A, SC.U_F32)),
             ('ce_rows -inf lse', SC.ratios('lse', lse.cpu(), x.double().logsumexp(1), x.logsumexp(1), lg.fam, lg.fams, A, SC.U_F32))])


def _softmax_case(n, M=20):
    def make():
        lg = SC.logit_rows(M, n, seed=n)
        return lg, lg.x.double().softmax(1), lg.x.softmax(1)
    return _cached(('softmax', n, M), make)


@pytest.mark.parametrize('n', [134, 1000])
def test_rowwise_softmax_argmax(dev, n):
    """`ops.rowwise_softmax_argmax`: probabilities and the maximum by the bound, the index exactly (no row but `tie` has two equal
    maxima; there the first index is the answer)"""
    lg, want, ref32 = _softmax_case(n)
    prob, maxv, arg = ops.rowwise_softmax_argmax(lg.x.to(dev))
    fam2 = lg.fam[:, None].expand(-1, n)
    _report([(f'rowwise_softmax_argmax n={n} prob', SC.ratios('out', prob.cpu(), want, ref32, fam2, lg.fams, None, SC.U_F32)),
             (f'rowwise_softmax_argmax n={n} max', SC.ratios('out', maxv.cpu(), want.amax(1), ref32.amax(1), lg.fam, lg.fams, None,
                                                             SC.U_F32))])
    x64 = lg.x.double()
    first = (x64 == x64.amax(1, keepdim=True)).int().argmax(1)                  # first index of the row maximum
    tie = lg.fam == lg.fams.index('tie')
    assert bool(((x64 == x64.amax(1, keepdim=True)).sum(1) == torch.where(tie, 2, 1)).all())
    assert torch.equal(arg.cpu(), first) and bool((first[tie] == SC.tie_keys(n)[0]).all())


@pytest.mark.parametrize('n', [134, 1000])
def test_class_topk(dev, n):
    """`ops.class_topk` over one table of n columns (the last is background): the k best (query, class) pairs of
    softmax(dots)[:, :-1]. Scores by the `out` bound of the row's family; indices exactly wherever the float64 probabilities of
    neighbours in the order differ by more than both their bounds, or are equal because their logits are (the `tie` rows)."""
    Q, k = 10, 64
    lg, want, ref32 = _softmax_case(n, M=Q)
    assert ops.class_topk_supported(Q, [n], k)
    labels, scores, qidx = (t.cpu()[0, 0] for t in ops.class_topk(lg.x.to(dev), 1, [0], [n], k))
    fam2 = lg.fam[:, None].expand(-1, n)
    base = torch.tensor(SC.family_bounds('out', want, ref32, fam2, lg.fams, None, SC.U_F32), dtype=torch.float64)
    p, bound = want[:, :-1].reshape(-1), base[lg.fam][:, None].expand(-1, n - 1).reshape(-1)
    order = p.sort(descending=True, stable=True).indices[:k + 1]
    got = qidx * (n - 1) + labels
    err = (scores.double() - p[got]).abs() / bound[got]
    print(f'class_topk n={n}: worst score error / bound {err.max().item():.3g}')
    assert bool((err <= 1.0).all()), err
    pw = p[order]
    gap = pw[:-1] - pw[1:]
    x = lg.x[:, :-1].reshape(-1)[order]
    exact_tie = (gap == 0) & (x[:-1] == x[1:]) & (order[:-1] // (n - 1) == order[1:] // (n - 1))
    clear = (gap > bound[order][:-1] + bound[order][1:]) | exact_tie
    sure = torch.cat([torch.ones(1, dtype=torch.bool), clear[:-1]]) & clear                    # clear on both sides
    assert int(sure.sum()) >= k // 2 and bool(exact_tie.any())
    assert torch.equal(got[sure], order[:k][sure]), (got.tolist(), order[:k].tolist())
    assert sorted(got.tolist()) == sorted(order[:k].tolist()) or not bool(clear.all())


# ------------------------------------------------------------------------------------------------
# grounding pair costs
# ------------------------------------------------------------------------------------------------
GROUNDING_FAMS = ('large', 'shift_pos')
TEMPERATURE = 10.0


def _grounding_case(shape):
    """image 0: sim / temperature ~ N(0, 6^2); image 1: ~ N(100, 1). Caption 0 has a token whose score with query 5 of either image
    is 40 higher; caption 1 has no nouns. Channel 0 / 1 of the embeddings carry the offset / the spike, the others are randn."""
    def make():
        B, Q, T, d = shape
        g = torch.Generator().manual_seed(Q + T)
        cap = torch.randn(B, T, d, generator=g)
        pred = torch.randn(B, Q, d, generator=g) * TEMPERATURE / (d - 2) ** 0.5
        pred[0] *= SC.LARGE
        cap[..., :2], pred[..., :2] = 0.0, 0.0
        cap[..., 0] = 1.0
        pred[1, :, 0] = SC.SHIFT * TEMPERATURE
        cap[0, 2, 1] = 1.0
        pred[:, 5, 1] = SC.SPIKE * TEMPERATURE
        ntok = torch.tensor([min(T, 7), 0])
        mask = (torch.arange(T)[None] < ntok[:, None]).long()
        gcost = torch.randn(2, B, B, generator=g)

        def run(dt):
            raw = torch.einsum('itd,jqd->ijtq', cap.to(dt), pred.to(dt)).requires_grad_()
            sim = raw / TEMPERATURE
            l2v = ((sim.softmax(3) * mask[:, None, :, None]) * -sim).sum((2, 3)) / ntok.clamp(min=1)[:, None]
            v2l = (sim.softmax(2) * -sim).sum((2, 3)) / Q
            cost = torch.stack([l2v, v2l])
            draw, = torch.autograd.grad(cost, raw, gcost.to(dt))
            return cost.detach(), draw.permute(1, 0, 2, 3).reshape(B, B * T, Q)
        A = torch.einsum('itd,jqd->ijtq', cap.double().abs(), pred.double().abs()).amax((2, 3)) / TEMPERATURE      # (Bc, Bp)
        return dict(cap=cap, pred=pred, mask=mask, gcost=gcost, want=run(torch.float64), ref32=run(torch.float32), A=A)
    return _cached(('grounding', shape), make)


@pytest.mark.parametrize('shape', [(2, 100, 35, 64), (2, 129, 33, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_grounding_pair_costs(dev, shape):
    """`ops.grounding_pair_costs` / `_backward` against float64 of the formulation in test_grounding_loss_kernel_vs_oracle; the
    family of a cost or a dsim entry is its image's"""
    B, Q, T, d = shape
    k = _grounding_case(shape)
    pred, cap, mask = k['pred'].to(dev), k['cap'].to(dev), k['mask'].to(torch.int32).to(dev)
    cost = ops.grounding_pair_costs(pred, cap, mask, 1.0 / TEMPERATURE).cpu()
    dsim = ops.grounding_pair_costs_backward(pred, cap, mask, k['gcost'].to(dev), 1.0 / TEMPERATURE).cpu()
    (wc, wd), (rc, rd) = k['want'], k['ref32']
    fam_c = torch.arange(B)[None, None, :].expand(2, B, B)
    fam_d = torch.arange(B)[:, None, None].expand(B, B * T, Q)
    A_c = k['A'][None].expand(2, B, B)
    _report([(f'grounding {shape} cost', SC.ratios('lse', cost, wc, rc, fam_c, GROUNDING_FAMS, A_c, SC.U_F32)),
             (f'grounding {shape} dsim', SC.ratios('grad_rows', dsim, wd, rd, fam_d, GROUNDING_FAMS, (k['A'], fam_c[0]), SC.U_F32))])


# ------------------------------------------------------------------------------------------------
# MSDeformAttn prologue softmax
# ------------------------------------------------------------------------------------------------
MSDA_FAMS = ('shift_pos', 'shift_neg', 'spike', 'flat')
MSDA_SHAPES = [(5, 7), (10, 14), (20, 28)]


def _msda_case():
    """the L P = 12 attention logits of (query, head) row r are of family r % 4: N(+-100, 1), N(0, 1) with one +40, all 50"""
    def make():
        B, Hm, D, L, P = 2, 8, 32, 3, 4
        starts, Nv = [], 0
        for h, w in MSDA_SHAPES:
            starts.append(Nv)
            Nv += h * w
        g = torch.Generator().manual_seed(5)
        value = torch.randn(B, Nv, Hm, D, generator=g)
        n_off = Hm * L * P * 2
        offs = 2.0 * torch.randn(B, Nv, n_off, generator=g)
        logit = torch.randn(B * Nv * Hm, L * P, generator=g)
        fam = torch.arange(B * Nv * Hm) % 4
        logit[fam == 0] += SC.SHIFT
        logit[fam == 1] -= SC.SHIFT
        spike = logit[fam == 2]
        spike[torch.arange(spike.shape[0]), torch.arange(spike.shape[0]) % (L * P)] += SC.SPIKE
        logit[fam == 2] = spike
        logit[fam == 3] = 50.0
        raw = torch.cat([offs, logit.view(B, Nv, Hm * L * P)], -1).contiguous()
        refp = torch.rand(Nv, 2, generator=g)
        go = torch.randn(B, Nv, Hm * D, generator=g)
        norm = torch.tensor([[w, h] for h, w in MSDA_SHAPES], dtype=torch.float32)

        def run(dt):
            v, r = value.to(dt).requires_grad_(), raw.to(dt).requires_grad_()
            off = r[..., :n_off].view(B, Nv, Hm, L, P, 2)
            aw = r[..., n_off:].view(B, Nv, Hm, L * P).softmax(-1).view(B, Nv, Hm, L, P)
            loc = refp.to(dt)[None, :, None, None, None, :] + off / norm.to(dt)[None, None, None, :, None, :]
            out = ref.msda_core(v, torch.tensor(MSDA_SHAPES), loc, aw)
            gv, gr = torch.autograd.grad(out, (v, r), go.to(dt))
            return out.detach(), gv, gr[..., n_off:]
        fam = fam.view(B, Nv, Hm)
        A = raw[..., n_off:].view(B, Nv, Hm, L * P).double().abs().amax(-1)
        return dict(value=value, raw=raw, refp=refp, go=go, starts=starts, P=P, n_off=n_off, fam=fam, A=A, D=D, LP=L * P,
                    want=run(torch.float64), ref32=run(torch.float32))
    return _cached('msda', make)


def test_msda_prologue_softmax(dev):
    """`ops.msda_forward_fused` and `ops.msda_rows_backward` on the ragged pyramid: out per family, grad_value globally, the logit
    part of grad_rows per family"""
    k = _msda_case()
    value, raw, refp = k['value'].to(dev), k['raw'].to(dev), k['refp'].to(dev)
    out = ops.msda_forward_fused(value, MSDA_SHAPES, k['starts'], raw, refp, k['P']).cpu()
    gv, grows = ops.msda_rows_backward(value, raw, refp, MSDA_SHAPES, k['starts'], k['P'], k['go'].to(dev))
    (wo, wv, wr), (ro, rv, rr) = k['want'], k['ref32']
    fam, A = k['fam'], k['A']
    ex = lambda n: fam[..., None].expand(*fam.shape, n).reshape(fam.shape[0], fam.shape[1], -1)           # noqa: E731
    _report([('msda_forward_fused out', SC.ratios('out', out, wo, ro, ex(k['D']), MSDA_FAMS, None, SC.U_F32)),
             ('msda_rows_backward grad_value', SC.ratios('grad_sum', gv.cpu(), wv, rv, None, MSDA_FAMS, A, SC.U_F32)),
             ('msda_rows_backward grad_logits', SC.ratios('grad_rows', grows[..., k['n_off']:].cpu(), wr, rr, ex(k['LP']), MSDA_FAMS,
                                                         (A, fam), SC.U_F32))])
