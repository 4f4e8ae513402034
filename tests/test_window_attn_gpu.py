"""GPU tests of the fused (shifted-)window attention (csrc/window_attn.hip -> ops.window_attention / WindowAttentionFn ->
swin.ShiftWindowMSA). The float64 reference is the DENSE formulation of oracle/swin.py (`_WMSA`: per-pair window membership after
the cyclic shift, three-slice region labels, coordinate-difference bias lookup over all tokens of the padded map) -- no roll, no
window partition, no index buffer -- so it shares nothing with the addressing under test."""
import os
import subprocess
import sys

import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops, registry, runtime, swin
from oracle.swin import OracleSwin, _WMSA
from util import randomize

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coords(Hp, Wp, ws, s):
    """per token of the padded map (row-major): window id, region label, in-window (y, x) -- after the cyclic shift by -s"""
    ys, xs = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing='ij')
    ysh, xsh = (ys.flatten() - s) % Hp, (xs.flatten() - s) % Wp
    win = (ysh // ws) * (Wp // ws) + xsh // ws

    def region(c, n):
        return torch.where(c < n - ws, 0, torch.where(c < n - s, 1, 2)) if s > 0 else torch.zeros_like(c)
    return win, region(ysh, Hp) * 3 + region(xsh, Wp), ysh % ws, xsh % ws


def dense_ref(qkv, table, hw, ws, s, heads, scale=None):
    """oracle/swin.py `_WMSA.forward` between its qkv and proj linears, on given qkv rows: (out (B, L, C), lse (B, heads, L))"""
    Hp, Wp = hw
    B, L, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    win, reg, ly, lx = _coords(Hp, Wp, ws, s)
    same_win = win[:, None] == win[None, :]
    ridx = (ly[:, None] - ly[None, :] + ws - 1) * (2 * ws - 1) + (lx[:, None] - lx[None, :] + ws - 1)
    ridx = torch.where(same_win, ridx, torch.zeros_like(ridx))
    bias = table[ridx.flatten()].view(L, L, heads).permute(2, 0, 1)
    add = torch.where(reg[:, None] != reg[None, :], -100.0, 0.0).to(qkv.dtype)
    q, k, v = (qkv.view(B, L, 3, heads, D)[:, :, i].transpose(1, 2) for i in range(3))
    logits = (q * (D ** -0.5 if scale is None else scale)) @ k.transpose(-2, -1) + bias[None] + add[None, None]
    logits = logits.masked_fill(~same_win[None, None], float('-inf'))
    out = (logits.softmax(-1) @ v).transpose(1, 2).reshape(B, L, C)
    return out, torch.logsumexp(logits, -1)


CASES = [(ws, hw, shift, heads) for ws, hw in ((7, (14, 21)), (12, (24, 36))) for shift in (0, ws // 2) for heads in (2, 4)]


@pytest.mark.parametrize('ws,hw,shift,heads', CASES)
def test_window_attention_forward_backward_vs_float64_dense(dev, ws, hw, shift, heads):
    """Op forward (out, lse within 1e-4 absolute) and backward (grad_qkv, grad_table within 2e-5 max|ref| + 1e-6) against float64
    autograd of the dense formulation; several windows in both directions, Hp != Wp, B = 2. The backward is bit-reproducible and,
    being exact f32 products, linear in grad_out to the last bit for a power-of-two factor."""
    check_window_attention(dev, ws, hw, shift, heads)


def check_window_attention(dev, ws, hw, shift, heads):
    g = torch.Generator().manual_seed(1000 * ws + 10 * shift + heads)
    B, L, C = 2, hw[0] * hw[1], heads * 32
    qkv = torch.randn(B, L, 3 * C, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    go = torch.randn(B, L, C, generator=g)
    qd, td = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    want, want_lse = dense_ref(qd, td, hw, ws, shift, heads)
    wgq, wgt = torch.autograd.grad(want, (qd, td), go.double())
    out, lse = ops.window_attention(qkv.to(dev), table.to(dev), hw, ws, shift, heads, return_lse=True)
    e_out = (out.cpu().double() - want.detach()).abs().max().item()
    e_lse = (lse.cpu().double() - want_lse.detach()).abs().max().item()
    print(f'window_attn fwd ws={ws} hw={hw} shift={shift} heads={heads}: |out - f64| = {e_out:.3e}, |lse - f64| = {e_lse:.3e}')
    assert e_out <= 1e-4 and e_lse <= 1e-4, (e_out, e_lse)
    assert torch.equal(out, ops.window_attention(qkv.to(dev), table.to(dev), hw, ws, shift, heads))
    gq, gt = ops.window_attention_backward(qkv.to(dev), table.to(dev), lse, go.to(dev), hw, ws, shift, heads)
    gq3, gt3 = ops.window_attention_backward(qkv.to(dev), table.to(dev), lse, (go * 2.0 ** -20).to(dev), hw, ws, shift, heads)
    for got, got3, ref_, name in ((gq, gq3, wgq, 'grad_qkv'), (gt, gt3, wgt, 'grad_table')):
        scale = ref_.abs().max().item()
        err = (got.cpu().double() - ref_).abs().max().item()
        err3 = (got3.cpu().double() * 2.0 ** 20 - ref_).abs().max().item()
        print(f'window_attn bwd ws={ws} hw={hw} shift={shift} heads={heads}: {name} err = {err:.3e} (2^-20 grad_out: {err3:.3e}) '
              f'of max|ref| = {scale:.3e}')
        assert err <= 2e-5 * scale + 1e-6, (name, err, scale)
        assert err3 <= 2e-5 * scale + 1e-6, (name, err3, scale)
    # run to run bit-identical (no floating-point atomics)
    gq2, gt2 = ops.window_attention_backward(qkv.to(dev), table.to(dev), lse, go.to(dev), hw, ws, shift, heads)
    assert torch.equal(gq, gq2) and torch.equal(gt, gt2)
    assert torch.equal(gq3 * 2.0 ** 20, gq) and torch.equal(gt3 * 2.0 ** 20, gt)


@pytest.mark.parametrize('ws,hw', [(7, (14, 21)), (12, (24, 36))])
@pytest.mark.parametrize('shifted', [False, True])
def test_zero_scores_give_group_means_of_v(dev, ws, hw, shifted):
    """Zero q / k and a zero table: every token's output is the mean of v over its window (shift 0) or over its window-and-region
    group (shifted: the other tokens of the window keep weight e^-100 each)."""
    g = torch.Generator().manual_seed(ws)
    heads, B, L = 2, 2, hw[0] * hw[1]
    C = heads * 32
    s = ws // 2 if shifted else 0
    qkv = torch.zeros(B, L, 3 * C)
    qkv[..., 2 * C:] = torch.randn(B, L, C, generator=g)
    out = ops.window_attention(qkv.to(dev), torch.zeros((2 * ws - 1) ** 2, heads, device=dev), hw, ws, s, heads).cpu()
    win, reg, _, _ = _coords(hw[0], hw[1], ws, s)
    group = win * 9 + reg
    want = torch.zeros(B, L, C, dtype=torch.float64)
    for gid in group.unique():
        sel = group == gid
        want[:, sel] = qkv[:, sel, 2 * C:].double().mean(1, keepdim=True)
    assert int(group.unique().numel()) > (hw[0] // ws) * (hw[1] // ws) or not shifted
    assert (out.double() - want).abs().max().item() <= 1e-5


@pytest.mark.parametrize('ws,hw', [(7, (14, 21)), (12, (24, 36))])
def test_asymmetric_table_recovers_softmax_of_bias_rows(dev, ws, hw):
    """Zero q / k, table value = 0.01 x row index (x (head + 1)) and one-hot v over the in-window position: the output rows ARE
    softmax(bias) rows, so a transposed (i, j) lookup or swapped dy / dx fails."""
    heads, B, L, N = 2, 1, hw[0] * hw[1], ws * ws
    C, T1 = heads * 32, 2 * ws - 1
    table = 0.01 * torch.arange(T1 * T1, dtype=torch.float32)[:, None] * torch.arange(1, heads + 1, dtype=torch.float32)[None]
    _, _, ly, lx = _coords(hw[0], hw[1], ws, 0)
    local = ly * ws + lx                                            # in-window position of every token
    yi, xi = torch.arange(N) // ws, torch.arange(N) % ws
    ridx = (yi[:, None] - yi[None, :] + ws - 1) * T1 + (xi[:, None] - xi[None, :] + ws - 1)
    probs = table.double()[ridx.flatten()].view(N, N, heads).softmax(1)           # [i, j, head]
    for blk in range((N + 31) // 32):
        qkv = torch.zeros(B, L, 3 * C)
        d = local - 32 * blk
        hit = (d >= 0) & (d < 32)
        for h in range(heads):
            qkv[0, hit, 2 * C + 32 * h + d[hit]] = 1.0
        out = ops.window_attention(qkv.to(dev), table.to(dev), hw, ws, 0, heads).cpu().double()
        n = min(32, N - 32 * blk)
        for h in range(heads):
            want = probs[local, 32 * blk:32 * blk + n, h]                             # (L, n)
            assert (out[0, :, 32 * h:32 * h + n] - want).abs().max().item() <= 1e-5, (blk, h)


@pytest.mark.parametrize('ws,hw', [(7, (14, 21)), (12, (24, 36))])
def test_rolling_the_map_by_one_window_permutes_the_output(dev, ws, hw):
    g = torch.Generator().manual_seed(5)
    heads, B = 2, 2
    C = heads * 32
    qkv = torch.randn(B, hw[0], hw[1], 3 * C, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).to(dev)
    a = ops.window_attention(qkv.view(B, -1, 3 * C).to(dev), table, hw, ws, 0, heads)
    b = ops.window_attention(qkv.roll(ws, dims=2).reshape(B, -1, 3 * C).to(dev), table, hw, ws, 0, heads)
    assert torch.equal(a.view(B, hw[0], hw[1], C).roll(ws, dims=2), b.view(B, hw[0], hw[1], C))


def test_window_attention_argument_checks(dev):
    qkv = torch.randn(1, 24 * 24, 3 * 64, device=dev)
    table = torch.randn(23 * 23, 2, device=dev)
    assert ops.window_attention_ok(qkv, 12, 2, (24, 24), 6)
    assert not ops.window_attention_ok(qkv.half(), 12, 2, (24, 24), 6)
    assert not ops.window_attention_ok(qkv[:, ::2], 12, 2)
    for bad in (dict(hw=(24, 25)), dict(num_heads=4), dict(ws=7), dict(shift=12), dict(qkv=qkv.half()), dict(qkv=qkv[:, :, :96]),
                dict(qkv=qkv.transpose(0, 1)), dict(table=table.double()), dict(table=table.cpu())):
        kw = dict(qkv=qkv, table=table, hw=(24, 24), ws=12, shift=0, num_heads=2)
        kw.update(bad)
        with pytest.raises(ops.CggError):
            ops.window_attention(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
def _count_native(monkeypatch):
    calls = []
    real = ops.window_attention

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, 'window_attention', counted)
    return calls


def _param_grads(loss, module):
    names, params = zip(*sorted(module.named_parameters()))
    return dict(zip(names, torch.autograd.grad(loss, params)))


def _compare_grads(what, ref, native, existing):
    """per parameter: err_native <= max(2 err_existing, 2e-5 max|ref|) + 1e-6 (both paths sum the same terms in another order)"""
    assert sorted(ref) == sorted(native) == sorted(existing)
    bad = []
    for n in sorted(ref):
        scale = ref[n].abs().max().item()
        en = (native[n].cpu().double() - ref[n]).abs().max().item()
        ee = (existing[n].cpu().double() - ref[n]).abs().max().item()
        if n.endswith(('relative_position_bias_table', 'qkv.bias', 'qkv.weight', 'proj.weight', 'proj.bias')) or '.' not in n:
            print(f'{what} grad {n}: max|ref| = {scale:.3e}  err native = {en:.3e}  err existing = {ee:.3e}')
        if not en <= max(2 * ee, 2e-5 * scale) + 1e-6:
            bad.append((n, en, ee, scale))
    assert not bad, bad


def _stage_case():
    """`ShiftWindowMSA(64, 2, 12, shift 6)` on a 30 x 41 map (-> 36 x 48), B = 2: module, its float64 oracle, input, loss weights"""
    g = torch.Generator().manual_seed(77)
    m = swin.ShiftWindowMSA(64, 2, 12, 6)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.125 if p.dim() > 1 and p.shape[-1] == 64 else 1.0))
    orc = _WMSA(64, 2, 12, 6).double()
    missing, unexpected = orc.load_state_dict(m.state_dict(), strict=False)
    assert not missing and unexpected == ['w_msa.relative_position_index']
    x = torch.randn(2, 30 * 41, 64, generator=g)
    w = torch.randn(2, 30 * 41, 64, generator=g)
    return m, orc, x, w, (30, 41)


def _feature_bound(want):
    return 2e-4 * max(1.0, want.abs().max().item())


def test_shift_window_msa_ws12_stage_vs_float64_oracle(dev, monkeypatch):
    m, orc, x, w, hw = _stage_case()
    xd = x.double().requires_grad_(True)
    want = orc(xd, hw)
    ref = _param_grads((want * w.double()).sum(), orc)
    ref['input'] = torch.autograd.grad((orc(xd, hw) * w.double()).sum(), xd)[0]
    m = m.to(dev)
    got = {}
    calls = _count_native(monkeypatch)
    for path, flag in (('native', True), ('existing', False)):
        monkeypatch.setattr(swin, 'WINATTN', flag)
        xg = x.to(dev).requires_grad_(True)
        with runtime.precision_scope('fp32'):
            f = m(xg, hw)
            grads = _param_grads((f * w.to(dev)).sum(), m)
            grads['input'] = torch.autograd.grad((m(xg, hw) * w.to(dev)).sum(), xg)[0]
        err = (f.detach().cpu().double() - want.detach()).abs().max().item()
        print(f'ShiftWindowMSA(64, 2, 12, 6) 30x41 features, {path}: |f - f64| = {err:.3e} (bound {_feature_bound(want):.1e})')
        assert err <= _feature_bound(want), (path, err)
        got[path] = grads
        assert len(calls) == 2, calls                             # two forwards of the fused op, in the native pass only
    _compare_grads('ShiftWindowMSA(64, 2, 12, 6) 30x41', ref, got['native'], got['existing'])


def test_swin_backbone_ws7_vs_float64_oracle(dev, monkeypatch):
    """The configuration of test_swin_product_module_equals_dense_oracle (ws 7, depths (2, 2, 2, 2), sizes that are not patch / window
    multiples) at embed_dims 64 -- its 32 gives head dim 16, which the kernels do not take -- on the device in parity mode against
    `OracleSwin` in float64: features, and the gradient of every backbone parameter after sum(f * w), native vs existing path."""
    kw = dict(embed_dims=64, depths=(2, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=7, mlp_ratio=4, out_indices=(0, 1, 2, 3),
              patch_norm=True)
    bb = registry.build_backbone(dict(type='SwinTransformer', drop_path_rate=0.1, **kw))
    randomize(bb, seed=3)
    with torch.no_grad():
        for n, p in bb.named_parameters():
            if n.endswith('relative_position_bias_table'):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))))     # O(1) biases
    bb.eval()
    orc = OracleSwin(**kw).double()
    missing, unexpected = orc.load_state_dict(bb.state_dict(), strict=False)
    assert not missing and all(k.endswith('relative_position_index') for k in unexpected), (missing, unexpected)
    orc.eval()
    bb = bb.to(dev)
    calls = _count_native(monkeypatch)
    for shape in ((1, 3, 90, 128), (2, 3, 112, 84)):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
        want = orc(x.double())
        ws_ = [torch.randn(f.shape, generator=torch.Generator().manual_seed(i)) for i, f in enumerate(want)]
        ref = _param_grads(sum((f * w.double()).sum() for f, w in zip(want, ws_)), orc)
        got = {}
        for path, flag in (('native', True), ('existing', False)):
            monkeypatch.setattr(swin, 'WINATTN', flag)
            n0 = len(calls)
            with runtime.precision_scope('fp32'):
                feats = bb(x.to(dev))
                got[path] = _param_grads(sum((f * w.to(dev)).sum() for f, w in zip(feats, ws_)), bb)
            assert len(calls) - n0 == (8 if flag else 0)            # every block of the four stages took the fused op
            for i, (a, b) in enumerate(zip(feats, want)):
                err = (a.detach().cpu().double() - b.detach()).abs().max().item()
                print(f'Swin ws 7 {shape} stage {i} features, {path}: |f - f64| = {err:.3e} (bound {_feature_bound(b):.1e})')
                assert a.shape == b.shape and err <= _feature_bound(b), (path, i, err)
        _compare_grads(f'Swin ws 7 {shape}', ref, got['native'], got['existing'])


class _SdpaReached(RuntimeError):
    pass


def test_native_path_runs_without_sdpa_at_configs3_shapes(dev, monkeypatch):
    """Parity-mode forward + backward of one shifted block per configs[3] stage (Swin-B at 1024^2: ws 12, heads 4 / 8 / 16 / 32, maps
    256 / 128 / 64 / 32 squared, padded to 264 / 132 / 72 / 36) with scaled_dot_product_attention patched to raise; throughput mode
    and attention dropout in training DO reach it."""
    def raiser(*a, **k):
        raise _SdpaReached()
    monkeypatch.setattr(torch.nn.functional, 'scaled_dot_product_attention', raiser)
    g = torch.Generator().manual_seed(9)
    for C, heads, side in ((128, 4, 256), (256, 8, 128), (512, 16, 64), (1024, 32, 32)):
        blk = swin.SwinBlock(C, heads, 4 * C, window_size=12, shift=True)
        randomize(blk, seed=C)
        blk = blk.to(dev).train()
        x = torch.randn(1, side * side, C, generator=g).to(dev).requires_grad_(True)
        with runtime.precision_scope('fp32'):
            y = blk(x, (side, side))
            y.square().mean().backward()
        t = blk.attn.w_msa.relative_position_bias_table
        for name, gr in (('input', x.grad), ('table', t.grad), ('qkv.bias', blk.attn.w_msa.qkv.bias.grad)):
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, (C, name)
    blk = swin.SwinBlock(128, 4, 512, window_size=12, shift=True).to(dev).eval()
    x = torch.randn(1, 24 * 24, 128, device=dev)
    with runtime.precision_scope('bf16'), torch.no_grad(), pytest.raises(_SdpaReached):
        with runtime.autocast():
            blk(x, (24, 24))
    drop = swin.SwinBlock(128, 4, 512, window_size=12, shift=True, attn_drop_rate=0.1).to(dev).train()
    with runtime.precision_scope('fp32'), pytest.raises(_SdpaReached):
        drop(x, (24, 24))
    drop.eval()
    with runtime.precision_scope('fp32'), torch.no_grad():
        drop(x, (24, 24))                                             # dropout inactive: the fused path again


def _child_main(path):
    """(run in a fresh process with CGG_SWIN_WINATTN=0) the ws-12 stage case on the device -> features saved to `path`"""
    assert swin.WINATTN is False
    m, _, x, _, hw = _stage_case()
    dev = torch.device('cuda:0')
    with runtime.precision_scope('fp32'), torch.no_grad():
        f = m.to(dev)(x.to(dev), hw)
    torch.save(f.cpu(), path)


def test_switch_off_in_a_child_process_reproduces_the_features(dev, tmp_path):
    m, orc, x, _, hw = _stage_case()
    with torch.no_grad():
        want = orc(x.double(), hw)
    out = str(tmp_path / 'features.pt')
    code = (f'import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]; import test_window_attn_gpu as t; '
            f't._child_main({out!r})')
    env = dict(os.environ, CGG_SWIN_WINATTN='0')
    subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, check=True, timeout=300)
    got = torch.load(out)
    err = (got.double() - want).abs().max().item()
    assert err <= _feature_bound(want), err
    assert swin.WINATTN is True                                        # this process kept the default
