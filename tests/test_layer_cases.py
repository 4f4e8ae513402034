"""The bound of tests/layer_cases.py before it meets a kernel: ROOM -- an f32 emulation of every kernel's design (layer_cases.Emu)
sits under it on the cases that tests/test_layer_edges_gpu.py runs -- and TEETH -- every seeded fault of the emulation (layer_cases.FAULTS)
exceeds it on at least one of them. CPU only, a few seconds.

Worst error / bound of the emulated designs (printed by test_room; f32-class outputs): decoder_tail 0.19 (bf16 and x3), decoder_mid
0.22, decoder_ffn 0.01 (bf16) / 0.065 (x3), linear_rows + LayerNorm 0.42 (the tight family at N = 49; 0.16 / 0.14 on random rows), layernorm_chain 0.25, encoder_ffn_ln 0.14,
encoder_layer_tail 0.009 (bf16) / 0.21 (x3, x3a). The bf16 OUTPUTS of the encoder kernels reach 0.98: `extra` is one bf16 rounding and
the rounding of a correct output uses all of it, so they are held to 1 and the others to 1 / 2.

Two things the grid needed before every fault was caught: eps_b = 1e-3 on the conditioning rows (with equal eps a swap is no fault),
and the 'round' case of `layer_cases.tail_case` -- on ordinary operands a hidden block rounded one stage late moves an output by at
most 2^-8 S, inside FACTOR 2^-9 S, so a case was built where the rounding point decides the hidden values themselves."""
import pytest
import torch

import layer_cases as LC

_OUTS = dict(tail=('y', 'yp', 'me', 'qn'), chain=('y', 'yp', 'z'), mid=('x1', 'q', 'kv'), ffn=('planes', 'sum'), linear=('y', 'yp'))


def grid():
    """(label, kernel, case) of every case: the shapes of tests/test_layer_edges_gpu.py"""
    for kind in LC.KINDS:
        for (M, pr), nsum in zip(LC.M_POS, (1, 3, 8, 8, 8)):
            yield f'tail {kind} M={M} pos={pr} nsum={nsum}', 'tail', LC.tail_case(kind, M, pr, nsum)
            yield f'mid {kind} M={M} pos={pr}', 'mid', LC.mid_case(kind, M, pr)
        yield f'tail {kind} cond', 'tail', LC.tail_case(kind, 43, 20, 3, cond=True)
        yield f'tail {kind} round', 'tail', LC.tail_case(kind, 33, 20, 3, cond='round')
        yield f'tail {kind} second', 'tail', LC.tail_case(kind, 43, 20, 3, cond='second')
        yield f'mid {kind} cond', 'mid', LC.mid_case(kind, 43, 20, cond=True)
        for M, Fw in ((1, 256), (33, 768), (77, 2048), (32, 4096)):
            yield f'ffn {kind} M={M} F={Fw}', 'ffn', LC.ffn_case(kind, M, Fw)
        for N in (32, 49, 256):
            for K in (16, 256):
                yield f'linear {kind} N={N} K={K}', 'linear', LC.linear_ln_case(kind, 77, N, K, 20)
            yield f'linear {kind} N={N} cond', 'linear', LC.linear_ln_case(kind, 43, N, 256, 20, cond=True)
    for kind, variant in LC.ENC_KERNELS:
        for M, FF, pr in zip(LC.ENC_M, (256, 512, 1024, 256, 512), (1, 50, 1, 50, 50)):
            yield f'enc {variant} {kind} M={M} FF={FF} pos={pr}', 'enc', LC.enc_case(kind, variant, M, FF, pr)
        yield f'enc {variant} {kind} cond', 'enc', LC.enc_case(kind, variant, 43, 512, 50, cond=True)
        if variant == 'tail':
            yield f'enc {variant} {kind} second', 'enc', LC.enc_case(kind, variant, 43, 512, 50, cond='second')
        if kind == 'bf16':
            yield f'enc {variant} {kind} kv', 'enc', LC.enc_case(kind, variant, 196, 512, 98, levels=LC.ENC_LEVELS)
    for (M, pr), nsum in zip(LC.M_POS, (1, 3, 8, 9, 16)):
        yield f'chain M={M} pos={pr} nsum={nsum}', 'chain', LC.tail_case('f32', M, pr, nsum)
    yield 'chain cond', 'chain', LC.tail_case('f32', 43, 20, 9, cond=True)
    yield 'chain second', 'chain', LC.tail_case('f32', 43, 20, 3, cond='second')


def emulated(kernel, case, fault=None):
    r = case.chain(LC.Emu(case.kind, fault), case.o)
    if kernel != 'enc':
        return LC.all_ratios(case, {k: r[k] for k in _OUTS[kernel]})
    if not case.b16:
        return LC.all_ratios(case, LC.enc_outs(case, r['y'], None, r['yp']))
    b = {k: LC.rb(r[k]) if k in r else None for k in ('y', 'yp', 'm', 'mp')}         # the bf16 outputs: roundings of the f32 ones
    return LC.all_ratios(case, LC.enc_outs(case, r['y'], b['y'], b['yp'], b['m'], b['mp']))


def test_room():
    worst = {}
    for label, kernel, case in grid():
        r = emulated(kernel, case)
        print(f'{label}: ' + '  '.join(f'{k}={v:.3g}' for k, v in r.items()))
        for k, v in r.items():
            # a bf16 output spends up to the whole of `extra` on its own rounding: it is held to 1, the f32-class outputs to 1 / 2
            key = f'{kernel} {label.split()[1] if kernel == "enc" else ""} {case.kind} {"bf16 out" if k.endswith("16") else "f32 out"}'
            worst[key] = max(worst.get(key, 0.0), v)
    print('worst error / bound of the emulated designs:', {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= (1.0 if k.endswith('bf16 out') else 0.5) for k, v in worst.items()), worst


@pytest.mark.parametrize('fault', LC.FAULTS)
def test_teeth(fault):
    caught = {}
    worst = 0.0
    for label, kernel, case in grid():
        if fault.startswith('x3_') and case.kind != 'x3' or fault == 'hidden_rounded_late' and case.kind != 'bf16':
            continue
        r = emulated(kernel, case, fault)
        worst = max(worst, max(r.values()))
        bad = {k: round(v, 2) for k, v in r.items() if not v <= 1.0}
        if bad:
            caught[label] = bad
    print(f'{fault}: worst error / bound {worst:.3g}; caught by', caught)
    assert caught, f'{fault}: no case exceeds the bound (worst error / bound {worst:.3g})'


def test_bf16_rounding_is_half_an_ulp():
    w = torch.tensor([0.0, 1.0, 1.0039, 1.99, 2.0, -3.0, 2.0 ** -20])
    assert torch.equal(LC.bf16_rounding(w), torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -28],
                                                         dtype=torch.float64))
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1)).double()
    assert bool(((LC.rb(x) - x).abs() <= LC.bf16_rounding(x)).all())
