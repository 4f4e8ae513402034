"""Rows on which a softmax kernel's arithmetic matters, and the bound its outputs are held to. Plain torch on the CPU.

A row is the set of scores one softmax is taken over: the keys of one (batch, head, query) for attention, the columns of one
row of logits for the row kernels. One tensor holds rows of every family, row r being of family r % len(families), so that
one launch covers them all:

  unit            N(0, 1), the control
  large           N(0, 6^2)
  shift_pos/_neg  N(+-100, 1): without the subtraction of the maximum f32 overflows / underflows
  spike_first/_mid/_last
                  N(0, 1) with one visible key 40 above the rest: key 0, an interior key (`mid_key`), the last key (which sits
                  in the ragged tail of the last tile)
  ramp            0 .. 60 rising along the keys: the running maximum changes at every tile
  tie             two equal maxima (+30) at `tie_keys`, in different tiles and chunks
  masked_max      the largest score (+100, at `mid_key`) is on a blocked key                      (masked kernels only)
  single_visible  exactly one visible key, the last one, with score -100                          (masked kernels only)
  underflow       a ramp 0 .. 300: most visible keys underflow to p = 0

No row is fully masked and every value is finite. Attention operands stay inside the f16 x 3 range (|scale q|, |k|, |v| < 4094).

`ratios` states the bound, per family and with no element left out:

    |got - want| <= FACTOR * max(e_ref, u * S)

`want` is the float64 formulation of the same f32 inputs, e_ref the largest error over the family of torch's own f32
formulation on the CPU, FACTOR = norm_cases.FACTOR (three bits for another summation order and a hardware exp / log),
u = U_F32 / U_X3 / U_BF16 by the kernel's operand format, and S by kind of output (A = the row's largest
scale * sum_d |q_d k_d| over the keys, |logit| for given logits):

  out                                the family's max |want|
  lse / loss row                     the family's max (|want| + A)
  gradient indexed by the row        (1 + A_family) * max |want| over the whole tensor
  gradient summed over the rows      max((1 + max A) * max |want|, S_rows), one bound for the tensor (S_rows: see `ratios`)

The (1 + A) on gradients: a relative error u in a score of size A changes P by a relative u A. On a spike row
dS = P (dP - delta) cancels to zero, the true gradient is ~1e-15, and any algorithm that recomputes P from a stored f32 lse is
left with an absolute error u A |terms|."""
import math

import torch

import norm_cases as NC

FACTOR = NC.FACTOR
U_F32 = 2.0 ** -24
U_X3 = 2.0 ** -22            # csrc/x3.h: 22 significand bits for the (hi, lo) pair
U_BF16 = 2.0 ** -9

FAMILIES = ('unit', 'large', 'shift_pos', 'shift_neg', 'spike_first', 'spike_mid', 'spike_last', 'ramp', 'tie', 'masked_max',
            'single_visible', 'underflow')
MASKED_ONLY = ('masked_max', 'single_visible')
SPIKE, TIE, RAMP, UNDERFLOW, SHIFT, BLOCKED_MAX, LARGE = 40.0, 30.0, 60.0, 300.0, 100.0, 100.0, 6.0
TILE, CHUNK = 32, 64         # keys per tile / per chunk of the attention kernels (what "another tile" is measured in)
D_HEAD, N_CONTROL = 32, 6
X3_RANGE = 4094.0


def families(masked=True):
    return tuple(f for f in FAMILIES if masked or f not in MASKED_ONLY)


def mid_key(S):
    return S // 2 + 3


def tie_keys(S):
    return S // 4, S - S // 4 - 1


# ------------------------------------------------------------------------------------------------
# attention operands
# ------------------------------------------------------------------------------------------------
class Attn:
    """q (B, Q, E), k, v (B, S, E) f32; mask (B, Q, S) bool, True = blocked (None when unmasked); scale; fams: the family names;
    fam (B, Q) family index of every query row; A (B, H, Q) = max over keys of scale * sum_d |q_d k_d|"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def kv(self):
        return torch.cat([self.k, self.v], -1).contiguous()

    def fam_of(self, kind):
        """family index per element of an output: 'rows' (B, Q, E) | 'lse' (B, H, Q)"""
        B, Q = self.fam.shape
        if kind == 'rows':
            return self.fam[:, :, None].expand(B, Q, self.H * D_HEAD)
        return self.fam[:, None, :].expand(B, self.H, Q)


def key_patterns(S):
    """(S, 6): the key side of the control channels -- all ones; 1 at key 0; 1 at key S - 1; 1 at `mid_key`; key / S; 1 at both
    `tie_keys`"""
    p = torch.zeros(S, N_CONTROL)
    p[:, 0] = 1.0
    p[0, 1] = 1.0
    p[S - 1, 2] = 1.0
    p[mid_key(S), 3] = 1.0
    p[:, 4] = torch.arange(S) / S
    p[list(tie_keys(S)), 5] = 1.0
    return p


# family -> (control channel, amplitude of the score it adds)
_CONTROL = dict(shift_pos=(0, SHIFT), shift_neg=(0, -SHIFT), spike_first=(1, SPIKE), spike_last=(2, SPIKE), spike_mid=(3, SPIKE),
                ramp=(4, RAMP * 1.0), tie=(5, TIE), masked_max=(3, BLOCKED_MAX), single_visible=(2, -SHIFT), underflow=(4, UNDERFLOW))


def attention(B, Q, S, H, seed, masked=True, bf16=False, scale=None, only=None):
    """The operands of one masked (or unmasked) attention whose score rows are of the families above, while the kernel still
    contracts 32 channels per head: channels 0 .. 5 of every head are the control channels (`key_patterns` on the key side, the
    family's amplitude / scale in its own channel on the query side), the other 26 are randn, scaled on the query side so that
    their part of the score is N(0, 1) (N(0, 6^2) for `large`). The two tie keys share their random channels, so their scores
    are equal to the bit. The ramps end at amplitude * (S - 1) / S. only: every row is of that one family."""
    D, E = D_HEAD, H * D_HEAD
    scale = D ** -0.5 if scale is None else scale
    fams = (only,) if only else families(masked)
    assert B * Q >= len(fams) and S >= 3 * TILE
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Q, H, D, generator=g) / (scale * math.sqrt(D - N_CONTROL))
    k = torch.randn(B, S, H, D, generator=g)
    v = torch.randn(B, S, E, generator=g)
    fam = (torch.arange(B * Q) % len(fams)).view(B, Q)
    q[..., :N_CONTROL] = 0.0
    k[..., :N_CONTROL] = key_patterns(S)[None, :, None, :]
    t1, t2 = tie_keys(S)
    k[:, t2, :, N_CONTROL:] = k[:, t1, :, N_CONTROL:]
    mask = (torch.rand(B, Q, S, generator=g) < 0.5) if masked else None
    for i, f in enumerate(fams):
        rows = fam == i
        if f == 'large':
            q[rows] = q[rows] * LARGE
        if f in _CONTROL:
            c, amp = _CONTROL[f]
            sel = q[rows]
            sel[..., c] = amp / scale
            q[rows] = sel
        if mask is None:
            continue
        if f == 'single_visible':
            mask[rows] = True
            mask[rows, S - 1:] = False
            continue
        mask[rows, 1:2] = False                                  # never fully masked, whatever the random bits say
        for key in dict(spike_first=[0], spike_mid=[mid_key(S)], spike_last=[S - 1], tie=[t1, t2]).get(f, []):
            mask[rows, key:key + 1] = False
        if f == 'masked_max':
            mask[rows, mid_key(S):mid_key(S) + 1] = True
    q, k = q.reshape(B, Q, E), k.reshape(B, S, E)
    if bf16:
        q, k, v = (t.bfloat16().float() for t in (q, k, v))
    qa = (q.double().abs() * scale).view(B, Q, H, D).transpose(1, 2)
    ka = k.double().abs().view(B, S, H, D).transpose(1, 2)
    A = (qa @ ka.transpose(-1, -2)).amax(-1)
    return Attn(q=q, k=k, v=v, mask=mask, scale=scale, fams=fams, fam=fam, A=A, B=B, Q=Q, S=S, H=H)


def scores(c, dtype=torch.float64):
    """(B, H, Q, S) scale q . k of a case, unmasked"""
    D = D_HEAD
    qh = (c.q.to(dtype) * c.scale).view(c.B, c.Q, c.H, D).transpose(1, 2)
    kh = c.k.to(dtype).view(c.B, c.S, c.H, D).transpose(1, 2)
    return qh @ kh.transpose(-1, -2)


def attention_refs(c, grad_out=None, dtype=torch.float64, p_dtype=None):
    """torch's own formulation in `dtype`: masked_fill(-inf) -> softmax -> matmul, logsumexp, autograd of these. p_dtype: round P
    to it before the PV product (what a bf16-operand kernel does). -> dict(out (B, Q, E), lse (B, H, Q)[, grad_q, grad_kv])"""
    B, Q, S, H, D, E = c.B, c.Q, c.S, c.H, D_HEAD, c.H * D_HEAD
    q = c.q.to(dtype).requires_grad_(grad_out is not None)
    kv = c.kv.to(dtype).requires_grad_(grad_out is not None)
    qh = (q * c.scale).view(B, Q, H, D).transpose(1, 2)
    kh = kv[..., :E].view(B, S, H, D).transpose(1, 2)
    vh = kv[..., E:].view(B, S, H, D).transpose(1, 2)
    att = qh @ kh.transpose(-1, -2)
    if c.mask is not None:
        att = att.masked_fill(c.mask[:, None], float('-inf'))
    p = att.softmax(-1)
    if p_dtype is not None:
        p = p.to(p_dtype).to(dtype)
    out = (p @ vh).transpose(1, 2).reshape(B, Q, E)
    r = dict(out=out.detach(), lse=att.logsumexp(-1).detach())
    if grad_out is not None:
        r['grad_q'], r['grad_kv'] = torch.autograd.grad(out, (q, kv), grad_out.to(dtype))
        go = grad_out.to(dtype).view(B, Q, H, D).transpose(1, 2)
        r['S_rows'] = max(summed_scale(p.detach(), go @ vh.detach().transpose(-1, -2), c.A.to(dtype), qh.detach().abs(), go.abs())[:2])
    return r


def summed_scale(p, dp, A, q_abs, go_abs):
    """The scale of one row's contribution to the gradients summed over the query rows (see `ratios`): the largest
    (1 + A_i) P_ij |delta_i| |scale q_id| (grad_k), (1 + A_i) P_ij |grad_out_id| (grad_v) and (1 + A_i) P_ij |delta_i| (a bias
    table) over i, j, d. p, dp (..., Q, S); A (..., Q); q_abs = |scale q|, go_abs (..., Q, D)"""
    delta = (p * dp).sum(-1)
    w = (1.0 + A) * p.amax(-1)
    return ((w * delta.abs() * q_abs.amax(-1)).max().item(), (w * go_abs.amax(-1)).max().item(), (w * delta.abs()).max().item())


# ------------------------------------------------------------------------------------------------
# plain logit rows
# ------------------------------------------------------------------------------------------------
class Logits:
    """x (M, N) f32; fams; fam (M,) family index; A (M,) = the row's largest |logit|"""

    def __init__(self, x, fams, fam):
        self.x, self.fams, self.fam = x, fams, fam
        self.A = x.double().abs().amax(1)


def logit_rows(M, N, seed, bf16=False):
    """(M, N) logits whose rows are of the unmasked families; the spikes and tie sit at column 0, `mid_key(N)`, N - 1 and
    `tie_keys(N)`; the ramps end at their amplitude"""
    fams = families(masked=False)
    assert M >= len(fams) and N >= 8
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g, dtype=torch.float64)
    fam = torch.arange(M) % len(fams)
    ramp = torch.arange(N, dtype=torch.float64) / (N - 1)
    for r in range(M):
        f = fams[r % len(fams)]
        if f == 'large':
            x[r] *= LARGE
        elif f in ('shift_pos', 'shift_neg'):
            x[r] += SHIFT if f == 'shift_pos' else -SHIFT
        elif f.startswith('spike'):
            x[r, dict(spike_first=0, spike_mid=mid_key(N), spike_last=N - 1)[f]] += SPIKE
        elif f == 'ramp':
            x[r] = RAMP * ramp
        elif f == 'underflow':
            x[r] = UNDERFLOW * ramp
        elif f == 'tie':
            t1, t2 = tie_keys(N)
            x[r, t1] = x[r, t2] = TIE
    x = x.float()
    if bf16:
        x = x.bfloat16().float()
    return Logits(x, fams, fam)


# ------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------
def _finite_ratio(err, bound):
    r = err / bound
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))           # NaN in got -> inf


def ratios(kind, got, want, ref32, fam, fams, A, u, extra=None, S_rows=0.0):
    """{family: (largest |got - want|, its bound, worst |got - want| / bound)} over every element.
    kind: 'out' | 'lse' | 'grad_rows' (per family) | 'grad_sum' (one bound for the tensor, key 'all').
    got / want / ref32 of one shape; fam: family index per element (unused for 'grad_sum'); A: per element for 'lse', any shape
    with `A_fam` (family index per entry of A) for 'grad_rows' -> pass A = (A, A_fam); the tensor for 'grad_sum'.
    extra: elementwise addition to the bound (the rounding of a bf16 output). S_rows ('grad_sum'): `summed_scale`, see below.

    'grad_sum' takes S = max((1 + max A) max |want|, S_rows). The first term alone, as first stated, takes max |want| for the
    size of the terms. But an lse-recompute backward scales every P of row i by a common (1 + e_i), |e_i| <= u A_i (the
    rounding of the stored f32 lse, which is of size A_i), and dS_ij = P_ij (dP_ij - delta_i) is then off by e_i P_ij delta_i.
    That term does not cancel within the row as dS itself does, so grad_k = dS^T (scale q) is off by u A_i P_ij |delta_i|
    |scale q_id| whatever |want| is: S_rows, which `summed_scale` states in float64 for the largest single row (rows add with
    random signs, which FACTOR covers). tests/test_softmax_cases.py shows a correct emulation of this design above the first
    term alone and inside the maximum of the two."""
    got, want, ref32 = got.double(), want.double(), ref32.double()
    assert got.shape == want.shape == ref32.shape, (got.shape, want.shape, ref32.shape)
    err, eref = (got - want).abs(), (ref32 - want).abs()
    ex = extra.double() if extra is not None else torch.zeros_like(want)
    if kind == 'grad_sum':
        base = FACTOR * max(eref.max().item(), u * max((1.0 + A.max().item()) * want.abs().max().item(), S_rows))
        return {'all': (err.max().item(), base, _finite_ratio(err, base + ex).max().item())}
    base = family_bounds(kind, want, ref32, fam, fams, A, u)
    out = {}
    for i, name in enumerate(fams):
        m = fam == i
        out[name] = (err[m].max().item(), base[i], _finite_ratio(err[m], base[i] + ex[m]).max().item())
    return out


def family_bounds(kind, want, ref32, fam, fams, A, u):
    """[FACTOR * max(e_ref, u * S) per family] for the per-family kinds of `ratios`"""
    want, ref32 = want.double(), ref32.double()
    assert fam.shape == want.shape == ref32.shape
    eref = (ref32 - want).abs()
    base = []
    for i, name in enumerate(fams):
        m = fam == i
        assert bool(m.any()), f'no element of family {name}'
        if kind == 'out':
            S = want[m].abs().max().item()
        elif kind == 'lse':
            S = (want[m].abs() + A.double()[m]).max().item()
        elif kind == 'grad_rows':
            a, a_fam = A
            S = (1.0 + a.double()[a_fam == i].max().item()) * want.abs().max().item()
        else:
            raise ValueError(kind)
        base.append(FACTOR * max(eref[m].max().item(), u * S))
    return base


assert_within = NC.assert_within


# ------------------------------------------------------------------------------------------------
# a correct kernel, emulated: online-softmax forward in the log2 domain and the lse-recompute backward, f32 arithmetic
# ------------------------------------------------------------------------------------------------
def split22(x):
    """x f32 -> the value the f16 (hi, lo) pair of csrc/x3.h holds: hi = f16(x), lo = f16(x - hi); 22 significand bits"""
    hi = x.half().float()
    return hi + (x - hi).half().float()


LOG2E = 1.4426950408889634


def emulate(c, grad_out, x3, bf16=False):
    """out, lse, grad_q, grad_kv of a correct kernel of this design in f32: operands rounded to 22 bits when x3, scores times
    log2(e), exp2 against the row maximum, lse = ln 2 (m + log2 l) stored in f32; the backward recomputes P = exp(s - lse) from
    that f32 lse and forms dS = P (dP - delta) with delta = rowsum(grad_out * out)."""
    B, Q, S, H, D, E = c.B, c.Q, c.S, c.H, D_HEAD, c.H * D_HEAD
    r = (lambda t: t.bfloat16().float()) if bf16 else split22 if x3 else (lambda t: t)
    heads = lambda t, n: t.view(B, n, H, D).transpose(1, 2)                 # noqa: E731
    qs, kh, vh = heads(r(c.q * c.scale), Q), heads(r(c.k), S), heads(r(c.v), S)
    s = qs @ kh.transpose(-1, -2)
    blocked = c.mask[:, None] if c.mask is not None else torch.zeros(1, 1, 1, 1, dtype=torch.bool)
    s2 = (s * LOG2E).masked_fill(blocked, float('-inf'))
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    out = (r(p) @ vh) / l
    lse = ((m + torch.log2(l)) * (1.0 / LOG2E)).squeeze(-1)
    go = heads(grad_out, Q)
    P = torch.exp(s - lse[..., None]).masked_fill(blocked, 0.0)
    delta = (go * out).sum(-1, keepdim=True)
    dP = r(go) @ vh.transpose(-1, -2)
    dS = P * (dP - delta)
    back = lambda t, n: t.transpose(1, 2).reshape(B, n, E)                  # noqa: E731
    gq = back((r(dS) @ kh) * c.scale, Q)
    gk = back(r(dS).transpose(-1, -2) @ qs, S)
    gv = back(r(P).transpose(-1, -2) @ r(go), S)
    return dict(out=back(out, Q), lse=lse, grad_q=gq, grad_kv=torch.cat([gk, gv], -1))


def attention_ratios(c, got, want, ref32, u, rows_term=True):
    """{output: ratios} of whichever of out / lse / grad_q / grad_kv `got` holds (rows_term=False: grad_kv without S_rows)"""
    res = {}
    for name, g in got.items():
        if name == 'out':
            res[name] = ratios('out', g, want[name], ref32[name], c.fam_of('rows'), c.fams, None, u)
        elif name == 'lse':
            res[name] = ratios('lse', g, want[name], ref32[name], c.fam_of('lse'), c.fams, c.A, u)
        elif name == 'grad_q':
            res[name] = ratios('grad_rows', g, want[name], ref32[name], c.fam_of('rows'), c.fams, (c.A, c.fam_of('lse')), u)
        else:
            res[name] = ratios('grad_sum', g, want[name], ref32[name], None, c.fams, c.A, u, S_rows=want['S_rows'] if rows_term else 0.0)
    return res


# ------------------------------------------------------------------------------------------------
# window attention operands
# ------------------------------------------------------------------------------------------------
WINDOW_FAMILIES = tuple(f for f in FAMILIES if f not in MASKED_ONLY)
BEATS = 150.0                # above the row's same-region keys: still 50 ahead after the additive -100 of the shifted-window mask
TABLE_LARGE = 20.0


def window_qkv(B, heads, win, reg, local, N, seed, shifted, table_large=False):
    """qkv (B, L, 3 heads 32) rows of a (shifted-)window attention whose score rows (a token against the N tokens of its window)
    are of the unmasked families, by the control-channel construction of `attention` with the in-window position `local` (L,) in
    place of the key index; win / reg (L,): window id and region label of every token after the cyclic shift.
    shifted adds the family `beats_the_mask`: the query puts 150 on the first or the last token of its window, whichever lies in
    another region than its own (on the first where the window has one region: a plain spike there). table_large: every row is of
    the one family `table_large` (randn q and k; the table carries the scale).
    -> (qkv, fams, fam (B, L))"""
    D, L = D_HEAD, win.numel()
    C = heads * D
    scale = D ** -0.5
    fams = ('table_large',) if table_large else WINDOW_FAMILIES + (('beats_the_mask',) if shifted else ())
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, L, heads, D, generator=g) / (scale * math.sqrt(D - N_CONTROL))
    k = torch.randn(B, L, heads, D, generator=g)
    v = torch.randn(B, L, heads, D, generator=g)
    fam = (torch.arange(B * L) % len(fams)).view(B, L)
    pat = key_patterns(N)                                           # by in-window position
    if not table_large:
        q[..., :N_CONTROL] = 0.0
        k[..., :N_CONTROL] = pat[local][None, :, None, :]
        # the two tie tokens of a window share their random channels
        t1, t2 = tie_keys(N)
        src = {int(w): int(i) for i, w in enumerate(win.tolist()) if int(local[i]) == t1}
        for i in (local == t2).nonzero().flatten().tolist():
            k[:, i, :, N_CONTROL:] = k[:, src[int(win[i])], :, N_CONTROL:]
        first = {int(w): int(reg[i]) for i, w in enumerate(win.tolist()) if int(local[i]) == 0}
        first_reg = torch.tensor([first[int(w)] for w in win.tolist()])
        for i, f in enumerate(fams):
            rows = fam == i
            if f == 'large':
                q[rows] = q[rows] * LARGE
            if f in _CONTROL:
                c, amp = _CONTROL[f]
                sel = q[rows]
                sel[..., c] = amp / scale
                q[rows] = sel
            if f == 'beats_the_mask':
                on_first = (first_reg != reg)[None].expand(B, L) | ~_multi_region(win, reg)[None].expand(B, L)
                for c, m in ((1, rows & on_first), (2, rows & ~on_first)):
                    sel = q[m]
                    sel[..., c] = BEATS / scale
                    q[m] = sel
    return torch.cat([t.reshape(B, L, C) for t in (q, k, v)], -1).contiguous(), fams, fam


def _multi_region(win, reg):
    """(L,) bool: the token's window holds more than one region"""
    lo = torch.full((int(win.max()) + 1,), 99).scatter_reduce(0, win, reg, 'amin')
    hi = torch.full((int(win.max()) + 1,), -1).scatter_reduce(0, win, reg, 'amax')
    return (lo != hi)[win]


def window_logits(qkv, table, win, reg, ly, lx, ws, heads):
    """The dense formulation once more, for the emulation and the scales only (the reference is test_window_attn_gpu.dense_ref)
    -> (logits (B, heads, L, L) with the bias and the additive -100 between regions, -inf outside the window; q scale, k, v
    (B, heads, L, 32); ridx (L, L) table row of every pair; same (L, L))"""
    B, L, _ = qkv.shape
    same = win[:, None] == win[None, :]
    ridx = (ly[:, None] - ly[None, :] + ws - 1) * (2 * ws - 1) + (lx[:, None] - lx[None, :] + ws - 1)
    ridx = torch.where(same, ridx, torch.zeros_like(ridx))
    bias = table[ridx.flatten()].view(L, L, heads).permute(2, 0, 1)
    add = torch.where(reg[:, None] != reg[None, :], -100.0, 0.0).to(qkv.dtype)
    q, k, v = (qkv.view(B, L, 3, heads, D_HEAD)[:, :, i].transpose(1, 2) for i in range(3))
    qs = q * D_HEAD ** -0.5
    logits = (qs @ k.transpose(-2, -1) + bias[None] + add[None, None]).masked_fill(~same[None, None], float('-inf'))
    return logits, qs, k, v, ridx, same


def window_scales(qkv, table, go, win, reg, ly, lx, ws, heads):
    """float64: A (B, heads, L) = the row's largest scale sum_d |q_d k_d| + |bias| + 100 [regions differ] over the keys of its
    window, and `summed_scale` of the case (S for grad_k, grad_v, grad_table)"""
    qkv, table, go = qkv.double(), table.double(), go.double()
    B, L, _ = qkv.shape
    logits, qs, k, v, ridx, same = window_logits(qkv, table, win, reg, ly, lx, ws, heads)
    a, _, _, _, _, _ = window_logits(qkv.abs(), table.abs(), win, torch.zeros_like(reg), ly, lx, ws, heads)
    a = a + torch.where(reg[:, None] != reg[None, :], 100.0, 0.0)[None, None]
    A = a.masked_fill(~same[None, None], 0.0).amax(-1)
    p = logits.softmax(-1)
    goh = go.view(B, L, heads, D_HEAD).transpose(1, 2)
    return A, summed_scale(p, goh @ v.transpose(-2, -1), A, qs.abs(), goh.abs())


def emulate_window(qkv, table, go, win, reg, ly, lx, ws, heads):
    """A correct kernel of the window attention's design in f32: exact-f32 products, lse stored in f32, the backward recomputing
    P = exp(s - lse) and dS = P (dP - delta), delta = rowsum(grad_out * out). -> out, lse, grad_qkv, grad_table"""
    B, L, _ = qkv.shape
    C = heads * D_HEAD
    s, qs, k, v, ridx, same = window_logits(qkv, table, win, reg, ly, lx, ws, heads)
    m = s.amax(-1, keepdim=True)
    lse = (m + (s - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)
    P = torch.exp(s - lse[..., None])
    out = P @ v
    goh = go.view(B, L, heads, D_HEAD).transpose(1, 2)
    dS = P * (goh @ v.transpose(-2, -1) - (goh * out).sum(-1, keepdim=True))
    back = lambda t: t.transpose(1, 2).reshape(B, L, C)                    # noqa: E731
    gq = back(dS @ k) * D_HEAD ** -0.5
    gk, gv = back(dS.transpose(-2, -1) @ qs), back(P.transpose(-2, -1) @ goh)
    gt = torch.zeros_like(table).index_add_(0, ridx.flatten(), (dS * same[None, None]).sum(0).permute(1, 2, 0).reshape(L * L, heads))
    return dict(out=back(out), lse=lse, grad_qkv=torch.cat([gq, gk, gv], -1), grad_table=gt)
