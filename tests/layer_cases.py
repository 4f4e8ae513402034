"""Operands, references and the bound for the fused layer kernels: the query decoder's (csrc/decoder_tail.hip: decoder_tail,
decoder_mid, decoder_ffn; cgg_layernorm_chain; the LayerNorm epilogue of cgg_linear_rows) and the pixel decoder's encoder layers
(csrc/encoder_ffn.hip: encoder_ffn_ln, encoder_layer_tail; csrc/encoder_tail_x3.hip: the x3 / x3a twin). Plain torch on the CPU.

Every chain is written ONCE, over an arithmetic object:

  Ref(float64, kind)   the reference. kind 'bf16': the operands of every GEMM (activations and weights) rounded to bf16 where the
                       kernels' header comments say so ("bf16 operands, f32 accumulate, f32 LayerNorm": each linear's input is
                       stored as bf16 A fragments, hidden blocks included; biases, residuals, positions, plane sums and LayerNorms
                       are not rounded). kind 'x3' / 'f32': no rounding points.
  Ref(float32, kind)   torch's own f32 formulation of the same chain with the same rounding points: its largest error is e_ref.
  Emu(kind, fault)     an f32 emulation of the kernels' design (tests/test_layer_cases.py): GEMMs accumulate 16-wide K chunks in
                       f32, last chunk first (not torch's order); x3 GEMMs by hi / lo f16 pieces of the pre-scaled operands as
                       csrc/x3.h describes (a' = 16 a, weight rows scaled to [2^10, 2^11), al bh + ah bh per chunk, then ah bl,
                       column scale, then bias); LayerNorm in two passes in the kernels' order (four columns per lane, xor
                       butterfly over 64 lanes); planes summed in index order. `fault` seeds one wrong design (FAULTS).

The bound, per output and over every element:

    |got - want| <= FACTOR * max(e_ref, T) + extra

FACTOR = norm_cases.FACTOR. e_ref = the largest |Ref(float32) - Ref(float64)| of the output over the case. T per element is u S
of the LAST stage that forms the output:
  GEMM       S = |a| |W|^T + |bias| + |residual| from the float64 reference (the rounded operands for 'bf16');
             u = 2^-9 ('bf16': a hidden value that the kernel and the reference round to different bf16 neighbours),
             u = 2^-22 ('x3'), plus the x3 operand representation (2^-22 |a| + 2^-29) |W|^T: the pair (hi, lo) holds 16 a to 22
             bits, and a lo piece below f16's normal range is off by up to the subnormal step 2^-24 / 2, divided by the pre-scale 16.
  LayerNorm  S = norm_cases.ln_scale, u = 2^-24 (the LayerNorms are f32 in every mode); when the normalised sum holds an x3 GEMM,
             its operand representation term is propagated by |gamma| rstd.
  + pos      adds |pos| (and |shift|) to S.
  WIDENED for the encoder kernels' LayerNorm 1, whose sum x1 + W2 h + b2 holds operands rounded on the way (`enc_case`): one hidden
  value on the other bf16 neighbour moves the sum by 2^-8 |h_k| |W2_nk| -- torch's f32 formulation does that to a few elements per
  case, the kernel to a few others, so e_ref alone (9e-7 without such an element, 6e-5 .. 7e-4 with one) is a lottery. T gains, times
  |gamma| rstd: `flip_term` of the hidden block, the x3 operand term, and for the bf16 layer tail (which stores x1 itself as bf16, the
  FFN's input and the residual) 2^-8 |x1| and x1's flip through both linears. FACTOR stays.
NOT PINNED: cgg_encoder_layer_tail_bf16 is exempt from the per-family f32-class conditioning bound. It stores x1 = LN0(..) as bf16
before anything reads it, so the issue's premise "nothing is rounded" does not hold for it, and with 2^-8 |x1| in T a wrong variance
formula in its LN0 (relative error ~1e-4 on the offset rows) stays inside the bound: the seeded one-pass variance is caught by no
bf16 layer-tail case. Its LN1 is the code `encoder_ffn_ln` runs (same kernel template), which is held per family; its LN0 is held
only to the bf16-class bound. The x3 / x3a twins are held per family for both.
The SECOND LayerNorm of a kernel (LN_b of the decoder tail and of layernorm_chain, LN1 of the encoder layer tails) normally sees
only the centred O(1) output of the first; the cond='second' cases give the first gamma 2^-10 and beta 64, so that the second
normalises rows of mean 64 (32) and spread 1e-3 (5e-4).
extra = one bf16 rounding of want for a bf16 output (`bf16_rounding`), 2^-22 |want| for an x3a output.
Nothing here is fitted to the kernels: tests/test_layer_cases.py shows that the emulated design sits under the bound and that every
seeded fault it can see exceeds it."""
import functools
import types

import torch
import torch.nn.functional as F

import norm_cases as NC

FACTOR = NC.FACTOR
U_F32 = 2.0 ** -24
U_X3 = 2.0 ** -22
U_BF16 = 2.0 ** -9
X3_SUB = 2.0 ** -29             # f16 subnormal half-step 2^-25 of the pre-scaled value, / 16
C = 256

KINDS = ('bf16', 'x3')
M_POS = [(1, 1), (31, 100), (32, 20), (33, 100), (77, 20)]     # (M, pos_rows): see tests/test_layer_edges_gpu.py

ENC_KERNELS = [('bf16', 'ffn'), ('bf16', 'tail'), ('x3', 'tail'), ('x3a', 'tail')]      # (kind, variant) of layer_cases.enc_case
ENC_M = [1, 63, 64, 65, 130]                                                            # 64 rows per workgroup
ENC_LEVELS = (2, ((2, 3), (4, 5), (8, 9)))                                              # B, level (h, w): S = 98, M = 196

FAULTS = ('planes_ge_8_dropped', 'pos_index_block_local', 'eps_swapped', 'second_ln_first_mean', 'one_pass_variance',
          'x3_lo_hi_dropped', 'x3_scale_after_bias', 'relu2_missing', 'ffn_bias_every_plane', 'hidden_rounded_late')


def bf16_rounding(want):
    """half a bf16 ulp at |want| (0 at 0)"""
    w = want.double().abs()
    e = torch.floor(torch.log2(w.clamp_min(2.0 ** -126)))
    return torch.where(w > 0, torch.exp2(e - 8), torch.zeros_like(w))


def rb(t):
    """t rounded to bf16, in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def pos_index(M, pos_rows):
    return torch.arange(M) % pos_rows


# ------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------
class Ref:
    fault = None

    def __init__(self, dt, kind):
        assert kind in ('bf16', 'x3', 'f32')
        self.dt, self.kind = dt, kind

    def c(self, t):
        return t.to(self.dt)

    def rnd(self, t):
        return rb(t) if self.kind == 'bf16' else t

    def lin(self, a, W, b=None, hidden=False):
        y = self.rnd(a) @ self.rnd(self.c(W)).t()
        return y if b is None else y + self.c(b)

    def ln(self, x, norm, keep_mean=False, use_mean=False):
        g, b, eps = norm
        return F.layer_norm(x, (x.shape[-1],), self.c(g), self.c(b), eps)

    def psum(self, planes):
        return self.c(planes).sum(0)

    def pos_index(self, M, pos_rows):
        return pos_index(M, pos_rows)


def x3_split(t):
    """f32 -> the two f16 pieces (as f32 values): hi = f16(t), lo = f16(t - hi)"""
    h = t.half().float()
    return h, (t - h).half().float()


def x3_weight(W):
    """W (N, K) f32 -> (hi, lo, colscale): rows scaled by 2^e_n so that max_k |w'_nk| lies in [2^10, 2^11); colscale = 2^-e_n / 16"""
    mx = W.abs().amax(1)
    e = 10 - torch.floor(torch.log2(mx.clamp_min(2.0 ** -100)))
    sc = torch.where(mx > 0, torch.exp2(e), torch.zeros_like(mx))
    h, l = x3_split(W * sc[:, None])
    return h, l, torch.where(mx > 0, torch.exp2(-e) / 16, torch.zeros_like(mx))


class Emu(Ref):
    def __init__(self, kind, fault=None):
        super().__init__(torch.float32, kind)
        assert fault is None or fault in FAULTS
        self.fault = fault
        self.mean = None

    @staticmethod
    def _acc(acc, a, w):
        for c in reversed(range(a.shape[1] // 16)):
            acc = acc + a[:, 16 * c:16 * c + 16] @ w[:, 16 * c:16 * c + 16].t()
        return acc

    def lin(self, a, W, b=None, hidden=False):
        acc = torch.zeros(a.shape[0], W.shape[0])
        if self.kind == 'x3':
            ah, al = x3_split(a * 16.0)
            bh, bl, cs = x3_weight(W)
            for c in reversed(range(a.shape[1] // 16)):
                s = slice(16 * c, 16 * c + 16)
                if self.fault != 'x3_lo_hi_dropped':
                    acc = acc + al[:, s] @ bh[:, s].t()
                acc = acc + ah[:, s] @ bh[:, s].t()
            acc = self._acc(acc, ah, bl)
            if self.fault == 'x3_scale_after_bias' and b is not None:
                return (acc + b) * cs
            y = acc * cs
        else:
            late = hidden and self.fault == 'hidden_rounded_late'
            y = self._acc(acc, a if late else self.rnd(a), self.rnd(W))
            if late:
                y = self.rnd(y)
        return y if b is None else y + b

    def ln(self, x, norm, keep_mean=False, use_mean=False):
        g, b, eps = norm
        M, N = x.shape
        if N == C:                      # lane l holds columns 4l .. 4l+3; butterfly over the 64 lanes
            lanes = torch.arange(64)

            def total(t):
                t = t.view(M, 64, 4)
                s = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
                for o in (32, 16, 8, 4, 2, 1):
                    s = s + s[:, lanes ^ o]
                return s[:, :1]
        else:                           # another order than torch's: last column first
            def total(t):
                s = torch.zeros(M, 1)
                for k in reversed(range(N)):
                    s = s + t[:, k:k + 1]
                return s
        inv_n = torch.tensor(1.0 / N)
        mean = total(x) * inv_n
        if self.fault == 'one_pass_variance':
            var = total(x * x) * inv_n - mean * mean
        else:
            if use_mean and self.fault == 'second_ln_first_mean':
                mean = self.mean
            d = x - mean
            var = total(d * d) * inv_n
        if keep_mean:
            self.mean = mean
        return (x - mean) * torch.rsqrt(var + eps) * g + b

    def psum(self, planes):
        n = planes.shape[0]
        if self.fault == 'planes_ge_8_dropped':
            n = min(n, 8)
        s = torch.zeros_like(planes[0])
        for p in range(n):
            s = s + planes[p]
        return s

    def pos_index(self, M, pos_rows):
        m = torch.arange(M)
        return (m % 32) % pos_rows if self.fault == 'pos_index_block_local' else m % pos_rows


# ------------------------------------------------------------------------------------------------
# the chains; o = namespace of f32 operands. Each returns a dict of outputs and of the intermediates S needs.
# ------------------------------------------------------------------------------------------------
def chain_ln(A, o):
    """cgg_layernorm_chain: y = LN_a(sum planes), yp = y + pos, z = LN_b(y)"""
    s = A.psum(o.planes)
    y = A.ln(s, o.norm_a, keep_mean=True)
    r = dict(s=s, y=y)
    if o.pos is not None:
        r['yp'] = y + A.c(o.pos)[A.pos_index(y.shape[0], o.pos.shape[0])]
    if o.norm_b is not None:
        r['z'] = A.ln(y, o.norm_b, use_mean=True)
    return r


def chain_tail(A, o):
    """cgg_decoder_tail: chain_ln, me = W3 relu(W2 relu(W1 z + b1) + b2) + b3, qn = Wq (y + pos) + bq"""
    na, nb = o.norm_a, o.norm_b
    if A.fault == 'eps_swapped':
        na, nb = (na[0], na[1], nb[2]), (nb[0], nb[1], na[2])
    r = chain_ln(A, types.SimpleNamespace(planes=o.planes, norm_a=na, norm_b=nb, pos=o.pos))
    w1, b1, w2, b2, w3, b3 = o.mlp
    h1 = A.lin(r['z'], w1, b1).relu()
    h2 = A.lin(h1, w2, b2, hidden=True)
    if A.fault != 'relu2_missing':
        h2 = h2.relu()
    r.update(h2=h2, me=A.lin(h2, w3, b3, hidden=True))
    if o.qproj is not None:
        r['qn'] = A.lin(r['yp'], o.qproj[0], o.qproj[1])
    return r


def chain_mid(A, o):
    """cgg_decoder_mid: x1 = LN(core Wo^T + bo + res); q | k = (x1 + pos) W^T + b, v = x1 Wv^T + bv"""
    t = A.lin(A.c(o.core), o.wo, o.bo) + A.c(o.res)
    x1 = A.ln(t, o.norm)
    r = dict(t=t, x1=x1)
    if o.qkv is not None:
        w, b = o.qkv
        xp = x1 + A.c(o.pos)[A.pos_index(x1.shape[0], o.pos.shape[0])]
        r.update(xp=xp, q=A.lin(xp, w[:C], b[:C]), kv=torch.cat([A.lin(xp, w[C:2 * C], b[C:2 * C]), A.lin(x1, w[2 * C:], b[2 * C:])], 1))
    return r


def chain_ffn(A, o):
    """cgg_decoder_ffn: planes[cb] = relu(x W1[cb]^T + b1[cb]) W2[:, cb]^T (+ b2 + x in plane 0)"""
    x = A.c(o.x)
    planes, hs = [], []
    for cb in range(o.w1.shape[0] // C):
        s = slice(cb * C, (cb + 1) * C)
        h = A.lin(x, o.w1[s], o.b1[s]).relu()
        p = A.lin(h, o.w2[:, s], hidden=True)
        if cb == 0 or A.fault == 'ffn_bias_every_plane':
            p = p + A.c(o.b2) + x
        planes.append(p)
        hs.append(h)
    planes = torch.stack(planes)
    return dict(planes=planes, h=torch.cat(hs, 1), sum=planes.sum(0))


def chain_linear_ln(A, o):
    """cgg_linear_rows with the LayerNorm epilogue: y = LN(x W^T + b + res), yp = y + pos"""
    t = A.lin(A.c(o.x), o.w, o.b) + A.c(o.res)
    y = A.ln(t, o.norm)
    return dict(t=t, y=y, yp=y + A.c(o.pos)[A.pos_index(y.shape[0], o.pos.shape[0])])


def chain_enc(A, o):
    """cgg_encoder_layer_tail_{bf16,x3,x3a} (o.a given) and cgg_encoder_ffn_ln_bf16 (o.a None):
    x1 = LN0(x + a Wo^T + bo) | x;  y = LN1(x1 + W2 relu(W1 x1 + b1) + b2);  yp = y + pos;  kv: m = y + shift, mp = m + pos.
    'bf16': x1 lives in the row image as bf16 -- the FFN's input AND LayerNorm 1's residual; x3 keeps x1 in f32 registers."""
    x = A.c(o.x)
    r = {}
    if o.a is not None:
        r['t0'] = A.lin(A.c(o.a), o.wo, o.bo) + x
        x = A.ln(r['t0'], o.norm0, keep_mean=True)
    x1 = A.rnd(x)
    h = A.lin(x1, o.w1, o.b1).relu()
    t1 = A.lin(h, o.w2, o.b2, hidden=True) + x1
    y = A.ln(t1, o.norm1, use_mean=o.a is not None)
    idx = A.pos_index(y.shape[0], o.pos.shape[0])
    r.update(x1=x1, h=h, t1=t1, y=y, yp=y + A.c(o.pos)[idx])
    if o.shift is not None:
        r['m'] = y + A.c(o.shift)[idx]
        r['mp'] = r['m'] + A.c(o.pos)[idx]
    return r


# ------------------------------------------------------------------------------------------------
# S and T
# ------------------------------------------------------------------------------------------------
def _w(W, kind):
    W = W.double()
    return (rb(W) if kind == 'bf16' else W).abs()


def _a(a, kind):
    return (rb(a) if kind == 'bf16' else a).abs()


def gemm_opnd(a, W, kind):
    """the x3 operand representation of a GEMM's activations, per output element (0 for bf16: the reference rounds them too)"""
    if kind != 'x3':
        return 0.0
    return (U_X3 * a.abs() + X3_SUB) @ W.double().abs().t()


def gemm_T(a, W, kind, *added):
    """a: the float64 reference's input of the GEMM (before its rounding point); added: bias / residual terms"""
    S = _a(a, kind) @ _w(W, kind).t()
    for t in added:
        S = S + t.double().abs()
    return (U_BF16 if kind == 'bf16' else U_X3) * S + gemm_opnd(a, W, kind)


def ln_T(x, norm, opnd=0.0):
    """x: the float64 sum that is normalised; opnd: representation error of x, propagated by |gamma| rstd"""
    g, b, eps = norm
    _, _, var = NC.two_pass(x, eps)
    return U_F32 * NC.ln_scale(x, g.double(), b.double(), eps) + g.double().abs() / torch.sqrt(var + eps) * opnd


class Spec:
    """one output of a case: want (float64), ref32, T (per element), extra (per element or 0.0)"""

    def __init__(self, want, ref32, T, extra=0.0):
        self.want, self.ref32, self.T, self.extra = want, ref32.double(), T, extra
        self.e_ref = (self.ref32 - want).abs().max().item()

    def bound(self):
        return FACTOR * torch.clamp_min(self.T + torch.zeros_like(self.want), self.e_ref) + self.extra

    def ratio(self, got):
        """(largest |got - want| / bound over every element, largest error); a NaN in got -> inf"""
        got = got.detach().cpu().double()
        assert got.shape == self.want.shape, (got.shape, self.want.shape)
        err = (got - self.want).abs()
        r = err / self.bound()
        r = torch.where(err == 0, torch.zeros_like(r), torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf'))))
        return r.max().item(), err.max().item()


def ratios(spec, outs):
    """{name: worst error / bound} for the outputs `outs` ({name: tensor}) of a case's spec ({name: Spec})"""
    return {k: spec[k].ratio(v)[0] for k, v in outs.items() if v is not None}


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, k=1.0: torch.randn(*s, generator=g) * k


def _norm(r, eps=1e-5):
    return (1 + 0.3 * r(C), 0.3 * r(C), eps)


def signed_perm(N, seed, exps=(-1, 0, 1)):
    """(N, N) weight = signed permutation times powers of two: every product with a bf16 value is exact in bf16, f16 x 3 and f32"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(N, generator=g)
    sign = torch.randint(0, 2, (N,), generator=g) * 2.0 - 1.0
    mag = torch.exp2(torch.tensor(exps, dtype=torch.float32)[torch.randint(0, len(exps), (N,), generator=g)])
    W = torch.zeros(N, N)
    W[torch.arange(N), perm] = sign * mag
    return W, perm, sign * mag


def cond_rows(nrows, seed):
    """(values, family index per element) of norm_cases rows, at least 11 so that every kind occurs. Row r is of kind r % 11: with
    nrows = 43 the ragged last block (rows 32 .. 42) holds every kind, the flat and the offset rows included."""
    c = NC.ln_rows(nrows, C, seed)
    return c.x, c.fam


def _finish(o, kind, chain, spec_of, lns):
    """lns = {LayerNorm output: (its norm, the name of the sum it normalises)} for the conditioning bound"""
    w, r32 = chain(Ref(torch.float64, kind), o), chain(Ref(torch.float32, kind), o)
    return types.SimpleNamespace(o=o, kind=kind, chain=chain, want=w, spec=spec_of(w, r32), lns=lns)


@functools.lru_cache(maxsize=None)
def tail_case(kind, M, pos_rows, nsum, cond=False, seed=0):
    """decoder_tail / layernorm_chain (kind 'f32': no MLP). cond: the plane sum equals norm_cases rows up to f32 roundings (planes
    p >= 1 are x 2^-(p+2), plane 0 the rest; exact on the flat rows), eps_b = 1e-3 so that swapped eps show on the tight rows.
    cond='second': the same rows with gamma_a 2^-10 and beta_a = 64, which hands the SECOND LayerNorm rows of mean 64 and spread
    1e-3 -- LN_a's own output is otherwise always centred and O(1). cond='round': see `_tail_round_case`."""
    r = _gen(1000 + seed + 7 * M + nsum)
    fam = None
    if cond == 'round':
        return _tail_round_case(kind, M, pos_rows, nsum, r)
    if cond:
        x, fam = cond_rows(M, 50 + seed)
        planes = torch.stack([x * 2.0 ** -(p + 2) for p in range(nsum)])
        planes[0] = x - planes[1:].sum(0)
    else:
        planes = r(nsum, M, C, k=0.5)
    second = cond == 'second'
    mlp = qproj = None
    if kind != 'f32':
        mlp = tuple(t for _ in range(3) for t in (r(C, C, k=1 / 16), r(C, k=0.5)))
        qproj = (r(C, C, k=1 / 16), r(C, k=0.5))
    na, nb = _norm(r), _norm(r, 1e-3 if cond is True else 1e-5)
    if second:                          # y = 64 + 2^-10 (..): every row LN_b sees is off-centre AND tight (spread 1e-3, variance below eps)
        na = (2.0 ** -10 * na[0], torch.full((C,), 64.0), na[2])
    return _tail_finish(kind, M, pos_rows, planes, na, nb, r(pos_rows, C), mlp, qproj, fam)


def _tail_round_case(kind, M, pos_rows, nsum, r):
    """cond='round': a tail whose mask MLP is decided by WHERE the hidden blocks are rounded, with no luck involved. Every plane row is
    flat and beta_a is constant, so y = beta_a and z = beta_b hold exactly in f32 and float64 alike; beta_b is bf16, W1 the identity
    and b1 = j 2^-12, so h1 = beta_b + b1 is exact but not bf16; W2 takes 64 x the difference of two h1 that are neighbours in sorted
    order (about one bf16 step apart), so h2 = relu(64 (bf16(h1_a) - bf16(h1_b))) is exact, of the size of the rounding itself, and
    b3 = 0 leaves S = |h2| |W3|^T that small. A design that rounds h1 anywhere else gets another h2 altogether."""
    planes = torch.stack([torch.full((M, C), 3.0 * 2.0 ** -(p + 2)) for p in range(nsum)])
    planes[0] = 3.0 - planes[1:].sum(0)
    g = torch.Generator().manual_seed(77)
    beta_b = rb(1.0 + 0.5 * torch.rand(C, generator=g))
    b1 = torch.randint(1, 16, (C,), generator=g) * 2.0 ** -12
    order = torch.argsort(beta_b + b1)
    w2 = torch.zeros(C, C)
    n = torch.arange(C)
    sign = torch.where(n % 2 == 0, 64.0, -64.0)
    w2[n, order[n]] = -sign
    w2[n, order[(n + 1) % C]] = sign
    mlp = (torch.eye(C), b1, w2, torch.zeros(C), r(C, C, k=1 / 16), torch.zeros(C))
    na = (1 + 0.3 * r(C), torch.full((C,), 0.5), 1e-5)
    nb = (1 + 0.3 * r(C), beta_b, 1e-5)
    return _tail_finish(kind, M, pos_rows, planes, na, nb, r(pos_rows, C), mlp, (r(C, C, k=1 / 16), r(C, k=0.5)), None)


def _tail_finish(kind, M, pos_rows, planes, na, nb, pos, mlp, qproj, fam):
    o = types.SimpleNamespace(planes=planes, norm_a=na, norm_b=nb, pos=pos, mlp=mlp, qproj=qproj, fam=fam)

    def spec_of(w, r32):
        p = o.pos.double().abs()[pos_index(M, pos_rows)]
        Ty = ln_T(w['s'], na)
        sp = dict(y=Spec(w['y'], r32['y'], Ty), yp=Spec(w['yp'], r32['yp'], Ty + U_F32 * p),
                  z=Spec(w['z'], r32['z'], ln_T(w['y'], nb)))
        if kind != 'f32':
            sp['me'] = Spec(w['me'], r32['me'], gemm_T(w['h2'], mlp[4], kind, mlp[5]))
            sp['qn'] = Spec(w['qn'], r32['qn'], gemm_T(w['yp'], qproj[0], kind, qproj[1]))
        return sp
    return _finish(o, kind, chain_ln if kind == 'f32' else chain_tail, spec_of, dict(y=(na, 's'), z=(nb, 'y')))


@functools.lru_cache(maxsize=None)
def mid_case(kind, M, pos_rows, cond=False, seed=0):
    """decoder_mid. cond: Wo a signed permutation times powers of two, core bf16 values with core Wo^T = bf16(x / 4) exactly, bo = +-0.5,
    res = x - core Wo^T - bo: the normalised sum is x up to f32 roundings (exactly x on the flat rows)."""
    r = _gen(2000 + seed + 7 * M)
    fam = None
    if cond:
        x, fam = cond_rows(M, 60 + seed)
        wo, perm, val = signed_perm(C, 61 + seed, exps=(0, 1))
        proj = rb(0.25 * x)
        core = torch.zeros(M, C)
        core[:, perm] = proj / val
        bo = torch.where(torch.arange(C) % 2 == 0, 0.5, -0.5)
        res = x - proj - bo
        assert torch.equal(core @ wo.t(), proj) and torch.equal(rb(core), core) and core.abs().max() < 4094
    else:
        core, res, wo, bo = r(M, C), r(M, C), r(C, C, k=1 / 16), r(C, k=0.5)
    norm = _norm(r)
    o = types.SimpleNamespace(core=core, res=res, wo=wo, bo=bo, norm=norm, pos=r(pos_rows, C),
                              qkv=(r(3 * C, C, k=1 / 16), r(3 * C, k=0.5)), fam=fam)

    def spec_of(w, r32):
        wq, bq = o.qkv
        sp = dict(x1=Spec(w['x1'], r32['x1'], ln_T(w['t'], norm, gemm_opnd(core.double(), wo, kind))),
                  q=Spec(w['q'], r32['q'], gemm_T(w['xp'], wq[:C], kind, bq[:C])))
        sp['kv'] = Spec(w['kv'], r32['kv'], torch.cat([gemm_T(w['xp'], wq[C:2 * C], kind, bq[C:2 * C]),
                                                       gemm_T(w['x1'], wq[2 * C:], kind, bq[2 * C:])], 1))
        return sp
    return _finish(o, kind, chain_mid, spec_of, dict(x1=(norm, 't')))


@functools.lru_cache(maxsize=None)
def ffn_case(kind, M, Fw, seed=0):
    """decoder_ffn at FFN width Fw: every plane, and their float64 sum"""
    r = _gen(3000 + seed + 7 * M + Fw)
    o = types.SimpleNamespace(x=r(M, C), w1=r(Fw, C, k=1 / 16), b1=r(Fw, k=0.5), w2=r(C, Fw, k=Fw ** -0.5), b2=r(C, k=0.5))

    def spec_of(w, r32):
        x = o.x.double()
        Tp = torch.stack([gemm_T(w['h'][:, cb * C:(cb + 1) * C], o.w2[:, cb * C:(cb + 1) * C], kind,
                                 *((o.b2, x) if cb == 0 else ())) for cb in range(Fw // C)])
        return dict(planes=Spec(w['planes'], r32['planes'], Tp), sum=Spec(w['sum'], r32['sum'], gemm_T(w['h'], o.w2, kind, o.b2, x)))
    return _finish(o, kind, chain_ffn, spec_of, {})


@functools.lru_cache(maxsize=None)
def linear_ln_case(kind, M, N, K, pos_rows, cond=False, seed=0):
    """linear_rows_bf16(ln=...): N outputs from K inputs, with res, pos and want_pos. cond (N <= K): W has one signed power of two
    per row, x is bf16 with x W^T = bf16(rows / 4) exactly, b = +-0.5, res = rows - x W^T - b: the normalised sum is the
    norm_cases rows (of N elements) up to f32 roundings, exactly on the flat rows."""
    r = _gen(4000 + seed + 7 * M + N + K)
    norm = (1 + 0.3 * r(N), 0.3 * r(N), 1e-5)
    fam = None
    if cond:
        c = NC.ln_rows(M, N, 80 + seed + N)
        fam = c.fam
        g = torch.Generator().manual_seed(81 + seed + N)
        perm = torch.randperm(K, generator=g)[:N]
        val = (torch.randint(0, 2, (N,), generator=g) * 2.0 - 1.0) * torch.exp2(torch.randint(0, 2, (N,), generator=g).float())
        w = torch.zeros(N, K)
        w[torch.arange(N), perm] = val
        proj = rb(0.25 * c.x)
        x = torch.zeros(M, K)
        x[:, perm] = proj / val
        b = torch.where(torch.arange(N) % 2 == 0, 0.5, -0.5)
        res = c.x - proj - b
        assert torch.equal(x @ w.t(), proj) and torch.equal(rb(x), x) and x.abs().max() < 4094
    else:
        x, w, b, res = r(M, K), r(N, K, k=K ** -0.5), r(N, k=0.5), r(M, N)
    o = types.SimpleNamespace(x=x, w=w, b=b, res=res, norm=norm, pos=r(pos_rows, N), fam=fam)

    def spec_of(w, r32):
        Ty = ln_T(w['t'], norm, gemm_opnd(o.x.double(), o.w, kind))
        return dict(y=Spec(w['y'], r32['y'], Ty), yp=Spec(w['yp'], r32['yp'], Ty + U_F32 * o.pos.double().abs()[pos_index(M, pos_rows)]))
    return _finish(o, kind, chain_linear_ln, spec_of, dict(y=(norm, 't')))


def all_ratios(case, outs):
    """{output: worst error / bound} over every element of the outputs `outs` of a case; on a conditioning case also
    {'output/family': ...} for its LayerNorm outputs under norm_cases.family_ratios (S = ln_scale, u = 2^-24: nothing before the
    LayerNorm is rounded there)"""
    r = ratios(case.spec, outs)
    if getattr(case.o, 'fam', None) is not None:
        for name, (norm, xname) in case.lns.items():
            if outs.get(name) is None:
                continue
            g, b, eps = norm
            sp = case.spec[name]
            S = NC.ln_scale(case.want[xname], g.double(), b.double(), eps)
            for f, v in NC.family_ratios(outs[name].detach().cpu(), sp.want, sp.ref32, S, case.o.fam).items():
                r[f'{name}/{f}'] = v[2]
    return r


def assert_all(label, case, outs):
    """prints every ratio of `all_ratios`, then asserts them"""
    r = all_ratios(case, outs)
    print(f'{label}: ' + '  '.join(f'{k}={v:.3g}' for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f'{label}: error / bound {bad}'
    return r


# ------------------------------------------------------------------------------------------------
# encoder kernels (64 rows per workgroup)
# ------------------------------------------------------------------------------------------------
def x3a_values(x):
    """the values an x3a row holds for f32 x: (f16(16 x) + f16(16 x - f16(16 x))) / 16 (csrc/x3.h)"""
    h, l = x3_split(x * 16.0)
    return (h + l) / 16.0


def level_major(t, B, level_hw):
    """(B S, 256) rows in image order -> the level-major order of the K / V outputs: level l = rows [B start_l, B start_{l+1}) laid
    out (B, hw_l, 256)"""
    S = sum(h * w for h, w in level_hw)
    t = t.view(B, S, -1)
    out, s0 = [], 0
    for h, w in level_hw:
        out.append(t[:, s0:s0 + h * w].reshape(B * h * w, -1))
        s0 += h * w
    return torch.cat(out, 0)


def flip_term(a, W, kind):
    """'bf16': what ONE operand of a GEMM rounded to the other bf16 neighbour (2^-8 |a_k|) moves an output by, at most:
    2^-8 max_k |a_k| max_k |W_nk| per element"""
    if kind != 'bf16':
        return 0.0
    return 2.0 ** -8 * a.abs().amax(1, keepdim=True) * rb(W.double()).abs().amax(1)[None]


@functools.lru_cache(maxsize=None)
def enc_case(kind, variant, M, FF, pos_rows, cond=False, levels=None, seed=0):
    """kind 'bf16' | 'x3' | 'x3a'; variant 'ffn' (encoder_ffn_ln, bf16 only) | 'tail' (encoder_layer_tail*). levels = (B, level_hw):
    the K / V variants (M = B S, pos and shift have S rows). cond: norm_cases rows (bf16 kinds for the bf16 kernels) in front of the
    FIRST LayerNorm of the kernel, with an exactly computable GEMM part: 'tail': a Wo^T = the quarter of split_ab, x the rest,
    bo = 0; and in either variant W1 a permutation and W2 = -P^T / 2, b1 = b2 = 0, so that FFN(x1) = -relu(x1) / 2 exactly."""
    assert (kind == 'bf16' or variant == 'tail') and FF % C == 0
    r = _gen(5000 + seed + 7 * M + FF + (100 if variant == 'tail' else 0))
    ak = 'x3' if kind == 'x3a' else kind
    b16 = kind == 'bf16'
    q = (lambda t: rb(t)) if b16 else (lambda t: t)
    fam = a = wo = bo = norm0 = shift = None
    if cond:
        c = NC.ln_rows(M, C, 70 + seed, bf16=b16)
        fam = c.fam
        w1, perm, _ = signed_perm(C, 71 + seed, exps=(0,))
        w1 = torch.cat([w1.abs(), torch.zeros(FF - C, C)])
        w2 = torch.cat([-0.5 * w1[:C].t(), torch.zeros(C, FF - C)], 1).contiguous()
        b1, b2 = torch.zeros(FF), torch.zeros(C)
        x = c.x
        if variant == 'tail':
            wo, permo, val = signed_perm(C, 72 + seed, exps=(0, 1))
            xa, proj, _ = NC.split_ab(c.x, torch.bfloat16 if b16 else torch.float32, torch.bfloat16)
            x, proj = xa.float(), proj.float()
            a = torch.zeros(M, C)
            a[:, permo] = proj / val
            bo = torch.zeros(C)
            assert torch.equal(a @ wo.t(), proj) and torch.equal(rb(a), a) and max(a.abs().max(), x.abs().max()) < 4094
    else:
        x = q(r(M, C))
        w1, b1, w2, b2 = r(FF, C, k=1 / 16), r(FF, k=0.5), r(C, FF, k=FF ** -0.5), r(C, k=0.5)
        if variant == 'tail':
            a, wo, bo = q(r(M, C)), r(C, C, k=1 / 16), r(C, k=0.5)
    if variant == 'tail':
        norm0 = _norm(r)
        if cond == 'second':            # x1 = 64 + 2^-10 (..): LayerNorm 1 sees off-centre, tight sums x1 - relu(x1) / 2 = x1 / 2
            norm0 = (2.0 ** -10 * norm0[0], torch.full((C,), 64.0), norm0[2])
    if kind == 'x3a':
        x = x3a_values(x)
    norm1 = _norm(r)
    B = 1
    if levels is not None:
        B, level_hw = levels
        assert M == B * sum(h * w for h, w in level_hw) == B * pos_rows
        shift = r(pos_rows, C)
    o = types.SimpleNamespace(x=x, a=a, wo=wo, bo=bo, norm0=norm0, w1=w1, b1=b1, w2=w2, b2=b2, norm1=norm1, pos=r(pos_rows, C),
                              shift=shift, fam=fam, levels=levels)

    def spec_of(w, r32):
        idx = pos_index(M, pos_rows)
        p = o.pos.double().abs()[idx]
        g1, _, eps1 = norm1
        _, _, var = NC.two_pass(w['t1'], eps1)
        slope = g1.double().abs() / torch.sqrt(var + eps1)
        # the sum LayerNorm 1 normalises holds operands that were ROUNDED on the way (bf16: the hidden block, and x1 when the
        # kernel formed it) or split (x3): one such operand on the other neighbour moves the sum by flip_term / by x1's own rounding
        wide = gemm_opnd(w['h'], w2, ak) + flip_term(w['h'], w2, ak)
        if b16 and variant == 'tail':
            wide = wide + 2.0 ** -8 * w['x1'].abs() + flip_term(w['x1'], w1, ak) @ rb(w2.double()).abs().t()
        T = ln_T(w['t1'], norm1) + slope * wide
        sp = {}

        def put(name, want, ref, Tn):
            if b16:
                sp[name + '32'] = Spec(want, ref, Tn)
                sp[name + '16'] = Spec(want, ref, Tn, bf16_rounding(want))
            else:
                sp[name] = Spec(want, ref, Tn, U_X3 * want.abs() if kind == 'x3a' else 0.0)
        put('y', w['y'], r32['y'], T)
        put('yp', w['yp'], r32['yp'], T + U_F32 * p)
        if shift is not None:
            sh = o.shift.double().abs()[idx]
            put('m', w['m'], r32['m'], T + U_F32 * sh)
            put('mp', w['mp'], r32['mp'], T + U_F32 * (sh + p))
        return sp
    # per-family conditioning bound on y: where nothing in front of LayerNorm 1 is rounded (the bf16 tail rounds x1)
    lns = {'y32' if b16 else 'y': (norm1, 't1')} if variant == 'ffn' or not b16 else {}
    case = _finish(o, ak, chain_enc, spec_of, lns)
    case.b16 = b16
    return case


def enc_outs(case, y, y16=None, yp=None, m=None, mp=None):
    """the outputs of an encoder kernel under the names of the case's spec (bf16 kernels: y in f32 is 'y32', the others are bf16)"""
    if case.b16:
        named = dict(y32=y, y16=y16, yp16=yp, m16=m, mp16=mp)
    else:
        named = dict(y=y, yp=yp)
    return {k: v for k, v in named.items() if v is not None}
