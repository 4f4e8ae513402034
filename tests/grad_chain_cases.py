"""Exact operands for the training backward chain of parity mode. Host only: builders and float64 references, no kernel.

    add_layernorm_backward(want_amax)               -> dz, max |dz|       csrc/ln_bwd.hip
      wgrad_x3(dz, h, want_bias, amax)              -> dW2, db2           csrc/wgrad_x3.hip  (cgg_wgrad_x3_scaled)
      gemm_x3_bwd(dz, W2^T, amax, mask=h, want_amax)-> dh, max |dh|       csrc/x3_gemm.hip   (cgg_gemm_x3_bwd)
        wgrad_x3(dh, x, want_bias, amax_h)          -> dW1, db1
        gemm_x3(dh, W1^T, res=dz, amax=amax_h)      -> dx

tests/test_grad_chain_cases.py proves on the CPU what is derived here; tests/test_grad_chain_edges_gpu.py then asserts every bit.

THE ARITHMETIC (csrc/x3.h). An f32 operand a is pre-scaled by a power of two s and split into f16 pieces hi = f16(s a),
lo = f16(s a - hi); a product is al bh + ah bl + ah bh in the MFMA's f32 accumulator, and the epilogue un-scales by powers of two.
s = 2^4 for activations and 2^7-class row scales for packed weights; for a gradient operand with a known maximum it is
`x3_scale(amax)` = 2^(9 - floor(log2 amax)), exponent clamped to +-100, and 2^4 when amax is 0, denormal or not finite.

OPERANDS. I = integers in [-15, 15] (4 bits).
  g, dy   I x 2^p (one p per tensor), optionally x 2^-(r % 4) per row r ("row factors"); element [0][0] is 15 x 2^p, so amax = 15 x 2^p
  x, h    I; as a mask h also holds 0.0, -0.0, negative values, whole zero rows (r % 61 == 3) and whole zero columns (c % 29 == 5)
  W       I with an entry of magnitude >= 8 in every row and every column: max |w| of a row lies in [8, 16), so the packer's row
          scale is 2^7 for W and for W^T (frexp exponent 4 -> 2^(11 - 4)) and 2^7 w <= 1920 is an exact f16
  r       I (the residual of gemm_x3(res=))

FIT (no rounding when the pieces are made). floor(log2 (15 x 2^p)) = p + 3, so s = 2^(6 - p) while |6 - p| <= 100, and
s g = I x 2^6 x 2^-(r % 4): at most 4 significant bits, between 2^3 and 960 -- an exact normal f16 with an EMPTY low piece. x and h
are scaled by 2^4: 16 I <= 240, exact. p = -110 clamps the exponent to 100: s g = I x 2^-10 x 2^-(r % 4) >= 2^-13. That is still a
NORMAL f16 (the smallest is 2^-14), so p = -110 tests the clamp and its matching un-scale but not subnormal operands; p = -118 is
added for those: s g = I x 2^-18 x 2^-(r % 4) lies in [2^-21, 15 x 2^-18], all below 2^-14 and all multiples of the subnormal
unit 2^-24 -- exact f16 subnormals, which x3.h documents as produced by the conversion and consumed by the MFMA without flushing.
Every f32 value involved stays normal (2^-121 at the smallest). An all-zero g has amax = 0, hence s = 2^4, hence zero pieces.
The CPU test makes the pieces with torch's f16 conversion (round to nearest even, subnormals kept) and asserts hi == s a, lo == 0.

SUMS (no rounding in the accumulator, in any order). With empty low pieces a product is ah bh alone: an integer multiple of the
product of the two units, of magnitude at most 225 units x 2^3 (the row factors make the smallest unit 2^-3 of the largest).
  GEMM  out[m][n] = sum_k g[m][k] w[n][k]: the row factor is common to the K terms, so |partial sum| <= K x 225 units; K <= 288
        gives 64 800 < 2^24: every partial sum in every order is an integer below 2^24 in its unit, i.e. an exact f32.
  wgrad dW[n][k] = sum_m dy[m][n] x[m][k]: the row factors differ between terms: |partial sum| <= M x 225 x 2^3 smallest units,
        below 2^24 while M <= 9320 (M_CAP_WGRAD; 9320 x 1800 = 16 776 000 < 16 777 216). The largest M used is 1000.
  bias  db[n] = sum_m dy[m][n], plain f32 adds: M x 15 x 2^3 units, far below 2^24.
The float64 matmul is therefore THE result, not an approximation of it; the CPU test shows it equal to f32 matmuls in two different
summation orders, and equal again after the power-of-two un-scale. No tolerance appears in the GPU tests of these cases.

CHAIN (amax hand-off). dh = mask(dz W2) holds integers up to 32 x 225 = 7200 (13 bits) x 2^p: too wide for one f16, but
s dh = hi + lo EXACTLY with s = x3_scale(max |dh|) -- 11 bits in hi, the rest (<= 4 bits, far above 2^-24) in lo -- and x has an empty
low piece, so the dropped al bl term is zero and every product (ah + al) bh is exact. The sum bound is data dependent there and is
proven from the data: sum_m |dh[m][n]| |x[m][k]| < 2^24 units for every (n, k) (70 x 7200 x 15 = 7 560 000 at the worst).

TILES. `xg_tiles` restates xg_launch's choice of the workgroup tile (64 tm x 64 tn) and `wgrad_plan` restates csrc/wgrad_x3.hip's
split of the rows; the CPU test pins the expected values per case. With the rule as it stands the interior form of the generic
epilogue (full tile, but no buffer-store fast path) needs a periodic residual or an operand of 4 GiB, neither of which
cgg_gemm_x3_bwd can have at test size: the mask forms reached are the buffer-store form (interior tiles) and the per-element form
with tiles ragged in M and tiles ragged in N.

OBSERVED on MI355X: every case below, p = -110 and p = -118 included, returned the float64 result bit for bit; the f16 subnormal
operands of p = -118 are consumed unflushed, as x3.h says."""
import functools
import struct
from types import SimpleNamespace

import torch

INT = 15
P_SET = (-40, -20, 0, 20, 40)
P_CLAMP = -110                      # exponent clamped to 100; pre-scaled values still normal f16
P_SUBNORMAL = -118                  # exponent clamped to 100; pre-scaled values on the f16 subnormal grid
P_ALL = P_SET + (P_CLAMP, P_SUBNORMAL)
M_CAP_WGRAD = 9320                  # M x 225 x 2^3 < 2^24
ASCALE = 16.0


# ------------------------------------------------------------------------------------------------
# restated rules
# ------------------------------------------------------------------------------------------------
def x3_scale(amax):
    """cgg_x3_scale_from_amax (csrc/x3.h) on the bits of the f32 `amax`"""
    b = struct.unpack('<I', struct.pack('<f', amax))[0]
    e = (b >> 23) & 0xff
    if e == 0 or e == 255:
        return ASCALE
    se = 9 - (e - 127)
    se = 100 if se > 100 else (-100 if se < -100 else se)
    return 2.0 ** se


def xg_tiles(M, N):
    """xg_launch (csrc/x3_gemm.hip): the largest tile (tm, tn) whose grid still has 192 workgroups"""
    tiles = lambda tm, tn: -(-M // (64 * tm)) * -(-N // (64 * tn))      # noqa: E731
    tm, tn = 2, (1 if N <= 64 else 2)
    if tiles(tm, tn) < 192:
        tm = 1
    if tiles(tm, tn) < 192 and tn == 2:
        tn = 1
    return tm, tn


def xg_tile_forms(M, N):
    """{'interior', 'ragged_m', 'ragged_n'} that occur among the workgroup tiles of an (M, N) output (the kernel's `full` test)"""
    tm, tn = xg_tiles(M, N)
    bm, bn = 64 * tm, 64 * tn
    forms = set()
    for m0 in range(0, M, bm):
        for n0 in range(0, N, bn):
            fm, fn = m0 + bm <= M, n0 + bn <= N
            forms.add('interior' if fm and fn else None)
            if not fm:
                forms.add('ragged_m')
            if not fn:
                forms.add('ragged_n')
    forms.discard(None)
    return forms


def wgrad_tile(N, K):
    return 256 if N % 256 == 0 and K % 256 == 0 else 128


def wgrad_plan(M, N, K):
    """csrc/wgrad_x3.hip -> (splits, rows_per_split)"""
    bt = wgrad_tile(N, K)
    tiles = -(-N // bt) * -(-K // bt)
    sp = ((768 if bt == 128 else 256) + tiles - 1) // tiles
    sp = max(1, min(sp, (M + 255) // 256))
    rps = (-(-M // sp) + 31) // 32 * 32
    return -(-M // rps), rps


def wgrad_split_kind(M, N, K):
    """'one' split | 'full': several splits, every one of rows_per_split rows | 'ragged': several, the last one shorter"""
    sp, rps = wgrad_plan(M, N, K)
    return 'one' if sp == 1 else ('full' if sp * rps == M else 'ragged')


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def ints(shape, gen, top=INT):
    return torch.randint(-top, top + 1, shape, generator=gen).float()


def weight(N, K, seed):
    """(N, K) integers with |w| >= 8 somewhere in every row and every column"""
    w = ints((N, K), _gen(1, N, K, seed))
    n, k = torch.arange(N), torch.arange(K)
    w[n, n % K] = (8 + n % 8).float() * (1 - 2 * (n % 2)).float()
    w[k % N, k] = (15 - k % 8).float() * (2 * (k % 2) - 1).float()
    return w


def grad(M, K, p, seed, row_factors=True):
    """(M, K) integers x 2^p (x 2^-(r % 4) per row); [0][0] = 15 x 2^p is the maximum. p None: all zero"""
    if p is None:
        return torch.zeros(M, K)
    g = ints((M, K), _gen(2, M, K, seed))
    g[0, 0] = INT
    g = g * 2.0 ** p
    if row_factors:
        g = g * (2.0 ** -(torch.arange(M) % 4).float()).view(M, 1)
    return g


def mask(M, N, seed):
    """integers with 0.0 and -0.0, negative values, whole zero rows (r % 61 == 3) and whole zero columns (c % 29 == 5)"""
    h = ints((M, N), _gen(3, M, N, seed))
    r, c = torch.arange(M).view(M, 1), torch.arange(N).view(1, N)
    h[(r % 61 == 3).expand(M, N)] = 0.0
    h[(c % 29 == 5).expand(M, N)] = 0.0
    h[(h == 0) & ((r + c) % 2 == 1)] = -0.0
    return h


# ------------------------------------------------------------------------------------------------
# 1. gemm_x3_bwd / gemm_x3(res=)
# ------------------------------------------------------------------------------------------------
#               M      N    K   (tm, tn)
GEMM_SPECS = {
    't22': (12200, 256, 32, (2, 2)),         # 96 row tiles, the last with 40 rows
    't12': (6100, 256, 32, (1, 2)),
    't21': (24500, 36, 32, (2, 1)),          # ragged N inside one tile
    't11': (70, 100, 32, (1, 1)),
    't11_one_row': (1, 32, 32, (1, 1)),
    't11_k96': (70, 100, 96, (1, 1)),        # odd chunk counts: 3 ...
    't12_k288': (6100, 256, 288, (1, 2)),    # ... and 9 (the merged offsets | logits width)
    't11_interior': (128, 128, 32, (1, 1)),  # four tiles, all interior (gemm_x3(res=) in place)
}
GEMM_RAGGED_M = ('t22', 't12', 't21', 't11')       # the amax-edge variants
VARIANTS = ('plain', 'last_row_max', 'masked_last_row')


@functools.lru_cache(maxsize=None)
def gemm_case(name, p=0, variant='plain', row_factors=True):
    """g (M, K), w (N, K), mask (M, N), ref64 = g w^T (float64), amax = max |g|.
    last_row_max: row M - 1 of g is 15 sign(w[n*]) -- the largest product any row can form -- and mask[M - 1][n*] > 0: the maximum of
        the output sits in the last live row.
    masked_last_row: the same row, but mask[M - 1] is a whole zero row: the output's maximum lies elsewhere, and a kernel that
        counted the clamped duplicates of row M - 1 (rows past M read row M - 1) under the live rows of a taller mask buffer
        (`mask_tall`: rows past M all positive) would report the dominating value."""
    M, N, K, _ = GEMM_SPECS[name]
    g, w, h = grad(M, K, p, 11, row_factors), weight(N, K, 12), mask(M, N, 13)
    if variant != 'plain':
        assert p is not None and M > 1
        nstar = int(w.abs().sum(1).argmax())
        sgn = torch.where(w[nstar] < 0, -1.0, 1.0)
        g[M - 1] = INT * sgn * 2.0 ** p
        h[M - 1] = torch.where(torch.arange(N) % 2 == 0, 0.0, -0.0) if variant == 'masked_last_row' else h[M - 1]
        if variant == 'last_row_max':
            h[M - 1, nstar] = 7.0
    ref64 = g.double() @ w.double().t()
    tall = torch.ones(M + 160, N)
    tall[:M] = h
    return SimpleNamespace(name=name, M=M, N=N, K=K, p=p, g=g, w=w, mask=h, mask_tall=tall, ref64=ref64,
                           ref_masked64=torch.where(h > 0, ref64, torch.zeros((), dtype=torch.float64)),
                           amax=float(g.abs().max()), res=ints((M, N), _gen(4, M, N)))


# ------------------------------------------------------------------------------------------------
# 2. wgrad_x3 (scaled)
# ------------------------------------------------------------------------------------------------
WGRAD_NK = ((256, 256),        # 256-wide tile, two LDS stages
            (128, 128),        # 128-wide, interior buffer-store path
            (288, 256),        # 128-wide, ragged N tile
            (36, 68))          # ragged on both sides
# 512 is the one row count here that gives several FULL splits (256 rows is the smallest split, so no smaller count can)
WGRAD_M = (1, 31, 32, 33, 256, 257, 300, 512, 1000)


@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K, p=0):
    """dy (M, N) with row factors, x (M, K); dw64 = dy^T x, db64 = column sums of dy (float64)"""
    dy, x = grad(M, N, p, 21), ints((M, K), _gen(5, M, K))
    return SimpleNamespace(M=M, N=N, K=K, p=p, dy=dy, x=x, dw64=dy.double().t() @ x.double(), db64=dy.double().sum(0),
                           amax=float(dy.abs().max()))


def split_pieces(a, s):
    """(hi, lo) of the f32 tensor a pre-scaled by s, as float64: hi = f16(s a), lo = f16(s a - hi)"""
    t = (a.double() * s).float()
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi.double(), lo.double()


def selector_case(M, N, K, mag, seed=31):
    """x one-hot per column (column k selects row m_k = (7 k + 3) % M), dy = randn x mag: dW[n][k] is the split of dy[m_k][n] alone"""
    gen = _gen(6, M, N, K, seed)
    dy = torch.randn(M, N, generator=gen) * mag
    rows = (7 * torch.arange(K) + 3) % M
    x = torch.zeros(M, K)
    x[rows, torch.arange(K)] = 1.0
    return SimpleNamespace(dy=dy, x=x, rows=rows)


def selector_ref(case, s):
    hi, lo = split_pieces(case.dy[case.rows], s)          # (K, N)
    return ((hi + lo) / s).float().t().contiguous()


# ------------------------------------------------------------------------------------------------
# 3. add_layernorm_backward
# ------------------------------------------------------------------------------------------------
LN_ROWS = (1, 16, 17, 255, 256, 257, 513)
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(rows):
    """b: multiples of 2^-6 below 4 (8 bits: bf16); a: multiples of 2^-10 below 8; s = a + b is exact (14 bits) in f32.
    dy = d32 + d16a + d16b, each a multiple of 2^-6 below 4 (bf16; the sum has 10 bits: exact in any order). The LAST row of every
    piece is the largest in its tensor by a factor of 2 or more (|k| in [192, 255] against <= 96 elsewhere): a clamped duplicate of
    it in dgamma / dbeta / the maximum is far outside any bound."""
    gen = _gen(7, rows)
    N = 256
    b = torch.randint(-255, 256, (rows, N), generator=gen).float() / 64
    a = torch.randint(-8191, 8192, (rows, N), generator=gen).float() / 1024
    gamma = 1 + 0.25 * torch.randn(N, generator=gen)
    beta = 0.1 * torch.randn(N, generator=gen)
    pieces = []
    for _ in range(3):
        d = torch.randint(-96, 97, (rows, N), generator=gen).float()
        d[rows - 1] = torch.randint(192, 256, (N,), generator=gen).float() * (1 - 2 * torch.randint(0, 2, (N,), generator=gen)).float()
        pieces.append(d / 64)
    return SimpleNamespace(rows=rows, a=a, b=b, s=a + b, gamma=gamma, beta=beta, d32=pieces[0], d16a=pieces[1], d16b=pieces[2],
                           dy=pieces[0] + pieces[1] + pieces[2])


# ------------------------------------------------------------------------------------------------
# 4. chain: gemm_x3_bwd -> wgrad_x3, amax handed from epilogue to pre-scale
# ------------------------------------------------------------------------------------------------
CHAIN_KX = 68
CHAIN_P = (0, -20)


@functools.lru_cache(maxsize=None)
def chain_case(p):
    """the (70, 100, 32) case of part 1 without row factors: dh64 = mask(dz W2), then dw1 = dh^T x, db1 = column sums of dh"""
    c = gemm_case('t11', p, 'plain', row_factors=False)
    x = ints((c.M, CHAIN_KX), _gen(8, c.M))
    dh = c.ref_masked64
    return SimpleNamespace(c=c, x=x, dh64=dh, amax_h=float(dh.abs().max()), dw1=dh.t() @ x.double(), db1=dh.sum(0))
