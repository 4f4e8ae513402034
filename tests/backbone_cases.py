"""Operands, float64 references and conditions for the throughput-mode (bf16) ResNet kernels: stem_conv7x7 (csrc/stem_conv.hip),
bottleneck64 (csrc/bottleneck.hip), bias_relu_maxpool_nhwc / _f32 / _f32 x3a, im2col3x3_nhwc, subsample_nhwc, bias_act_nhwc_
(csrc/epilogue.hip) and the library GEMM behind gemm_bias_res_act_bf16. Plain torch on the CPU, no project kernel.
tests/test_backbone_cases.py shows that this module delivers what it claims; tests/test_backbone_edges_gpu.py runs the kernels.

EXACT OPERANDS. The bf16 kernels multiply bf16 operands exactly in f32 and accumulate in f32. When every operand, every intermediate
the kernel rounds to bf16 (t1, t2 of the bottleneck) and every output is an integer of magnitude <= 256, every partial sum is an
integer below 2^24, f32 accumulation in ANY order is exact, every bf16 rounding is the identity (bf16 holds the integers up to 256),
and the kernel must equal the float64 reference bit for bit: the GPU tests use torch.equal, no tolerance. Each generator asserts
  (a) reference and rounded intermediates integer-valued, |.| <= 256, unchanged by a bf16 round trip (`assert_exact`);
  (b) for the sparse-integer cases, at least a quarter of every ReLU output positive (`assert_live`), so that a ReLU which zeroes
      everything cannot pass. (The coded cases below are mostly zero by design -- an impulse answers with one tap -- and are held to
      (a) only; the stem kernel's output is the RAW convolution, it has no ReLU.)
  sparse bottleneck: x in [-2, 2]; w1 (64 x 256) 8 nonzeros per row, w2 (64 x 64 x 3 x 3) 8 per output channel, w3 (256 x 64) 4 per
                     row, all +-1; b1 in [-2, 3], b2 in [-3, 3], b3 in [-4, 4].
  sparse stem:       image in [-4, 4]; 24 nonzero taps per output channel from {+-1, +-2}.
  sparse GEMM:       x in [-2, 2], 8 nonzeros +-1 per weight row, bias in [-2, 3], residual in [-4, 4].

CODED WEIGHTS, so that a failure names the tap:
  stem, tap-coded      w[co, c, ky, kx] = 1 + c + 3 (kx + 7 ky) <= 147, the same for every co: the answer to an impulse IS (c, ky, kx).
  stem, channel-coded  w[co, c0, ky0, kx0] = co + 1 on one tap: pins the output-channel order of the packed A fragments.
  impulse images       one image per (position, channel) with a single 1: every corner, the middle of every edge, the centre, and
                       the pixels on both sides of every tile boundary (`impulse_positions`), stacked as ONE batch (>= 2 images, so
                       an image boundary falls inside the grid).
  bottleneck 'taps'    w1 one-hot (t1[m] = x[4 m] + b1), b1 = 1 > 0, w2[co, (5 co + 3) % 64, ky, kx] = 1 + 3 ky + kx: t1 = relu(b1) = 1
                       everywhere inside the image, so t2 is the sum of the tap codes that fall INSIDE the image (45 in the interior)
                       -- any t1 that is not zero in conv2's padding changes a border sum -- plus the code of the tap that meets
                       the impulse.
  bottleneck 'chan'    the same t1; w2[0, :, ky0, kx0] = 1 sums one tap over all 64 channels, b2[0] = -64: t2[0] is 1 on the pixel whose
                       tap meets the impulse and 0 elsewhere; w3[co, 0] = co + 1: the answer is co + 1 in channel co, which pins
                       the row permutation of ops.pack_bottleneck64.

MAPS, the smallest at which the tiling can go wrong, B = 2 (STEM_MAPS, BOTTLENECK_MAPS, POOL_MAPS, PATCH_MAPS, BIAS_ACT_SHAPES).
Geometry notes (tests/test_backbone_cases.py checks them): the stem's window (7 wide, stride 2, padding 3) hangs over the top / left
by 3 - 2 o, i.e. by 3 or 1 only -- by 2 never; over the bottom / right by 1, 2 and 3. The centre tap of a 3 x 3 / padding-1 window is
never outside the map; the other 8 are.

X3A RANGE. cgg_bias_relu_maxpool_nhwc_f32 with x3a=True encodes its outputs as x3a rows: the encoder needs finite values v with
16 |v| inside f16's range (|v| < 4094, the bound of the x3 overflow flag); the outputs are >= 0 after the ReLU. `pool_case` keeps them
there and asserts it.

YARDSTICK for the outputs that are not exact (x3 stem, model level): err <= 4 e_ref + 2e-7 scale, e_ref = the error of torch's own
f32 formulation on the CPU against float64, scale = the largest reference magnitude (tests/test_x3s_gpu.py,
tests/test_conv3x3_halo_gpu.py use the same rule). An x3a output adds the format's storage term scale 2^-21 + 2^-28."""
import types

import torch
import torch.nn.functional as F

B = 2
STEM_TILE = (8, 32)                 # outputs per workgroup
BOTTLENECK_TILE = (8, 16)
STEM_MAPS = [(1, 1), (2, 3), (6, 6), (7, 7), (15, 63), (16, 64), (17, 65), (33, 130)]
BOTTLENECK_MAPS = [(8, 16), (8, 32), (16, 16), (16, 32), (24, 48)]
BOTTLENECK_OFF = [(7, 16), (9, 16), (8, 15), (8, 17), (16, 24), (12, 32)]     # H % 8 or W % 16 != 0: bottleneck64_ok is false
POOL_MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (4, 4), (9, 7), (18, 22)]
POOL_C = (8, 64)
PATCH_MAPS = [(1, 1), (1, 4), (4, 1), (2, 2), (3, 3), (5, 8), (7, 9)]
PATCH_C = (8, 24)
IM2COL_STRIDES = (1, 2)
SUBSAMPLE_STRIDES = (1, 2, 3)
BIAS_ACT_GRID = 8192 * 256          # vectors one trip of cgg_bias_act_kernel's grid-stride loop covers
# (rows, C): a small control, then totals just over the grid cap with 3 and 24 vectors per row (neither divides 2^21)
BIAS_ACT_SHAPES = [(126, 24), (87382, 192), (699051, 24)]
# (bias, res, relu): the five of tests/test_kernels_gpu.py, + (bias, no res, no relu) and (no bias, res, no relu)
BIAS_ACT_COMBOS = [(True, True, True), (True, False, True), (False, True, True), (True, True, False), (False, False, True),
                   (True, False, False), (False, True, False)]
GEMM_M, GEMM_N, GEMM_K = (1, 37, 520), (64, 72), (64, 576)
STEM_CHANNEL_TAPS = [(0, 0, 0), (1, 3, 4), (2, 6, 6)]      # (c, ky, kx) of the channel-coded stem filters
MODEL_IMAGES = [(64, 128), (70, 100)]                       # layer1 map 16 x 32 (bottleneck64) / 18 x 25 (three calls)
X3A_MAX = 4094.0


def rb(t):
    """round to bf16, back in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def assert_exact(t, what):
    t = t.double()
    assert torch.isfinite(t).all(), what
    assert torch.equal(t, t.round()), what + ': not integer-valued'
    assert t.abs().max().item() <= 256, what + ': magnitude %g > 256' % t.abs().max().item()
    assert torch.equal(rb(t), t), what + ': changed by a bf16 round trip'


def assert_live(t, what):
    frac = (t > 0).double().mean().item()
    assert frac >= 0.25, what + ': only %.3f of the ReLU output is positive' % frac


def yardstick(e_ref, scale):
    return 4 * e_ref + 2e-7 * scale


def x3a_storage(scale):
    return scale * 2.0 ** -21 + 2.0 ** -28


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _sparse(g, rows, cols, nnz, values):
    """(rows, cols): `nnz` entries per row, drawn from `values`"""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    vals = torch.tensor(values, dtype=torch.float64)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nnz]
        w[r, idx] = vals[torch.randint(0, len(values), (nnz,), generator=g)]
    return w


def impulse_positions(H, W, th, tw):
    """corners, edge middles, the 2 x 2 block at the centre (both parities of both coordinates: a stride-2 window meets an impulse
    only with the taps of its parity), and the pixels on both sides of every tile boundary (tiles of th x tw INPUT pixels): on the
    middle of the other axis and on the diagonal"""
    ys = {0, H // 2, H - 1}
    xs = {0, W // 2, W - 1}
    pos = {(y, x) for y in ys for x in xs}
    pos |= {(y, x) for y in (H // 2, H // 2 + 1) for x in (W // 2, W // 2 + 1) if y < H and x < W}
    by = [y for k in range(1, H // th + 1) for y in (k * th - 1, k * th) if y < H]
    bx = [x for k in range(1, W // tw + 1) for x in (k * tw - 1, k * tw) if x < W]
    pos |= {(y, W // 2) for y in by} | {(H // 2, x) for x in bx}
    pos |= {(y, x) for y, x in zip(by, bx)}
    pos |= {(y, bx[0]) for y in by[:2] if bx} | {(by[0], x) for x in bx[:2] if by}
    return sorted(pos)


# ------------------------------------------------------------------------------------------------ stem
def stem_ref(img, w):
    """float64 raw 7 x 7 / stride 2 / padding 3 convolution, channel-last (B, Ho, Wo, 64)"""
    return F.conv2d(img.double(), w.double(), None, stride=2, padding=3).permute(0, 2, 3, 1).contiguous()


def stem_tap_coded():
    c = torch.arange(3).view(3, 1, 1)
    ky = torch.arange(7).view(1, 7, 1)
    kx = torch.arange(7).view(1, 1, 7)
    w = (1 + c + 3 * (kx + 7 * ky)).double()
    assert w.max().item() == 147 and w.unique().numel() == 147
    return w.expand(64, 3, 7, 7).contiguous()


def stem_channel_coded(tap):
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
    w[:, tap[0], tap[1], tap[2]] = torch.arange(1, 65).double()
    return w


def stem_impulses(H, W):
    """(N, 3, H, W) f32: one image per (position, channel), N >= 2; -> (images, [(c, y, x)])"""
    pos = impulse_positions(H, W, 2 * STEM_TILE[0], 2 * STEM_TILE[1])
    keys = [(c, y, x) for (y, x) in pos for c in range(3)]
    img = torch.zeros(len(keys), 3, H, W)
    for n, (c, y, x) in enumerate(keys):
        img[n, c, y, x] = 1.0
    assert img.shape[0] >= 2
    return img, keys


def stem_coded_case(H, W, which):
    """which = 'tap' or a (c, ky, kx) of STEM_CHANNEL_TAPS"""
    img, keys = stem_impulses(H, W)
    w = stem_tap_coded() if which == 'tap' else stem_channel_coded(which)
    ref = stem_ref(img, w)
    assert_exact(ref, 'stem coded %s %dx%d' % (which, H, W))
    return types.SimpleNamespace(img=img, w=w.float(), ref=ref, keys=keys)


def stem_exact_case(H, W, seed=0):
    g = torch.Generator().manual_seed(7000 + 131 * H + W + seed)
    img = _ints(g, (B, 3, H, W), -4, 4)
    w = _sparse(g, 64, 147, 24, (-2.0, -1.0, 1.0, 2.0)).view(64, 3, 7, 7)
    ref = stem_ref(img, w)
    assert_exact(img, 'stem image')
    assert_exact(w, 'stem filter')
    assert_exact(ref, 'stem exact %dx%d' % (H, W))
    return types.SimpleNamespace(img=img.float(), w=w.float(), ref=ref)


def stem_x3_case(H, W):
    """random normal operands of tests/test_x3_gpu.py's x3 stem test; float64 raw convolution and pooled map + torch's f32 error"""
    g = torch.Generator().manual_seed(7700 + 131 * H + W)
    img = torch.randn(B, 3, H, W, generator=g) * 2
    w = torch.randn(64, 3, 7, 7, generator=g) / 12
    w[::5] *= 1e-2
    b = torch.randn(64, generator=g)
    raw = F.conv2d(img.double(), w.double(), None, stride=2, padding=3)
    pooled = F.max_pool2d(torch.relu(raw + b.double().view(1, -1, 1, 1)), 3, 2, 1)
    raw32 = F.conv2d(img, w, None, stride=2, padding=3)
    e_ref = (raw32.double() - raw).abs().max().item()
    e_ref_pooled = (F.max_pool2d(torch.relu(raw32 + b.view(1, -1, 1, 1)), 3, 2, 1).double() - pooled).abs().max().item()
    assert pooled.max().item() < X3A_MAX
    return types.SimpleNamespace(img=img, w=w, b=b, raw=raw.permute(0, 2, 3, 1).contiguous(),
                                 pooled=pooled.permute(0, 2, 3, 1).contiguous(), e_ref=e_ref, e_ref_pooled=e_ref_pooled,
                                 raw_scale=raw.abs().max().item(), pooled_scale=pooled.abs().max().item())


def stem_overhangs(H, W):
    """{(top, bottom, left, right)}: by how many pixels the 7 x 7 window of each output hangs over each side of the H x W image"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = set()
    for oy in range(Ho):
        for ox in range(Wo):
            out.add((max(0, 3 - 2 * oy), max(0, 2 * oy + 3 - (H - 1)), max(0, 3 - 2 * ox), max(0, 2 * ox + 3 - (W - 1))))
    return out


# ------------------------------------------------------------------------------------------------ bottleneck
def bottleneck_ref(x, w1, b1, w2, b2, w3, b3):
    """x (B, H, W, 256) -> (t1, t2, y) float64 channel-last, t1 / t2 rounded to bf16 where the kernel rounds them"""
    xd = x.double().permute(0, 3, 1, 2)
    t1 = rb(F.relu(F.conv2d(xd, w1.double().view(64, 256, 1, 1), b1.double())))
    t2 = rb(F.relu(F.conv2d(t1, w2.double(), b2.double(), padding=1)))
    y = F.relu(F.conv2d(t2, w3.double().view(256, 64, 1, 1), b3.double()) + xd)
    return tuple(t.permute(0, 2, 3, 1).contiguous() for t in (t1, t2, y))


def _bottleneck_ns(x, w1, b1, w2, b2, w3, b3, what, live):
    xd = x.double().permute(0, 3, 1, 2)
    raw1 = F.conv2d(xd, w1.view(64, 256, 1, 1), b1)
    t1, t2, y = bottleneck_ref(x, w1, b1, w2, b2, w3, b3)
    raw2 = F.conv2d(t1.permute(0, 3, 1, 2), w2, b2, padding=1)
    raw3 = F.conv2d(t2.permute(0, 3, 1, 2), w3.view(256, 64, 1, 1), b3) + xd
    for t, n in ((x, 'x'), (w1, 'w1'), (w2, 'w2'), (w3, 'w3'), (b1, 'b1'), (b2, 'b2'), (b3, 'b3'), (raw1, 'conv1'), (raw2, 'conv2'),
                 (raw3, 'conv3 + x'), (t1, 't1'), (t2, 't2'), (y, 'y')):
        assert_exact(t, what + ' ' + n)
    if live:
        for t, n in ((t1, 't1'), (t2, 't2'), (y, 'y')):
            assert_live(t, what + ' ' + n)
    return types.SimpleNamespace(x=x.to(torch.bfloat16), w1=w1.float(), b1=b1.float(), w2=w2.float(), b2=b2.float(), w3=w3.float(),
                                 b3=b3.float(), t1=t1, t2=t2, ref=y)


def bottleneck_exact_case(H, W, seed=0):
    g = torch.Generator().manual_seed(8000 + 131 * H + W + seed)
    x = _ints(g, (B, H, W, 256), -2, 2)
    w1 = _sparse(g, 64, 256, 8, (-1.0, 1.0))
    w2 = _sparse(g, 64, 576, 8, (-1.0, 1.0)).view(64, 64, 3, 3)
    w3 = _sparse(g, 256, 64, 4, (-1.0, 1.0))
    b1, b2, b3 = _ints(g, (64,), -2, 3), _ints(g, (64,), -3, 3), _ints(g, (256,), -4, 4)
    return _bottleneck_ns(x, w1, b1, w2, b2, w3, b3, 'bottleneck exact %dx%d' % (H, W), True)


def bottleneck_impulses(H, W):
    """(N, H, W, 256): a single 1 per image, at channel 4 ((7 n) % 64) (<= 252)"""
    pos = impulse_positions(H, W, *BOTTLENECK_TILE)
    x = torch.zeros(len(pos), H, W, 256, dtype=torch.float64)
    for n, (py, px) in enumerate(pos):
        x[n, py, px, 4 * ((7 * n) % 64)] = 1.0
    assert x.shape[0] >= 2
    return x, pos


def bottleneck_w2_tap_coded():
    w2 = torch.zeros(64, 64, 3, 3, dtype=torch.float64)
    code = (1 + 3 * torch.arange(3).view(3, 1) + torch.arange(3).view(1, 3)).double()
    for co in range(64):
        w2[co, (5 * co + 3) % 64] = code
    return w2


def bottleneck_w3_channel_coded():
    w3 = torch.zeros(256, 64, dtype=torch.float64)
    w3[:, 0] = torch.arange(1, 257).double()
    return w3


def bottleneck_coded_case(H, W, which, tap=(0, 2)):
    """which = 'taps' | 'chan' (see the module docstring); b1 = 1 > 0: relu(b1) is non-zero everywhere inside the image"""
    x, pos = bottleneck_impulses(H, W)
    w1 = torch.zeros(64, 256, dtype=torch.float64)
    w1[torch.arange(64), 4 * torch.arange(64)] = 1.0
    b1 = torch.ones(64, dtype=torch.float64)
    if which == 'taps':
        w2, b2 = bottleneck_w2_tap_coded(), torch.zeros(64, dtype=torch.float64)
        w3 = torch.zeros(256, 64, dtype=torch.float64)
        w3[torch.arange(256), (3 * torch.arange(256) + 1) % 64] = 1.0
        b3 = (torch.arange(256) % 4).double()
    else:
        # t2[0] = relu(sum over m of t1[m] at the pixel tap (ky, kx) points to - 64): 1 where the impulse is, 0 elsewhere
        w2 = torch.zeros(64, 64, 3, 3, dtype=torch.float64)
        w2[0, :, tap[0], tap[1]] = 1.0
        b2 = torch.zeros(64, dtype=torch.float64)
        b2[0] = -64.0
        w3, b3 = bottleneck_w3_channel_coded(), torch.zeros(256, dtype=torch.float64)
    ns = _bottleneck_ns(x, w1, b1, w2, b2, w3, b3, 'bottleneck %s %dx%d' % (which, H, W), False)
    assert (ns.t1 > 0).all()                     # relu(b1) > 0 on every pixel of the image: only the padding of conv2 is zero
    ns.pos = pos
    return ns


# ------------------------------------------------------------------------------------------------ pooling, patches, epilogue
def pool_case(H, W, C, kind, negative=False):
    """kind 'bf16': x, b bf16, reference max_pool2d(relu(bf16(x + b))) -- exact: rounding and ReLU are monotone, so pooling the raw
    map first (the kernel) gives the same bits. kind 'f32': x, b f32, reference max_pool2d(relu(x + b)) in f32, exact for the same
    reason (f32 addition of one b is monotone in x). `negative`: x + b < 0 everywhere, the output is all zero."""
    g = torch.Generator().manual_seed(8800 + 97 * H + 11 * W + C + (5 if negative else 0) + (1 if kind == 'f32' else 0))
    dt = torch.bfloat16 if kind == 'bf16' else torch.float32
    x = torch.randn(B, H, W, C, generator=g)
    b = torch.randn(C, generator=g)
    if negative:
        x, b = -x.abs() - 0.5, -b.abs()
    x, b = x.to(dt), b.to(dt)
    s = (x + b).to(dt)                                   # bf16: the library sequence's rounding of conv + bias
    if negative:
        assert (s.double() < 0).all()
    want = F.max_pool2d(s.relu().float().permute(0, 3, 1, 2), 3, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    assert torch.isfinite(want).all() and (want >= 0).all() and want.max().item() < X3A_MAX       # the x3a encoder's range
    return types.SimpleNamespace(x=x, b=b, want=want.to(dt))


def pool_window_counts(H, W):
    """{number of valid elements} over the 3 x 3 / stride 2 / padding 1 windows of an H x W map"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = [sum(0 <= 2 * o - 1 + d < H for d in range(3)) for o in range(Ho)]
    cols = [sum(0 <= 2 * o - 1 + d < W for d in range(3)) for o in range(Wo)]
    return {r * c for r in rows for c in cols}


def patch_case(H, W, C):
    g = torch.Generator().manual_seed(9000 + 97 * H + 11 * W + C)
    return torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)


def im2col_ref(x, stride):
    """(B Ho Wo, 9 C), columns (ky, kx, c), through F.unfold"""
    Bx, H, W, C = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    cols = F.unfold(x.permute(0, 3, 1, 2).float(), 3, padding=1, stride=stride)           # (B, C * 9, L)
    return cols.view(Bx, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(Bx * Ho * Wo, 9 * C).to(x.dtype), Ho, Wo


def im2col_taps_outside(H, W, stride):
    """{tap}: taps (3 ky + kx) that fall outside the H x W map for at least one output row"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = set()
    for oy in range(Ho):
        for ox in range(Wo):
            for tap in range(9):
                iy, ix = oy * stride + tap // 3 - 1, ox * stride + tap % 3 - 1
                if not (0 <= iy < H and 0 <= ix < W):
                    out.add(tap)
    return out


def bias_act_case(rows, C, seed=0):
    g = torch.Generator().manual_seed(9300 + C + seed)
    y = torch.randn(rows, C, generator=g).to(torch.bfloat16)
    b = torch.randn(C, generator=g).to(torch.bfloat16)
    r = torch.randn(rows, C, generator=g).to(torch.bfloat16)
    return y, b, r


def bias_act_ref(y, bias, res, relu):
    """the torch sequence with the kernel's rounding points: bf16 after the bias add, then residual and ReLU in f32, one final
    rounding"""
    t = y.float()
    if bias is not None:
        t = (t + bias.float()).to(torch.bfloat16).float()
    if res is not None:
        t = t + res.float()
    if relu:
        t = t.relu()
    return t.to(torch.bfloat16)


def gemm_exact_case(M, N, K, has_res, relu):
    g = torch.Generator().manual_seed(9500 + 7 * M + 3 * N + K)
    x = _ints(g, (M, K), -2, 2)
    w = _sparse(g, N, K, 8, (-1.0, 1.0))
    b = _ints(g, (N,), -2, 3)
    r = _ints(g, (M, N), -4, 4) if has_res else None
    raw = x @ w.t() + b + (r if has_res else 0)
    want = raw.relu() if relu else raw
    assert_exact(raw, 'gemm %d %d %d' % (M, N, K))
    if relu and M * N >= 64:
        assert_live(want, 'gemm %d %d %d' % (M, N, K))
    bf = lambda t: None if t is None else t.to(torch.bfloat16)
    return types.SimpleNamespace(x=bf(x), w=bf(w), b=bf(b), r=bf(r), want=want)


# ------------------------------------------------------------------------------------------------ model level
def randomise_bn(model, seed=3):
    """BN statistics as tests/test_kernels_gpu.py::test_bias_act_nhwc_and_folded_backbone randomises them"""
    torch.manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)


def folded_resnet_ref(model, folded, img):
    """float64 convolutions on the folded bf16 weights `folded` (the model's own list [(w4 | None, b, w2 | None)] in execution
    order, on the CPU), bf16 rounding after every convolution's bias / residual / ReLU and after the stem's max-pool; the image is
    rounded to bf16 as the stem kernel stages it. -> the stage outputs (B, C, H, W) float64 for model.out_indices."""
    seq = iter(folded)

    def conv(x, c, relu, res=None):
        w4, b, w2 = next(seq)
        w = (w4 if w4 is not None else w2.view(w2.shape[0], w2.shape[1], 1, 1)).double()
        y = F.conv2d(x, w, b.double(), stride=c.stride, padding=c.padding, dilation=c.dilation, groups=c.groups)
        if res is not None:
            y = y + res
        return rb(y.relu() if relu else y)

    x = conv(rb(img.double()), model.conv1, True)
    x = rb(F.max_pool2d(x, 3, 2, 1))
    outs = []
    for i, name in enumerate(model.res_layers):
        for blk in getattr(model, name):
            identity = x if blk.downsample is None else conv(x, blk.downsample[0], False)
            y = conv(x, blk.conv1, True)
            if hasattr(blk, 'conv3'):
                y = conv(y, blk.conv2, True)
                x = conv(y, blk.conv3, True, identity)
            else:
                x = conv(y, blk.conv2, True, identity)
        if i in model.out_indices:
            outs.append(x)
    return outs
