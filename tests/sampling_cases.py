"""Inputs on which the GEOMETRY of the two bilinear sampler families matters -- MSDeformAttn (csrc/msda.hip, msda_bwd.hip) and the
point samplers (cgg_point_sample_* in csrc/postproc.hip, mask_logits.hip) --, their float64 references and the bound their outputs
are held to. Plain torch on the CPU.

MSDeformAttn cases (`Msda`; H = 8 heads of D = 32 channels, P = 4 points, queries == the pixels of the pyramid):

  A  `off_lattice`   reference point + uniform +-4.5 px, mixed with locations uniform in [-0.2, 1.2]; the reference is float64
                     autograd of the op's definition; a grad_loc element is left out only where, in float64, a pixel coordinate
                     of its sample is within EXCLUDE_PX of an integer (`near_integer`) -- d out / d loc jumps there
  B  `lattice`       every pixel coordinate on the half-integer lattice -1.5 .. W + 0.5: exactly -1 (skipped), -0.5, 0, interior
                     integers and half-integers, W - 1 (right neighbour outside), W - 0.5, W (skipped), in every (x, y)
                     combination on every level (`lattice_classes`). On a pyramid of powers of two the coordinates, the fractions
                     and `ref + off / W` are exact in f32 (`exact`); on any other pyramid the points are nominal (f32 may floor the
                     other way) and only out / grad_value / grad_attn, which are continuous across the lattice, are compared
  C                  A and B on pyramids with one-row / one-column levels
  D  `collide`       every sample of the finest level inside ONE cell of it (the longest record list per pixel), the coarser
                     levels on the quarter-pixel lattice; `outside`: every sample outside every map -> four outputs of zeros
  E  `threshold`     small offsets, then a chosen number of one tile's samples moved far away inside the same level, so that
                     the tile's out-of-window corner count is exactly 255 / 256 (MSDA_DEFER_MIN) and a second-pass region's
                     deferred total exactly 767 / 768 (MSDA_LIGHT_MAX): `scatter_counts` / `deferred_totals` state the geometry
  F  `with_inf_row`  A with one query's grad_out row = +inf

`msda_closed_form` is mmcv's rule in float64 (the sample is skipped unless -1 < y H - 0.5 < H and -1 < x W - 0.5 < W; four integer
neighbours, those outside the map dropped). It is the reference wherever a coordinate may sit ON the lattice: float64 autograd of
`oracle.ops.msda_core` (F.grid_sample) equals it to 1e-10 everywhere except at a pixel coordinate of exactly -1, where grid_sample
keeps a one-sided grad_loc and the op's rule skips the sample (tests/test_sampling_cases.py shows both).

`sample_ratios` states the bound, per family of samples (level x kind of location) and with no element left out but A's:

    |got - want| <= FACTOR * max(e_ref, U * S)            FACTOR = norm_cases.FACTOR = 8, U = 2^-24

e_ref: the largest error over the family of torch's own f32 autograd of `msda_core` on the CPU (off-lattice cases); on lattice
cases, where f32 autograd and float64 agree but for the summation over the channels, of the closed form evaluated in f32.
S, per element, is the sum of the absolute values of the terms an f32 implementation forms for it (`_closed(..., scales=True)`):

  out[b, q, h, c]         sum_{l, p} |a| sum_k w_k |v_k[c]|
  grad_attn               sum_k w_k sum_c |v_k[c] g[c]|
  grad_loc x (y alike)    W_l |a| sum_k |coef_k| sum_c |v_k[c] g[c]|,  coef = (hh, hh, lh, lh): the kernels form the corner dots
                          d_k = sum_c v_k[c] g[c] first and difference them, so the cancellation in d_01 - d_00 is part of S
  grad_value              index_put(accumulate) of |w_k a g[c]|
  fused entries (rows = [offsets | logits] in, softmax in the kernel): S (1 + A), A = the row's largest |logit - max logit| -- the
                          argument of the exponential is of size A and its rounding changes every weight by a relative U A
  logit part of the row gradient   (1 + A) a_i (S_attn_i + sum_j a_j S_attn_j)

Point samplers: `points` (exactly 0, exactly 1, every pixel centre and boundary of the rows and columns, random ones), the f32
F.grid_sample on the CPU as the yardstick, float64 as the target, S = the sample of |feat| (the weights are >= 0)."""
import math

import torch
import torch.nn.functional as F

import norm_cases as NC
from oracle import ops as ref

FACTOR = NC.FACTOR
U = 2.0 ** -24
U_X3 = 2.0 ** -22              # csrc/x3.h: 22 significand bits for the (hi, lo) pair
H, D, P = 8, 32, 4
EXCLUDE_PX = 1e-3
DEFER_MIN, LIGHT_MAX = 256, 768                 # csrc/msda_bwd.hip MSDA_DEFER_MIN / MSDA_LIGHT_MAX at the time of writing
PASS_A, PASS_B = (2, 4), (4, 12)                # (tile edge in coarsest-level pixels, halo in destination pixels) of the two passes

assert_within = NC.assert_within


def levels(shapes):
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return starts, s


def pixel_centres(shapes):
    """(Nv, 2) (x, y) of every pixel of the pyramid, level after level: the encoder's reference points"""
    out = []
    for h, w in shapes:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        out.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return torch.cat(out, 0)


def _wh(shapes, dtype=torch.float32):
    return torch.tensor([[w, h] for h, w in shapes], dtype=dtype)


class Msda:
    """value (B, Nv, H, D), loc (B, Nq, H, L, P, 2), aw (B, Nq, H, L, P), go (B, Nq, H D): the operands of the mmcv-contract
    entries, f32. rows (B, Nq, 3 H L P) = [offsets | logits], refp (Nq, 2): the operands of the fused entries; their locations are
    `loc` up to the rounding of ref + off / W (none when `exact`), their weights softmax(logits), NOT `aw`.
    fam (B, Nq, H, L, P): family index of every sample, fams: the names. lattice: the closed form is the reference and the f32
    yardstick; exact: grad_loc is compared."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.starts, self.Nv = levels(self.shapes)
        self.B, self.Nq, self.L = self.loc.shape[0], self.loc.shape[1], len(self.shapes)

    def offs(self):
        n = H * self.L * P * 2
        return self.rows[..., :n].reshape(self.B, self.Nq, H, self.L, P, 2)

    def logits(self):
        n = H * self.L * P * 2
        return self.rows[..., n:].reshape(self.B, self.Nq, H, self.L * P)

    def fused_operands(self, dtype=torch.float64):
        """(loc, aw) as the fused entries define them, in `dtype` from the raw rows"""
        loc = self.refp.to(dtype)[None, :, None, None, None, :] + self.offs().to(dtype) / _wh(self.shapes, dtype)[None, None, None, :, None, :]
        aw = self.logits().to(dtype).softmax(-1).view(self.B, self.Nq, H, self.L, P)
        return loc, aw

    def logit_spread(self):
        """A (B, Nq, H): the row's largest |logit - max logit|"""
        lg = self.logits().double()
        return (lg.amax(-1, keepdim=True) - lg).amax(-1)


def _fam_names(L, kinds):
    return tuple(f'l{l}/{k}' for l in range(L) for k in kinds)


def _make(name, shapes, B, g, offs, refp, aw, fam, kinds, lattice, exact, go_scale=1.0, loc=None):
    starts, Nv = levels(shapes)
    L = len(shapes)
    value = torch.randn(B, Nv, H, D, generator=g)
    logits = torch.randn(B, Nv, H, L * P, generator=g)
    rows = torch.cat([offs.reshape(B, Nv, -1), logits.reshape(B, Nv, -1)], -1).contiguous()
    if loc is None:
        loc = refp[None, :, None, None, None, :] + offs / _wh(shapes)[None, None, None, :, None, :]
    if aw is None:
        aw = logits.softmax(-1).view(B, Nv, H, L, P)
    go = torch.randn(B, Nv, H * D, generator=g) * go_scale
    return Msda(name=name, shapes=list(shapes), value=value, loc=loc.contiguous(), aw=aw.contiguous(), go=go, rows=rows,
                refp=refp.contiguous(), fam=fam, fams=_fam_names(L, kinds), lattice=lattice, exact=exact)


def off_lattice(shapes, B, seed, amp=9.0):
    """family A: the query's own reference point + uniform +- amp / 2 px ('near'), half of the samples uniform in [-0.2, 1.2]
    instead ('uniform')"""
    g = torch.Generator().manual_seed(seed)
    _, Nv = levels(shapes)
    L = len(shapes)
    refp, wh = pixel_centres(shapes), _wh(shapes)
    off = (torch.rand(B, Nv, H, L, P, 2, generator=g) - 0.5) * amp
    far = torch.rand(B, Nv, H, L, P, generator=g) < 0.5
    u = torch.rand(B, Nv, H, L, P, 2, generator=g) * 1.4 - 0.2
    off = torch.where(far[..., None], (u - refp[None, :, None, None, None, :]) * wh[None, None, None, :, None, :], off)
    fam = torch.arange(L)[None, None, None, :, None] * 2 + far.long()
    return _make(f'A{shapes}', shapes, B, g, off, refp, None, fam, ('near', 'uniform'), False, False)


def _pow2(n):
    return n & (n - 1) == 0


def _signed_weights(shape, g):
    aw = torch.randn(shape, generator=g)
    return torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(()), aw)


def _lattice_ref_points(shapes, Nv, g, exact):
    """exact: multiples of 1 / (2 W_0), 1 / (2 H_0) of the coarsest level in [0, 1] -- ref W_l - 0.5 is then on the half-integer
    lattice of every level and ref + off / W_l exact in f32; otherwise the pixel centres"""
    if not exact:
        return pixel_centres(shapes)
    h0, w0 = min(h for h, _ in shapes), min(w for _, w in shapes)
    kx = torch.randint(0, 2 * w0 + 1, (Nv,), generator=g).float() / (2 * w0)
    ky = torch.randint(0, 2 * h0 + 1, (Nv,), generator=g).float() / (2 * h0)
    return torch.stack([kx, ky], -1)


def _from_pixel_coords(name, shapes, B, g, pc, kinds, fam, exact, aw=None):
    """pc (B, Nq, H, L, P, 2) pixel coordinates (wim, him) -> the case whose locations are (pc + 0.5) / (W, H)"""
    _, Nv = levels(shapes)
    wh = _wh(shapes)[None, None, None, :, None, :]
    loc = (pc + 0.5) / wh
    refp = _lattice_ref_points(shapes, Nv, g, exact)
    offs = (loc - refp[None, :, None, None, None, :]) * wh
    if exact:       # everything dyadic with few bits: the fused entries' ref + off / W is `loc` to the bit
        assert torch.equal(refp[None, :, None, None, None, :] + offs / wh, loc) and torch.equal(loc * wh - 0.5, pc)
    if aw is None:
        aw = _signed_weights((B, Nv, H, len(shapes), P), g)
    return _make(name, shapes, B, g, offs, refp, aw, fam, kinds, True, exact, loc=loc)


def lattice(shapes, B, seed):
    """family B: on every level the samples walk the whole half-integer lattice [-1.5, W + 0.5] x [-1.5, H + 0.5] (in a fixed
    random order), so every (x, y) combination of `lattice_classes` occurs; signed weights, a tenth of them exactly 0"""
    g = torch.Generator().manual_seed(seed)
    _, Nv = levels(shapes)
    L = len(shapes)
    n = B * Nv * H * P
    pc = torch.empty(B, Nv, H, L, P, 2)
    for l, (h, w) in enumerate(shapes):
        nx, ny = 2 * w + 5, 2 * h + 5
        assert n >= nx * ny, f'{n} samples cannot hold the {nx * ny} lattice points of level {l}'
        idx = (torch.randperm(n, generator=g) % (nx * ny)).view(B, Nv, H, P)
        pc[:, :, :, l, :, 0] = (idx % nx).float() * 0.5 - 1.5
        pc[:, :, :, l, :, 1] = (idx // nx).float() * 0.5 - 1.5
    exact = all(_pow2(h) and _pow2(w) for h, w in shapes)
    fam = torch.arange(L)[None, None, None, :, None].expand(B, Nv, H, L, P).contiguous()
    return _from_pixel_coords(f'B{shapes}', shapes, B, g, pc, ('lattice',), fam, exact)


LATTICE_CLASSES = ('-1', '-0.5', '0', 'int', 'half', 'W-1', 'W-0.5', 'W')


def lattice_classes(c, n):
    """class index (into LATTICE_CLASSES) of pixel coordinates c on a map of n pixels along that axis; -1 for -1.5, n + 0.5 and
    whatever a small map does not have. Where classes coincide on a small map (0 == W - 1 at n = 1) the first one is given."""
    out = torch.full(c.shape, -1, dtype=torch.long)
    frac = c - torch.floor(c)
    rules = [c == -1.0, c == -0.5, c == 0.0, (frac == 0) & (c > 0) & (c < n - 1), (frac == 0.5) & (c > 0) & (c < n - 1), c == n - 1.0,
             c == n - 0.5, c == float(n)]
    for k in reversed(range(len(rules))):
        out[rules[k]] = k
    return out


def collide(seed, shapes=((8, 8), (16, 16), (32, 32)), B=1, cell=(13, 9)):
    """family D: every sample of the finest level inside the cell [13, 14] x [9, 10] of it, fractions 0.25 / 0.5 / 0.75 (four
    pixels take all of them); the coarser levels on the quarter-pixel lattice of [-1.25, W + 0.25]. Exact in f32."""
    g = torch.Generator().manual_seed(seed)
    _, Nv = levels(shapes)
    L = len(shapes)
    pc = torch.empty(B, Nv, H, L, P, 2)
    for l, (h, w) in enumerate(shapes):
        for a, n in ((0, w), (1, h)):
            if l == L - 1:
                pc[:, :, :, l, :, a] = cell[a] + torch.randint(1, 4, (B, Nv, H, P), generator=g).float() * 0.25
            else:
                pc[:, :, :, l, :, a] = torch.randint(-5, 4 * n + 2, (B, Nv, H, P), generator=g).float() * 0.25
    fam = torch.arange(L)[None, None, None, :, None].expand(B, Nv, H, L, P).contiguous()
    return _from_pixel_coords('D/collide', list(shapes), B, g, pc, ('lattice',), fam, True)


def outside(seed, shapes=((8, 8), (16, 16), (32, 32)), B=1):
    """family D: every sample outside every map (pixel coordinates W + 0.5 .. 2 W or -W .. -1.5)"""
    g = torch.Generator().manual_seed(seed)
    _, Nv = levels(shapes)
    L = len(shapes)
    pc = torch.empty(B, Nv, H, L, P, 2)
    for l, (h, w) in enumerate(shapes):
        for a, n in ((0, w), (1, h)):
            k = torch.randint(0, 2 * n, (B, Nv, H, P), generator=g).float() * 0.5
            pc[:, :, :, l, :, a] = torch.where(torch.rand(B, Nv, H, P, generator=g) < 0.5, n + 0.5 + k, -1.5 - k)
    # one axis outside is enough to skip a sample: put the other one inside for half of them
    inside = torch.rand(B, Nv, H, L, P, generator=g) < 0.5
    axis = torch.randint(0, 2, (B, Nv, H, L, P), generator=g)
    for a in (0, 1):
        m = inside & (axis == a)
        pc[..., a] = torch.where(m, torch.full_like(pc[..., a], 2.5), pc[..., a])
    fam = torch.arange(L)[None, None, None, :, None].expand(B, Nv, H, L, P).contiguous()
    return _from_pixel_coords('D/outside', list(shapes), B, g, pc, ('lattice',), fam, True)


THRESHOLD_SHAPES = ((8, 8), (16, 16), (32, 32))
THRESHOLD_HEAD, THRESHOLD_LEVEL = 3, 2


def _tile_queries(shapes, tile, c):
    """query indices of pass tile (tx, ty) with edge c coarsest-level pixels, all query levels"""
    starts, _ = levels(shapes)
    w0 = min(w for _, w in shapes)
    q = []
    for (h, w), st in zip(shapes, starts):
        e = c * (w // w0)
        for y in range(tile[1] * e, min(h, (tile[1] + 1) * e)):
            for x in range(tile[0] * e, min(w, (tile[0] + 1) * e)):
                q.append(st + y * w + x)
    return q


def threshold(count, seed=5):
    """family E: offsets of +-1.5 px (every corner inside its first-pass window), then samples of first-pass tile (0, 0) -- for
    767 / 768 also of tile (1, 0), the same second-pass region -- of head THRESHOLD_HEAD moved far away inside level THRESHOLD_LEVEL:
    interior targets give 4 valid corners, one on the right edge 2, one in the map's corner 1.
      255 = 63 x 4 + 2 + 1, 256 = 64 x 4 in tile (0, 0);  767 = (127 x 4 + 2 + 1) + 256, 768 = 128 x 4 + 256 in tiles (0, 0) + (1, 0).
    Every fifth interior target lies beyond the second pass' window too (y = 29.5)."""
    shapes, hd, ld = list(THRESHOLD_SHAPES), THRESHOLD_HEAD, THRESHOLD_LEVEL
    g = torch.Generator().manual_seed(seed)
    L, Nv, refp = len(shapes), levels(shapes)[1], pixel_centres(shapes)
    off = (torch.rand(1, Nv, H, L, P, 2, generator=g) - 0.5) * 3.0
    pc_target = lambda i: (21.5 + (i % 6), 29.5 if i % 5 == 0 else 19.5 + (i // 6) % 4)      # noqa: E731
    plan = {255: [(63, 1, 1)], 256: [(64, 0, 0)], 767: [(127, 1, 1), (64, 0, 0)], 768: [(128, 0, 0), (64, 0, 0)]}[count]
    hl, wl = shapes[ld]
    for tile_x, (n_int, n_edge, n_corner) in enumerate(plan):
        qs = _tile_queries(shapes, (tile_x, 0), PASS_A[0])
        targets = [pc_target(i) for i in range(n_int)] + [(wl - 0.5, 20.5)] * n_edge + [(wl - 0.5, hl - 0.5)] * n_corner
        assert len(targets) <= len(qs) * P
        for i, (tx, ty) in enumerate(targets):
            q, p = qs[i // P], i % P
            off[0, q, hd, ld, p, 0] = (tx + 0.5) - refp[q, 0] * wl
            off[0, q, hd, ld, p, 1] = (ty + 0.5) - refp[q, 1] * hl
    fam = torch.arange(L)[None, None, None, :, None].expand(1, Nv, H, L, P).contiguous()
    return _make(f'E/{count}', shapes, 1, g, off, refp, None, fam, ('near',), False, False, go_scale=1e-3)


def with_inf_row(case, b, q):
    """family F: the same case with grad_out[b, q, :] = +inf"""
    go = case.go.clone()
    go[b, q] = float('inf')
    kw = dict(case.__dict__)
    kw.update(go=go, name=case.name + '+inf')
    for k in ('starts', 'Nv', 'B', 'Nq', 'L'):
        kw.pop(k)
    return Msda(**kw)


# ------------------------------------------------------------------------------------------------
# the op in closed form
# ------------------------------------------------------------------------------------------------
def _closed(value, shapes, loc, aw, grad_out, dtype=torch.float64, scales=False):
    """mmcv's forward and backward, vectorised, every operation in `dtype`. -> dict(out, grad_value, grad_loc, grad_attn) and,
    with scales, the S of each (see the module docstring) under the same keys in a second dict."""
    value, loc, aw, go = value.to(dtype), loc.to(dtype), aw.to(dtype), grad_out.to(dtype)
    B, Nv, Hh, Dd = value.shape
    _, Nq, _, L, Pp, _ = loc.shape
    starts, _ = levels(shapes)
    g = go.view(B, Nq, Hh, 1, Dd)
    out = torch.zeros(B, Nq, Hh, Dd, dtype=dtype)
    gv = torch.zeros(B, Nv, Hh, Dd, dtype=dtype)
    gl, ga = torch.zeros_like(loc), torch.zeros_like(aw)
    S = dict(out=torch.zeros_like(out), grad_value=torch.zeros_like(gv), grad_loc=torch.zeros_like(gl), grad_attn=torch.zeros_like(ga))
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, Nq, Hh, Pp)
    hi = torch.arange(Hh).view(1, 1, Hh, 1).expand(B, Nq, Hh, Pp)
    vt = value.permute(0, 2, 1, 3)                                            # (B, H, Nv, D)
    for l, (hl, wl) in enumerate(shapes):
        x, y, a = loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1], aw[:, :, :, l]
        him, wim = y * hl - 0.5, x * wl - 0.5
        inside = (him > -1) & (wim > -1) & (him < hl) & (wim < wl)
        h0, w0 = torch.floor(him), torch.floor(wim)
        lh, lw = him - h0, wim - w0
        hh, hw = 1 - lh, 1 - lw
        h0, w0 = h0.long(), w0.long()
        corners = ((0, 0, hh * hw, hh, hw), (0, 1, hh * lw, hh, lw), (1, 0, lh * hw, lh, hw), (1, 1, lh * lw, lh, lw))
        d, sd = [], []
        for dy, dx, wk, cx, cy in corners:
            yy, xx = h0 + dy, w0 + dx
            ok = inside & (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl)
            idx = starts[l] + yy.clamp(0, hl - 1) * wl + xx.clamp(0, wl - 1)                      # (B, Nq, H, P)
            gi = idx.permute(0, 2, 1, 3).reshape(B, Hh, Nq * Pp, 1).expand(-1, -1, -1, Dd)
            v = vt.gather(2, gi).view(B, Hh, Nq, Pp, Dd).permute(0, 2, 1, 3, 4)                  # (B, Nq, H, P, D)
            v = torch.where(ok[..., None], v, torch.zeros((), dtype=dtype))
            wk = torch.where(ok, wk, torch.zeros((), dtype=dtype))
            out += ((a * wk)[..., None] * v).sum(3)
            d.append((v * g).sum(-1))
            contrib = (wk * a)[..., None] * g                                                     # (B, Nq, H, P, D)
            gv.index_put_((bi[ok], idx[ok], hi[ok]), contrib[ok], accumulate=True)
            if scales:
                S['out'] += ((a.abs() * wk)[..., None] * v.abs()).sum(3)
                sd.append((v * g).abs().sum(-1))
                S['grad_value'].index_put_((bi[ok], idx[ok], hi[ok]), contrib[ok].abs(), accumulate=True)
        ga[:, :, :, l] = hh * (hw * d[0] + lw * d[1]) + lh * (hw * d[2] + lw * d[3])
        gl[:, :, :, l, :, 0] = wl * a * (hh * (d[1] - d[0]) + lh * (d[3] - d[2]))
        gl[:, :, :, l, :, 1] = hl * a * (hw * (d[2] - d[0]) + lw * (d[3] - d[1]))
        if scales:
            S['grad_attn'][:, :, :, l] = sum(c[2].abs() * s for c, s in zip(corners, sd))
            S['grad_loc'][:, :, :, l, :, 0] = wl * a.abs() * sum(c[3].abs() * s for c, s in zip(corners, sd))
            S['grad_loc'][:, :, :, l, :, 1] = hl * a.abs() * sum(c[4].abs() * s for c, s in zip(corners, sd))
    res = dict(out=out.view(B, Nq, Hh * Dd), grad_value=gv, grad_loc=gl, grad_attn=ga)
    if scales:
        S['out'] = S['out'].view(B, Nq, Hh * Dd)
        return res, S
    return res


def msda_closed_form(value, shapes, loc, aw, grad_out, dtype=torch.float64):
    """-> (out (B, Nq, H D), grad_value (B, Nv, H, D), grad_loc (B, Nq, H, L, P, 2), grad_attn (B, Nq, H, L, P))"""
    r = _closed(value, shapes, loc, aw, grad_out, dtype)
    return r['out'], r['grad_value'], r['grad_loc'], r['grad_attn']


def msda_autograd(value, shapes, loc, aw, grad_out, dtype=torch.float64):
    """the same four by torch's autograd of `oracle.ops.msda_core` (F.grid_sample) in `dtype`"""
    v, l, a = (t.detach().to(dtype).requires_grad_(True) for t in (value, loc, aw))
    out = ref.msda_core(v, torch.tensor(shapes), l, a)
    out.backward(grad_out.to(dtype))
    return dict(out=out.detach(), grad_value=v.grad, grad_loc=l.grad, grad_attn=a.grad)


def near_integer(case, loc64=None, tol=EXCLUDE_PX):
    """(B, Nq, H, L, P) bool: in float64 a pixel coordinate of the sample is within tol of an integer"""
    return near_integer_loc(case.loc if loc64 is None else loc64, case.shapes, tol)


def near_integer_loc(loc, shapes, tol=EXCLUDE_PX):
    pc = loc.double() * _wh(shapes, torch.float64)[None, None, None, :, None, :] - 0.5
    return ((pc - torch.round(pc)).abs() <= tol).any(-1)


def assert_grad_loc(label, value, shapes, loc, aw, grad_out, got, want64):
    """The grad_loc bound for a test that brings its own off-lattice operands (any H, D, P) and its own float64 gradient: families
    by level, S from the closed form, e_ref from torch's f32 autograd, the elements within EXCLUDE_PX of the lattice (at most 1 %)
    left out. Prints and asserts."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    _, S = _closed(value, shapes, loc, aw, grad_out, torch.float64, scales=True)
    r32 = msda_autograd(value, shapes, loc, aw, grad_out, torch.float32)['grad_loc']
    near = near_integer_loc(loc, shapes)
    share = near.double().mean().item()
    assert share <= 0.01, f'{label}: {share:.3%} of the samples within {EXCLUDE_PX} px of the lattice'
    L = len(shapes)
    fam = torch.arange(L)[None, None, None, :, None, None].expand_as(loc)
    keep = ~near[..., None].expand_as(loc)
    assert_within(f'{label} grad_loc (left out {share:.3%})',
                  sample_ratios(got, want64, r32, S['grad_loc'], fam, tuple(f'l{l}' for l in range(L)), keep))


def rows_gradient(case, grad_loc, grad_attn, aw, dtype=torch.float64):
    """(grad_loc, grad_attn) -> the gradient of the raw rows (B, Nq, 3 H L P): d off = d loc / (W, H); d logit = a (d a - sum a d a)"""
    B, Nq, L = case.B, case.Nq, case.L
    goff = grad_loc.to(dtype) / _wh(case.shapes, dtype)[None, None, None, :, None, :]
    a, ga = aw.to(dtype).view(B, Nq, H, L * P), grad_attn.to(dtype).view(B, Nq, H, L * P)
    glog = a * (ga - (a * ga).sum(-1, keepdim=True))
    return torch.cat([goff.reshape(B, Nq, -1), glog.reshape(B, Nq, -1)], -1)


class Refs:
    """want (float64) / ref32 (the f32 yardstick) / S of the four outputs of one case, for the mmcv-contract operands (fused=False)
    or for the fused entries' (loc, aw) from the raw rows (fused=True; also 'grad_rows' and `keep_rows`, and every S times
    (1 + A)). keep: the grad_loc elements compared (all of them unless the case is off-lattice); excluded: their share left out."""

    def __init__(self, case, fused=False):
        c = self.case = case
        loc64, aw64 = c.fused_operands(torch.float64) if fused else (c.loc.double(), c.aw.double())
        loc32, aw32 = c.fused_operands(torch.float32) if fused else (c.loc, c.aw)
        self.want, self.S = _closed(c.value, c.shapes, loc64, aw64, c.go, torch.float64, scales=True)
        if c.lattice:
            self.ref32 = _closed(c.value, c.shapes, loc32, aw32, c.go, torch.float32)
        else:
            self.ref32 = msda_autograd(c.value, c.shapes, loc32, aw32, c.go, torch.float32)
        near = near_integer(c, loc64)
        self.loc_compared = c.exact or not c.lattice
        self.keep = (torch.ones_like(near) if c.exact else torch.zeros_like(near)) if c.lattice else ~near
        self.excluded = 1.0 - self.keep.double().mean().item()
        self.keep_loc = self.keep[..., None].expand(-1, -1, -1, -1, -1, 2)
        self.aw64 = aw64
        if fused:
            A = 1.0 + c.logit_spread()                                            # (B, Nq, H)
            self.S['out'] = self.S['out'] * A[..., None].expand(-1, -1, -1, D).reshape(c.B, c.Nq, H * D)
            self.S['grad_attn'] = self.S['grad_attn'] * A[..., None, None]
            self.S['grad_loc'] = self.S['grad_loc'] * A[..., None, None, None]
            self.S['grad_value'] = self.S['grad_value'] * A.max().item()
            self.want['grad_rows'] = rows_gradient(c, self.want['grad_loc'], self.want['grad_attn'], aw64)
            self.ref32['grad_rows'] = self._rows32(loc32, aw32) if not c.lattice else \
                rows_gradient(c, self.ref32['grad_loc'], self.ref32['grad_attn'], aw32, torch.float32)
            sa = self.S['grad_attn'].view(c.B, c.Nq, H, c.L * P)                  # (already times 1 + A)
            a = aw64.view(c.B, c.Nq, H, c.L * P)
            s_log = a * (sa + (a * sa).sum(-1, keepdim=True))
            s_off = self.S['grad_loc'] / _wh(c.shapes, torch.float64)[None, None, None, :, None, :]
            self.S['grad_rows'] = torch.cat([s_off.reshape(c.B, c.Nq, -1), s_log.reshape(c.B, c.Nq, -1)], -1)
            n = H * c.L * P
            self.keep_rows = torch.cat([self.keep_loc.reshape(c.B, c.Nq, -1), torch.ones(c.B, c.Nq, n, dtype=torch.bool)], -1)
            fam_l = c.fam.view(c.B, c.Nq, H, c.L * P)
            self.fam_rows = torch.cat([c.fam[..., None].expand(-1, -1, -1, -1, -1, 2).reshape(c.B, c.Nq, -1),
                                       fam_l.reshape(c.B, c.Nq, -1)], -1)

    def _rows32(self, loc32, aw32):
        """torch's f32 autograd through the prologue (ref + off / W, softmax) and `msda_core`"""
        c = self.case
        rows = c.rows.clone().requires_grad_(True)
        n = H * c.L * P * 2
        loc = c.refp[None, :, None, None, None, :] + rows[..., :n].view(c.B, c.Nq, H, c.L, P, 2) / _wh(c.shapes)[None, None, None, :, None, :]
        aw = rows[..., n:].view(c.B, c.Nq, H, c.L * P).softmax(-1).view(c.B, c.Nq, H, c.L, P)
        ref.msda_core(c.value, torch.tensor(c.shapes), loc, aw).backward(c.go)
        return rows.grad

    def ratios(self, name, got, extra=None):
        """{family: (largest error, its bound, worst error / bound)} of output `name`"""
        c = self.case
        want, r32, S = self.want[name], self.ref32[name], self.S[name]
        if name == 'grad_loc':
            assert self.loc_compared, 'grad_loc of nominal lattice points is not compared'
            fam, keep = c.fam[..., None].expand(-1, -1, -1, -1, -1, 2), self.keep_loc
        elif name == 'grad_attn':
            fam, keep = c.fam, None
        elif name == 'grad_rows':
            fam, keep = self.fam_rows, self.keep_rows
        else:
            fam, keep = None, None
        return sample_ratios(got, want, r32, S, fam, c.fams, keep, extra)


def sample_ratios(got, want, ref32, S, fam=None, fams=('all',), keep=None, extra=None, u=U):
    """{family: (largest |got - want|, largest bound, worst |got - want| / bound)}; bound = FACTOR max(e_ref, u S) + extra per
    element, e_ref per family. fam None: one family. keep: the elements compared (and e_ref taken over). A non-finite `got` where
    `want` is finite counts as infinitely wrong; elements whose `want` is not finite are not compared."""
    got, want, ref32, S = got.double().cpu(), want.double(), ref32.double(), S.double()
    assert got.shape == want.shape == ref32.shape == S.shape, (got.shape, want.shape, ref32.shape, S.shape)
    finite = torch.isfinite(want)
    keep = finite if keep is None else (keep & finite)
    if fam is None:
        fam, fams = torch.zeros(want.shape, dtype=torch.long), ('all',)
    out = {}
    for i, name in enumerate(fams):
        m = (fam == i) & keep
        if not bool(m.any()):
            continue
        e32 = (ref32[m] - want[m]).abs()
        e_ref = e32[torch.isfinite(e32)].max().item() if bool(torch.isfinite(e32).any()) else 0.0
        s = S[m]
        bound = FACTOR * torch.maximum(torch.full_like(s, e_ref), u * torch.where(torch.isfinite(s), s, torch.zeros_like(s)))
        if extra is not None:
            bound = bound + extra.double()[m]
        err = (got[m] - want[m]).abs()
        ratio = err / bound
        ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)                            # 0 / 0: exact
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))  # NaN / inf in got -> inf
        out[name] = (err.max().item(), bound.max().item(), ratio.max().item())
    return out


# ------------------------------------------------------------------------------------------------
# the geometry of the sorted scatter (csrc/msda_bwd.hip), counted in float64
# ------------------------------------------------------------------------------------------------
def scatter_counts(case, tile_c=PASS_A[0], halo=PASS_A[1]):
    """(B, tiles_y, tiles_x, H, L) int64: per first-pass unit (tile of tile_c x tile_c coarsest-level pixels with the co-located
    pixels of the finer levels, head, destination level) the valid corners of its queries' samples that fall outside the unit's
    window = the tile's footprint on the destination level + `halo` pixels on every side."""
    shapes, loc = case.shapes, case.loc.double()
    B, Nq, L = case.B, case.Nq, case.L
    h0c, w0c = min(h for h, _ in shapes), min(w for _, w in shapes)
    ty_n, tx_n = -(-h0c // tile_c), -(-w0c // tile_c)
    # tile of every query
    tq = []
    for (h, w) in shapes:
        e = tile_c * (w // w0c)
        ys, xs = torch.meshgrid(torch.arange(h) // e, torch.arange(w) // e, indexing='ij')
        tq.append((ys * tx_n + xs).reshape(-1))
    tq = torch.cat(tq)                                                         # (Nq,)
    counts = torch.zeros(B, ty_n * tx_n, H, L, dtype=torch.long)
    for l, (hl, wl) in enumerate(shapes):
        ed = tile_c * (wl // w0c)
        him, wim = loc[:, :, :, l, :, 1] * hl - 0.5, loc[:, :, :, l, :, 0] * wl - 0.5
        inside = (him > -1) & (wim > -1) & (him < hl) & (wim < wl)
        y0, x0 = torch.floor(him).long(), torch.floor(wim).long()
        ox = ((tq % tx_n) * ed - halo).view(1, Nq, 1, 1)
        oy = ((tq // tx_n) * ed - halo).view(1, Nq, 1, 1)
        ww = ed + 2 * halo
        n = torch.zeros(B, Nq, H, dtype=torch.long)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                valid = inside & (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl)
                inw = (yy - oy >= 0) & (yy - oy < ww) & (xx - ox >= 0) & (xx - ox < ww)
                n += (valid & ~inw).sum(-1)
        counts[:, :, :, l].index_add_(1, tq, n)
    return counts.view(B, ty_n, tx_n, H, L)


def deferred_totals(counts, defer_min=DEFER_MIN):
    """(B, regions_y, regions_x, H, L): what the first pass leaves to each second-pass region (2 x 2 first-pass tiles) -- the
    counts of its units that reach defer_min; a unit below it scatters its corners itself"""
    B, ty, tx, Hh, L = counts.shape
    c = torch.where(counts >= defer_min, counts, torch.zeros_like(counts))
    c = F.pad(c, (0, 0, 0, 0, 0, tx % 2, 0, ty % 2))
    return c.view(B, (ty + 1) // 2, 2, (tx + 1) // 2, 2, Hh, L).sum((2, 4))


# ------------------------------------------------------------------------------------------------
# point samplers
# ------------------------------------------------------------------------------------------------
def axis_points(n):
    """exactly 0, exactly 1, every pixel boundary i / n and every pixel centre (i + 0.5) / n of an axis of n pixels"""
    return torch.cat([torch.arange(n + 1).float() / n, (torch.arange(n).float() + 0.5) / n])


def points(Hh, Ww, n_random, seed, full=True):
    """(N, 2) (x, y) and (N,) family index into POINT_FAMILIES. full: the whole product of the two axes' special values;
    otherwise the special x along the middle row, the special y along the middle column and the four corners of the map. Then
    n_random points uniform in [-0.05, 1.05]."""
    g = torch.Generator().manual_seed(seed)
    ax, ay = axis_points(Ww), axis_points(Hh)
    if full:
        ys, xs = torch.meshgrid(ay, ax, indexing='ij')
        lat = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1)
    else:
        row = torch.stack([ax, torch.full_like(ax, (Hh // 2 + 0.5) / Hh)], -1)
        col = torch.stack([torch.full_like(ay, (Ww // 2 + 0.5) / Ww), ay], -1)
        lat = torch.cat([row, col, torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])], 0)
    rnd = torch.rand(n_random, 2, generator=g) * 1.1 - 0.05
    fam = torch.cat([torch.zeros(len(lat), dtype=torch.long), torch.ones(n_random, dtype=torch.long)])
    return torch.cat([lat, rnd], 0), fam


def band_points(Hh, Ww, band, n, seed):
    """(n, 2), (n,) for the band-stationary backward of `point_sample_rows` (a workgroup owns `band` rows of the plane): the four
    corners of the map; for every band edge e (rows e - 1 | e in two workgroups) points whose tap rows are e - 1 and e -- y
    between the two rows' centres, on either centre and on the pixel boundary --, at x = 0, 1, the first and last pixels' centres
    and boundaries and random x; the rest uniform in [-0.05, 1.05]"""
    g = torch.Generator().manual_seed(seed)
    xs = [0.0, 1.0, 0.5 / Ww, 1.0 / Ww, 1.5 / Ww, (Ww - 1.0) / Ww, (Ww - 0.5) / Ww, (Ww // 2) / Ww, (Ww // 2 + 0.5) / Ww]
    lat = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]
    for e in range(band, Hh, band):
        ys = [(e - 0.5) / Hh, (e + 0.5) / Hh, float(e) / Hh] + ((e - 0.5 + torch.rand(4, generator=g)) / Hh).tolist()
        for y in ys:
            for x in xs[:5] + torch.rand(2, generator=g).tolist():
                lat.append([x, y])
        for x in xs:
            lat.append([x, (e - 0.25) / Hh])
    lat = torch.tensor(lat)[:n]
    rnd = torch.rand(n - len(lat), 2, generator=g) * 1.1 - 0.05
    fam = torch.cat([torch.zeros(len(lat), dtype=torch.long), torch.ones(len(rnd), dtype=torch.long)])
    return torch.cat([lat, rnd], 0), fam


POINT_FAMILIES = ('lattice', 'random')


def grid_sample_refs(feat, pts, grad_out=None):
    """feat (N, C, H, W) f32, pts (N, P, 2) -> dict(out=(want, ref32, S) (N, C, P)[, grad=(want, ref32, S) (N, C, H, W)]) by
    F.grid_sample(points * 2 - 1, bilinear, zeros, align_corners=False) in float64 / f32; S: the same sample (scatter) of the
    absolute values"""
    res = {}

    def run(f, dtype, go):
        f = f.detach().to(dtype).clone().requires_grad_(go is not None)
        o = F.grid_sample(f, (pts.to(dtype) * 2.0 - 1.0).unsqueeze(2), mode='bilinear', padding_mode='zeros', align_corners=False).squeeze(3)
        if go is None:
            return o.detach(), None
        o.backward(go.to(dtype))
        return o.detach(), f.grad

    w, gw = run(feat, torch.float64, grad_out)
    r, gr = run(feat, torch.float32, grad_out)
    s, gs = run(feat.abs(), torch.float64, None if grad_out is None else grad_out.abs())
    res['out'] = (w, r, s)
    if grad_out is not None:
        res['grad'] = (gw, gr, gs)
    return res


def x3_rounding(want):
    """what the f16 (hi, lo) pair of 16 x adds to a value's error: 2^-22 |x|, and the spacing of the low piece's subnormals / 16"""
    return U_X3 * want.double().abs() + 2.0 ** -28


# ------------------------------------------------------------------------------------------------
# the named cases, built once per process and shared by the tests (never modified)
# ------------------------------------------------------------------------------------------------
PYR_RAGGED = [(5, 7), (10, 14), (20, 28)]
PYR_POW2 = [(4, 4), (8, 8), (16, 16)]
PYR_TILED = [(8, 8), (16, 16), (32, 32)]
DEGENERATE = ([(1, 1), (2, 2), (4, 4)], [(1, 3), (2, 6), (4, 12)], [(3, 1), (6, 2)])
INF_ROW = (1, 700)

CASES = {
    'A/ragged': lambda: off_lattice(PYR_RAGGED, 2, seed=3),
    'A/tiled': lambda: off_lattice(PYR_TILED, 2, seed=4),
    'B/pow2': lambda: lattice(PYR_POW2, 2, seed=11),
    'B/ragged': lambda: lattice(PYR_RAGGED, 2, seed=13),
    'C/1x1': lambda: lattice(DEGENERATE[0], 2, seed=12),
    'C/1x3': lambda: lattice(DEGENERATE[1], 2, seed=14),
    'C/3x1': lambda: lattice(DEGENERATE[2], 2, seed=15),
    'C/1x1/off': lambda: off_lattice(DEGENERATE[0], 2, seed=16),
    'C/1x3/off': lambda: off_lattice(DEGENERATE[1], 2, seed=17),
    'C/3x1/off': lambda: off_lattice(DEGENERATE[2], 2, seed=18),
    'D/collide': lambda: collide(seed=19),
    'D/outside': lambda: outside(seed=20),
    'E/255': lambda: threshold(255),
    'E/256': lambda: threshold(256),
    'E/767': lambda: threshold(767),
    'E/768': lambda: threshold(768),
    'F': lambda: with_inf_row(case('A/tiled'), *INF_ROW),
}
_CASES, _REFS = {}, {}


def bf16_case(c):
    """the case whose values and raw rows are the bf16 roundings of c's (what the bf16 fused entries read); on an exact lattice the
    offsets are bf16 numbers already"""
    kw = {k: v for k, v in c.__dict__.items() if k not in ('starts', 'Nv', 'B', 'Nq', 'L')}
    kw.update(value=c.value.bfloat16().float(), rows=c.rows.bfloat16().float(), name=c.name + '/bf16')
    b = Msda(**kw)
    if c.exact:
        assert torch.equal(b.offs(), c.offs())
    return b


def case(name):
    """`CASES[name]()`, or with the suffix '/bf16' its `bf16_case`"""
    if name not in _CASES:
        _CASES[name] = bf16_case(case(name[:-5])) if name.endswith('/bf16') else CASES[name]()
    return _CASES[name]


def refs(name, fused=False):
    if (name, fused) not in _REFS:
        _REFS[(name, fused)] = Refs(case(name), fused)
    return _REFS[(name, fused)]
