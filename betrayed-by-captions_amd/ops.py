"""Torch-facing wrappers of the HIP kernels in libcgg_hip.so.

Every function takes/returns torch tensors on a ROCm device, allocates outputs with PyTorch's
caching allocator, and enqueues on torch's current stream. None of them has a CPU path: a CPU
tensor raises `CggError` (see _lib.dev_ptr). References are to the reference repo / SURVEY.md
kernel ids (K1..K19).
"""
import ctypes
import os
import math

import torch

from . import _lib
from ._lib import CGG_BF16, CGG_F32, CGG_F32_BF16MFMA, CGG_F32_X3, CONSTANTS, CggError, check, dev_ptr, host_ptr, stream_ptr

_WS_CACHE = {}

# bench.py sets this to a dict to collect (start, end) torch.cuda.Event pairs around selected launches
# (events are recorded on torch's current stream -- the stream the kernels are launched on).
KERNEL_EVENTS = None


KERNEL_META = None          # with KERNEL_EVENTS: name -> list of per-launch dicts (flops, bytes, shape) in launch order


class _timed:
    def __init__(self, name, **meta):
        self.name = name
        self.meta = meta
        self.on = KERNEL_EVENTS is not None and not torch.cuda.is_current_stream_capturing()

    def __enter__(self):
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if self.on:
            self.e.record()
            KERNEL_EVENTS.setdefault(self.name, []).append((self.s, self.e))
            if KERNEL_META is not None and self.meta:
                KERNEL_META.setdefault(self.name, []).append(self.meta)


def _lib_():
    return _lib._lib or _lib.load()       # (the loaded handle without a second frame: this runs once per launch)


def _call(symbol, *args, total=False):
    """The one call path of the status-returning entry points: `symbol` is looked up only now, after Python has evaluated (and
    `dev_ptr` has checked) every argument, and a non-zero status raises under the name of the symbol that ran. total=True: the
    entry point answers a byte count (the host RLE functions), only a negative value is a status. Returns what the symbol returned."""
    rc = getattr(_lib_(), symbol)(*args)
    if rc < 0 or (rc and not total):
        check(rc, symbol)
    return rc


def _ptr_at(t, elem_offset, name, dtype):
    """Device address `elem_offset` elements into tensor `t` (None -> NULL): the one place an offset address is formed. `t` passes
    the dtype and device tests of `dev_ptr`; what lies at the offset (a column block, a destination inside a larger tensor) is the
    caller's statement, so density is not tested."""
    if t is None:
        return None
    return ctypes.c_void_p(dev_ptr(t, name, dtype, dense=False).value + int(elem_offset) * t.element_size())


def _int_array(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _levels(level_hw, level_start):
    """host level table of the MSDeformAttn entries: (int32 [L, 2] = (H_l, W_l), int32 [L] first pixel)"""
    return _int_array([v for pair in level_hw for v in pair]), _int_array(level_start)


_F32_BF16 = (torch.float32, torch.bfloat16)


def _f32_bf16_tag(t, name):
    """CGG_F32 / CGG_BF16 for an operand whose element type crosses the C ABI as a tag (None: CGG_F32 beside a NULL pointer). Any
    other dtype raises, naming the argument, before a pointer is taken: the callee would read the buffer as one of the two."""
    if t is None or t.dtype == torch.float32:
        return CGG_F32
    if t.dtype == torch.bfloat16:
        return CGG_BF16
    raise CggError(f'{name} must be torch.float32 | torch.bfloat16 (got {t.dtype})')


# ------------------------------------------------------------------------------------------------
# K1/K2  MSDeformAttn core   ([3P] mmcv MultiScaleDeformableAttnFunction)
# ------------------------------------------------------------------------------------------------
def _msda_dims(value, sampling_loc):
    B, Nv, H, D = value.shape
    _, Nq, H2, L, P, two = sampling_loc.shape
    if H2 != H or two != 2:
        raise CggError(f'sampling_locations shape {tuple(sampling_loc.shape)} does not match value '
                       f'{tuple(value.shape)}')
    return B, Nv, H, D, L, Nq, P


def msda_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """value (B,Nv,H,D) f32|bf16; spatial_shapes (L,2) int64; level_start_index (L,) int64;
    sampling_locations (B,Nq,H,L,P,2) f32; attention_weights (B,Nq,H,L,P) f32 -> (B,Nq,H*D) f32."""
    B, Nv, H, D, L, Nq, P = _msda_dims(value, sampling_locations)
    vdt = _f32_bf16_tag(value, 'msda_forward: value')
    out = torch.empty((B, Nq, H * D), dtype=torch.float32, device=value.device)
    _call('cgg_msda_forward', dev_ptr(value, 'value', _F32_BF16), dev_ptr(spatial_shapes, 'spatial_shapes', torch.int64),
          dev_ptr(level_start_index, 'level_start_index', torch.int64),
          dev_ptr(sampling_locations, 'sampling_locations', torch.float32),
          dev_ptr(attention_weights, 'attention_weights', torch.float32), dev_ptr(out), B, Nv, H, D, L, Nq, P, vdt,
          stream_ptr(value.device))
    return out


def msda_forward_hostlevels(value, level_hw, level_start, sampling_locations, attention_weights):
    """Same op, level table as python lists (no D2H; legal under hipGraph capture)."""
    B, Nv, H, D, L, Nq, P = _msda_dims(value, sampling_locations)
    vdt = _f32_bf16_tag(value, 'msda_forward_hostlevels: value')
    out = torch.empty((B, Nq, H * D), dtype=torch.float32, device=value.device)
    hw, st = _levels(level_hw, level_start)
    _call('cgg_msda_forward_hostlevels', dev_ptr(value, 'value', _F32_BF16), hw, st,
          dev_ptr(sampling_locations, 'sampling_locations', torch.float32),
          dev_ptr(attention_weights, 'attention_weights', torch.float32), None, 0, dev_ptr(out), B, Nv, H, D, L, Nq, P, vdt, 0,
          stream_ptr(value.device))
    return out


def msda_forward_fused(value, level_hw, level_start, offs_logits, ref_points, num_points):
    """value (B,Nv,H,D); offs_logits (B,Nq,ld) raw [offsets | logits] of the two linears;
    ref_points (Nq,2) -> (B,Nq,H*D). Softmax over L*P and loc = ref + off/(W,H) run in-kernel."""
    B, Nv, H, D = value.shape
    Bq, Nq, ld = offs_logits.shape
    L = len(level_start)
    P = int(num_points)
    vdt = _f32_bf16_tag(value, 'msda_forward_fused: value')
    out = torch.empty((B, Nq, H * D), dtype=torch.float32, device=value.device)
    hw, st = _levels(level_hw, level_start)
    vld = _value_row_stride(value)
    if vld != H * D:                        # padded value rows (`padded_value_rows`): the strided-value form of the f32 kernel
        with _timed('msda_fused'):
            _call('cgg_msda_forward_fused_vld', dev_ptr(value, 'value', torch.float32, dense=False), vld, hw, st,
                  dev_ptr(offs_logits, 'offs_logits', torch.float32), ld, dev_ptr(ref_points, 'ref_points', torch.float32),
                  dev_ptr(out), B, Nv, H, D, L, Nq, P, stream_ptr(value.device))
        return out
    with _timed('msda_fused'):
        _call('cgg_msda_forward_hostlevels', dev_ptr(value, 'value', _F32_BF16), hw, st,
              dev_ptr(offs_logits, 'offs_logits', torch.float32), None, dev_ptr(ref_points, 'ref_points', torch.float32), ld,
              dev_ptr(out), B, Nv, H, D, L, Nq, P, vdt, 1, stream_ptr(value.device))
    return out


MSDA_VALUE_PAD = 32      # floats appended to a 256-float value row by `padded_value_rows`


def padded_value_rows(B, Nv, H, D, device):
    """A probe / test helper for the strided-value forms of the MSDeformAttn kernels (`cgg_msda_forward_fused_vld`, the backward's
    strided grad_value): NO production path allocates its value projection through it (tests/test_kernels_gpu.py and
    scratch/msda_vld_probe.py do; profiles/r6_msda_value_row_stride.txt). Returns
    (buffer (B, Nv, H D + pad) f32, value view (B, Nv, H, D) into it): MSDeformAttn value rows with a padded row stride. A stride
    that is a multiple of 512 bytes (H D = 256 floats = 1 KiB) sends the four corner lines of a tap, and neighbouring pixels' lines,
    to the same L2 channels; 288 floats per row instead of 256 made the forward gather 20 % faster at configs[1] / [2] shapes
    (scratch/msda_vld_probe.py: 256 -> 115 us, 288 -> 92, 320 -> 98, 384 -> 110, 512 -> 112, 544 -> 93) in that probe."""
    C = H * D
    buf = torch.empty((B, Nv, C + MSDA_VALUE_PAD), dtype=torch.float32, device=device)
    return buf, buf[..., :C].unflatten(-1, (H, D))


def _value_row_stride(value):
    """floats per pixel of a (B, Nv, H, D) value operand: H D when packed, more for a `padded_value_rows` view"""
    B, Nv, H, D = value.shape
    if value.is_contiguous():
        return H * D
    vld = value.stride(1)
    if value.dtype != torch.float32 or value.stride(3) != 1 or value.stride(2) != D or value.stride(0) != Nv * vld or vld < H * D \
            or vld % 4 or value.data_ptr() % 16:
        raise CggError(f'value: (B, Nv, H, D) f32 rows, packed or with a padded row stride, expected (strides {value.stride()})')
    return vld


def msda_forward_fused_rows(rows_all, level_hw, level_start, ref_points, num_points, num_heads, head_dim):
    """`msda_forward_fused` on the rows of the MERGED projection GEMM: rows_all (B, Nq, H D + 3 H L P) f32 = [value | offsets |
    logits] per token (queries == value pixels) -> (B, Nq, H D). The value operand is read as the first H D columns of the rows
    (`cgg_msda_forward_fused_vld`), the raw offsets / logits as the rest -- nothing is copied apart."""
    B, Nq, ldr = rows_all.shape
    H, D = int(num_heads), int(head_dim)
    L, P = len(level_start), int(num_points)
    if rows_all.dtype != torch.float32 or not rows_all.is_contiguous() or ldr != H * D + 3 * H * L * P or ldr % 32:
        raise CggError(f'msda_forward_fused_rows: rows {tuple(rows_all.shape)} for H={H} D={D} L={L} P={P}')
    out = torch.empty((B, Nq, H * D), dtype=torch.float32, device=rows_all.device)
    hw, st = _levels(level_hw, level_start)
    with _timed('msda_fused'):
        _call('cgg_msda_forward_fused_vld', dev_ptr(rows_all, 'rows_all', torch.float32), ldr, hw, st,
              _ptr_at(rows_all, H * D, 'rows_all', torch.float32), ldr, dev_ptr(ref_points, 'ref_points', torch.float32), dev_ptr(out),
              B, Nq, H, D, L, Nq, P, stream_ptr(rows_all.device))
    return out


def msda_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights,
                  grad_output):
    B, Nv, H, D, L, Nq, P = _msda_dims(value, sampling_locations)
    gv = torch.zeros_like(value)
    gl = torch.zeros_like(sampling_locations)
    gw = torch.zeros_like(attention_weights)
    # algorithmic bytes: value + locations + weights + grad_output in, the three gradients out
    nbytes = 4.0 * (2 * value.numel() + 2 * sampling_locations.numel() + 2 * attention_weights.numel() + grad_output.numel())
    with _timed('msda_backward', bytes=nbytes, flops=0.0, shape=(B, Nq, H, D, L, P)):
        _call('cgg_msda_backward', dev_ptr(value, 'value', torch.float32), dev_ptr(spatial_shapes, 'spatial_shapes', torch.int64),
              dev_ptr(level_start_index, 'level_start_index', torch.int64),
              dev_ptr(sampling_locations, 'sampling_locations', torch.float32),
              dev_ptr(attention_weights, 'attention_weights', torch.float32), dev_ptr(grad_output, 'grad_output', torch.float32),
              dev_ptr(gv), dev_ptr(gl), dev_ptr(gw), B, Nv, H, D, L, Nq, P, stream_ptr(value.device))
    return gv, gl, gw


def msda_backward_hostlevels(value, level_hw, level_start, sampling_locations, attention_weights, grad_output):
    """`msda_backward` with the level table as host integers: no device tensors for the shapes, no read-back / stream
    synchronisation inside the call (csrc/msda.hip `cgg_msda_backward_hostlevels`)."""
    B, Nv, H, D, L, Nq, P = _msda_dims(value, sampling_locations)
    hw, st = _levels(level_hw, level_start)
    # split backward on a tileable pyramid: grad_loc / grad_attn are written by the gather kernel (no zero-fill, no read of old values)
    ow = bool(_lib_().cgg_msda_backward_overwrites(hw, st, B, Nv, H, D, L, Nq, P)) and \
        sampling_locations.data_ptr() % 16 == 0 and attention_weights.data_ptr() % 16 == 0
    vld = _value_row_stride(value)
    if vld != H * D:                        # padded value rows: grad_value comes back in the same padded layout
        if not ow:
            raise CggError('msda_backward_hostlevels: padded value rows need the split backward (tileable pyramid, D = 32, P = 4)')
        gbuf = torch.zeros((B, Nv, vld), dtype=torch.float32, device=value.device)
        gv = gbuf[..., :H * D].unflatten(-1, (H, D))
    else:
        gv = torch.zeros_like(value)
    gl = torch.empty_like(sampling_locations) if ow else torch.zeros_like(sampling_locations)
    gw = torch.empty_like(attention_weights) if ow else torch.zeros_like(attention_weights)
    nbytes = 4.0 * (2 * value.numel() + 2 * sampling_locations.numel() + 2 * attention_weights.numel() + grad_output.numel())
    # split backward: the gather kernel (grad_loc / grad_attn) on a second stream next to the sorted-scatter kernel (grad_value); the
    # C call forks / joins by events, every result is ordered on the caller's stream (CGG_MSDA_BWD_2S=0: one stream)
    side = _msda_side_stream(value.device) if (ow and MSDA_BWD_2S) else None
    # two-pass sorted scatter (corners beyond the first pass' 4-pixel halo are re-sorted on larger tiles instead of costing one
    # 128-byte atomic each): a per-region counter workspace, 0 bytes where the geometry has no such form (CGG_MSDA_BWD_2P=0: A/B)
    wsb = int(_lib_().cgg_msda_backward_workspace_bytes(hw, st, B, Nv, H, D, L, Nq, P)) if MSDA_BWD_2P else 0
    ws = _workspace(wsb, value.device) if wsb > 0 else None
    with _timed('msda_backward', bytes=nbytes, flops=0.0, shape=(B, Nq, H, D, L, P)):
        _call('cgg_msda_backward_hostlevels_ws', dev_ptr(value, 'value', torch.float32, dense=False), vld, hw, st,
              dev_ptr(sampling_locations, 'sampling_locations', torch.float32),
              dev_ptr(attention_weights, 'attention_weights', torch.float32), dev_ptr(grad_output, 'grad_output', torch.float32),
              dev_ptr(gv, 'grad_value', dense=False), dev_ptr(gl), dev_ptr(gw), B, Nv, H, D, L, Nq, P, int(ow),
              dev_ptr(ws) if ws is not None else None, wsb, stream_ptr(value.device),
              ctypes.c_void_p(side.cuda_stream) if side is not None else None)
    return gv, gl, gw


MSDA_BWD_2S = os.environ.get('CGG_MSDA_BWD_2S', '1') != '0'
MSDA_BWD_2P = os.environ.get('CGG_MSDA_BWD_2P', '1') != '0'
_MSDA_SIDE = {}


def _msda_side_stream(dev):
    s = _MSDA_SIDE.get(dev)
    if s is None:
        s = _MSDA_SIDE[dev] = torch.cuda.Stream(dev)
    return s


def msda_read_levels(spatial_shapes, level_start_index, Nv):
    """mmcv's DEVICE level table -> host ((H_l, W_l), ...), (start_l, ...): `cgg_msda_read_levels`, the one synchronising call of
    the MSDeformAttn family. The result is remembered ON the `spatial_shapes` tensor object (with both tensors' version counters),
    so the six encoder layers of a forward pass and their backwards -- which share one tensor -- pay ONE device->host read, and
    every op call goes through the non-synchronising *_hostlevels entries."""
    key = (spatial_shapes._version, level_start_index.data_ptr(), level_start_index._version, int(Nv))
    hit = getattr(spatial_shapes, '_cgg_levels', None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    L = int(spatial_shapes.shape[0])
    hw, st = (ctypes.c_int32 * (2 * L))(), (ctypes.c_int32 * L)()
    _call('cgg_msda_read_levels', dev_ptr(spatial_shapes, 'spatial_shapes', torch.int64),
          dev_ptr(level_start_index, 'level_start_index', torch.int64), L, int(Nv), hw, st, stream_ptr(spatial_shapes.device))
    level_hw = tuple((int(hw[2 * l]), int(hw[2 * l + 1])) for l in range(L))
    level_start = tuple(int(st[l]) for l in range(L))
    try:
        spatial_shapes._cgg_levels = (key, level_hw, level_start)
    except Exception:
        pass
    return level_hw, level_start


class MultiScaleDeformableAttnFunction(torch.autograd.Function):
    """Drop-in for [3P] mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttnFunction (same positional signature incl. the
    unused im2col_step). The device level table is read once per `value_spatial_shapes` tensor (`msda_read_levels`); forward and
    backward then run the *_hostlevels entries: no per-call synchronisation, the split (sorted-scatter) backward where the pyramid
    allows it."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step=64):
        ctx.save_for_backward(value, sampling_locations, attention_weights)
        ctx.levels = msda_read_levels(value_spatial_shapes, value_level_start_index, value.shape[1])
        # mmcv's op takes half and double values too; the kernels read f32 | bf16 only, so any other float type is computed on an
        # f32 copy and the output returned in value's own type (backward upcasts likewise and casts grad_value back)
        v = value if value.dtype in _F32_BF16 else value.float()
        out = msda_forward_hostlevels(v.contiguous(), ctx.levels[0], ctx.levels[1], sampling_locations.contiguous(),
                                      attention_weights.contiguous())
        return out if v is value else out.to(value.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        value, loc, attw = ctx.saved_tensors
        gv, gl, gw = msda_backward_hostlevels(value.contiguous().float(), ctx.levels[0], ctx.levels[1], loc.contiguous(),
                                              attw.contiguous(), grad_output.contiguous().float())
        return gv.to(value.dtype), None, None, gl, gw, None


class MSDeformAttnRowsFunction(torch.autograd.Function):
    """Training form of the encoder's MSDeformAttn core on the RAW projection rows: out = msda(value, loc(rows), softmax(rows))
    with loc / softmax computed inside the forward kernel (`msda_forward_fused`) and, for the backward, by one prologue kernel,
    the gather's backward kernel and one kernel mapping (grad_loc, grad_attn) back to the rows -- the ~10 autograd-recorded
    elementwise passes over (B, Nq, H, L, P[, 2]) tensors of the un-fused formulation are gone.
    value (B, Nv, H, D) f32, rows (B, Nq, 3 H L P) f32 = [offsets | logits], ref_points (Nq, 2) f32."""

    @staticmethod
    def forward(ctx, value, rows, ref_points, level_hw, level_start, num_points):
        value, rows = value.contiguous(), rows.contiguous()
        ctx.save_for_backward(value, rows, ref_points)
        ctx.geom = (tuple(tuple(int(v) for v in hw) for hw in level_hw), tuple(int(s) for s in level_start), int(num_points))
        return msda_forward_fused(value, ctx.geom[0], ctx.geom[1], rows, ref_points, ctx.geom[2])

    @staticmethod
    def backward(ctx, grad_out):
        value, rows, ref_points = ctx.saved_tensors
        level_hw, level_start, P = ctx.geom
        gv, grows = msda_rows_backward(value, rows, ref_points, level_hw, level_start, P, grad_out)
        return gv, grows, None, None, None, None


def msda_rows_backward(value, rows, ref_points, level_hw, level_start, P, grad_out):
    """Backward of `msda_forward_fused` on the raw projection rows: (grad_value (B, Nv, H, D), grad_rows (B, Nq, 3 H L P)) for
    grad_out (B, Nq, H D) -- the prologue kernel (loc, softmax), the MSDeformAttn backward kernels, the kernel mapping
    (grad_loc, grad_attn) back to the rows."""
    B, Nv, H, D = value.shape
    _, Nq, ld = rows.shape
    L = len(level_hw)
    hw, _ = _levels(level_hw, level_start)
    loc = torch.empty((B, Nq, H, L, P, 2), dtype=torch.float32, device=value.device)
    aw = torch.empty((B, Nq, H, L, P), dtype=torch.float32, device=value.device)
    _call('cgg_msda_prologue', dev_ptr(rows, 'rows', torch.float32), ld, dev_ptr(ref_points, 'ref', torch.float32), hw, dev_ptr(loc),
          dev_ptr(aw), B, Nq, H, L, P, stream_ptr(value.device))
    gv, gl, gw = msda_backward_hostlevels(value, level_hw, level_start, loc, aw, grad_out.contiguous())
    grows = torch.empty_like(rows)
    _call('cgg_msda_prologue_backward', dev_ptr(gl), dev_ptr(gw), dev_ptr(rows), ld, hw, dev_ptr(grows), B, Nq, H, L, P,
          stream_ptr(value.device))
    return gv, grows


# ------------------------------------------------------------------------------------------------
# K3/K4/K5  mask logits  (open_set/models/mask2former_head.py:748-759, :825-826)
# ------------------------------------------------------------------------------------------------
# parity mode: contract the mask logits in exact f32 (f32 MFMA) instead of 3 x bf16 on (hi, lo) pairs; CGG_EXACT_F32_LOGITS=0
# restores the split kernel (A/B)
EXACT_F32_LOGITS = os.environ.get('CGG_EXACT_F32_LOGITS', '1') != '0'
# parity mode's inference cross-attention on the f16 x 3 contraction (CGG_XATTN_X3=0 = the f32-MFMA kernel, A/B)
XATTN_X3 = os.environ.get('CGG_XATTN_X3', '1') != '0'


def _throughput_mode():
    """bf16 (throughput) mode keeps the 3 x bf16 split GEMM for f32 rows: the exact-f32 MFMA form is parity mode's."""
    from . import runtime
    return runtime.is_bf16()


class PackedFeature:
    """mask_feature packed for the MFMA B operand (see include/cgg_hip.h)."""

    def __init__(self, hi, lo, B, C, h, w, f32=None):
        self.hi, self.lo, self.B, self.C, self.h, self.w = hi, lo, B, C, h, w
        self.npix = h * w
        self.words = (self.npix + 31) // 32
        self.f32 = f32        # parity mode: the un-packed f32 map (B, C, h, w) for the exact-f32 contraction


def pack_mask_feature(feat, pool=1, split=True):
    """feat (B,C,H,W) f32 -> PackedFeature of the map bilinear-downsampled by `pool`."""
    B, C, H, W = feat.shape
    if H % pool or W % pool:
        raise CggError(f'pack_mask_feature: {H}x{W} not divisible by pool={pool}')
    h, w = H // pool, W // pool
    T = (h * w + 31) // 32
    hi = torch.empty((B, T, C // 8, 32, 8), dtype=torch.bfloat16, device=feat.device)
    lo = torch.empty_like(hi) if split else None
    _call('cgg_pack_mask_feature', dev_ptr(feat, 'mask_feature', torch.float32), dev_ptr(hi), dev_ptr(lo), B, C, H, W, pool,
          stream_ptr(feat.device))
    f32 = None
    from . import runtime
    if split and C == 256 and EXACT_F32_LOGITS and not runtime.x3_enabled():
        # parity mode: keep the f32 map for `cgg_mask_logits_f32` (pool > 1: the same 2x2 mean, same association order
        # as the pack kernel and as torch's bilinear down-sampling with all lambdas 0.5)
        if pool == 1:
            f32 = feat
        else:
            o = pool // 2 - 1
            f32 = (((feat[:, :, o::pool, o::pool] + feat[:, :, o::pool, o + 1::pool])
                    + (feat[:, :, o + 1::pool, o::pool] + feat[:, :, o + 1::pool, o + 1::pool])) * 0.25).contiguous()
    return PackedFeature(hi, lo, B, C, h, w, f32)


def mask_logits(embed, packed, want_logits=True, want_bits=False, out=None):
    """embed (B,Q,C) f32 x PackedFeature -> (logits (B,Q,h,w) f32 | None, bits (B,Q,words) int32 | None). out: a contiguous f32
    tensor of B Q h w elements that receives the logits (packed kernels only)."""
    B, Q, C = embed.shape
    if out is not None and (packed.f32 is not None or not want_logits or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.numel() != B * Q * packed.npix):
        raise CggError('mask_logits: `out` must be a contiguous float32 tensor of B Q h w elements (packed kernels, want_logits)')
    if B != packed.B or C != packed.C:
        raise CggError(f'mask_logits: embed {tuple(embed.shape)} vs packed B={packed.B} C={packed.C}')
    if packed.f32 is not None and Q > 128:
        parts = [mask_logits(embed[:, s:s + 128].contiguous(), packed, want_logits, want_bits) for s in range(0, Q, 128)]
        return (torch.cat([p[0] for p in parts], 1) if want_logits else None,
                torch.cat([p[1] for p in parts], 1) if want_bits else None)
    if packed.f32 is not None:
        out = torch.empty((B, Q, packed.h, packed.w), dtype=torch.float32, device=embed.device) if want_logits else None
        bits = torch.empty((B, Q, packed.words), dtype=torch.int32, device=embed.device) if want_bits else None
        with _timed('mask_logits_full' if want_logits else 'mask_logits_bits'):
            _call('cgg_mask_logits_f32', dev_ptr(embed, 'mask_embed', torch.float32),
                  dev_ptr(packed.f32.contiguous(), 'mask_feature', torch.float32), dev_ptr(out), dev_ptr(bits), B, Q, C, packed.npix,
                  stream_ptr(embed.device))
        return out, bits
    if out is not None:
        out = out.view(B, Q, packed.h, packed.w)
    else:
        out = torch.empty((B, Q, packed.h, packed.w), dtype=torch.float32, device=embed.device) if want_logits else None
    bits = torch.empty((B, Q, packed.words), dtype=torch.int32, device=embed.device) \
        if want_bits else None
    tag = 'mask_logits_full' if want_logits else 'mask_logits_bits'
    with _timed(tag):
        _call('cgg_mask_logits', dev_ptr(embed, 'mask_embed', torch.float32), dev_ptr(packed.hi), dev_ptr(packed.lo), dev_ptr(out),
              dev_ptr(bits), B, Q, C, packed.npix, stream_ptr(embed.device))
    return out, bits


def mask_logits_ok(embed, packed):
    """operands `mask_logits` runs (its kernels are built for 256 channels; callers keep the torch contraction otherwise)"""
    return (embed.is_cuda and embed.dtype == torch.float32 and embed.dim() == 3 and embed.shape[-1] == 256 and packed.C == 256
            and embed.shape[0] == packed.B)


def mask_logits_launches(Q, split):
    """kernel launches of one `mask_logits` call on the packed (f16 x 3 / bf16) kernels: 1 -- split mode's row groups of 128 queries
    (LDS holds 4 query tiles of hi + lo fragments) are workgroups of ONE launch since round 6 (it was ceil(Q / 128) launches)."""
    return 1


def mask_logits_bits_astat(embed, packed):
    """embed (B, Q, 256) f32 x bf16 PackedFeature -> attn-mask bits (B, Q, words) int32 of (logit < 0), consumer-fused: the query
    tiles stay in registers, the logits are never stored (csrc/mask_logits_astat.hip). Same bits as `mask_logits(..., want_bits=True)`."""
    B, Q, C = embed.shape
    if B != packed.B or C != packed.C or packed.lo is not None:
        raise CggError('mask_logits_bits_astat: bf16 PackedFeature of the same batch / channels expected')
    bits = torch.empty((B, Q, packed.words), dtype=torch.int32, device=embed.device)
    with _timed('mask_logits_bits_astat'):
        _call('cgg_mask_logits_bits_astat', dev_ptr(embed, 'mask_embed', torch.float32), dev_ptr(packed.hi), dev_ptr(bits), B, Q, C,
              packed.npix, stream_ptr(embed.device))
    return bits


def mask_logits_backward_ok(embed, feat):
    """shapes the HIP backward kernels cover (otherwise the caller keeps the torch contractions)."""
    return (embed.is_cuda and embed.dtype == torch.float32 and feat.dtype == torch.float32 and embed.shape[-1] == 256
            and (feat.shape[-2] * feat.shape[-1]) % 8 == 0)


def mask_logits_backward(embed, feat, grad_out, split, need_embed=True, need_feat=True):
    """Gradients of einsum('bqc,bchw->bqhw', embed, feat): embed (B,Q,C) f32, feat (B,C,h,w) f32, grad_out (B,Q,h,w) f32
    -> (grad_embed (B,Q,C) | None, grad_feat (B,C,h,w) | None) on cgg_mask_logits_backward (any Q: the library walks the row
    groups of its kernels -- 128 rows in split mode, 256 otherwise -- on the operands in place and sums their grad_feat parts
    in the kernel's store; round 5: no row-group copies of grad_out, no partial grad_feat maps)."""
    B, Q, C = embed.shape
    h, w = feat.shape[-2:]
    npix = h * w
    feat = feat.contiguous()
    go = grad_out.contiguous()
    embed = embed.contiguous()
    ge = torch.empty((B, Q, C), dtype=torch.float32, device=embed.device) if need_embed else None
    gf = torch.empty((B, C, h, w), dtype=torch.float32, device=embed.device) if need_feat else None
    ws = _workspace(_lib_().cgg_mask_logits_backward_workspace_bytes(B, min(Q, 128), C, npix), embed.device)
    _call('cgg_mask_logits_backward', dev_ptr(embed, 'embed', torch.float32), dev_ptr(feat, 'feat', torch.float32),
          dev_ptr(go, 'grad_out', torch.float32), dev_ptr(ge), dev_ptr(gf), dev_ptr(ws), B, Q, C, npix, int(bool(split)),
          stream_ptr(embed.device))
    return ge, gf


def attn_mask_fix_full_rows(bits, npix):
    """In place: rows of the bit mask that block all `npix` keys are cleared."""
    rows = bits.numel() // bits.shape[-1]
    _call('cgg_attn_mask_fix_full_rows', dev_ptr(bits, 'bits', torch.int32), rows, npix, stream_ptr(bits.device))
    return bits


def attn_mask_from_logits(logits, size):
    """logits (B,Q,H,W) f32 -> bits (B,Q,ceil(h*w/32)) int32 of (bilinear-resized logit < 0)."""
    B, Q, H, W = logits.shape
    h, w = int(size[0]), int(size[1])
    words = (h * w + 31) // 32
    bits = torch.empty((B, Q, words), dtype=torch.int32, device=logits.device)
    _call('cgg_attn_mask_from_logits', dev_ptr(logits, 'logits', torch.float32), dev_ptr(bits), B * Q, H, W, h, w,
          stream_ptr(logits.device))
    return bits


def unpack_bits(bits, npix):
    """bits (..., words) int32 -> bool (..., npix)  (test / debugging helper, plain torch)."""
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    b = ((bits.unsqueeze(-1) >> shifts) & 1).bool()
    return b.flatten(-2)[..., :npix]


# ------------------------------------------------------------------------------------------------
# K6  masked cross attention core
# ------------------------------------------------------------------------------------------------
def _workspace(nbytes, device):
    """Per-(device, stream) scratch buffer shared by the kernels that need one (grown on demand, never shrunk)."""
    key = (device.index, stream_ptr(device).value)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = ws
    return ws


def _xattn_ws(lib_fn, q, B, Q, H, D, S):
    return _workspace(lib_fn(B, Q, H, D, S), q.device)


def masked_xattn(q, kv, bits, num_heads, scale=None, return_lse=False):
    """q (B,Q,E) f32 projected queries; kv (B,S,2E) f32 [K|V] projected; bits (B,Q,ceil(S/32)) int32
    (bit set = blocked) or None -> (B,Q,E) f32 = softmax(q k^T * scale + mask) v, per head.
    return_lse: also the (B,H,Q) log-sum-exp rows that `masked_xattn_backward` consumes."""
    B, Q, E = q.shape
    if Q > 128:     # the kernels hold <= 4 query tiles per workgroup: split the (independent) queries
        parts = [masked_xattn(q[:, s:s + 128].contiguous(), kv, None if bits is None else bits[:, s:s + 128].contiguous(),
                              num_heads, scale, return_lse) for s in range(0, Q, 128)]
        if return_lse:
            return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 2)
        return torch.cat(parts, 1)
    S = kv.shape[1]
    H = int(num_heads)
    D = E // H
    dev_ptr(q, 'q', torch.float32)       # refuses CPU tensors before any torch.cuda call
    if kv.shape[2] != 2 * E:
        raise CggError(f'masked_xattn: kv last dim {kv.shape[2]} != 2*{E}')
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    ws = _xattn_ws(_lib_().cgg_masked_xattn_workspace_bytes, q, B, Q, H, D, S)
    out = torch.empty((B, Q, E), dtype=torch.float32, device=q.device)
    from . import runtime
    if XATTN_X3 and not return_lse and runtime.x3_enabled() and kv.is_cuda and kv.dtype == torch.float32 \
            and kv.stride(2) == 1 and kv.stride(1) % 4 == 0 and kv.stride(0) % 4 == 0:
        # parity mode, inference: both products on the f32-class f16 x 3 contraction (csrc/xattn_x3.hip); kv may be a column
        # slice of a merged projection (rows / images at their strides)
        _call('cgg_masked_xattn_forward_x3', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32, dense=False),
              kv.stride(1), kv.stride(0), dev_ptr(bits, 'bits', torch.int32), dev_ptr(out), dev_ptr(ws), B, Q, H, D, S, float(scale),
              stream_ptr(q.device))
        return out
    if not kv.is_contiguous() and not return_lse:
        # a column slice of the merged [K | V] projection of the layers that read one level: rows / images at their strides
        if kv.stride(2) != 1:
            raise CggError('masked_xattn: a strided kv must have a contiguous last dim')
        _call('cgg_masked_xattn_forward_strided', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32, dense=False),
              kv.stride(1), kv.stride(0), dev_ptr(bits, 'bits', torch.int32), dev_ptr(out), dev_ptr(ws), B, Q, H, D, S, float(scale),
              stream_ptr(q.device))
        return out
    dev_ptr(kv, 'kv', torch.float32)
    if return_lse:
        lse = torch.empty((B, H, Q), dtype=torch.float32, device=q.device)
        _call('cgg_masked_xattn_forward_lse', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32),
              dev_ptr(bits, 'bits', torch.int32), dev_ptr(out), dev_ptr(lse), dev_ptr(ws), B, Q, H, D, S, float(scale),
              _xattn_train_dtype(forward=True), stream_ptr(q.device))
        return out, lse
    _call('cgg_masked_xattn_forward', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32),
          dev_ptr(bits, 'bits', torch.int32), dev_ptr(out), dev_ptr(ws), B, Q, H, D, S, float(scale), CGG_F32, stream_ptr(q.device))
    return out


XATTN_X3_TRAIN = os.environ.get('CGG_XATTN_X3_TRAIN', '1') != '0'
XATTN_X3_BWD = os.environ.get('CGG_XATTN_X3_BWD', '1') != '0'       # parity-mode training: the cross-attention backward on f16 x 3 (0: f32 MFMA)


def _xattn_train_dtype(forward=False):
    """kv_dtype of the training cross-attention kernels: throughput (bf16) mode multiplies on bf16 MFMA operands (f32 accumulate,
    f32 rows in memory) like its GEMMs do; parity mode runs the forward on the f32-class f16 x 3 contraction (the inference kernel,
    which also writes the log-sum-exp rows) and the backward on the exact f32 MFMA."""
    from . import runtime
    if runtime.is_bf16():
        return CGG_F32_BF16MFMA
    return CGG_F32_X3 if (forward and XATTN_X3_TRAIN and XATTN_X3 and runtime.x3_enabled()) else CGG_F32


def masked_xattn_backward(q, kv, bits, out, lse, grad_out, num_heads, scale=None):
    """Gradients of `masked_xattn` w.r.t. q (B,Q,E) and kv (B,S,2E) from the saved output / log-sum-exp rows: recomputes
    the probabilities tile by tile from the bit mask, nothing of size Q x S is stored (cgg_masked_xattn_backward)."""
    B, Q, E = q.shape
    S = kv.shape[1]
    H = int(num_heads)
    D = E // H
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    grad_out = grad_out.contiguous()
    if Q > 128:     # independent query groups: grad_q per group, grad_kv summed over the groups
        gq, gkv = [], None
        for s in range(0, Q, 128):
            a, b = masked_xattn_backward(q[:, s:s + 128].contiguous(), kv,
                                         None if bits is None else bits[:, s:s + 128].contiguous(),
                                         out[:, s:s + 128].contiguous(), lse[:, :, s:s + 128].contiguous(),
                                         grad_out[:, s:s + 128].contiguous(), num_heads, scale)
            gq.append(a)
            gkv = b if gkv is None else gkv.add_(b)
        return torch.cat(gq, 1), gkv
    ws = _xattn_ws(_lib_().cgg_masked_xattn_backward_workspace_bytes, q, B, Q, H, D, S)
    gq = torch.empty_like(q)
    gkv = torch.empty_like(kv)
    from . import runtime
    if XATTN_X3_BWD and XATTN_X3 and not runtime.is_bf16() and runtime.x3_enabled() and E % 4 == 0:
        # parity mode: the f16 x 3 form of the kernel (f32-class, 2.7 x less matrix-pipe time than the f32 MFMA); the gradient operands
        # take their pre-scale from max |grad_out|
        amax = absmax(grad_out.view(-1, E))
        _call('cgg_masked_xattn_backward_x3', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32),
              dev_ptr(bits, 'bits', torch.int32), dev_ptr(out, 'out', torch.float32), dev_ptr(lse, 'lse', torch.float32),
              dev_ptr(grad_out, 'grad_out', torch.float32), dev_ptr(amax), dev_ptr(gq), dev_ptr(gkv), dev_ptr(ws), B, Q, H, D, S,
              float(scale), stream_ptr(q.device))
        return gq, gkv
    _call('cgg_masked_xattn_backward', dev_ptr(q, 'q', torch.float32), dev_ptr(kv, 'kv', torch.float32),
          dev_ptr(bits, 'bits', torch.int32), dev_ptr(out, 'out', torch.float32), dev_ptr(lse, 'lse', torch.float32),
          dev_ptr(grad_out, 'grad_out', torch.float32), dev_ptr(gq), dev_ptr(gkv), dev_ptr(ws), B, Q, H, D, S, float(scale),
          _xattn_train_dtype(), stream_ptr(q.device))
    return gq, gkv


# ------------------------------------------------------------------------------------------------
# K6w  fused (shifted-)window self-attention of the Swin blocks (csrc/window_attn.hip)
# ------------------------------------------------------------------------------------------------
WINDOW_ATTN_HEAD_DIM = 32
WINDOW_ATTN_MAX_TOKENS = 144


def window_attention_shape_ok(channels, ws, num_heads, hw=None, shift=0):
    """The shapes `window_attention` is built for: head dim 32, ws^2 <= 144, 0 <= shift < ws and (when given) a padded map that is
    a window multiple. No stage shape of BASELINE configs[3] is gated off: the fused forward + backward beat the SDPA path at all
    four (profiles/window_attn_ab.txt)."""
    H, ws, shift = int(num_heads), int(ws), int(shift)
    if H <= 0 or channels != H * WINDOW_ATTN_HEAD_DIM or ws <= 0 or ws * ws > WINDOW_ATTN_MAX_TOKENS or not 0 <= shift < ws:
        return False
    return hw is None or (hw[0] > 0 and hw[1] > 0 and hw[0] % ws == 0 and hw[1] % ws == 0)


def window_attention_ok(qkv, ws, num_heads, hw=None, shift=0):
    """The supported set of `window_attention`, in one place: f32 contiguous (B, Hp*Wp, 3C) ROCm rows of a supported shape."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.is_contiguous()):
        return False
    if qkv.shape[2] % 3 or (hw is not None and qkv.shape[1] != hw[0] * hw[1]):
        return False
    return window_attention_shape_ok(qkv.shape[2] // 3, ws, num_heads, hw, shift)


def _window_attn_args(qkv, table, hw, ws, shift, num_heads, scale, who):
    dev_ptr(qkv, 'qkv', torch.float32)          # refuses CPU tensors before any torch.cuda call
    dev_ptr(table, 'table', torch.float32)
    if qkv.dim() != 3:
        raise CggError(f'{who}: qkv must be (B, Hp*Wp, 3C), got {tuple(qkv.shape)}')
    Hp, Wp = int(hw[0]), int(hw[1])
    ws, shift, H = int(ws), int(shift), int(num_heads)
    B, L, C3 = qkv.shape
    if L != Hp * Wp:
        raise CggError(f'{who}: qkv has {L} rows, the map {Hp} x {Wp} has {Hp * Wp}')
    if C3 % 3 or H <= 0 or C3 // 3 != H * WINDOW_ATTN_HEAD_DIM:
        raise CggError(f'{who}: qkv last dim {C3} is not 3 x {H} heads x {WINDOW_ATTN_HEAD_DIM}')
    if ws <= 0 or tuple(table.shape) != ((2 * ws - 1) ** 2, H):
        raise CggError(f'{who}: table must be ({(2 * ws - 1) ** 2}, {H}) for window {ws}, got {tuple(table.shape)}')
    if table.device != qkv.device:
        raise CggError(f'{who}: qkv and table live on different devices')
    if scale is None:
        scale = 1.0 / math.sqrt(WINDOW_ATTN_HEAD_DIM)
    return B, Hp, Wp, C3 // 3, H, ws, shift, float(scale)


def window_attention(qkv, table, hw, ws, shift, num_heads, scale=None, return_lse=False):
    """qkv (B, Hp*Wp, 3C) f32 rows of the qkv linear over the padded, un-rolled map ([q | k | v], each heads x 32); table
    ((2 ws - 1)^2, heads) the relative-position bias parameter; hw = (Hp, Wp), both window multiples -> (B, Hp*Wp, C) f32, the
    (shifted-)window attention of every token in the same token order (cyclic shift, window partition / reverse, bias lookup and the
    additive -100 shifted-window mask are address arithmetic inside the kernel).
    return_lse: also the (B, heads, Hp*Wp) log-sum-exp rows that `window_attention_backward` consumes."""
    B, Hp, Wp, C, H, ws, shift, scale = _window_attn_args(qkv, table, hw, ws, shift, num_heads, scale, 'window_attention')
    out = torch.empty((B, Hp * Wp, C), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, Hp * Wp), dtype=torch.float32, device=qkv.device)
    with _timed('window_attn_fwd'):
        _call('cgg_window_attn_forward', dev_ptr(qkv), dev_ptr(table), dev_ptr(out), dev_ptr(lse), B, Hp, Wp, C, H, ws, shift, scale,
              stream_ptr(qkv.device))
    return (out, lse) if return_lse else out


def window_attention_backward(qkv, table, lse, grad_out, hw, ws, shift, num_heads, scale=None):
    """Gradients of `window_attention` w.r.t. qkv (B, Hp*Wp, 3C) and table ((2 ws - 1)^2, heads) from the saved log-sum-exp rows: the
    probabilities are recomputed per window, grad_table is summed in a fixed order (no atomics: two calls give identical bits)."""
    B, Hp, Wp, C, H, ws, shift, scale = _window_attn_args(qkv, table, hw, ws, shift, num_heads, scale, 'window_attention_backward')
    dev_ptr(lse, 'lse', torch.float32)
    grad_out = grad_out.contiguous()
    dev_ptr(grad_out, 'grad_out', torch.float32)
    if tuple(lse.shape) != (B, H, Hp * Wp) or tuple(grad_out.shape) != (B, Hp * Wp, C):
        raise CggError(f'window_attention_backward: lse {tuple(lse.shape)} / grad_out {tuple(grad_out.shape)} do not match '
                       f'qkv {tuple(qkv.shape)}')
    wsb = _workspace(_lib_().cgg_window_attn_backward_workspace_bytes(B, Hp, Wp, H, ws), qkv.device)
    gqkv = torch.empty_like(qkv)
    gtab = torch.empty_like(table)
    with _timed('window_attn_bwd'):
        _call('cgg_window_attn_backward', dev_ptr(qkv), dev_ptr(table), dev_ptr(lse), dev_ptr(grad_out), dev_ptr(gqkv), dev_ptr(gtab),
              dev_ptr(wsb), B, Hp, Wp, C, H, ws, shift, scale, stream_ptr(qkv.device))
    return gqkv, gtab


class WindowAttentionFn(torch.autograd.Function):
    """`window_attention` with gradients for qkv and table (saves qkv, table and the log-sum-exp rows; not the output)."""

    @staticmethod
    def forward(ctx, qkv, table, hw, ws, shift, num_heads, scale):
        qkv = qkv.contiguous()
        table = table.contiguous()
        out, lse = window_attention(qkv, table, hw, ws, shift, num_heads, scale, return_lse=True)
        ctx.save_for_backward(qkv, table, lse)
        ctx.args = (tuple(hw), ws, shift, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, table, lse = ctx.saved_tensors
        hw, ws, shift, num_heads, scale = ctx.args
        gqkv, gtab = window_attention_backward(qkv, table, lse, grad_out, hw, ws, shift, num_heads, scale)
        return gqkv, gtab, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# K16  caption grounding pair costs
# ------------------------------------------------------------------------------------------------
def grounding_supported(pred, cap):
    return (pred.is_cuda and pred.dtype == torch.float32 and cap.dtype == torch.float32 and pred.shape[1] <= 256
            and cap.shape[1] <= 64 and pred.shape[2] % 8 == 0)


def grounding_pair_costs(pred, cap, cap_mask, inv_temperature):
    """pred (Bp,Q,d) f32, cap (Bc,T,d) f32, cap_mask (Bc,T) int32 -> cost (2,Bc,Bp) f32 (l2v, v2l) of
    grounding_loss.py:32-58 for every (caption, image) pair."""
    Bp, Q, d = pred.shape
    Bc, T, _ = cap.shape
    cost = torch.empty((2, Bc, Bp), dtype=torch.float32, device=pred.device)
    _call('cgg_grounding_pair_costs', dev_ptr(pred, 'pred', torch.float32), dev_ptr(cap, 'cap', torch.float32),
          dev_ptr(cap_mask, 'cap_mask', torch.int32), dev_ptr(cost), Bp, Bc, Q, T, d, float(inv_temperature), stream_ptr(pred.device))
    return cost


def grounding_pair_costs_backward(pred, cap, cap_mask, grad_cost, inv_temperature):
    """-> dsim (Bp, Bc*T, Q): d loss / d (cap[i,t] . pred[j,q]) from grad_cost (2,Bc,Bp)."""
    Bp, Q, d = pred.shape
    Bc, T, _ = cap.shape
    dsim = torch.empty((Bp, Bc * T, Q), dtype=torch.float32, device=pred.device)
    _call('cgg_grounding_pair_costs_backward', dev_ptr(pred, 'pred', torch.float32), dev_ptr(cap, 'cap', torch.float32),
          dev_ptr(cap_mask, 'cap_mask', torch.int32), dev_ptr(grad_cost.contiguous(), 'grad_cost', torch.float32), dev_ptr(dsim), Bp,
          Bc, Q, T, d, float(inv_temperature), stream_ptr(pred.device))
    return dsim


# ------------------------------------------------------------------------------------------------
# K18  generator + cross-entropy row kernels
# ------------------------------------------------------------------------------------------------
def _ce_dtype(logits):
    if logits.dtype == torch.float32:
        return CGG_F32
    if logits.dtype == torch.bfloat16:
        return CGG_BF16
    raise CggError(f'ce_rows: logits must be f32 or bf16 (got {logits.dtype})')


def ce_rows_forward(logits, target, ignore_index):
    """logits (M, N) f32 / bf16 (row stride >= N), target (M,) int64 -> (loss (M,), lse (M,)) f32.
    Columns of -inf count as probability 0, as in F.cross_entropy (a row of nothing but -inf is NaN there and here)."""
    M, N = logits.shape
    if logits.stride(1) != 1:
        raise CggError('ce_rows_forward: rows must be contiguous')
    loss = torch.empty(M, dtype=torch.float32, device=logits.device)
    lse = torch.empty(M, dtype=torch.float32, device=logits.device)
    _call('cgg_ce_rows_forward', dev_ptr(logits, 'logits', _F32_BF16, dense=False), dev_ptr(target, 'target', torch.int64),
          dev_ptr(loss), dev_ptr(lse), M, N, int(logits.stride(0)), int(-100 if ignore_index is None else ignore_index),
          _ce_dtype(logits), stream_ptr(logits.device))
    return loss, lse


def match_cost_rows(x, square=False):
    """x (..., P) f32 point-sampled mask logits (contiguous, P % 4 == 0) -> (sigmoid(x) (..., P), sum_p softplus(x) (...),
    sum_p sigmoid(x) [or sigmoid(x)^2 with square] (...)) in one pass (csrc/ce_rows.hip `cgg_match_cost_rows`): the prediction-only
    halves of the Hungarian mask / dice costs."""
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[-1] % 4:
        raise CggError('match_cost_rows: x must be a contiguous float32 ROCm tensor with a last dim that is a multiple of 4')
    P = x.shape[-1]
    rows = x.numel() // P
    sig = torch.empty_like(x)
    sp = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    ss = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _call('cgg_match_cost_rows', dev_ptr(x, 'x', torch.float32), dev_ptr(sig), dev_ptr(sp), dev_ptr(ss), rows, P, int(bool(square)),
          stream_ptr(x.device))
    return sig, sp, ss


def ce_rows_backward_(logits, target, lse, grad_rows, ignore_index):
    """logits (M, N) -> d loss / d logits IN PLACE: grad_rows[row] * (softmax - onehot); returns `logits`."""
    M, N = logits.shape
    _call('cgg_ce_rows_backward', dev_ptr(logits, 'logits', _F32_BF16, dense=False), dev_ptr(target, 'target', torch.int64),
          dev_ptr(lse, 'lse', torch.float32), dev_ptr(grad_rows.contiguous(), 'grad_rows', torch.float32), M, N, int(logits.stride(0)),
          int(-100 if ignore_index is None else ignore_index), _ce_dtype(logits), stream_ptr(logits.device))
    return logits


# ------------------------------------------------------------------------------------------------
# K19  inference tail
# ------------------------------------------------------------------------------------------------
def upsample_bilinear(x, size):
    """x (N,C,H,W) or (N,H,W) f32 -> bilinear (align_corners=False) resize to `size`."""
    shp = x.shape
    H, W = shp[-2:]
    h, w = int(size[0]), int(size[1])
    n = x.numel() // (H * W)
    y = torch.empty(tuple(shp[:-2]) + (h, w), dtype=torch.float32, device=x.device)
    _call('cgg_upsample_bilinear', dev_ptr(x, 'x', torch.float32), dev_ptr(y), n, H, W, h, w, stream_ptr(x.device))
    return y


def instance_masks(logits, sel, up_size, crop_size, out_size):
    """logits (Q,H,W) f32 low-res; sel (n,) int32 -> masks (n,oh,ow) bool, mask_score (n,), bbox (n,4)."""
    Q, H, W = logits.shape
    n = sel.numel()
    oh, ow = int(out_size[0]), int(out_size[1])
    masks = torch.empty((n, oh, ow), dtype=torch.uint8, device=logits.device)
    score = torch.empty((n,), dtype=torch.float32, device=logits.device)
    bbox = torch.empty((n, 4), dtype=torch.float32, device=logits.device)
    if n == 0:
        return masks.bool(), score, bbox
    ws = torch.empty((n, 8), dtype=torch.int32, device=logits.device)
    _call('cgg_instance_masks', dev_ptr(logits, 'logits', torch.float32), dev_ptr(sel, 'sel', torch.int32), dev_ptr(masks),
          dev_ptr(score), dev_ptr(bbox), dev_ptr(ws), Q, H, W, int(up_size[0]), int(up_size[1]), int(crop_size[0]), int(crop_size[1]),
          oh, ow, n, stream_ptr(logits.device))
    return masks.view(torch.bool), score, bbox


def panoptic_argmax(logits, keep, score, up_size, crop_size, out_size):
    """-> ids (oh,ow) int32 in [0,n), win_half (oh,ow) uint8, counts (n,3) int32."""
    Q, H, W = logits.shape
    n = keep.numel()
    oh, ow = int(out_size[0]), int(out_size[1])
    ids = torch.empty((oh, ow), dtype=torch.int32, device=logits.device)
    half = torch.empty((oh, ow), dtype=torch.uint8, device=logits.device)
    counts = torch.empty((n, 3), dtype=torch.int32, device=logits.device)
    _call('cgg_panoptic_argmax', dev_ptr(logits, 'logits', torch.float32), dev_ptr(keep, 'keep', torch.int32),
          dev_ptr(score, 'score', torch.float32), dev_ptr(ids), dev_ptr(half), dev_ptr(counts), Q, H, W, int(up_size[0]),
          int(up_size[1]), int(crop_size[0]), int(crop_size[1]), oh, ow, n, stream_ptr(logits.device))
    return ids, half, counts


def panoptic_paint(ids, win_half, lut_val, lut_half, void_label):
    seg = torch.empty_like(ids)
    _call('cgg_panoptic_paint', dev_ptr(ids, 'ids', torch.int32), dev_ptr(win_half, 'win_half', torch.uint8),
          dev_ptr(lut_val, 'lut_val', torch.int32), dev_ptr(lut_half, 'lut_half', torch.int32), dev_ptr(seg), ids.numel(),
          int(void_label), stream_ptr(ids.device))
    return seg


PANOPTIC_FUSE_MAX_Q = CONSTANTS['CGG_PANOPTIC_FUSE_MAX_Q']


def panoptic_fuse_geometry(out_sizes, crop_sizes, device):
    """Geometry of a batch for `panoptic_fuse_batched`: (device table (B, 5) int64 [crop_h, crop_w, out_h, out_w, first pixel
    in the flat map], (max out_h, max out_w), total pixels, [(first pixel, out_h, out_w)])."""
    rows, views, off = [], [], 0
    for (oh, ow), (ch, cw) in zip(out_sizes, crop_sizes):
        rows.append([int(ch), int(cw), int(oh), int(ow), off])
        views.append((off, int(oh), int(ow)))
        off += int(oh) * int(ow)
    table = torch.tensor(rows, dtype=torch.int64).to(device)
    return table, (max(r[2] for r in rows), max(r[3] for r in rows)), off, views


def panoptic_fuse_batched(logits, score, label, geometry, up_size, num_classes, num_things, object_mask_thr, iou_thr,
                          filter_low_score, stuff_area_limit, defer_stuff, debug=False):
    """logits (B,Q,H,W) f32, score (B,Q) f32 / label (B,Q) int64 of `rowwise_softmax_argmax`, `geometry` of
    `panoptic_fuse_geometry` -> (flat int32 map, n_kept (B,), segments (B,Q,4) int32 [value, category, area, query], kept scores
    (B,Q)); no host read, four launches (`cgg_panoptic_fuse_batched`). `debug` adds the (B, 2) int32 count of argmax blocks that
    staged their footprint in LDS / read global memory."""
    B, Q, H, W = logits.shape
    table, (moh, mow), total, _ = geometry
    if table.shape != (B, 5) or tuple(score.shape) != (B, Q) or tuple(label.shape) != (B, Q):
        raise CggError(f'panoptic_fuse_batched: logits {tuple(logits.shape)}, score {tuple(score.shape)}, label {tuple(label.shape)}, '
                       f'geometry {tuple(table.shape)} disagree')
    dev = logits.device
    seg = torch.empty((total,), dtype=torch.int32, device=dev)
    n_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    segments = torch.empty((B, Q, 4), dtype=torch.int32, device=dev)
    kscore = torch.empty((B, Q), dtype=torch.float32, device=dev)
    nbytes = int(_lib_().cgg_panoptic_fuse_batched_workspace_bytes(B, Q, total))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=dev)
    _call('cgg_panoptic_fuse_batched', dev_ptr(logits, 'logits', torch.float32), dev_ptr(score, 'score', torch.float32),
          dev_ptr(label, 'label', torch.int64), dev_ptr(table, 'geometry', torch.int64), dev_ptr(seg), dev_ptr(n_kept),
          dev_ptr(segments), dev_ptr(kscore), dev_ptr(ws), nbytes, B, Q, H, W, int(up_size[0]), int(up_size[1]), moh, mow, total,
          int(num_classes), int(num_things), float(object_mask_thr), float(iou_thr), int(bool(filter_low_score)),
          int(math.ceil(stuff_area_limit)), int(bool(defer_stuff)), stream_ptr(dev))
    if debug:
        return seg, n_kept, segments, kscore, ws[:2 * B].view(B, 2)
    return seg, n_kept, segments, kscore


def rowwise_softmax_argmax(x, want_prob=True):
    """x (rows,n) f32 -> (prob (rows,n) | None, max prob (rows,), argmax (rows,) int64)."""
    rows, n = x.shape
    prob = torch.empty_like(x) if want_prob else None
    maxv = torch.empty((rows,), dtype=torch.float32, device=x.device)
    arg = torch.empty((rows,), dtype=torch.int64, device=x.device)
    _call('cgg_rowwise_softmax_argmax', dev_ptr(x, 'x', torch.float32), dev_ptr(prob), dev_ptr(maxv), dev_ptr(arg), rows, n,
          stream_ptr(x.device))
    return prob, maxv, arg


# ------------------------------------------------------------------------------------------------
# K7/K11  skinny linear / residual LayerNorm (query side of the decoder)
# ------------------------------------------------------------------------------------------------
def linear_rows(x, weight, bias=None, relu=False, res=None, split=True, out=None):
    """x (..., K) f32 (last dim contiguous) @ weight (N,K)^T + bias -> (..., N) f32; optional ReLU, then + res."""
    K = x.shape[-1]
    N = weight.shape[0]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    else:
        y = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
        if y.stride(-1) != 1 or y.shape[0] != M or y.shape[1] != N or y.dtype != torch.float32:
            raise CggError('linear_rows: bad `out` view')
    r2 = None
    if res is not None:
        r2 = res.reshape(-1, N)
        if r2.stride(-1) != 1:
            r2 = r2.contiguous()
    if not weight.is_contiguous():
        weight = weight.contiguous()
    _call('cgg_linear_rows', dev_ptr(x2, 'x', torch.float32, dense=False), x2.stride(0), dev_ptr(weight, 'weight', torch.float32),
          dev_ptr(bias, 'bias', torch.float32), dev_ptr(r2, 'res', torch.float32, dense=False), r2.stride(0) if r2 is not None else 0,
          dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), M, N, K, 1 if relu else 0,
          (2 if EXACT_F32_LOGITS and not _throughput_mode() else 1) if split else 0, stream_ptr(x.device))
    return y.view(*x.shape[:-1], N) if out is None else out


def add_layernorm(a, b, gamma, beta, eps=1e-5):
    """LayerNorm(a + b) over the last dim (b may be None)."""
    N = a.shape[-1]
    a2 = a.contiguous()
    b2 = b.contiguous() if b is not None else None
    y = torch.empty_like(a2)
    _call('cgg_add_layernorm', dev_ptr(a2, 'a', torch.float32), dev_ptr(b2, 'b', torch.float32), dev_ptr(gamma, 'gamma', torch.float32),
          dev_ptr(beta, 'beta', torch.float32), dev_ptr(y), a2.numel() // N, N, float(eps), stream_ptr(a.device))
    return y


def group_norm(x, gamma, beta, groups, eps=1e-5, relu=False):
    """x (B,C,H,W) f32 NCHW -> GroupNorm(groups)(x) (* gamma + beta) (+ ReLU)."""
    B, C, H, W = x.shape
    x = x.contiguous()
    nbytes = _lib_().cgg_group_norm_workspace_bytes(B, C, H, W, int(groups))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    _call('cgg_group_norm', dev_ptr(x, 'x', torch.float32), dev_ptr(gamma, 'gamma', torch.float32),
          dev_ptr(beta, 'beta', torch.float32), dev_ptr(y), dev_ptr(ws), B, C, H, W, int(groups), float(eps), 1 if relu else 0,
          stream_ptr(x.device))
    return y


# ------------------------------------------------------------------------------------------------
# throughput-mode encoder stream (bf16 activations between the library GEMMs, f32 residual stream)
# ------------------------------------------------------------------------------------------------
def msda_forward_fused_bf16(value, level_hw, level_start, offs_logits, ref_points, num_points, head_major=False):
    """value (B,Nv,H,D) bf16 -- or, head_major=True, (B,H,Nv,D) as `encoder_proj(..., value_head_major=True)` writes it --,
    offs_logits (B,Nq,ld) bf16 raw [offsets | logits], ref_points (Nq,2) f32 -> (B,Nq,H*D) bf16."""
    if head_major:
        B, H, Nv, D = value.shape
    else:
        B, Nv, H, D = value.shape
    _, Nq, ld = offs_logits.shape
    out = torch.empty((B, Nq, H * D), dtype=torch.bfloat16, device=value.device)
    hw, st = _levels(level_hw, level_start)
    with _timed('msda_fused'):
        _call('cgg_msda_forward_fused_bf16_hm' if head_major else 'cgg_msda_forward_fused_bf16',
              dev_ptr(value, 'value', torch.bfloat16), hw, st, dev_ptr(offs_logits, 'offs_logits', torch.bfloat16), ld,
              dev_ptr(ref_points, 'ref_points', torch.float32), dev_ptr(out), B, Nv, H, D, len(level_start), Nq, int(num_points),
              stream_ptr(value.device))
    return out


def add_layernorm_stream(a, b, gamma, beta, eps=1e-5, pos=None, want_f32=True, want_bf16=True, want_pos=False):
    """LN(a + b) over the last dim (256). a f32, b f32|bf16|None. Returns (y f32 | None, bf16(y) | None,
    bf16(y + pos[row % len(pos)]) | None) from ONE pass."""
    N = a.shape[-1]
    rows = a.numel() // N
    y32 = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_f32 else None
    y16 = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if want_bf16 else None
    yp16 = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if want_pos else None
    adt = _f32_bf16_tag(a, 'add_layernorm_stream: a')
    bdt = _f32_bf16_tag(b, 'add_layernorm_stream: b')
    _call('cgg_add_layernorm_ex', dev_ptr(a, 'a', _F32_BF16), adt, dev_ptr(b, 'b', _F32_BF16), bdt,
          dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32), dev_ptr(pos, 'pos', torch.float32),
          pos.shape[0] if pos is not None else 0, dev_ptr(y32), dev_ptr(y16), dev_ptr(yp16), rows, N, float(eps), stream_ptr(a.device))
    return y32, y16, yp16


def pack_bottleneck64(w1, b1, w2, b2, w3, b3):
    """BN-folded weights of a ResNet layer1 identity Bottleneck -> the packed operands of `bottleneck64`:
    w1 (64, 256), w2 (64, 64, 3, 3), w3 (256, 64) (any float dtype), biases (64,), (64,), (256,)."""
    dev = w1.device
    w1p = pack_linear_weight(w1.reshape(64, 256).float())
    w2p = pack_linear_weight(w2.float().permute(0, 2, 3, 1).reshape(64, 576).contiguous())
    T = torch.arange(8, device=dev).view(8, 1)
    jj = torch.arange(32, device=dev).view(1, 32)
    perm = (64 * (T // 2) + 4 * (jj // 2) + 2 * (T % 2) + (jj % 2)).reshape(-1)          # packed row 32 T + j <- output channel
    w3p = pack_linear_weight(w3.reshape(256, 64).float()[perm].contiguous())
    return (w1p, b1.float().contiguous(), w2p, b2.float().contiguous(), w3p, b3.float().contiguous())


def bottleneck64_ok(x):
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[3] == 256 and x.is_contiguous()
            and x.shape[1] % 8 == 0 and x.shape[2] % 16 == 0 and x.numel() < (1 << 31))


def bottleneck64(x, packed):
    """x (B, H, W, 256) bf16 channel-last -> relu(conv3(relu(conv2(relu(conv1 x)))) + x) of a BN-folded ResNet layer1 identity
    Bottleneck in ONE launch; `packed` from `pack_bottleneck64`."""
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    w1p, b1, w2p, b2, w3p, b3 = packed
    with _timed('bottleneck64'):
        _call('cgg_bottleneck64_bf16', dev_ptr(x, 'x', torch.bfloat16), dev_ptr(w1p), dev_ptr(b1, 'b1', torch.float32), dev_ptr(w2p),
              dev_ptr(b2, 'b2', torch.float32), dev_ptr(w3p), dev_ptr(b3, 'b3', torch.float32), dev_ptr(y), B, H, W, C, 64,
              stream_ptr(x.device))
    return y


def pack_decoder_k_weight(weight):
    """weight (n * 256, 256) f32 (stacked key projections) -> packed bf16 operand of `decoder_kv_proj` (uint8 tensor)."""
    N, K = weight.shape
    out = torch.empty((_lib_().cgg_linear_rows_packed_bytes(N, K),), dtype=torch.uint8, device=weight.device)
    w = weight.detach().float().contiguous()
    _call('cgg_decoder_kv_pack_k', dev_ptr(w, 'weight', torch.float32), dev_ptr(out), N, K, stream_ptr(weight.device))
    return out


def decoder_kv_proj(m16, mp16, wkp, bk, wvp):
    """k (B, hw, NK) = mp16 Wk^T + bk and vt (B, NK, hw) = Wv m16^T (bf16) for one memory level in ONE launch; m16 / mp16
    (B, hw, 256) bf16, wkp from `pack_decoder_k_weight`, wvp from `pack_linear_weight`, bk (NK,) f32."""
    B, hw, C = m16.shape
    NK = bk.numel()
    k = torch.empty((B, hw, NK), dtype=torch.bfloat16, device=m16.device)
    vt = torch.empty((B, NK, hw), dtype=torch.bfloat16, device=m16.device)
    with _timed('decoder_kv_proj'):
        _call('cgg_decoder_kv_proj_bf16', dev_ptr(m16, 'm16', torch.bfloat16), dev_ptr(mp16, 'mp16', torch.bfloat16), dev_ptr(wkp),
              dev_ptr(bk, 'bk', torch.float32), dev_ptr(wvp), dev_ptr(k), dev_ptr(vt), B, hw, C, NK, stream_ptr(m16.device))
    return k, vt


def pack_encoder_proj_weight(weight):
    """weight (256 .. 384 in steps of 32, 256) f32 -> packed bf16 operand of `encoder_proj` (uint8 tensor)."""
    N, K = weight.shape
    out = torch.empty((_lib_().cgg_linear_rows_packed_bytes(N, K),), dtype=torch.uint8, device=weight.device)
    w = weight.detach().float().contiguous()
    _call('cgg_encoder_proj_pack', dev_ptr(w, 'weight', torch.float32), dev_ptr(out), N, K, stream_ptr(weight.device))
    return out


def encoder_proj(x16, xp16, wvp, bv, wcp, bc, pos16=None, value_head_major=False):
    """value = x16 Wv^T + bv (..., 256) and offs = xp16 Wc^T + bc (..., NC), both bf16, in ONE launch over the bf16 rows
    (weights from `pack_encoder_proj_weight`, biases f32). xp16=None: xp = bf16(x16 + pos16[row % len(pos16)]) is formed
    inside the kernel from the bf16 table pos16. value_head_major (x16 (B, N, 256)): value comes back (B, 8, N, 32)."""
    C = x16.shape[-1]
    M = x16.numel() // C
    hm_rows = 0
    if value_head_major:
        if x16.dim() != 3 or bv.numel() != 256:
            raise CggError('encoder_proj: value_head_major needs x16 (B, N, 256) and 256 value columns')
        hm_rows = x16.shape[1]
        value = torch.empty((x16.shape[0], 8, hm_rows, 32), dtype=torch.bfloat16, device=x16.device)
    else:
        value = torch.empty(x16.shape[:-1] + (bv.numel(),), dtype=torch.bfloat16, device=x16.device)
    offs = torch.empty(x16.shape[:-1] + (bc.numel(),), dtype=torch.bfloat16, device=x16.device)
    with _timed('encoder_proj'):
        _call('cgg_encoder_proj_bf16', dev_ptr(x16, 'x16', torch.bfloat16), dev_ptr(xp16, 'xp16', torch.bfloat16),
              dev_ptr(pos16, 'pos16', torch.bfloat16), pos16.shape[0] if pos16 is not None else 0, dev_ptr(wvp),
              dev_ptr(bv, 'bv', torch.float32), dev_ptr(wcp), dev_ptr(bc, 'bc', torch.float32), dev_ptr(value), dev_ptr(offs), M, C,
              bv.numel(), bc.numel(), hm_rows, stream_ptr(x16.device))
    return value, offs


def encoder_ffn_ln(x16, w1p, b1, w2p, b2, gamma, beta, eps=1e-5, pos=None, want_f32=False, want_bf16=True, want_pos=False):
    """LN(x + W2 relu(W1 x + b1) + b2) on (..., 256) bf16 rows in ONE launch (hidden activation stays on chip); w1p / w2p
    from `pack_linear_weight`. Returns (y f32 | None, bf16(y) | None, bf16(y + pos[row % len(pos)]) | None)."""
    C = x16.shape[-1]
    M = x16.numel() // C
    F_ = b1.numel()
    y32 = torch.empty(x16.shape, dtype=torch.float32, device=x16.device) if want_f32 else None
    y16 = torch.empty(x16.shape, dtype=torch.bfloat16, device=x16.device) if want_bf16 else None
    yp16 = torch.empty(x16.shape, dtype=torch.bfloat16, device=x16.device) if want_pos else None
    _call('cgg_encoder_ffn_ln_bf16', dev_ptr(x16, 'x16', torch.bfloat16), dev_ptr(w1p), dev_ptr(b1, 'b1', torch.float32), dev_ptr(w2p),
          dev_ptr(b2, 'b2', torch.float32), dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32), float(eps),
          dev_ptr(pos, 'pos', torch.float32), pos.shape[0] if pos is not None else 0, dev_ptr(y16), dev_ptr(yp16), dev_ptr(y32), M, C,
          F_, stream_ptr(x16.device))
    return y32, y16, yp16


def encoder_ffn_ln_kv(x16, w1p, b1, w2p, b2, gamma, beta, eps, shift, pos, level_start, want_f32=True):
    """Last encoder layer: `encoder_ffn_ln` whose LayerNorm also emits the query decoder's K / V operands like
    `add_layernorm_kv` (x16 (B, S, 256) bf16). Returns (y f32 | None, m16, mp16), the bf16 pair level-major."""
    B, S, C = x16.shape
    y32 = torch.empty(x16.shape, dtype=torch.float32, device=x16.device) if want_f32 else None
    m16 = torch.empty((B * S, C), dtype=torch.bfloat16, device=x16.device)
    mp16 = torch.empty((B * S, C), dtype=torch.bfloat16, device=x16.device)
    _call('cgg_encoder_ffn_ln_kv_bf16', dev_ptr(x16, 'x16', torch.bfloat16), dev_ptr(w1p), dev_ptr(b1, 'b1', torch.float32),
          dev_ptr(w2p), dev_ptr(b2, 'b2', torch.float32), dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32),
          float(eps), dev_ptr(shift, 'shift', torch.float32), dev_ptr(pos, 'pos', torch.float32), S, _int_array(level_start),
          len(level_start), dev_ptr(y32), dev_ptr(m16), dev_ptr(mp16), B * S, C, b1.numel(), stream_ptr(x16.device))
    return y32, m16, mp16


def encoder_layer_tail(a16, x16, wop, bo, norm0, w1p, b1, w2p, b2, norm1, pos=None, kv=None, want_f32=False, want_bf16=True,
                       want_pos=False):
    """Post-attention half of an encoder layer in ONE launch: x1 = LN0(x16 + a16 Wo^T + bo), y = LN1(x1 + FFN(x1)).
    norm0 / norm1 = (gamma, beta, eps); weights from `pack_linear_weight`. kv=None: returns (y f32 | None, bf16(y) | None,
    bf16(y + pos[row % len(pos)]) | None) like `encoder_ffn_ln`; kv=(shift, pos, level_start) (x16 (B, S, 256)): returns
    (y f32 | None, m16, mp16) like `encoder_ffn_ln_kv`."""
    C = x16.shape[-1]
    M = x16.numel() // C
    dev = x16.device
    y32 = torch.empty(x16.shape, dtype=torch.float32, device=dev) if want_f32 else None
    if kv is not None:
        shift, pos, level_start = kv
        S = x16.shape[-2]
        y16 = torch.empty((M, C), dtype=torch.bfloat16, device=dev)
        yp16 = torch.empty((M, C), dtype=torch.bfloat16, device=dev)
        pos_rows, ls, nl = S, _int_array(level_start), len(level_start)
    else:
        shift, ls, nl = None, None, 0
        y16 = torch.empty(x16.shape, dtype=torch.bfloat16, device=dev) if want_bf16 else None
        yp16 = torch.empty(x16.shape, dtype=torch.bfloat16, device=dev) if want_pos else None
        pos_rows = pos.shape[0] if pos is not None else 0
    with _timed('encoder_tail_kv' if kv is not None else 'encoder_tail'):
        _call('cgg_encoder_layer_tail_bf16', dev_ptr(a16, 'a16', torch.bfloat16), dev_ptr(x16, 'x16', torch.bfloat16), dev_ptr(wop),
              dev_ptr(bo, 'bo', torch.float32), dev_ptr(norm0[0], 'gamma0', torch.float32), dev_ptr(norm0[1], 'beta0', torch.float32),
              float(norm0[2]), dev_ptr(w1p), dev_ptr(b1, 'b1', torch.float32), dev_ptr(w2p), dev_ptr(b2, 'b2', torch.float32),
              dev_ptr(norm1[0], 'gamma1', torch.float32), dev_ptr(norm1[1], 'beta1', torch.float32), float(norm1[2]),
              dev_ptr(pos, 'pos', torch.float32), pos_rows, dev_ptr(shift, 'shift', torch.float32), ls, nl, dev_ptr(y16), dev_ptr(yp16),
              dev_ptr(y32), M, C, b1.numel(), stream_ptr(dev))
    return y32, y16, yp16


def add_layernorm_backward(dy, a, b, gamma, eps, want_bf16=False, dy16a=None, dy16b=None, want_amax=False):
    """Backward of LN(a + b) (b None: LN(a)) over the last dim (256) for the upstream gradient dy (f32) + dy16a + dy16b (bf16; any
    subset): returns (dx f32, bf16(dx) | None, dgamma, dbeta); d/da = d/db = dx. want_amax: -> (..., max |dx| as a device scalar),
    the pre-scale of the x3 contractions that consume dx as grad_output (no `absmax` pass)."""
    N = a.shape[-1]
    rows = a.numel() // N
    bdt = _f32_bf16_tag(b, 'add_layernorm_backward: b')
    dx = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    dx16 = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if want_bf16 else None
    nb = _lib_().cgg_add_layernorm_backward_partials(rows)
    partial = torch.empty((nb, 2 * N), dtype=torch.float32, device=a.device)
    if want_amax:
        amax = torch.empty(1, dtype=torch.float32, device=a.device)
        _call('cgg_add_layernorm_backward_amax', dev_ptr(dy, 'dy', torch.float32), dev_ptr(dy16a, 'dy16a', torch.bfloat16),
              dev_ptr(dy16b, 'dy16b', torch.bfloat16), dev_ptr(a, 'a', torch.float32), dev_ptr(b, 'b', _F32_BF16), bdt,
              dev_ptr(gamma, 'gamma', torch.float32), float(eps), dev_ptr(dx), dev_ptr(dx16), dev_ptr(partial), dev_ptr(amax), rows, N,
              stream_ptr(a.device))
        sums = partial.sum(0)
        return dx, dx16, sums[:N], sums[N:], amax
    _call('cgg_add_layernorm_backward', dev_ptr(dy, 'dy', torch.float32), dev_ptr(dy16a, 'dy16a', torch.bfloat16),
          dev_ptr(dy16b, 'dy16b', torch.bfloat16), dev_ptr(a, 'a', torch.float32), dev_ptr(b, 'b', _F32_BF16), bdt,
          dev_ptr(gamma, 'gamma', torch.float32), float(eps), dev_ptr(dx), dev_ptr(dx16), dev_ptr(partial), rows, N,
          stream_ptr(a.device))
    sums = partial.sum(0)
    return dx, dx16, sums[:N], sums[N:]


class _AddLayerNormFn(torch.autograd.Function):
    """(y, bf16(y) | None, bf16(y + pos) | None) = LayerNorm(a + b) (a f32, b f32 | bf16, 256 channels) with the one-pass HIP
    forward and backward; the bf16 outputs feed the next bf16 GEMMs directly (no cast pass) and their bf16 gradients are summed
    with dy inside the backward kernel (no accumulation pass)."""

    @staticmethod
    def forward(ctx, a, b, gamma, beta, eps, pos, want16, wantp):
        a = a.contiguous()
        b = b.contiguous()
        y, y16, yp16 = add_layernorm_stream(a, b, gamma, beta, eps, pos=pos if wantp else None, want_f32=True,
                                            want_bf16=bool(want16), want_pos=bool(wantp))
        ctx.save_for_backward(a, b, gamma)
        ctx.eps = eps
        ctx.pos_shape = tuple(pos.shape) if (pos is not None and wantp) else None
        return y, y16, yp16

    @staticmethod
    def backward(ctx, gy, gy16, gyp16):
        a, b, gamma = ctx.saved_tensors
        c = lambda t, dt: None if t is None else t.contiguous().to(dt)
        dx, dx16, dgamma, dbeta = add_layernorm_backward(c(gy, torch.float32), a, b, gamma, ctx.eps,
                                                         want_bf16=b.dtype == torch.bfloat16 and ctx.needs_input_grad[1],
                                                         dy16a=c(gy16, torch.bfloat16), dy16b=c(gyp16, torch.bfloat16))
        gb = None
        if ctx.needs_input_grad[1]:
            gb = dx16 if b.dtype == torch.bfloat16 else dx
        gpos = None
        if ctx.pos_shape is not None and gyp16 is not None and ctx.needs_input_grad[5]:
            # yp = y + pos[row % len(pos)]: the table's gradient is the sum of the bf16 gradient over the repeats (the batch)
            gpos = gyp16.reshape((-1,) + ctx.pos_shape).sum(0, dtype=torch.float32)
        return (dx if ctx.needs_input_grad[0] else None), gb, dgamma, dbeta, None, gpos, None, None


def add_layernorm_train_ok(a, b, norm):
    return (a.is_cuda and a.dtype == torch.float32 and a.shape[-1] == 256 and b.shape == a.shape
            and b.dtype in (torch.float32, torch.bfloat16) and tuple(norm.normalized_shape) == (256,) and norm.elementwise_affine
            and norm.bias is not None)


def add_layernorm_train(a, b, norm, pos=None, want_bf16=False, want_pos=False):
    """LayerNorm(a + b) of an `nn.LayerNorm(256)` for the training step (autograd-aware). Returns y, or with want_bf16 / want_pos
    the triple (y, bf16(y) | None, bf16(y + pos[row % len(pos)]) | None)."""
    y, y16, yp16 = _AddLayerNormFn.apply(a, b, norm.weight, norm.bias, norm.eps, pos, want_bf16, want_pos)
    if want_bf16 or want_pos:
        return y, y16, yp16
    return y


def add_layernorm_kv(a, b, gamma, beta, eps, shift, pos, level_start, want_f32=True):
    """Last encoder LayerNorm of the inference stream: y = LN(a + b) (a (B, S, 256) f32, b f32|bf16|None) plus the
    query decoder's K / V operands m16 = bf16(y + shift[s]), mp16 = bf16(y + shift[s] + pos[s]) (shift, pos (S, 256)
    f32), both LEVEL-MAJOR: (B * S, 256) with level l = rows [B * start_l, B * start_{l+1}) laid out (B, hw_l, 256).
    Returns (y f32 | None, m16, mp16)."""
    B, S, N = a.shape
    y32 = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_f32 else None
    m16 = torch.empty((B * S, N), dtype=torch.bfloat16, device=a.device)
    mp16 = torch.empty((B * S, N), dtype=torch.bfloat16, device=a.device)
    adt = _f32_bf16_tag(a, 'add_layernorm_kv: a')
    bdt = _f32_bf16_tag(b, 'add_layernorm_kv: b')
    _call('cgg_add_layernorm_kv', dev_ptr(a, 'a', _F32_BF16), adt, dev_ptr(b, 'b', _F32_BF16), bdt,
          dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32), dev_ptr(shift, 'shift', torch.float32),
          dev_ptr(pos, 'pos', torch.float32), S, _int_array(level_start), len(level_start), dev_ptr(y32), dev_ptr(m16), dev_ptr(mp16),
          B * S, N, float(eps), stream_ptr(a.device))
    return y32, m16, mp16


def bias_act_nhwc_(y, bias=None, res=None, relu=True):
    """In place on a channel-last bf16 activation `y` (..., C): y <- act(y + bias[C] + res)."""
    C = y.shape[-1]
    _call('cgg_bias_act_nhwc', dev_ptr(y, 'y', torch.bfloat16), dev_ptr(bias, 'bias', torch.bfloat16),
          dev_ptr(res, 'res', torch.bfloat16), y.numel() // C, C, int(bool(relu)), stream_ptr(y.device))
    return y


def group_norm_nhwc_workspace(B, HW, groups, device):
    """f32 scratch for `group_norm_nhwc` ((mean, variance) per (b, group) + per-block partial statistics)."""
    n = _lib_().cgg_group_norm_nhwc_workspace_bytes(int(B), int(HW), int(groups))
    return torch.empty((max(n // 4, 1),), dtype=torch.float32, device=device)


def group_norm_nhwc(x, gamma, beta, groups, eps, ws, relu=False, up=None, W=0, out32=None, out16=None, pos=None,
                    outp16=None):
    """GroupNorm of a channel-last bf16 activation x (B, HW, C), C / groups == 8 (see include/cgg_hip.h).
      up     = (f32 tensor, element offset, batch stride, h, w): low-res NHWC map, bilinearly up-sampled and added
      out32  = (f32 tensor, element offset, batch stride) destination of y
      out16  / outp16 = (bf16 tensor, element offset, batch stride) destinations of bf16(y) / bf16(y + pos)
      pos    = (f32 tensor, element offset) rows [HW, C]
    Destinations are raw (tensor, offset, stride) triples so the three encoder levels can land directly inside the
    (B, N, C) stream tensors."""
    B, HW, C = x.shape
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise CggError(f'group_norm_nhwc: x dtype {x.dtype}')
    need = _lib_().cgg_group_norm_nhwc_workspace_bytes(B, HW, int(groups))
    if ws is None or ws.numel() * ws.element_size() < need:
        raise CggError(f'group_norm_nhwc: workspace too small ({need} bytes needed; see group_norm_nhwc_workspace)')
    b16 = out16[2] if out16 is not None else (outp16[2] if outp16 is not None else 0)
    if out16 is not None and outp16 is not None and out16[2] != outp16[2]:
        raise CggError('group_norm_nhwc: out16 and outp16 must share the batch stride')
    _call('cgg_group_norm_nhwc' if x.dtype == torch.bfloat16 else 'cgg_group_norm_nhwc_f32', dev_ptr(x, 'x', x.dtype),
          dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32), dev_ptr(ws, 'ws', torch.float32), B, HW, C,
          int(groups), float(eps), int(bool(relu)), _ptr_at(*up[:2], 'up', torch.float32) if up is not None else None,
          up[3] if up is not None else 0, up[4] if up is not None else 0, up[2] if up is not None else 0, int(W),
          _ptr_at(*out32[:2], 'out32', torch.float32) if out32 is not None else None, out32[2] if out32 is not None else 0,
          _ptr_at(*out16[:2], 'out16', torch.bfloat16) if out16 is not None else None,
          _ptr_at(*pos[:2], 'pos', torch.float32) if pos is not None else None,
          _ptr_at(*outp16[:2], 'outp16', torch.bfloat16) if outp16 is not None else None, b16, stream_ptr(x.device))


def group_norm_nhwc_x3a(x, gamma, beta, groups, eps, ws, out, relu=False, up=None, W=0, pos=None, outp=None):
    """GroupNorm of a channel-last F32 map x (B, HW, C) with the result written as x3a rows (csrc/x3.h):
      out  = (tensor, element offset, batch stride) destination of y (may alias x);
      outp = (tensor, element offset) destination of y + pos (same batch stride), pos = (f32 tensor, element offset) rows [HW, C];
      up   = (x3a tensor, element offset, batch stride, h, w): low-res x3a map, bilinearly up-sampled and added before the ReLU."""
    B, HW, C = x.shape
    if x.dtype != torch.float32:
        raise CggError(f'group_norm_nhwc_x3a: x dtype {x.dtype}')
    need = _lib_().cgg_group_norm_nhwc_workspace_bytes(B, HW, int(groups))
    if ws is None or ws.numel() * ws.element_size() < need:
        raise CggError(f'group_norm_nhwc_x3a: workspace too small ({need} bytes needed; see group_norm_nhwc_workspace)')
    _call('cgg_group_norm_nhwc_f32_x3a', dev_ptr(x, 'x', torch.float32), dev_ptr(gamma, 'gamma', torch.float32),
          dev_ptr(beta, 'beta', torch.float32), dev_ptr(ws, 'ws', torch.float32), B, HW, C, int(groups), float(eps), int(bool(relu)),
          _ptr_at(*up[:2], 'up', None) if up is not None else None, up[3] if up is not None else 0, up[4] if up is not None else 0,
          up[2] if up is not None else 0, int(W), _ptr_at(*out[:2], 'out', None), out[2],
          _ptr_at(*pos[:2], 'pos', torch.float32) if pos is not None else None,
          _ptr_at(*outp[:2], 'outp', None) if outp is not None else None, stream_ptr(x.device))


def group_norm_nhwc_stats(x, groups, ws):
    """The statistics passes of `group_norm_nhwc` alone on a channel-last F32 map x (B, HW, C): ws[:B * groups * 2] = (mean,
    variance) per (b, group), the bits the full call computes. For `mask_feature_head_x3`, which applies the normalisation itself."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise CggError('group_norm_nhwc_stats: x must be a contiguous (B, HW, C) float32 tensor')
    B, HW, C = x.shape
    need = _lib_().cgg_group_norm_nhwc_workspace_bytes(B, HW, int(groups))
    if ws is None or ws.dtype != torch.float32 or ws.numel() * ws.element_size() < need:
        raise CggError(f'group_norm_nhwc_stats: workspace too small ({need} bytes needed; see group_norm_nhwc_workspace)')
    _call('cgg_group_norm_nhwc_f32_stats', dev_ptr(x, 'x', torch.float32), dev_ptr(ws, 'ws', torch.float32), B, HW, C, int(groups),
          stream_ptr(x.device))


def zero_border_map(B, H, W, C, device):
    """(B, H + 2, W + 2, C) f32 channel-last map whose one-pixel border is zero and whose interior is uninitialised (four thin fills)."""
    y = torch.empty((B, H + 2, W + 2, C), dtype=torch.float32, device=device)
    y[:, 0].zero_()
    y[:, H + 1].zero_()
    y[:, 1:H + 1, 0].zero_()
    y[:, 1:H + 1, W + 1].zero_()
    return y


def group_norm_nhwc_padout(x, gamma, beta, groups, eps, ws, hw, y_padded, relu=False, lo=None, lo_hw=None):
    """`group_norm_nhwc` of f32 rows x (B, HW, C) (+ bilinear up-sample of lo (B, lo_h lo_w, C)) with y written into the interior of
    `y_padded` (B, H + 2, W + 2, C) (`zero_border_map`): the x3 training convolution's padded input without a padding copy."""
    B, HW, C = x.shape
    H, W = int(hw[0]), int(hw[1])
    if x.dtype != torch.float32 or not x.is_contiguous() or tuple(y_padded.shape) != (B, H + 2, W + 2, C) or not y_padded.is_contiguous():
        raise CggError('group_norm_nhwc_padout: x (B, HW, C) float32 contiguous and y_padded (B, H + 2, W + 2, C) expected')
    if lo is not None and (not lo.is_contiguous() or lo.dtype != torch.float32):
        raise CggError('group_norm_nhwc_padout: lo must be contiguous float32 rows')
    _call('cgg_group_norm_nhwc_f32_padout', dev_ptr(x), dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(beta, 'beta', torch.float32),
          dev_ptr(ws), B, HW, C, int(groups), float(eps), int(bool(relu)), dev_ptr(lo) if lo is not None else None,
          int(lo_hw[0]) if lo is not None else 0, int(lo_hw[1]) if lo is not None else 0, int(lo.shape[1]) * C if lo is not None else 0,
          W, dev_ptr(y_padded), stream_ptr(x.device))


def group_norm_nhwc_backward(x, y, dy, stats, gamma, groups, eps, relu, hw, lo_hw=None, dx_padded=None):
    """Backward of the channel-last f32 GroupNorm (`cgg_group_norm_nhwc_f32_backward`): x, dy (and y when relu) (B, HW, C), stats
    (B * groups * 2) = the forward workspace's head. -> (dx, dgamma, dbeta, dlo | None); dx_padded: a `zero_border_map` that receives
    dx in its interior (then returned as dx)."""
    B, HW, C = x.shape
    ws = torch.empty(max(_lib_().cgg_group_norm_nhwc_backward_workspace_bytes(B, HW, int(groups)) // 4, 1), dtype=torch.float32, device=x.device)
    dx = dx_padded if dx_padded is not None else torch.empty_like(x)
    tot = torch.empty((B, int(groups), 16), dtype=torch.float32, device=x.device)
    dlo = torch.empty((B, lo_hw[0] * lo_hw[1], C), dtype=torch.float32, device=x.device) if lo_hw is not None else None
    _call('cgg_group_norm_nhwc_f32_backward', dev_ptr(x), dev_ptr(y) if relu else None, dev_ptr(dy), dev_ptr(stats),
          dev_ptr(gamma, 'gamma', torch.float32), dev_ptr(ws), B, HW, C, int(groups), float(eps), int(bool(relu)), dev_ptr(dx),
          dev_ptr(tot), dev_ptr(dlo) if dlo is not None else None, lo_hw[0] if lo_hw else 0, lo_hw[1] if lo_hw else 0, int(hw[1]),
          int(dx_padded is not None), stream_ptr(x.device))
    t = tot.sum(0)                                        # (groups, 16)
    return dx, t[:, :8].reshape(C), t[:, 8:].reshape(C), dlo


class GroupNormRowsFn(torch.autograd.Function):
    """y = act(GroupNorm(x) [+ bilinear up-sample of `lo`]) on CHANNEL-LAST f32 rows for the training step (parity mode;
    `cgg_group_norm_nhwc_f32` forward, `cgg_group_norm_nhwc_f32_backward`): x (B, HW, C) with C / groups == 8, lo (B, lo_h * lo_w, C) |
    None (the [3P] lateral ConvModule has no activation: relu only without `lo`, the output ConvModule). Returns y (B, HW, C)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, lo, hw, lo_hw):
        B, HW, C = x.shape
        x = x.contiguous()
        ws = group_norm_nhwc_workspace(B, HW, groups, x.device)
        y = torch.empty_like(x)
        up = None
        if lo is not None:
            lo = lo.contiguous()
            up = (lo, 0, lo.shape[1] * C, int(lo_hw[0]), int(lo_hw[1]))
        group_norm_nhwc(x, gamma.detach(), beta.detach(), groups, eps, ws, relu=relu, up=up, W=int(hw[1]), out32=(y, 0, HW * C))
        stats = ws[:B * groups * 2].clone()
        ctx.save_for_backward(x, y if relu else x.new_empty(0), stats, gamma)
        ctx.cfg = (int(groups), float(eps), bool(relu), tuple(hw), tuple(lo_hw) if lo is not None else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, stats, gamma = ctx.saved_tensors
        groups, eps, relu, hw, lo_hw = ctx.cfg
        dx, dgamma, dbeta, dlo = group_norm_nhwc_backward(x, y, gy.contiguous(), stats, gamma, groups, eps, relu, hw, lo_hw)
        return dx, dgamma, dbeta, None, None, None, dlo, None, None


def pack_mask_feature_nhwc(feat, pool=1):
    """feat (B, H, W, C) bf16 channel-last -> PackedFeature (hi image only; throughput mode)."""
    B, H, W, C = feat.shape
    if H % pool or W % pool:
        raise CggError(f'pack_mask_feature_nhwc: {H}x{W} not divisible by pool={pool}')
    h, w = H // pool, W // pool
    T = (h * w + 31) // 32
    hi = torch.empty((B, T, C // 8, 32, 8), dtype=torch.bfloat16, device=feat.device)
    _call('cgg_pack_mask_feature_nhwc', dev_ptr(feat, 'mask_feature', torch.bfloat16), dev_ptr(hi), B, C, H, W, int(pool),
          stream_ptr(feat.device))
    return PackedFeature(hi, None, B, C, h, w)


def pack_mask_feature_nhwc_x3(feat, pools):
    """feat (B, H, W, C) F32 channel-last -> [PackedFeature with hi / lo x3 images for each pool in `pools`] (<= 4) from ONE
    launch: parity mode's packed mask feature (split mode of `mask_logits`)."""
    B, H, W, C = feat.shape
    if feat.dtype != torch.float32 or not feat.is_contiguous():
        raise CggError('pack_mask_feature_nhwc_x3: feat must be a contiguous (B, H, W, C) float32 tensor')
    outs, hp, lp = [], [], []
    for pool in pools:
        if H % pool or W % pool:
            raise CggError(f'pack_mask_feature_nhwc_x3: {H}x{W} not divisible by pool={pool}')
        h, w = H // pool, W // pool
        hi = torch.empty((B, (h * w + 31) // 32, C // 8, 32, 8), dtype=torch.bfloat16, device=feat.device)
        lo = torch.empty_like(hi)
        outs.append(PackedFeature(hi, lo, B, C, h, w))
        hp.append(hi.data_ptr())
        lp.append(lo.data_ptr())
    n = len(pools)
    _call('cgg_pack_mask_feature_nhwc_f32_x3', dev_ptr(feat, 'mask_feature', torch.float32), (ctypes.c_void_p * n)(*hp),
          (ctypes.c_void_p * n)(*lp), _int_array([int(p) for p in pools]), n, B, C, H, W, stream_ptr(feat.device))
    return outs


_MFH_C = 256                                        # the one width csrc/mask_feature_head.hip is built for
_MFH_W_BYTES = 2 * (_MFH_C // 32) * (_MFH_C // 16) * 64 * 16 + (_MFH_C // 32) * 32 * 4     # cgg_x3_packed_bytes(256, 256)


def _mfh_problem(z, ws, gn, weight_x3, bias, pools):
    """Why `mask_feature_head_x3` does not apply to these operands (None when it does). No native call."""
    def f32_dev(t, n=None):
        return (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0
                and (n is None or t.numel() == n))
    if not (torch.is_tensor(z) and z.dim() == 4 and f32_dev(z)):
        return 'z must be a contiguous, 16-byte aligned (B, H, W, C) float32 ROCm tensor'
    B, H, W, C = (int(s) for s in z.shape)
    if C != _MFH_C or B < 1 or B > 65535:
        return f'C={C} (only {_MFH_C} is built) / B={B}'
    if H < 8 or W < 8 or H % 8 or W % 8:
        return f'{H}x{W} is not a multiple of the 8 x 8 tile'
    if not (isinstance(gn, (tuple, list)) and len(gn) == 4):
        return 'gn must be (gamma, beta, eps, groups)'
    gamma, beta, _, groups = gn
    if int(groups) != 32 or not f32_dev(gamma, C) or not f32_dev(beta, C):
        return 'GroupNorm must have 32 groups and contiguous float32 ROCm gamma / beta of 256'
    if not (f32_dev(ws) and ws.numel() >= B * 32 * 2):
        return 'ws must be the float32 GroupNorm workspace (>= B * 32 * 2 floats)'
    if not (is_x3(weight_x3) and weight_x3.is_cuda and weight_x3.is_contiguous() and weight_x3.data_ptr() % 16 == 0
            and weight_x3.numel() * weight_x3.element_size() == _MFH_W_BYTES):
        return 'weight_x3 must be the x3 image of a (256, 256) weight'
    if bias is not None and not f32_dev(bias, _MFH_C):
        return 'bias must be a contiguous float32 ROCm tensor of 256'
    pools = list(pools) if pools is not None else []
    if not 1 <= len(pools) <= 4 or any(p not in (1, 2, 4, 8) or H % p or W % p for p in pools) or len(set(pools)) != len(pools):
        return f'pools={pools}: 1 to 4 distinct values out of 1, 2, 4, 8 that divide {H}x{W}'
    devs = {t.device for t in (z, ws, gamma, beta, weight_x3) + ((bias,) if bias is not None else ())}
    if len(devs) != 1:
        return 'operands on different devices'
    return None


def mask_feature_head_x3_ok(z, ws, gn, weight_x3, bias, pools, want_f32=False):
    """True when `mask_feature_head_x3` takes these operands: C_in = C_out = 256, 32 groups, H and W multiples of 8, pools out of
    {1, 2, 4, 8}, contiguous 16-byte aligned float32 ROCm tensors. Never raises; anything else goes GroupNorm -> GEMM -> pack."""
    try:
        return _mfh_problem(z, ws, gn, weight_x3, bias, pools) is None
    except Exception:
        return False


def mask_feature_head_x3(z, ws, gn, weight_x3, bias, pools, want_f32=False, cfg=-1):
    """The pixel decoder's mask-feature head in ONE launch (csrc/mask_feature_head.hip): z (B, H, W, 256) f32 channel-last = the raw
    3 x 3 output, ws = the GroupNorm workspace whose head holds (mean, variance) per (b, group) (the statistics passes ran),
    gn = (gamma, beta, eps, groups) -> relu(GN(z)) -> 1 x 1 convolution with `weight_x3` (x3 image of the (256, 256) weight) + bias ->
    {pool: PackedFeature (hi / lo x3 images)} for each pool in `pools`, bit-identical to `group_norm_nhwc_x3a(relu=True)` ->
    `runtime.linear_x3s` -> `pack_mask_feature_nhwc_x3`. want_f32: also the f32 mask feature (B, H, W, 256) -> (images, mf)."""
    why = _mfh_problem(z, ws, gn, weight_x3, bias, pools)
    if why is not None:
        raise CggError(f'mask_feature_head_x3: {why}')
    B, H, W, C = (int(s) for s in z.shape)
    gamma, beta, eps, groups = gn
    pools = [int(p) for p in pools]
    outs, hp, lp = {}, [], []
    for pool in pools:
        h, w = H // pool, W // pool
        hi = torch.empty((B, (h * w + 31) // 32, C // 8, 32, 8), dtype=torch.bfloat16, device=z.device)
        lo = torch.empty_like(hi)
        outs[pool] = PackedFeature(hi, lo, B, C, h, w)
        hp.append(hi.data_ptr())
        lp.append(lo.data_ptr())
    mf = torch.empty((B, H, W, C), dtype=torch.float32, device=z.device) if want_f32 else None
    n = len(pools)
    with _timed('mask_feature_head_x3', flops=2.0 * B * H * W * C * C, bytes=4.0 * B * H * W * C * (2.4 + (1 if want_f32 else 0)),
                shape=(B * H * W, C, C)):
        _call('cgg_mask_feature_head_x3_cfg', dev_ptr(z), dev_ptr(ws), dev_ptr(gamma), dev_ptr(beta), float(eps), int(groups),
              dev_ptr(weight_x3), dev_ptr(bias) if bias is not None else None, (ctypes.c_void_p * n)(*hp), (ctypes.c_void_p * n)(*lp),
              _int_array(pools), n, dev_ptr(mf) if mf is not None else None, B, H, W, C, C, int(cfg), stream_ptr(z.device))
    return (outs, mf) if want_f32 else outs


def pack_mask_feature_nhwc_multi(feat, pools):
    """feat (B, H, W, C) bf16 channel-last -> [PackedFeature for each pool in `pools`] (<= 4) from ONE launch."""
    B, H, W, C = feat.shape
    outs, ptrs = [], []
    for pool in pools:
        if H % pool or W % pool:
            raise CggError(f'pack_mask_feature_nhwc: {H}x{W} not divisible by pool={pool}')
        h, w = H // pool, W // pool
        hi = torch.empty((B, (h * w + 31) // 32, C // 8, 32, 8), dtype=torch.bfloat16, device=feat.device)
        outs.append(PackedFeature(hi, None, B, C, h, w))
        ptrs.append(hi.data_ptr())
    n = len(pools)
    _call('cgg_pack_mask_feature_nhwc_multi', dev_ptr(feat, 'mask_feature', torch.bfloat16), (ctypes.c_void_p * n)(*ptrs),
          _int_array([int(p) for p in pools]), n, B, C, H, W, stream_ptr(feat.device))
    return outs


# ------------------------------------------------------------------------------------------------
# throughput-mode query-side linear (packed bf16 weights, fused LayerNorm / `+ pos` / split-K)
# ------------------------------------------------------------------------------------------------
class X3Image(torch.Tensor):
    """uint8 buffer holding the x3 image of a weight (csrc/x3.h): the query-side wrappers route to the *_x3 kernels when they
    are handed one instead of a bf16 packed buffer."""

    def __deepcopy__(self, memo):       # cached images sit in module __dict__s that get deep-copied with the module
        return self.as_subclass(torch.Tensor).clone().as_subclass(X3Image)


def is_x3(packed):
    return isinstance(packed, X3Image)


def _x3_check(packed, N, K, who):
    """An x3 image carries no shape: its byte size must be the one `cgg_x3_packed_bytes(N, K)` prescribes (a wrong
    (N, K) made the kernel read past the image)."""
    want = _lib_().cgg_x3_packed_bytes(int(N), int(K))
    if want <= 0 or packed.numel() * packed.element_size() != want:
        raise CggError(f'{who}: the x3 image holds {packed.numel() * packed.element_size()} bytes, an (N={N}, K={K}) weight needs {want}')


def _x3_fn(name, *packed):
    """Symbol of the C entry point `cgg_<name>_bf16` or of its f32-class twin `cgg_<name>_x3`; all packed operands must be of one
    kind."""
    kinds = {is_x3(p) for p in packed if p is not None}
    if len(kinds) > 1:
        raise CggError(f'{name}: bf16 and x3 packed weights mixed in one call')
    return f'cgg_{name}_x3' if True in kinds else f'cgg_{name}_bf16'


def pack_linear_weight_x3(weight):
    """weight (N, K) f32 -> x3 image (hi / lo f16 MFMA-B fragments + per-column scales) for the parity-mode kernels."""
    N, K = weight.shape
    nbytes = _lib_().cgg_x3_packed_bytes(N, K)
    if nbytes <= 0:
        raise CggError(f'pack_linear_weight_x3: unsupported shape {tuple(weight.shape)} (K % 16)')
    out = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
    w = weight.detach().float().contiguous()
    _call('cgg_x3_pack', dev_ptr(w, 'weight', torch.float32), dev_ptr(out), N, K, stream_ptr(weight.device))
    return out.as_subclass(X3Image)


def pack_conv_weight_x3(weight):
    """conv filter (N, C, KH, KW) -> x3 image with k = (ky, kx, c), the order `conv_x3_nhwc` walks a channel-last map in."""
    N = weight.shape[0]
    return pack_linear_weight_x3(weight.detach().float().permute(0, 2, 3, 1).reshape(N, -1))


def topk_select(x, k):
    """x (rows, N) float32 ROCm (last dim contiguous) -> (rows, k) int64: the indices of each row's k largest values as a SET
    (no order, ties at the threshold arbitrary) -- csrc/topk_select.hip, a radix select instead of torch.topk's sort."""
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or not 0 < k <= x.shape[1]:
        raise CggError('topk_select: (rows, N) float32 matrix with a contiguous last dim and 0 < k <= N expected')
    rows, N = x.shape
    px = dev_ptr(x, 'x', torch.float32, dense=False)
    out = torch.empty((rows, k), dtype=torch.int64, device=x.device)
    if rows:
        _call('cgg_topk_select', px, int(x.stride(0)), rows, N, int(k), dev_ptr(out), stream_ptr(x.device))
    return out


def absmax(x):
    """max |x| of a float32 ROCm matrix / tensor (last dim contiguous, % 4) -> device scalar (1,) f32: the per-tensor pre-scale
    of the x3 contractions' grad_output operands (`gemm_x3(..., amax=)`, `wgrad_x3(..., amax=)`; csrc/x3.h). Exact: one streaming
    pass over the tensor (a sampled maximum is NOT safe for gradients -- they are sparse, see runtime._X3LinearFn.backward)."""
    x2 = x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x
    if x2.dim() != 2 or x2.stride(1) != 1:
        raise CggError('absmax: a 2-D view with a contiguous last dim expected')
    if x2.is_contiguous() and x2.numel() % 4 == 0:
        x2 = x2.view(1, -1)                       # dense: one long row
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    M, N = x2.shape
    _call('cgg_absmax_f32', dev_ptr(x2, 'x', torch.float32, dense=False), int(x2.stride(0)) if M > 1 else N, M, N, dev_ptr(out),
          stream_ptr(x.device))
    return out


def relu_backward_absmax(gy, y):
    """(g, amax): g = gy where y > 0 else 0 (the ReLU whose output is y), amax = max |g| as a device scalar -- one pass
    (`cgg_relu_bwd_absmax_f32`) instead of threshold_backward + `absmax`. gy, y contiguous float32 ROCm tensors of one shape, numel % 4 == 0."""
    if gy.dtype != torch.float32 or y.dtype != torch.float32 or not gy.is_cuda or gy.shape != y.shape or not gy.is_contiguous() \
            or not y.is_contiguous() or gy.numel() % 4 or gy.numel() == 0:
        raise CggError('relu_backward_absmax: two contiguous float32 ROCm tensors of one shape with numel % 4 == 0 expected')
    g = torch.empty_like(gy)
    amax = torch.empty(1, dtype=torch.float32, device=gy.device)
    _call('cgg_relu_bwd_absmax_f32', dev_ptr(gy), dev_ptr(y), dev_ptr(g), gy.numel(), dev_ptr(amax), stream_ptr(gy.device))
    return g, amax


def gemm_x3(a, packed, N, bias=None, res=None, relu=False, out=None, amax=None):
    """a (M, K) f32 rows (row stride free, last dim contiguous) x x3 image -> act(a W^T + bias (+ res)) (M, N) f32:
    parity mode's large linear (csrc/x3_gemm.hip). amax: device scalar max |a| (`absmax`) -> a is pre-scaled per tensor instead
    of by the fixed 2^4 (operands that are not unit scale: gradients)."""
    if a.dim() != 2 or a.stride(1) != 1 or a.dtype != torch.float32 or not is_x3(packed):
        raise CggError('gemm_x3: a must be a 2-D float32 tensor with a contiguous last dim, packed an x3 image')
    M, K = a.shape
    _x3_check(packed, N, K, 'gemm_x3')
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    if y.dim() != 2 or y.stride(1) != 1 or y.shape != (M, N) or y.dtype != torch.float32:
        raise CggError('gemm_x3: bad `out` view')
    if res is not None and (res.dim() != 2 or res.stride(1) != 1 or res.shape != (M, N) or res.dtype != torch.float32):
        raise CggError('gemm_x3: bad `res` view')
    with _timed('gemm_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * K + M * N * (2 if res is not None else 1)) + 4.0 * N * K,
                shape=(M, N, K)):
        if amax is not None:
            _call('cgg_gemm_x3_scaled', dev_ptr(a, 'a', torch.float32, dense=False), a.stride(0), dev_ptr(amax, 'amax', torch.float32),
                  dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32), dev_ptr(res, 'res', torch.float32, dense=False),
                  res.stride(0) if res is not None else 0, dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), M, N, K,
                  int(bool(relu)), stream_ptr(a.device))
        else:
            _call('cgg_gemm_x3', dev_ptr(a, 'a', torch.float32, dense=False), a.stride(0), dev_ptr(packed),
                  dev_ptr(bias, 'bias', torch.float32), dev_ptr(res, 'res', torch.float32, dense=False),
                  res.stride(0) if res is not None else 0, dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), M, N, K,
                  int(bool(relu)), stream_ptr(a.device))
    return y


def gemm_x3_bwd(g, packed, N, amax=None, mask=None, out=None, want_amax=False):
    """Backward-side x3 GEMM (csrc/x3_gemm.hip `cgg_gemm_x3_bwd`): out (M, N) = g (M, K) W^T with g pre-scaled per tensor (`amax`),
    the result zeroed where `mask` (M, N) <= 0 (ReLU backward of the layer whose output `mask` is) and, with want_amax, max |out|
    from the epilogue as a device scalar -> (out, out_amax | None)."""
    if g.dim() != 2 or g.stride(1) != 1 or g.dtype != torch.float32 or not is_x3(packed):
        raise CggError('gemm_x3_bwd: g must be a 2-D float32 tensor with a contiguous last dim, packed an x3 image')
    M, K = g.shape
    _x3_check(packed, N, K, 'gemm_x3_bwd')
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=g.device)
    if y.dim() != 2 or y.stride(1) != 1 or y.shape != (M, N) or y.dtype != torch.float32:
        raise CggError('gemm_x3_bwd: bad `out` view')
    if mask is not None and (mask.dim() != 2 or mask.stride(1) != 1 or mask.shape != (M, N) or mask.dtype != torch.float32):
        raise CggError('gemm_x3_bwd: bad `mask` view')
    oa = torch.empty(1, dtype=torch.float32, device=g.device) if want_amax else None
    with _timed('gemm_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * K + M * N * (2 if mask is not None else 1)) + 4.0 * N * K,
                shape=(M, N, K)):
        _call('cgg_gemm_x3_bwd', dev_ptr(g, 'g', torch.float32, dense=False), g.stride(0), dev_ptr(amax, 'amax', torch.float32),
              dev_ptr(packed), dev_ptr(mask, 'mask', torch.float32, dense=False), mask.stride(0) if mask is not None else 0,
              dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), dev_ptr(oa), M, N, K, stream_ptr(g.device))
    return y, oa


def encoder_layer_tail_x3(a, x, wo, bo, norm0, w1, b1, w2, b2, norm1, pos=None, want_pos=False, x3a=False):
    """Parity mode's encoder layer tail in ONE launch: a (attention rows), x (layer input) (..., 256) f32 ->
    y = LN1(x1 + FFN(x1)), x1 = LN0(x + a Wo^T + bo) (and y + pos[row % len(pos)] when want_pos); wo / w1 / w2 x3 images,
    norm_* = (gamma, beta, eps). x3a=True: x and both outputs are x3a rows (csrc/x3.h), a stays f32."""
    C = a.shape[-1]
    M = a.numel() // C
    for t in (a, x):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != a.shape or not t.is_cuda:
            raise CggError('encoder_layer_tail_x3: a / x must be matching contiguous float32 ROCm tensors')
    if not (is_x3(wo) and is_x3(w1) and is_x3(w2)):
        raise CggError('encoder_layer_tail_x3: weights must be x3 images')
    F = b1.numel()
    y = torch.empty_like(a)
    yp = torch.empty_like(a) if want_pos else None
    with _timed('encoder_tail_x3', flops=2.0 * M * (C * C + 2 * C * F), bytes=4.0 * M * C * (3 + (1 if want_pos else 0)),
                shape=(M, C, F)):
        _call('cgg_encoder_layer_tail_x3a' if x3a else 'cgg_encoder_layer_tail_x3', dev_ptr(a), dev_ptr(x), dev_ptr(wo),
              dev_ptr(bo, 'bo', torch.float32), dev_ptr(norm0[0], 'gamma0', torch.float32), dev_ptr(norm0[1], 'beta0', torch.float32),
              float(norm0[2]), dev_ptr(w1), dev_ptr(b1, 'b1', torch.float32), dev_ptr(w2), dev_ptr(b2, 'b2', torch.float32),
              dev_ptr(norm1[0], 'gamma1', torch.float32), dev_ptr(norm1[1], 'beta1', torch.float32), float(norm1[2]),
              dev_ptr(pos, 'pos', torch.float32) if want_pos else None, pos.shape[0] if want_pos else 0, dev_ptr(y), dev_ptr(yp), M, C,
              int(F), stream_ptr(a.device))
    return y, yp


def transpose_f32(x):
    """x (B, R, C) contiguous f32 -> (B, C, R) contiguous (csrc/epilogue.hip: tiled through LDS); `nchw_to_nhwc` / `nhwc_to_nchw`
    are this on the (B, C, H W) / (B, H W, C) views."""
    if x.dim() != 3 or not x.is_contiguous() or x.dtype != torch.float32 or not x.is_cuda:
        raise CggError('transpose_f32: contiguous (B, R, C) float32 ROCm tensor expected')
    B, R, C = x.shape
    y = torch.empty((B, C, R), dtype=torch.float32, device=x.device)
    _call('cgg_transpose_f32', dev_ptr(x), dev_ptr(y), B, R, C, stream_ptr(x.device))
    return y


def nchw_to_nhwc(x):
    """(B, C, H, W) f32 (any strides) -> (B, H, W, C) contiguous."""
    B, C, H, W = x.shape
    if x.permute(0, 2, 3, 1).is_contiguous():
        return x.permute(0, 2, 3, 1)
    return transpose_f32(x.contiguous().view(B, C, H * W)).view(B, H, W, C)


def nchw_to_nhwc_pad1(x):
    """(B, C, H, W) f32 -> (B, H + 2, W + 2, C) channel-last with a ZERO one-pixel border (interior by the tiled transpose kernel,
    border by four thin fills): what `F.pad(nchw_to_nhwc(x), (0, 0, 1, 1, 1, 1))` returns, without the 1-GB padding copy."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise CggError('nchw_to_nhwc_pad1: (B, C, H, W) float32 ROCm tensor expected')
    B, C, H, W = x.shape
    x = x.contiguous()
    y = zero_border_map(B, H, W, C, x.device)
    _call('cgg_nchw_to_nhwc_pad1_f32', dev_ptr(x), dev_ptr(y), B, C, H, W, stream_ptr(x.device))
    return y


def nhwc_to_nchw(x):
    """(B, H, W, C) contiguous f32 -> (B, C, H, W) contiguous."""
    B, H, W, C = x.shape
    return transpose_f32(x.view(B, H * W, C)).view(B, C, H, W)


def wgrad_x3(dy, x, want_bias=False, amax=None):
    """dW (N, K) = dy^T x for dy (M, N), x (M, K) f32 rows (contiguous last dim, row strides % 4 == 0; N, K % 4 == 0) on the
    f32-class f16 x 3 contraction with transpose reads (csrc/wgrad_x3.hip): the weight gradient of a linear layer.
    want_bias: -> (dW, db) with db (N) = dy.sum(0) from the same pass over dy. amax: device scalar max |dy| (`absmax`) -> dy is
    pre-scaled per tensor instead of by the fixed 2^4 (gradients are not unit scale, csrc/x3.h)."""
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0] or dy.dtype != torch.float32 or x.dtype != torch.float32 \
            or dy.stride(1) != 1 or x.stride(1) != 1:
        raise CggError('wgrad_x3: dy (M, N) and x (M, K) must be float32 matrices with contiguous rows')
    M, N = dy.shape
    K = x.shape[1]
    pdy, px = dev_ptr(dy, 'dy', torch.float32, dense=False), dev_ptr(x, 'x', torch.float32, dense=False)
    nbytes = _lib_().cgg_wgrad_x3_workspace_bytes(M, N, K)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device)
    splits = ctypes.c_int(0)
    wsb = torch.empty((nbytes // (4 * N * K)) * N, dtype=torch.float32, device=dy.device) if want_bias else None
    with _timed('wgrad_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * N + M * K + N * K), shape=(M, N, K)):
        if amax is not None:
            _call('cgg_wgrad_x3_scaled', pdy, dy.stride(0), dev_ptr(amax, 'amax', torch.float32), px, x.stride(0), dev_ptr(ws),
                  dev_ptr(wsb), ctypes.byref(splits), M, N, K, stream_ptr(dy.device))
        elif want_bias:
            _call('cgg_wgrad_bias_x3', pdy, dy.stride(0), px, x.stride(0), dev_ptr(ws), dev_ptr(wsb), ctypes.byref(splits), M, N, K,
                  stream_ptr(dy.device))
        else:
            _call('cgg_wgrad_x3', pdy, dy.stride(0), px, x.stride(0), dev_ptr(ws), ctypes.byref(splits), M, N, K, stream_ptr(dy.device))
    gw = ws.view(splits.value, N, K).sum(0) if splits.value > 1 else ws.view(N, K).clone()
    if want_bias:
        return gw, wsb.view(-1, N)[:splits.value].sum(0)
    return gw


def gemm_x3_split(a, packed, N, col2, bias=None, res_table=None):
    """a (M, K) f32 rows x x3 image of an (N, K) weight -> (y1 (M, col2), y2 (M, N - col2)) = column blocks of
    a W^T + bias + res_table[row % len(res_table)] (res_table (R, N) f32 | None), one launch (`cgg_gemm_x3_ex`)."""
    if a.dim() != 2 or a.stride(1) != 1 or a.dtype != torch.float32 or not is_x3(packed):
        raise CggError('gemm_x3_split: a must be a 2-D float32 tensor with a contiguous last dim, packed an x3 image')
    M, K = a.shape
    _x3_check(packed, N, K, 'gemm_x3_split')
    y1 = torch.empty((M, col2), dtype=torch.float32, device=a.device)
    y2 = torch.empty((M, N - col2), dtype=torch.float32, device=a.device)
    if res_table is not None and (res_table.dim() != 2 or res_table.shape[1] != N or not res_table.is_contiguous()
                                  or res_table.dtype != torch.float32):
        raise CggError('gemm_x3_split: res_table must be a contiguous (R, N) float32 tensor')
    with _timed('gemm_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * K + M * N + N * K), shape=(M, N, K)):
        _call('cgg_gemm_x3_ex', dev_ptr(a, 'a', torch.float32, dense=False), a.stride(0), dev_ptr(packed),
              dev_ptr(bias, 'bias', torch.float32), dev_ptr(res_table), N if res_table is not None else 0,
              res_table.shape[0] if res_table is not None else 0, dev_ptr(y1), col2, dev_ptr(y2), N - col2, int(col2), M, N, K, 0,
              stream_ptr(a.device))
    return y1, y2


def gemm_x3_table(a, packed, N, res_table, bias=None, out=None):
    """a (M, K) f32 rows x x3 image of an (N, K) weight -> a W^T + bias + res_table[row % len(res_table)] (M, N) f32, one launch
    (`cgg_gemm_x3_ex` with a row-periodic residual): a linear layer whose bias is a per-token table shared by the images of a batch."""
    if a.dim() != 2 or a.stride(1) != 1 or a.dtype != torch.float32 or not is_x3(packed):
        raise CggError('gemm_x3_table: a must be a 2-D float32 tensor with a contiguous last dim, packed an x3 image')
    M, K = a.shape
    _x3_check(packed, N, K, 'gemm_x3_table')
    if res_table.dim() != 2 or res_table.shape[1] != N or not res_table.is_contiguous() or res_table.dtype != torch.float32 \
            or M % res_table.shape[0]:
        raise CggError('gemm_x3_table: res_table must be a contiguous (R, N) float32 tensor with R dividing the row count')
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    if y.shape != (M, N) or not y.is_contiguous() or y.dtype != torch.float32:
        raise CggError('gemm_x3_table: bad `out`')
    with _timed('gemm_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * K + M * N + N * K), shape=(M, N, K)):
        _call('cgg_gemm_x3_ex', dev_ptr(a, 'a', torch.float32, dense=False), a.stride(0), dev_ptr(packed),
              dev_ptr(bias, 'bias', torch.float32), dev_ptr(res_table), N, res_table.shape[0], dev_ptr(y), N, None, 0, 0, M, N, K, 0,
              stream_ptr(a.device))
    return y


def conv_x3_nhwc(x, packed, N, kernel, stride=1, pad=0, bias=None, res=None, relu=False, amax=None):
    """x (B, H, W, C) f32 channel-last (contiguous) -> act(conv + bias (+ res)) (B, OH, OW, N) f32 as an implicit GEMM on the
    x3 image made by `pack_conv_weight_x3` (C % 32 == 0). amax: device scalar max |x| -> per-tensor pre-scale (gradient maps)."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float32 or not x.is_cuda or not is_x3(packed):
        raise CggError('conv_x3_nhwc: x must be a contiguous (B, H, W, C) float32 ROCm tensor, packed an x3 image')
    B, H, W, C = x.shape
    KH, KW = (kernel, kernel) if isinstance(kernel, int) else kernel
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    _x3_check(packed, N, C * KH * KW, 'conv_x3_nhwc')
    y = torch.empty((B, OH, OW, N), dtype=torch.float32, device=x.device)
    if res is not None and (tuple(res.shape) != (B, OH, OW, N) or not res.is_contiguous() or res.dtype != torch.float32):
        raise CggError('conv_x3_nhwc: res must be a contiguous (B, OH, OW, N) float32 tensor')
    with _timed('gemm_x3', flops=2.0 * B * OH * OW * N * C * KH * KW,
                bytes=4.0 * (B * H * W * C + B * OH * OW * N * (2 if res is not None else 1) + N * C * KH * KW),
                shape=(B * OH * OW, N, C * KH * KW)):
        if amax is not None:
            _call('cgg_conv_x3_nhwc_scaled', dev_ptr(x), dev_ptr(amax, 'amax', torch.float32), dev_ptr(packed),
                  dev_ptr(bias, 'bias', torch.float32), dev_ptr(res), dev_ptr(y), B, H, W, C, N, KH, KW, int(stride), int(pad),
                  int(bool(relu)), stream_ptr(x.device))
        else:
            _call('cgg_conv_x3_nhwc', dev_ptr(x), dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32), dev_ptr(res), dev_ptr(y), B, H,
                  W, C, N, KH, KW, int(stride), int(pad), int(bool(relu)), stream_ptr(x.device))
    return y


# ---- round 4: pre-split activation rows ("x3a", csrc/x3.h) and the LDS-DMA GEMM that consumes them (csrc/x3s_gemm.hip) ----
X3A_F32, X3A_SPLIT = 1, 2


class X3ATensor(torch.Tensor):
    """float32-tagged tensor whose storage holds x3a rows (csrc/x3.h: per 8 channels [8 f16 hi | 8 f16 lo] of 16 x): the marker
    the stream modules hand each other (a ResNet's parity-mode outputs, the encoder memories). Views keep the tag; arithmetic on
    it is meaningless -- `x3a_to_f32` gives the values."""


def is_x3a(t):
    return isinstance(t, X3ATensor)


def as_x3a(t):
    return t.as_subclass(X3ATensor)


def x3a_to_f32(t):
    """values of an x3a-tagged tensor whose channel dim is contiguous in memory (e.g. the (B, C, H, W)-shaped permuted view of a
    channel-last map) -> plain float32 tensor of the same shape."""
    base = t.as_subclass(torch.Tensor)
    if base.dim() == 4 and base.stride(1) == 1 and not base.is_contiguous():      # (B, C, H, W) view of (B, H, W, C)
        return x3a_decode(base.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    return x3a_decode(base.contiguous())


def x3a_encode(x):
    """f32 tensor (contiguous, numel % 8 == 0, channel groups of 8 contiguous) -> x3a tensor of the same shape / dtype tag
    (float32 storage holding [8 f16 hi | 8 f16 lo] of 16 x per group)."""
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.numel() % 8:
        raise CggError('x3a_encode: contiguous float32 ROCm tensor with numel % 8 == 0 expected')
    y = torch.empty_like(x)
    _call('cgg_x3a_encode', dev_ptr(x), dev_ptr(y), x.numel(), stream_ptr(x.device))
    return y


def x3a_decode(x):
    """x3a tensor -> the f32 values it stands for (22 significant bits)."""
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.numel() % 8:
        raise CggError('x3a_decode: contiguous float32-tagged ROCm tensor with numel % 8 == 0 expected')
    y = torch.empty_like(x)
    _call('cgg_x3a_decode', dev_ptr(x), dev_ptr(y), x.numel(), stream_ptr(x.device))
    return y


def x3_overflow_check(device, reset=True):
    """-> True if an x3a producer on `device` has stored a value outside f16's range (|a| >= 4094) since the last reset.
    Synchronises the current stream."""
    v = ctypes.c_int(0)
    with torch.cuda.device(device):
        _call('cgg_x3_overflow_check', int(bool(reset)), ctypes.byref(v), stream_ptr(device))
    return v.value != 0


def _x3s_fmt(split):
    return X3A_SPLIT if split else X3A_F32


def gemm_x3s(a, packed, N, bias=None, res=None, res_split=False, res_mod=0, relu=False, out=None, out_split=False, cfg=-1):
    """a (M, K) x3a rows (row stride free, multiples of 8) x x3 image -> act(a W^T + bias (+ res)) (M, N), f32 or x3a
    (`out_split`); res (M, N) | (res_mod, N) in f32 or x3a (`res_split`). csrc/x3s_gemm.hip."""
    if a.dim() not in (2, 3) or a.stride(-1) != 1 or a.dtype != torch.float32 or not is_x3(packed):
        raise CggError('gemm_x3s: a must be a 2-D / 3-D float32-tagged tensor with a contiguous last dim, packed an x3 image')
    rpb, bstride = 0, 0
    if a.dim() == 3:                    # (B, R, K) view of a stack of images (row stride and image stride free): rows = B * R
        rpb, bstride = int(a.shape[1]), int(a.stride(0))
        M, K, lda = a.shape[0] * a.shape[1], a.shape[2], int(a.stride(1))
    else:
        (M, K), lda = a.shape, int(a.stride(0))
    _x3_check(packed, N, K, 'gemm_x3s')
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    if y.dim() != 2 or y.stride(1) != 1 or y.shape != (M, N) or y.dtype != torch.float32:
        raise CggError('gemm_x3s: bad `out` view')
    if res is not None and (res.dim() != 2 or res.stride(1) != 1 or res.shape != ((res_mod or M), N) or res.dtype != torch.float32):
        raise CggError('gemm_x3s: bad `res` view')
    with _timed('gemm_x3', flops=2.0 * M * N * K, bytes=4.0 * (M * K + M * N * (2 if res is not None and not res_mod else 1)) +
                4.0 * N * K, shape=(M, N, K)):
        pa = dev_ptr(a, 'a', torch.float32, dense=False)
        # the operands after a and its image geometry are those of both entry points
        rest = (dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32), dev_ptr(res, 'res', torch.float32, dense=False),
                res.stride(0) if res is not None else 0, 0 if res is None else _x3s_fmt(res_split), int(res_mod),
                dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), _x3s_fmt(out_split), M, N, K, int(bool(relu)))
        if rpb:
            _call('cgg_gemm_x3s_batched', pa, lda, rpb, bstride, *rest, stream_ptr(a.device))
        else:
            _call('cgg_gemm_x3s_cfg', pa, lda, *rest, int(cfg), stream_ptr(a.device))
    return y


def conv_x3s_nhwc(x, packed, N, kernel, stride=1, pad=0, bias=None, res=None, res_split=True, relu=False, out_split=True, cfg=-1):
    """x (B, H, W, C) x3a channel-last -> act(conv + bias (+ res)) (B, OH, OW, N), x3a (default) or f32: implicit GEMM on the
    x3 image made by `pack_conv_weight_x3` (C % 32 == 0)."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float32 or not x.is_cuda or not is_x3(packed):
        raise CggError('conv_x3s_nhwc: x must be a contiguous (B, H, W, C) float32-tagged ROCm tensor, packed an x3 image')
    B, H, W, C = x.shape
    KH, KW = (kernel, kernel) if isinstance(kernel, int) else kernel
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    _x3_check(packed, N, C * KH * KW, 'conv_x3s_nhwc')
    y = torch.empty((B, OH, OW, N), dtype=torch.float32, device=x.device)
    if res is not None and (tuple(res.shape) != (B, OH, OW, N) or not res.is_contiguous() or res.dtype != torch.float32):
        raise CggError('conv_x3s_nhwc: res must be a contiguous (B, OH, OW, N) float32-tagged tensor')
    with _timed('gemm_x3', flops=2.0 * B * OH * OW * N * C * KH * KW,
                bytes=4.0 * (B * H * W * C + B * OH * OW * N * (2 if res is not None else 1) + N * C * KH * KW),
                shape=(B * OH * OW, N, C * KH * KW)):
        _call('cgg_conv_x3s_nhwc_cfg', dev_ptr(x), dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32), dev_ptr(res),
              0 if res is None else _x3s_fmt(res_split), dev_ptr(y), _x3s_fmt(out_split), B, H, W, C, N, KH, KW, int(stride), int(pad),
              int(bool(relu)), int(cfg), stream_ptr(x.device))
    return y


def pack_linear_weight(weight):
    """weight (N, K) f32 -> opaque packed bf16 buffer for `linear_rows_bf16` (uint8 tensor)."""
    N, K = weight.shape
    nbytes = _lib_().cgg_linear_rows_packed_bytes(N, K)
    if nbytes <= 0:
        raise CggError(f'pack_linear_weight: unsupported shape {tuple(weight.shape)} (K % 16)')
    out = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
    w = weight.detach().float().contiguous()
    _call('cgg_linear_rows_pack', dev_ptr(w, 'weight', torch.float32), dev_ptr(out), N, K, stream_ptr(weight.device))
    return out


def linear_rows_bf16(x, packed, N, bias=None, res=None, relu_cols=0, ln=None, pos=None, want_pos=False, ksplit=1,
                     out=None):
    """x (M, K) f32 rows (row stride free, last dim contiguous) @ packed weight -> y (M, N) f32.
    ln = (gamma, beta, eps) fuses a LayerNorm over the N <= 256 outputs; pos (rows, N) with want_pos returns
    (y, y + pos[row % rows]). `out` may be a 2-D view with its own row stride. ksplit > 1 returns the (ksplit, M, N)
    split-K partial planes (bias / res in plane 0) for `layernorm_chain` to add."""
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
        raise CggError('linear_rows_bf16: x must be a 2-D float32 tensor with a contiguous last dim')
    M, K = x.shape
    symbol = _x3_fn('linear_rows', packed)
    if ksplit > 1:
        if out is not None or want_pos or ln is not None or relu_cols:
            raise CggError('linear_rows_bf16: split-K returns (ksplit, M, N) partial planes; no out / ln / pos / relu')
        y = torch.empty((int(ksplit), M, N), dtype=torch.float32, device=x.device)
        _call(symbol, dev_ptr(x, 'x', torch.float32, dense=False), x.stride(0), dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32),
              dev_ptr(res, 'res', torch.float32, dense=False), res.stride(0) if res is not None else 0, dev_ptr(y), N, None, None, 0.0,
              None, 0, None, 0, M, N, K, 0, int(ksplit), None, 0, 0, None, 0, 0, stream_ptr(x.device))
        return y
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=x.device)
    if y.dim() != 2 or y.stride(1) != 1 or y.shape != (M, N) or y.dtype != torch.float32:
        raise CggError('linear_rows_bf16: bad `out` view')
    if res is not None and (res.dim() != 2 or res.stride(1) != 1 or res.shape != (M, N)):
        raise CggError('linear_rows_bf16: bad `res` view')
    yp = torch.empty((M, N), dtype=torch.float32, device=x.device) if want_pos else None
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    _call(symbol, dev_ptr(x, 'x', torch.float32, dense=False), x.stride(0), dev_ptr(packed), dev_ptr(bias, 'bias', torch.float32),
          dev_ptr(res, 'res', torch.float32, dense=False), res.stride(0) if res is not None else 0,
          dev_ptr(y, 'out', torch.float32, dense=False), y.stride(0), dev_ptr(g, 'gamma', torch.float32),
          dev_ptr(b, 'beta', torch.float32), float(eps), dev_ptr(pos, 'pos', torch.float32) if want_pos else None,
          pos.shape[0] if want_pos else 0, dev_ptr(yp), N if want_pos else 0, M, N, K, int(relu_cols), int(ksplit), None, 0, 0, None, 0,
          0, stream_ptr(x.device))
    return (y, yp) if want_pos else y


def linear_rows_bf16_qkv(xqk, xv, packed, bias, E):
    """Self-attention projections as ONE launch over the concatenated packed [Wq; Wk; Wv] (3E x E, E % 256 == 0):
    q, k from xqk (= query + query_pos), v from xv (= query); all (M, E) f32 rows -> (q (M, E), kv (M, 2E))."""
    M, K = xqk.shape
    for t in (xqk, xv):
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32 or t.shape != (M, K):
            raise CggError('linear_rows_bf16_qkv: inputs must be matching 2-D float32 tensors')
    if E % 256:
        raise CggError('linear_rows_bf16_qkv: E must be a multiple of 256')
    q = torch.empty((M, E), dtype=torch.float32, device=xqk.device)
    kv = torch.empty((M, 2 * E), dtype=torch.float32, device=xqk.device)
    _call(_x3_fn('linear_rows', packed), dev_ptr(xqk, 'xqk', torch.float32, dense=False), xqk.stride(0), dev_ptr(packed),
          dev_ptr(bias, 'bias', torch.float32), None, 0, dev_ptr(q), E, None, None, 0.0, None, 0, None, 0, M, 3 * E, K, 0, 1,
          dev_ptr(xv, 'xv', torch.float32, dense=False), xv.stride(0), 2 * E, dev_ptr(kv), 2 * E, E, stream_ptr(xqk.device))
    return q, kv


def layernorm_chain(a, norm_a, pos=None, norm_b=None):
    """a (M, N) f32 -> (y = LN_a(a), yp = y + pos[row % len(pos)] | None, z = LN_b(y) | None); norm_* are
    (gamma, beta, eps) triples."""
    nsum, plane = 1, 0
    if a.dim() == 3:                       # split-K partial planes (nsum, M, N): summed in the kernel, fixed order
        if not a.is_contiguous():
            raise CggError('layernorm_chain: partial planes must be contiguous')
        nsum, plane = a.shape[0], a.shape[1] * a.shape[2]
        a = a[0]
    M, N = a.shape
    if a.stride(1) != 1:
        raise CggError('layernorm_chain: last dim must be contiguous')
    y = torch.empty((M, N), dtype=torch.float32, device=a.device)
    yp = torch.empty_like(y) if pos is not None else None
    z = torch.empty_like(y) if norm_b is not None else None
    gb, bb, eb = norm_b if norm_b is not None else (None, None, 0.0)
    _call('cgg_layernorm_chain', dev_ptr(a, 'a', torch.float32, dense=False), a.stride(0), dev_ptr(norm_a[0], 'gamma', torch.float32),
          dev_ptr(norm_a[1], 'beta', torch.float32), float(norm_a[2]), dev_ptr(pos, 'pos', torch.float32),
          pos.shape[0] if pos is not None else 0, dev_ptr(gb, 'gamma_b', torch.float32), dev_ptr(bb, 'beta_b', torch.float32),
          float(eb), dev_ptr(y), dev_ptr(yp), dev_ptr(z), M, N, int(nsum), int(plane), stream_ptr(a.device))
    return y, yp, z


def decoder_mid(core, wo, bo, res, norm, pos=None, qkv=None):
    """x1 = LN(core @ Wo^T + bo + res) on (M, 256) f32 rows; with qkv = (packed [Wq; Wk; Wv], bias (768,)) and pos (Q, 256)
    also q = (x1 + pos) Wq^T + bq (M, 256) and kv = [(x1 + pos) Wk^T + bk | x1 Wv^T + bv] (M, 512). -> (x1, q, kv)."""
    M, C = core.shape
    for t in (core, res):
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32 or t.shape != (M, C):
            raise CggError('decoder_mid: core / res must be matching (M, C) float32 rows')
    dev = core.device
    x1 = torch.empty((M, C), dtype=torch.float32, device=dev)
    q = kv = None
    wqkv = bqkv = None
    if qkv is not None:
        wqkv, bqkv = qkv
        q = torch.empty((M, C), dtype=torch.float32, device=dev)
        kv = torch.empty((M, 2 * C), dtype=torch.float32, device=dev)
    _call(_x3_fn('decoder_mid', wo, wqkv), dev_ptr(core, 'core', torch.float32, dense=False), core.stride(0), dev_ptr(wo),
          dev_ptr(bo, 'bo', torch.float32), dev_ptr(res, 'res', torch.float32, dense=False), res.stride(0),
          dev_ptr(norm[0], 'gamma', torch.float32), dev_ptr(norm[1], 'beta', torch.float32), float(norm[2]),
          dev_ptr(pos, 'pos', torch.float32), pos.shape[0] if pos is not None else 0, dev_ptr(wqkv),
          dev_ptr(bqkv, 'bqkv', torch.float32), dev_ptr(x1), dev_ptr(q), dev_ptr(kv), M, C, stream_ptr(dev))
    return x1, q, kv


def decoder_ffn(x, w1, b1, w2, b2, F):
    """x (M, 256) f32 rows -> (F / 256, M, 256) partial planes of x + relu(x W1^T + b1) W2^T + b2 (sum them in plane
    order: `decoder_tail` / `layernorm_chain`). w1 (F x 256), w2 (256 x F) packed by `pack_linear_weight`."""
    M, C = x.shape
    if x.stride(1) != 1 or x.dtype != torch.float32 or F % 256:
        raise CggError('decoder_ffn: x must be (M, C) float32 rows and F a multiple of 256')
    planes = torch.empty((F // 256, M, C), dtype=torch.float32, device=x.device)
    _call(_x3_fn('decoder_ffn', w1, w2), dev_ptr(x, 'x', torch.float32, dense=False), x.stride(0), dev_ptr(w1),
          dev_ptr(b1, 'b1', torch.float32), dev_ptr(w2), dev_ptr(b2, 'b2', torch.float32), dev_ptr(planes), M, C, int(F),
          stream_ptr(x.device))
    return planes


def self_attn_rows_bf16(q, kv, B, num_heads, scale=None):
    """q (M, E), kv (M, 2E) f32 rows (M = B*Q, Q <= 128, head dim 32) -> softmax(scale q k^T) v, (M, E) f32."""
    M, E = q.shape
    D = E // num_heads
    if q.stride(1) != 1 or kv.stride(1) != 1 or kv.shape != (M, 2 * E) or q.dtype != torch.float32 or kv.dtype != torch.float32:
        raise CggError('self_attn_rows_bf16: q (M, E) / kv (M, 2E) float32 rows expected')
    out = torch.empty((M, E), dtype=torch.float32, device=q.device)
    _call('cgg_self_attn_rows_bf16', dev_ptr(q, 'q', torch.float32, dense=False), q.stride(0),
          dev_ptr(kv, 'kv', torch.float32, dense=False), kv.stride(0), dev_ptr(out), B, M // B, num_heads, D,
          float(scale if scale is not None else D ** -0.5), stream_ptr(q.device))
    return out


DECODER_TAIL_MAX_PLANES = CONSTANTS['CGG_DECODER_TAIL_MAX_PLANES']   # more planes are refused (CGG_EUNSUPPORTED), not dropped


def decoder_tail(planes, norm_a, pos, norm_b, mlp, qproj=None, want_pos=False):
    """planes (nsum, M, 256) f32 (FFN split-K partials, bias + residual in plane 0), nsum <= DECODER_TAIL_MAX_PLANES ->
    (y = LN_a(sum), y + pos | None, mask_embed = MLP3(LN_b(y)), qn = Wq (y + pos) + bq | None). norm_* = (gamma, beta, eps);
    mlp = (w1, b1, w2, b2, w3, b3) and qproj = (wq, bq) with weights packed by `pack_linear_weight` (256 x 256)."""
    if planes.dim() != 3 or not planes.is_contiguous() or planes.dtype != torch.float32:
        raise CggError('decoder_tail: planes must be a contiguous (nsum, M, C) float32 tensor')
    nsum, M, C = planes.shape
    dev = planes.device
    y = torch.empty((M, C), dtype=torch.float32, device=dev)
    yp = torch.empty_like(y) if want_pos else None
    me = torch.empty_like(y)
    qn = torch.empty_like(y) if qproj is not None else None
    wq, bq = qproj if qproj is not None else (None, None)
    _call(_x3_fn('decoder_tail', mlp[0], mlp[2], mlp[4], wq), dev_ptr(planes), nsum, M * C, C,
          dev_ptr(norm_a[0], 'gamma_a', torch.float32), dev_ptr(norm_a[1], 'beta_a', torch.float32), float(norm_a[2]),
          dev_ptr(pos, 'pos', torch.float32), pos.shape[0], dev_ptr(norm_b[0], 'gamma_b', torch.float32),
          dev_ptr(norm_b[1], 'beta_b', torch.float32), float(norm_b[2]), dev_ptr(mlp[0]), dev_ptr(mlp[1], 'b1', torch.float32),
          dev_ptr(mlp[2]), dev_ptr(mlp[3], 'b2', torch.float32), dev_ptr(mlp[4]), dev_ptr(mlp[5], 'b3', torch.float32), dev_ptr(wq),
          dev_ptr(bq, 'bq', torch.float32), dev_ptr(y), dev_ptr(yp), dev_ptr(me), dev_ptr(qn), M, C, stream_ptr(dev))
    return y, yp, me, qn


def masked_xattn_bf16(q, k, vt, bits, num_heads, scale=None, fix_full_rows=False):
    """q (B,Q,E) f32; k (B,S,E) bf16; vt (B,E,S) bf16 (value projection, transposed); bits as `masked_xattn`.
    fix_full_rows: rows whose mask blocks every key attend to all keys (what `attn_mask_fix_full_rows` does to `bits`
    beforehand), decided inside the kernels; `bits` itself is not modified."""
    B, Q, E = q.shape
    if Q > 128:
        return torch.cat([masked_xattn_bf16(q[:, s:s + 128].contiguous(), k, vt,
                                            None if bits is None else bits[:, s:s + 128].contiguous(), num_heads,
                                            scale, fix_full_rows) for s in range(0, Q, 128)], 1)
    S = k.shape[1]
    H = int(num_heads)
    D = E // H
    if tuple(k.shape) != (B, S, E) or tuple(vt.shape) != (B, E, S):
        raise CggError(f'masked_xattn_bf16: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not match q {tuple(q.shape)}')
    # k may be a column slice of a wider (B, S, n*E) projection, vt a row block of a taller (B, n*E, S) one
    if k.stride(2) != 1 or k.stride(0) != S * k.stride(1) or vt.stride(2) != 1 or vt.stride(1) != S or \
            k.dtype != torch.bfloat16 or vt.dtype != torch.bfloat16:
        raise CggError('masked_xattn_bf16: unsupported k / vt strides or dtype')
    ldk, vtb = k.stride(1), vt.stride(0)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    pq = dev_ptr(q, 'q', torch.float32)       # refuses CPU tensors before any torch.cuda call
    ws = _xattn_ws(_lib_().cgg_masked_xattn_workspace_bytes, q, B, Q, H, D, S)
    out = torch.empty((B, Q, E), dtype=torch.float32, device=q.device)
    _call('cgg_masked_xattn_forward_bf16', pq, dev_ptr(k, 'k', torch.bfloat16, dense=False),
          dev_ptr(vt, 'vt', torch.bfloat16, dense=False), dev_ptr(bits, 'bits', torch.int32), dev_ptr(out), dev_ptr(ws), B, Q, H, D, S,
          float(scale), int(ldk), int(vtb), int(bool(fix_full_rows)), stream_ptr(q.device))
    return out


def instance_masks_multi(logits, index_lists, up_size, crop_size, out_size):
    """logits (Q,H,W) f32 low-res; index_lists = [query indices (n_t,) long, ...] (one per evaluation type)
    -> ([masks (n_t,oh,ow) bool ...], mask_score (Q,), bbox (Q,4)). Every picked query's mask is interpolated ONCE and
    written to all its detections; score / bbox are per QUERY (index them with the query indices)."""
    Q, H, W = logits.shape
    oh, ow = int(out_size[0]), int(out_size[1])
    dev = logits.device
    sizes = [int(ix.numel()) for ix in index_lists]
    total = sum(sizes)
    score = torch.empty((Q,), dtype=torch.float32, device=dev)
    bbox = torch.empty((Q, 4), dtype=torch.float32, device=dev)
    masks = torch.empty((total, oh, ow), dtype=torch.uint8, device=dev)
    if total == 0:
        return [masks[:0].view(torch.bool) for _ in sizes], score, bbox
    cat = torch.cat([ix.reshape(-1) for ix in index_lists]) if len(index_lists) > 1 else index_lists[0].reshape(-1)
    order = torch.argsort(cat, stable=True).to(torch.int32)
    # (torch.bincount synchronises to size its output -> not capturable in a hipGraph; scatter_add is)
    counts = torch.zeros((Q,), dtype=torch.int32, device=dev).scatter_add_(
        0, cat, torch.ones_like(cat, dtype=torch.int32))
    off = torch.zeros((Q + 1,), dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(counts, 0)
    ws = torch.empty((Q, 8), dtype=torch.int32, device=dev)
    _call('cgg_instance_masks_multi', dev_ptr(logits, 'logits', torch.float32), dev_ptr(off), dev_ptr(order), dev_ptr(masks),
          dev_ptr(score), dev_ptr(bbox), dev_ptr(ws), Q, H, W, int(up_size[0]), int(up_size[1]), int(crop_size[0]), int(crop_size[1]),
          oh, ow, stream_ptr(dev))
    out, o = [], 0
    for n in sizes:
        out.append(masks[o:o + n].view(torch.bool))
        o += n
    return out, score, bbox


def class_topk(dots, B, col0, ncols, k):
    """dots (B*Q, ld) f32 class-embedding dot products against concatenated class tables; evaluation type t owns columns
    col0[t] .. col0[t]+ncols[t] (last = background). -> (labels, scores, query indices), each (B, T, k): the k best
    (query, class) pairs of softmax(dots_t)[:, :-1], descending score (ties: ascending flat index)."""
    rows, ld = dots.shape
    Q, T = rows // B, len(col0)
    dev = dots.device
    labels = torch.empty((B, T, k), dtype=torch.int64, device=dev)
    qidx = torch.empty((B, T, k), dtype=torch.int64, device=dev)
    scores = torch.empty((B, T, k), dtype=torch.float32, device=dev)
    _call('cgg_class_topk', dev_ptr(dots, 'dots', torch.float32), ld, B, Q, T, _int_array(col0), _int_array(ncols), int(k),
          dev_ptr(labels), dev_ptr(scores), dev_ptr(qidx), stream_ptr(dev))
    return labels, scores, qidx


def class_topk_supported(Q, ncols, k):
    return (0 < k <= 1024 and 1 <= len(ncols) <= 8 and all(n >= 2 and k <= Q * (n - 1) for n in ncols)
            and 8 * k + 4 * Q * (max(ncols) - 1) + 4 * Q <= 62 * 1024)


def instance_masks_picks(logits, qidx, cls_scores, up_size, crop_size, out_size, bitpack=False):
    """logits (Q,H,W) f32 low-res; qidx (n,) long / cls_scores (n,) f32: the picks of ALL evaluation types of one image
    -> masks (n,oh,ow) bool, bboxes (n,5) f32 = (box of the picked query, class score x mask score)."""
    Q, H, W = logits.shape
    oh, ow = int(out_size[0]), int(out_size[1])
    dev = logits.device
    n = int(qidx.numel())
    if bitpack and ow % 16:
        raise CggError('instance_masks_picks: bit-packed masks need out_w % 16 == 0')
    masks = torch.empty((n, oh, ow // 8 if bitpack else ow), dtype=torch.uint8, device=dev)
    bboxes = torch.empty((n, 5), dtype=torch.float32, device=dev)
    ws = torch.empty((int(_lib_().cgg_instance_masks_picks_workspace_bytes(Q, n)) + 3) // 4, dtype=torch.int32, device=dev)
    _call('cgg_instance_masks_picks', dev_ptr(logits, 'logits', torch.float32), dev_ptr(qidx, 'qidx', torch.int64),
          dev_ptr(cls_scores, 'cls_scores', torch.float32), n, dev_ptr(masks), dev_ptr(bboxes), dev_ptr(ws), Q, H, W, int(up_size[0]),
          int(up_size[1]), int(crop_size[0]), int(crop_size[1]), oh, ow, int(bool(bitpack)), stream_ptr(dev))
    return (masks if bitpack else masks.view(torch.bool)), bboxes


def instance_masks_bitpack_ok(logits_hw, up_size, crop_size, out_size):
    """Shapes the bit-packed mask output supports: integer up-scale 2 / 4 / 8, no second resize, width % 16 == 0."""
    h, w = logits_hw
    s = up_size[0] // h if h else 0
    return (s in (2, 4, 8) and s * h == up_size[0] and s * w == up_size[1] and tuple(crop_size) == tuple(out_size)
            and out_size[1] % 16 == 0)


def bias_relu_maxpool_nhwc(x, bias):
    """x (B, H, W, C) channel-last bf16 raw convolution output -> relu(maxpool3x3/s2/p1(x) + bias) (B, Ho, Wo, C)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    _call('cgg_bias_relu_maxpool_nhwc', dev_ptr(x, 'x', torch.bfloat16), dev_ptr(bias, 'bias', torch.bfloat16), dev_ptr(y), B, H, W, C,
          stream_ptr(x.device))
    return y


_BLASLT_READY = False


def _blaslt_init():
    """dlopen the hipBLASLt copy torch itself uses (one library instance per process)."""
    global _BLASLT_READY
    if not _BLASLT_READY:
        import os
        cand = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libhipblaslt.so')
        path = cand if os.path.exists(cand) else 'libhipblaslt.so'
        _call('cgg_blaslt_init', path.encode())
        _call('cgg_blaslt_set_tuning', int(os.environ.get('CGG_GEMM_TUNE', '16')))
        _BLASLT_READY = True


def blaslt_last_tuning():
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    _lib_().cgg_blaslt_last_tuning(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def gemm_bias_res_act_bf16(x, w, bias, res=None, relu=True):
    """y = act(x @ w^T + bias + res): x (M, K), w (N, K), bias (N,), res (M, N) bf16 contiguous -> (M, N) bf16, one
    hipBLASLt call (residual through beta = 1, bias + ReLU in the epilogue)."""
    _blaslt_init()
    M, K = x.shape
    N = w.shape[0]
    for t, n in ((x, 'x'), (w, 'w'), (res, 'res'), (bias, 'bias')):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous()):
            raise CggError('gemm_bias_res_act_bf16: %s must be a contiguous bfloat16 tensor' % n)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    _call('cgg_gemm_bias_res_act_bf16', dev_ptr(x, 'x', torch.bfloat16), dev_ptr(w, 'w', torch.bfloat16), dev_ptr(bias), dev_ptr(res),
          dev_ptr(y), M, N, K, int(bool(relu)), stream_ptr(x.device))
    return y


def im2col3x3_nhwc(x, stride=1):
    """x (B, H, W, C) channel-last bf16 -> patch matrix (B * Ho * Wo, 9 * C) of a 3x3 / padding-1 convolution, columns
    ordered (ky, kx, c); returns (matrix, Ho, Wo)."""
    B, H, W, C = x.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise CggError('im2col3x3_nhwc: x must be a contiguous (B, H, W, C) bfloat16 tensor')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((B * Ho * Wo, 9 * C), dtype=torch.bfloat16, device=x.device)
    _call('cgg_im2col3x3_nhwc', dev_ptr(x), dev_ptr(y), B, H, W, C, int(stride), stream_ptr(x.device))
    return y, Ho, Wo


def pack_stem_weight(w):
    """w (64, 3, 7, 7) (BN already folded) -> bf16 MFMA A fragments for `stem_conv7x7` (uint8 tensor)."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise CggError(f'pack_stem_weight: expected (64, 3, 7, 7), got {tuple(w.shape)}')
    wk = torch.zeros((64, 7, 8, 3), dtype=torch.float32, device=w.device)      # (cout, ky, kx padded to 8, c)
    wk[:, :, :7, :] = w.detach().float().permute(0, 2, 3, 1)
    wk = torch.cat([wk.reshape(64, 168), torch.zeros((64, 8), dtype=torch.float32, device=w.device)], 1)   # K = 176
    frag = wk.view(2, 32, 11, 2, 8).permute(0, 2, 3, 1, 4).contiguous().to(torch.bfloat16)    # (mt, ks, hi, j, e)
    out = frag.view(torch.uint8).reshape(-1)
    assert out.numel() == _lib_().cgg_stem_conv7x7_packed_bytes()
    return out


def stem_conv7x7(img, packed):
    """img (B, 3, H, W) f32 NCHW -> raw 7x7 / stride-2 / padding-3 convolution (B, Ho, Wo, 64) bf16 channel-last."""
    B, C, H, W = img.shape
    if C != 3 or img.dtype != torch.float32 or not img.is_contiguous():
        raise CggError('stem_conv7x7: img must be a contiguous (B, 3, H, W) float32 tensor')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, 64), dtype=torch.bfloat16, device=img.device)
    _call('cgg_stem_conv7x7_nchw', dev_ptr(img), dev_ptr(packed), dev_ptr(y), B, H, W, stream_ptr(img.device))
    return y


def pack_stem_weight_x3(w):
    """w (64, 3, 7, 7) f32 (BN folded) -> (hi | lo f16 MFMA A fragments (uint8), un-scaling factors (64,) f32) for
    `stem_conv7x7_x3`: rows scaled by a power of two so that max |w'| is in [2^10, 2^11) (csrc/x3.h)."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise CggError(f'pack_stem_weight_x3: expected (64, 3, 7, 7), got {tuple(w.shape)}')
    wk = torch.zeros((64, 7, 8, 3), dtype=torch.float32, device=w.device)      # (cout, ky, kx padded to 8, c)
    wk[:, :, :7, :] = w.detach().float().permute(0, 2, 3, 1)
    wk = torch.cat([wk.reshape(64, 168), torch.zeros((64, 8), dtype=torch.float32, device=w.device)], 1)   # K = 176
    amax = wk.abs().amax(1).clamp_min(1e-30)
    e = torch.floor(torch.log2(amax)) + 1                                      # amax = f 2^e, f in [0.5, 1)
    s = torch.pow(2.0, 11 - e)
    ws = wk * s[:, None]
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    frag = lambda t: t.view(2, 32, 11, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(torch.uint8).reshape(-1)   # (mt, ks, hi, j, e)
    packed = torch.cat([frag(hi), frag(lo)])
    assert packed.numel() == 2 * _lib_().cgg_stem_conv7x7_packed_bytes()
    return packed, (1.0 / (s * 16.0)).float().contiguous()


def stem_conv7x7_x3(img, packed, wscale):
    """img (B, 3, H, W) f32 NCHW -> raw 7x7 / stride-2 / padding-3 convolution (B, Ho, Wo, 64) F32 channel-last, f32-class."""
    B, C, H, W = img.shape
    if C != 3 or img.dtype != torch.float32 or not img.is_contiguous():
        raise CggError('stem_conv7x7_x3: img must be a contiguous (B, 3, H, W) float32 tensor')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, 64), dtype=torch.float32, device=img.device)
    _call('cgg_stem_conv7x7_x3_nchw', dev_ptr(img), dev_ptr(packed), dev_ptr(wscale, 'wscale', torch.float32), dev_ptr(y), B, H, W,
          stream_ptr(img.device))
    return y


def bias_relu_maxpool_nhwc_f32(x, bias, x3a=False):
    """x (B, H, W, C) channel-last F32 raw convolution output -> relu(maxpool3x3/s2/p1(x) + bias) (B, Ho, Wo, C) f32, or the
    same map as x3a rows (`x3a=True`: the layout the x3s convolutions consume)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    _call('cgg_bias_relu_maxpool_nhwc_f32_x3a' if x3a else 'cgg_bias_relu_maxpool_nhwc_f32', dev_ptr(x, 'x', torch.float32),
          dev_ptr(bias, 'bias', torch.float32), dev_ptr(y), B, H, W, C, stream_ptr(x.device))
    return y


def linear_sum_assignment_batch(costs):
    """costs: list of 2-D float32 CPU tensors -> list of (rows, cols) int64 CPU tensors; every problem of a step in ONE
    call into the C++ solver (same indices as scipy.optimize.linear_sum_assignment, incl. ties)."""
    if not costs:
        return []
    flat = torch.cat([c.detach().to(device='cpu', dtype=torch.float32).contiguous().reshape(-1) for c in costs]) \
        if len(costs) > 1 else costs[0].detach().to(device='cpu', dtype=torch.float32).contiguous().reshape(-1)
    nr = [int(c.shape[0]) for c in costs]
    nc = [int(c.shape[1]) for c in costs]
    sizes = [min(a, b) for a, b in zip(nr, nc)]
    total = sum(sizes)
    rows = torch.empty((max(total, 1),), dtype=torch.int64)
    cols = torch.empty((max(total, 1),), dtype=torch.int64)
    _call('cgg_linear_sum_assignment_f32', host_ptr(flat, 'costs', torch.float32) if flat.numel() else None, len(costs), _int_array(nr),
          _int_array(nc), host_ptr(rows, 'rows', torch.int64), host_ptr(cols, 'cols', torch.int64))
    out, o = [], 0
    for n in sizes:
        out.append((rows[o:o + n], cols[o:o + n]))
        o += n
    return out


LSAP_MAX_SIDE = CONSTANTS['CGG_LSAP_MAX_SIDE']     # cgg_lsap_device_f32: sides of a problem
LSAP_OK, LSAP_INVALID, LSAP_INFEASIBLE, LSAP_BAD_DESCRIPTOR = 0, 1, 2, 3


def lsap_device_lds_bytes(nr, nc):
    """LDS one problem of `cgg_lsap_device_f32` needs: the staged f32 cost matrix plus the solver's state."""
    return int(_lib_().cgg_lsap_device_lds_bytes(int(nr), int(nc)))


def lsap_device_ok(nr, nc):
    """Gate of the device solver: both sides in 1 .. 1024 and the staged cost + state within the dynamic-LDS limit of the current
    device (gfx950's 160 KiB where there is none). Host arithmetic only."""
    nr, nc = int(nr), int(nc)
    if min(nr, nc) < 1 or max(nr, nc) > LSAP_MAX_SIDE:
        return False
    return lsap_device_lds_bytes(nr, nc) <= int(_lib_().cgg_dynamic_lds_limit())


def lsap_device_launch(cost_flat, desc, lds_bytes, q_out, g_out, status, gt_labels=None, labels=None, weights=None):
    """One launch of `cgg_lsap_device_f32`: cost_flat (f32), desc (P, 6) int64 (cost offset, nr, nc, output offset, label-row
    offset, gt-label offset) and every output on the device; lds_bytes = the largest `lsap_device_lds_bytes` of the table.
    Enqueues on the current stream and waits for nothing."""
    P = int(desc.shape[0])
    if P == 0:
        return
    if desc.dim() != 2 or desc.shape[1] != 6 or q_out.numel() != g_out.numel() or status.numel() != 2:
        raise CggError('lsap_device_launch: desc must be (P, 6), q_out / g_out of one size, status two words')
    if (gt_labels is None) != (labels is None) or (labels is None) != (weights is None):
        raise CggError('lsap_device_launch: the epilogue needs gt_labels, labels and weights together')
    if labels is not None and labels.numel() != weights.numel():
        raise CggError('lsap_device_launch: labels and weights must have one size')
    _call('cgg_lsap_device_f32', dev_ptr(cost_flat, 'cost_flat', torch.float32), cost_flat.numel(), dev_ptr(desc, 'desc', torch.int64),
          P, int(lds_bytes), dev_ptr(q_out, 'q_out', torch.int64), dev_ptr(g_out, 'g_out', torch.int64), q_out.numel(),
          dev_ptr(gt_labels, 'gt_labels', torch.int64), 0 if gt_labels is None else gt_labels.numel(),
          dev_ptr(labels, 'labels', torch.int64), dev_ptr(weights, 'weights', torch.float32), 0 if labels is None else labels.numel(),
          dev_ptr(status, 'status', torch.int32), stream_ptr(cost_flat.device))


def linear_sum_assignment_device(cost_flat, nr, nc):
    """cost_flat: the f32 row-major cost matrices of all problems, concatenated, on the device; problem p is nr[p] x nc[p]
    (host ints, every one inside `lsap_device_ok`). -> (rows, cols, status): int64 device tensors with min(nr[p], nc[p]) pairs
    per problem, concatenated in problem order, rows ascending (scipy's indices, ties included), and the two int32 status words
    [code, first failing problem + 1] for `lsap_status_check`. One launch (csrc/lsap_device.hip); nothing waits for the device."""
    nr, nc = [int(v) for v in nr], [int(v) for v in nc]
    if len(nr) != len(nc):
        raise CggError('linear_sum_assignment_device: nr and nc differ in length')
    dev = cost_flat.device
    table, coff, ooff, lds = [], 0, 0, 0
    for a, b in zip(nr, nc):
        if not lsap_device_ok(a, b):
            raise CggError(f'linear_sum_assignment_device: a {a} x {b} problem is outside lsap_device_ok')
        table.append((coff, a, b, ooff, 0, 0))
        coff += a * b
        ooff += min(a, b)
        lds = max(lds, lsap_device_lds_bytes(a, b))
    if cost_flat.dim() != 1 or cost_flat.numel() != coff:
        raise CggError(f'linear_sum_assignment_device: cost_flat has {cost_flat.numel()} elements, the problems {coff}')
    rows = torch.zeros((ooff,), dtype=torch.int64, device=dev)
    cols = torch.zeros((ooff,), dtype=torch.int64, device=dev)
    status = torch.zeros((2,), dtype=torch.int32, device=dev)
    if table:
        desc = torch.tensor(table, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        lsap_device_launch(cost_flat, desc, lds, rows, cols, status)
    return rows, cols, status


def lsap_status_check(status):
    """Reads the two status words of the device solver (this WAITS for the device) and raises, naming the problem, with the host
    solver's messages. `status`: the device tensor, or its two values."""
    code, where = (int(v) for v in (status.tolist() if torch.is_tensor(status) else status))
    if code == LSAP_OK:
        return
    what = {LSAP_INVALID: 'matrix contains invalid numeric entries', LSAP_INFEASIBLE: 'cost matrix is infeasible',
            LSAP_BAD_DESCRIPTOR: 'descriptor outside the buffers or the LDS of the launch'}.get(code, f'status {code}')
    raise CggError(f'cgg_lsap_device_f32: problem {where - 1}: {what}')


def point_sample_planes(planes, index, points):
    """planes (N, H, W) f32, index (rows,) int32, points (rows, P, 2) f32 in [0, 1] (x, y) -> (rows, P): row j = bilinear
    sample (grid_sample arithmetic, zeros outside) of planes[index[j]] at points[j]."""
    N, H, W = planes.shape
    rows, P, _ = points.shape
    out = torch.empty((rows, P), dtype=torch.float32, device=planes.device)
    if rows == 0:
        return out
    _call('cgg_point_sample_planes', dev_ptr(planes, 'planes', torch.float32), dev_ptr(index, 'index', torch.int32),
          dev_ptr(points.contiguous(), 'points', torch.float32), dev_ptr(out), N, H, W, rows, P, stream_ptr(planes.device))
    return out


class _PointSampleRowsFn(torch.autograd.Function):
    """out (rows, P) = bilinear samples of planes[j] (rows, H, W) f32 at points[j] (rows, P, 2) (grid_sample arithmetic, zeros
    outside, align_corners=False); differentiable wrt the planes only (the points are constants of the loss)."""

    @staticmethod
    def forward(ctx, planes, points):
        planes = planes.contiguous()
        points = points.contiguous()
        rows, H, W = planes.shape
        idx = torch.arange(rows, dtype=torch.int32, device=planes.device)
        ctx.save_for_backward(points)
        ctx.shape = (rows, H, W)
        return point_sample_planes(planes, idx, points)

    @staticmethod
    def backward(ctx, gout):
        (points,) = ctx.saved_tensors
        rows, H, W = ctx.shape
        if rows and rows <= 65535 and W <= 16384:
            # every row has its own plane: band-stationary LDS accumulation, planes written once (no zero-fill, no global atomics)
            gp = torch.empty((rows, H, W), dtype=torch.float32, device=gout.device)
            _call('cgg_point_sample_planes_backward_rows', dev_ptr(gout.contiguous().float(), 'grad', torch.float32),
                  dev_ptr(points, 'points', torch.float32), dev_ptr(gp), H, W, rows, points.shape[1], stream_ptr(gout.device))
            return gp, None
        gp = torch.zeros((rows, H, W), dtype=torch.float32, device=gout.device)
        if rows:
            _call('cgg_point_sample_planes_backward', dev_ptr(gout.contiguous().float(), 'grad', torch.float32), None,
                  dev_ptr(points, 'points', torch.float32), dev_ptr(gp), rows, H, W, rows, points.shape[1], stream_ptr(gout.device))
        return gp, None


def point_sample_rows(planes, points):
    """planes (rows, H, W) f32 (may require grad), points (rows, P, 2) f32 in [0, 1] -> (rows, P); == [3P] mmcv point_sample of
    planes.unsqueeze(1) at the same points (F.grid_sample bilinear / zeros / align_corners=False)."""
    return _PointSampleRowsFn.apply(planes, points)


def point_sample_rows_ok(planes, points):
    return (planes.is_cuda and planes.dtype == torch.float32 and planes.dim() == 3 and points.dim() == 3
            and points.dtype == torch.float32 and points.shape[0] == planes.shape[0] and points.shape[2] == 2)


def point_sample_nhwc(feat, points):
    """feat (B, H, W, C) f32 channel-last, points (B, P, 2) in [0, 1] (x, y) -> (B, P, C): [3P] mmcv point_sample
    (grid_sample bilinear / zeros / align_corners=False) with the layout that makes a point's taps contiguous rows."""
    B, H, W, C = feat.shape
    P = points.shape[1]
    if feat.dtype != torch.float32 or not feat.is_contiguous() or points.dtype != torch.float32 or tuple(points.shape) != (B, P, 2):
        raise CggError('point_sample_nhwc: feat (B, H, W, C) contiguous float32, points (B, P, 2) float32 expected')
    pts = points.contiguous()
    out = torch.empty((B, P, C), dtype=torch.float32, device=feat.device)
    _call('cgg_point_sample_nhwc', dev_ptr(feat), dev_ptr(pts), dev_ptr(out), B, H, W, C, P, stream_ptr(feat.device))
    return out


def point_sample_nhwc_x3_ok(feat, points, groups):
    """shapes `point_sample_nhwc_x3` covers. The sampler itself packs any C % 8 == 0, but its images have one consumer, `mask_logits`,
    which is built for C == 256: a feature of another width takes `point_sample_nhwc` + bmm."""
    return (feat.dim() == 4 and feat.dtype == torch.float32 and feat.is_cuda and feat.is_contiguous() and feat.shape[-1] == 256
            and points.dim() == 3 and points.dtype == torch.float32 and groups > 0
            and points.shape[1] % groups == 0 and (points.shape[1] // groups) % 32 == 0)


def point_sample_nhwc_x3(feat, points, groups):
    """feat (B, H, W, C) f32 channel-last, points (B, groups * P, 2) in [0, 1] (x, y), group g's points at [g P, (g + 1) P) ->
    [PackedFeature] * groups: the samples of group g as the x3 images of a (B, C, 1, P) "map" (`cgg_point_sample_nhwc_x3`: sampler and
    pack kernel in one, no f32 sample tensor) -- `mask_logits(embed_g, packed[g])` is then mask_embed_g . sample(feat) at the group's
    points, the training loss' point logits of one decoder layer, on the f32-class MFMA einsum."""
    B, H, W, C = feat.shape
    Pt = points.shape[1]
    if not point_sample_nhwc_x3_ok(feat, points, groups) or tuple(points.shape) != (B, Pt, 2):
        raise CggError('point_sample_nhwc_x3: feat (B, H, W, C) contiguous float32 (C == 256), points (B, groups * P, 2) float32 '
                       'with P % 32 == 0 expected')
    P = Pt // groups
    pts = points.contiguous()
    hi = torch.empty((groups * B, P // 32, C // 8, 32, 8), dtype=torch.bfloat16, device=feat.device)     # (16-bit pieces: f16 bits)
    lo = torch.empty_like(hi)
    _call('cgg_point_sample_nhwc_x3', dev_ptr(feat), dev_ptr(pts), dev_ptr(hi), dev_ptr(lo), B, H, W, C, Pt, P, stream_ptr(feat.device))
    return [PackedFeature(hi[g * B:(g + 1) * B], lo[g * B:(g + 1) * B], B, C, 1, P) for g in range(groups)]


def subsample_nhwc(x, stride):
    """x (B, H, W, C) channel-last bf16 -> x[:, ::stride, ::stride, :] as a new contiguous tensor."""
    B, H, W, C = x.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or C % 8:
        return x[:, ::stride, ::stride, :].contiguous()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    _call('cgg_subsample_nhwc', dev_ptr(x), dev_ptr(y), B, H, W, C, int(stride), stream_ptr(x.device))
    return y


# ------------------------------------------------------------------------------------------------
# input side: the reference's test pipeline on raw uint8 images (image_prep.py states the rule)
# ------------------------------------------------------------------------------------------------
# The staged-batch contract of the four entry families below, stated once. `staged` is a 1-D DEVICE uint8 buffer that carries the
# descriptor tables (int32 rows, by default back to back from byte `*_table_offset`) and the raw planes, moved with one H2D copy;
# every table is also handed over as a contiguous HOST int32 copy, which the library validates before any launch. A call is refused
# on types and shapes first, then on `staged_bytes`, then on where the tensors live. The widths are include/cgg_hip.h's.
IMAGE_PREP_TABLE_COLS = CONSTANTS['CGG_IMAGE_PREP_TABLE_COLS']
TRAIN_PREP_IMG_COLS = CONSTANTS['CGG_TRAIN_PREP_IMG_COLS']
TRAIN_PREP_INST_COLS = CONSTANTS['CGG_TRAIN_PREP_INST_COLS']
TRAIN_PREP_PAN_COLS = CONSTANTS['CGG_TRAIN_PREP_PAN_COLS']
TRAIN_PREP_SEG_COLS = CONSTANTS['CGG_TRAIN_PREP_SEG_COLS']
TRAIN_PREP_MAX_SEGMENTS = CONSTANTS['CGG_TRAIN_PREP_MAX_SEGMENTS']
TRAIN_PREP_POLY_INST_COLS = CONSTANTS['CGG_TRAIN_PREP_POLY_INST_COLS']
TRAIN_PREP_POLY_PART_COLS = CONSTANTS['CGG_TRAIN_PREP_POLY_PART_COLS']
TRAIN_PREP_MAX_COORD = CONSTANTS['CGG_IMAGE_PREP_MAX_DIM']      # |coordinate| of a polygon vertex: it bounds the edge walk
POLY_LDS_BITS = CONSTANTS['CGG_POLY_LDS_BITS']                  # a plane of more pixels keeps its toggle plane in the workspace
POLY_SCAN_BITS = CONSTANTS['CGG_POLY_SCAN_BITS']                # pixels of one scan block of the fill kernel


def three_floats(v, name):
    """one number, or three of them (per channel; grayscale sources are out of scope) -> a tuple of 3 floats"""
    vals = tuple(float(x) for x in (v if hasattr(v, '__len__') else [v] * 3))
    if len(vals) != 3:
        raise CggError(f'{name} must be one number or three (got {len(vals)})')
    return vals


def _norm3(me, mean, std, pad_val):
    """the three per-channel float arrays of a prep call"""
    return ((ctypes.c_float * 3)(*three_floats(mean, f'{me}: mean')), (ctypes.c_float * 3)(*three_floats(std, f'{me}: std')),
            (ctypes.c_float * 3)(*three_floats(pad_val, f'{me}: pad_val')))


def _shaped(me, name, t, shape, dtype, like=None):
    """`t` is a tensor of `dtype` and `shape` (None: any extent), on the device of the img tensor `like` where one is given"""
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or \
            any(want is not None and want != got for want, got in zip(shape, t.shape)):
        want = ', '.join('?' if n is None else str(n) for n in shape)
        raise CggError(f'{me}: {name} must be a ({want}{"," if len(shape) == 1 else ""}) {dtype} tensor '
                       f'(got {getattr(t, "dtype", type(t))}, shape {tuple(getattr(t, "shape", ()))})')
    if like is not None and t.device != like.device:
        raise CggError(f'{me}: {name} ({t.device}) and img ({like.device}) live on different devices')


def _host_tables(me, *tables):
    """every (name, tensor, cols) is a contiguous HOST int32 (rows, cols) tensor, and the first, with one row per image, is not
    empty -> the row counts"""
    for name, t, cols in tables:
        _shaped(me, name, t, (None, cols), torch.int32)
        if t.is_cuda or not t.is_contiguous():
            raise CggError(f'{me}: {name} must be a contiguous HOST tensor (the copy of the rows that `staged` carries)')
    if tables[0][1].shape[0] < 1:
        raise CggError(f'{me}: an empty batch')
    return [int(t.shape[0]) for _, t, _ in tables]


def _staged_u8(me, staged, staged_bytes, staged_host=None, with_host=False):
    """`staged` is 1-D uint8 (with_host: and `staged_host` its 1-D uint8 HOST copy) and holds `staged_bytes` -> that byte count
    (all of `staged` by default)"""
    _shaped(me, 'staged', staged, (None,), torch.uint8)
    nbytes = staged.numel() if staged_bytes is None else int(staged_bytes)
    if with_host:
        _shaped(me, 'staged_host', staged_host, (None,), torch.uint8)
        if staged_host.is_cuda:
            raise CggError(f'{me}: staged_host must be a HOST tensor, the copy of the staged bytes')
        if nbytes > staged_host.numel():
            raise CggError(f'{me}: staged_bytes {nbytes} exceeds the {staged_host.numel()} bytes of staged_host')
    if nbytes > staged.numel():
        raise CggError(f'{me}: staged_bytes {nbytes} exceeds the {staged.numel()} bytes of staged')
    return nbytes


def _staged_and_img(me, staged, img, name='img'):
    """device addresses of `staged` and of the image batch, which live on one device"""
    sp, ip = dev_ptr(staged, f'{me}: staged'), dev_ptr(img, f'{me}: {name}')
    if staged.device != img.device:
        raise CggError(f'{me}: staged ({staged.device}) and {name} ({img.device}) live on different devices')
    return sp, ip


def _back_to_back(first, *following):
    """byte offsets of the tables: `first`, then per (offset or None, cols, rows of the table before) the offset given, or by
    default the byte after the table before"""
    offsets = [int(first)]
    for off, cols, rows in following:
        offsets.append(offsets[-1] + 4 * cols * rows if off is None else int(off))
    return offsets


def image_prep_u8(staged, table, out, mean, std, pad_val=0.0, to_rgb=True, pad_before_norm=True, table_offset=0, staged_bytes=None):
    """Resize (8-bit bilinear) + Pad + Normalize(to_rgb) + collate of a whole batch in one launch (`cgg_image_prep_u8`, no
    synchronisation). staged: DEVICE uint8 (n,) -- the raw HWC images back to back and the descriptor table at byte `table_offset`;
    table: HOST int32 (B, IMAGE_PREP_TABLE_COLS) copy of those rows (byte offset, h, w, pitch, new_h, new_w, pad_h, pad_w), read for
    validation during the call; out: DEVICE float32 (B, 3, Hb, Wb) contiguous, every element of which is written. Returns `out`."""
    me = 'image_prep_u8'
    B, = _host_tables(me, ('table', table, IMAGE_PREP_TABLE_COLS))
    _shaped(me, 'out', out, (B, 3, None, None), torch.float32)
    nbytes = _staged_u8(me, staged, staged_bytes)
    sp, op = _staged_and_img(me, staged, out, 'out')
    m, s, p = _norm3(me, mean, std, pad_val)
    Hb, Wb = int(out.shape[2]), int(out.shape[3])
    with _timed(me, bytes=float(nbytes + out.numel() * 4), shape=(B, Hb, Wb)):
        _call('cgg_image_prep_u8', sp, nbytes, int(table_offset), host_ptr(table, 'table', torch.int32), B, m, s, p, int(bool(to_rgb)),
              int(bool(pad_before_norm)), op, Hb, Wb, stream_ptr(out.device))
    return out


def _train_outputs(me, img, B, N, masks, seg, stats):
    """img (B, 3, H, W) f32, masks (N, H, W) u8 (N None: as many as it has), seg (B, 1, H, W) u8 or None, stats (N, 5) i32, all on
    img's device -> N, H, W"""
    _shaped(me, 'img', img, (B, 3, None, None), torch.float32)
    H, W = int(img.shape[2]), int(img.shape[3])
    _shaped(me, 'masks', masks, (N, H, W), torch.uint8, img)
    N = int(masks.shape[0])
    if seg is not None:
        _shaped(me, 'seg', seg, (B, 1, H, W), torch.uint8, img)
    _shaped(me, 'stats', stats, (N, 5), torch.int32, img)
    return N, H, W


def train_prep_u8(staged, img_table, inst_table, img, masks, seg, stats, mean, std, pad_val=0.0, to_rgb=True, crop_size=None, seg_pad=255,
                  img_table_offset=0, inst_table_offset=None, staged_bytes=None):
    """Flip + jittered Resize + RandomCrop + Pad + Normalize(to_rgb) of a whole batch of raw samples -- images, instance bitmaps,
    semantic maps -- in two launches (`cgg_train_prep_u8`, no synchronisation; train_prep.py states the rule). staged: DEVICE uint8
    (n,) -- the two tables at bytes `img_table_offset` / `inst_table_offset` and the planes; img_table (B, TRAIN_PREP_IMG_COLS) /
    inst_table (N, TRAIN_PREP_INST_COLS): HOST int32 copies of those rows, read for validation during the call; img (B, 3, H, W) f32,
    masks (N, H, W) u8, seg (B, 1, H, W) u8 or None, stats (N, 5) i32: DEVICE, contiguous, every element written (the caller clears
    nothing). crop_size (h, w) defaults to the plane. Returns (img, masks, seg, stats)."""
    me = 'train_prep_u8'
    B, N = _host_tables(me, ('img_table', img_table, TRAIN_PREP_IMG_COLS), ('inst_table', inst_table, TRAIN_PREP_INST_COLS))
    N, H, W = _train_outputs(me, img, B, N, masks, seg, stats)
    nbytes = _staged_u8(me, staged, staged_bytes)
    sp, ip = _staged_and_img(me, staged, img)
    mp = dev_ptr(masks, f'{me}: masks') if N else None
    tp = dev_ptr(stats, f'{me}: stats') if N else None
    gp = dev_ptr(seg, f'{me}: seg')
    m, s, p = _norm3(me, mean, std, pad_val)
    ch, cw = (H, W) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    img_off, inst_off = _back_to_back(img_table_offset, (inst_table_offset, TRAIN_PREP_IMG_COLS, B))
    with _timed(me, bytes=float(nbytes + img.numel() * 4 + N * H * W + (B * H * W if seg is not None else 0)), shape=(B, N, H, W)):
        _call('cgg_train_prep_u8', sp, nbytes, img_off, inst_off, host_ptr(img_table, 'img_table', torch.int32),
              host_ptr(inst_table, 'inst_table', torch.int32) if N else None, B, N, m, s, p, int(bool(to_rgb)), int(seg_pad), ch, cw,
              ip, mp, gp, tp, H, W, stream_ptr(img.device))
    return img, masks, seg, stats


def train_prep_panoptic_u8(staged, img_table, pan_table, seg_table, img, masks, seg, stats, mean, std, pad_val=0.0, to_rgb=True,
                           crop_size=None, seg_pad=255, img_table_offset=0, pan_table_offset=None, seg_table_offset=None,
                           staged_bytes=None):
    """`train_prep_u8` for panoptic samples: the thing masks, the semantic plane and the statistics come from ONE gather of the staged
    id map per output pixel (`cgg_train_prep_panoptic_u8`, two launches, no synchronisation; train_prep.py states the rule). staged:
    DEVICE uint8 (n,) -- the three tables at bytes `img_table_offset` / `pan_table_offset` / `seg_table_offset` (by default back to
    back), the images and the id maps; img_table (B, TRAIN_PREP_IMG_COLS) with the thing counts and -1 for the semantic-map offset,
    pan_table (B, TRAIN_PREP_PAN_COLS), seg_table (S, TRAIN_PREP_SEG_COLS) rows sorted by id within an image: HOST int32 copies, read
    for validation during the call; img (B, 3, H, W) f32, masks (N, H, W) u8, seg (B, 1, H, W) u8 or None, stats (N, 5) i32: DEVICE,
    contiguous, every element written (the caller clears nothing). Returns (img, masks, seg, stats)."""
    me = 'train_prep_panoptic_u8'
    B, Bp, S = _host_tables(me, ('img_table', img_table, TRAIN_PREP_IMG_COLS), ('pan_table', pan_table, TRAIN_PREP_PAN_COLS),
                            ('seg_table', seg_table, TRAIN_PREP_SEG_COLS))
    if Bp != B:
        raise CggError(f'{me}: pan_table must have one row per image ({B}), got {Bp}')
    N, H, W = _train_outputs(me, img, B, None, masks, seg, stats)
    nbytes = _staged_u8(me, staged, staged_bytes)
    sp, ip = _staged_and_img(me, staged, img)
    mp = dev_ptr(masks, f'{me}: masks') if N else None
    tp = dev_ptr(stats, f'{me}: stats') if N else None
    gp = dev_ptr(seg, f'{me}: seg')
    m, s, p = _norm3(me, mean, std, pad_val)
    ch, cw = (H, W) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    img_off, pan_off, seg_off = _back_to_back(img_table_offset, (pan_table_offset, TRAIN_PREP_IMG_COLS, B),
                                              (seg_table_offset, TRAIN_PREP_PAN_COLS, B))
    with _timed(me, bytes=float(nbytes + img.numel() * 4 + N * H * W + (B * H * W if seg is not None else 0)), shape=(B, N, H, W)):
        _call('cgg_train_prep_panoptic_u8', sp, nbytes, img_off, pan_off, seg_off, host_ptr(img_table, 'img_table', torch.int32),
              host_ptr(pan_table, 'pan_table', torch.int32), host_ptr(seg_table, 'seg_table', torch.int32) if S else None, B, N, S, m,
              s, p, int(bool(to_rgb)), int(seg_pad), ch, cw, ip, mp, gp, tp, H, W, stream_ptr(img.device))
    return img, masks, seg, stats


def train_prep_polygons_workspace_bytes(img_table, N, force_workspace=False):
    """bytes of workspace `train_prep_polygons_u8` / `polygon_fill_bits` need for these (B, TRAIN_PREP_IMG_COLS) HOST image rows and
    N instances"""
    _shaped('train_prep_polygons_workspace_bytes', 'img_table', img_table, (None, TRAIN_PREP_IMG_COLS), torch.int32)
    return int(_call('cgg_train_prep_polygons_workspace_bytes', host_ptr(img_table, 'img_table', torch.int32), int(img_table.shape[0]),
                     int(N), int(bool(force_workspace)), total=True))


def _poly_call(symbol, sp, nbytes, offsets, img_table, inst_table, part_table, staged_host, B, N, P, *rest):
    """the argument head the two polygon entry points share: staged bytes, the three table offsets and HOST copies, the counts"""
    _call(symbol, sp, nbytes, *offsets, host_ptr(img_table, 'img_table', torch.int32),
          host_ptr(inst_table, 'inst_table', torch.int32) if N else None, host_ptr(part_table, 'part_table', torch.int32) if P else None,
          host_ptr(staged_host, 'staged_host', torch.uint8), B, N, P, *rest)


def polygon_fill_bits(staged, img_table, inst_table, part_table, staged_host, workspace, img_table_offset=0, inst_table_offset=None,
                      part_table_offset=None, staged_bytes=None, force_workspace=False):
    """The polygon fill kernel alone (`cgg_polygon_fill_bits`, one launch, no synchronisation): every instance's parts -> its
    column-major bit plane at source resolution, plane i at word i * plane_words of `workspace` (rule 6 of train_prep.py). Arguments
    as for `train_prep_polygons_u8`; of an image row only h, w, first instance, instances are used. force_workspace (tests): toggle
    planes in the workspace whatever their size. Returns (workspace, plane_words); `polygon_bits_to_mask` unpacks a plane."""
    me = 'polygon_fill_bits'
    B, N, P = _host_tables(me, ('img_table', img_table, TRAIN_PREP_IMG_COLS), ('inst_table', inst_table, TRAIN_PREP_POLY_INST_COLS),
                           ('part_table', part_table, TRAIN_PREP_POLY_PART_COLS))
    _shaped(me, 'workspace', workspace, (None,), torch.int32)
    nbytes = _staged_u8(me, staged, staged_bytes, staged_host, with_host=True)
    if workspace.device != staged.device:
        raise CggError(f'{me}: workspace ({workspace.device}) and staged ({staged.device}) live on different devices')
    offsets = _back_to_back(img_table_offset, (inst_table_offset, TRAIN_PREP_IMG_COLS, B),
                            (part_table_offset, TRAIN_PREP_POLY_INST_COLS, N))
    with _timed(me, bytes=float(nbytes), shape=(B, N, P)):
        _poly_call('cgg_polygon_fill_bits', dev_ptr(staged, f'{me}: staged'), nbytes, offsets, img_table, inst_table, part_table,
                   staged_host, B, N, P, dev_ptr(workspace, f'{me}: workspace'), 4 * workspace.numel(), int(bool(force_workspace)),
                   stream_ptr(staged.device))
    hw = [int(r[1]) * int(r[2]) for r in img_table.tolist() if r[10] > 0]
    return workspace, (max(hw) + 31) // 32 if hw else 0


def polygon_bits_to_mask(workspace, plane_words, i, h, w):
    """plane i of `polygon_fill_bits`' workspace as an (h, w) uint8 tensor on its device (torch ops; test-facing)"""
    words = workspace[i * plane_words:i * plane_words + (h * w + 31) // 32]
    bits = (words.view(-1, 1) >> torch.arange(32, device=workspace.device, dtype=torch.int32)) & 1
    return bits.reshape(-1)[:h * w].to(torch.uint8).view(w, h).t().contiguous()


def train_prep_polygons_u8(staged, img_table, inst_table, part_table, staged_host, img, masks, stats, workspace, mean, std, pad_val=0.0,
                           to_rgb=True, crop_size=None, img_table_offset=0, inst_table_offset=None, part_table_offset=None,
                           staged_bytes=None, force_workspace=False):
    """`train_prep_u8` for instance samples whose masks are COCO polygons, rasterised on the device (`cgg_train_prep_polygons_u8`:
    image kernel, polygon fill kernel, plane kernel over the bit planes; no synchronisation; train_prep.py states the rule, rule 6
    for the raster). staged: DEVICE uint8 (n,) -- the three tables at bytes `img_table_offset` / `inst_table_offset` /
    `part_table_offset` (by default back to back), the images and the float64 coordinates; img_table (B, TRAIN_PREP_IMG_COLS) with -1
    for the semantic-map offset, inst_table (N, TRAIN_PREP_POLY_INST_COLS) = image index, first part, parts, part_table
    (P, TRAIN_PREP_POLY_PART_COLS) = byte offset (a multiple of 8), vertices: HOST int32 copies; staged_host: HOST uint8 copy of the
    staged bytes (the coordinates are validated from it); img (B, 3, H, W) f32, masks (N, H, W) u8, stats (N, 5) i32, workspace 1-D
    int32 of `train_prep_polygons_workspace_bytes` or more: DEVICE, contiguous; the caller clears nothing. Returns (img, masks,
    stats)."""
    me = 'train_prep_polygons_u8'
    B, N, P = _host_tables(me, ('img_table', img_table, TRAIN_PREP_IMG_COLS), ('inst_table', inst_table, TRAIN_PREP_POLY_INST_COLS),
                           ('part_table', part_table, TRAIN_PREP_POLY_PART_COLS))
    N, H, W = _train_outputs(me, img, B, N, masks, None, stats)
    _shaped(me, 'workspace', workspace, (None,), torch.int32, img)
    nbytes = _staged_u8(me, staged, staged_bytes, staged_host, with_host=True)
    sp, ip = _staged_and_img(me, staged, img)
    mp = dev_ptr(masks, f'{me}: masks') if N else None
    tp = dev_ptr(stats, f'{me}: stats') if N else None
    m, s, p = _norm3(me, mean, std, pad_val)
    ch, cw = (H, W) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    offsets = _back_to_back(img_table_offset, (inst_table_offset, TRAIN_PREP_IMG_COLS, B),
                            (part_table_offset, TRAIN_PREP_POLY_INST_COLS, N))
    with _timed(me, bytes=float(nbytes + img.numel() * 4 + N * H * W), shape=(B, N, H, W)):
        _poly_call('cgg_train_prep_polygons_u8', sp, nbytes, offsets, img_table, inst_table, part_table, staged_host, B, N, P, m, s,
                   p, int(bool(to_rgb)), ch, cw, ip, mp, tp, H, W, dev_ptr(workspace, f'{me}: workspace'), 4 * workspace.numel(),
                   int(bool(force_workspace)), stream_ptr(img.device))
    return img, masks, stats


# ------------------------------------------------------------------------------------------------
# caption search: one beam-search step for a whole batch, decided on the device (caption_search.py states the rule)
# ------------------------------------------------------------------------------------------------
BEAM_STEP_MAX_BEAM = CONSTANTS['CGG_BEAM_STEP_MAX_BEAM']
BEAM_STEP_MAX_LEN = CONSTANTS['CGG_BEAM_STEP_MAX_LEN']


class BeamState:
    """The fixed-slot state of a batched caption search (`caption_search.beam_step_host` / `beam_step`): `beam` slots per image,
    rows of `max_len` tokens, zero-initialised except for the one live sequence [BOS] of every image. Lives wherever `device` says
    (the host rule runs on a CPU state; `float_dtype=torch.float64` is its comparison form)."""

    INT_FIELDS = ('seqs', 'nlive', 'fin_seqs', 'fin_len', 'nfin', 'best_idx', 'done', 'ndone')
    FLOAT_FIELDS = ('weights', 'fin_score')
    FIELDS = INT_FIELDS + FLOAT_FIELDS

    def __init__(self, B, beam, max_len, BOS, EOS, device='cpu', float_dtype=torch.float32):
        B, beam, max_len = int(B), int(beam), int(max_len)
        if B < 1 or not 1 <= beam <= BEAM_STEP_MAX_BEAM:
            raise CggError(f'BeamState: B >= 1 and 1 <= beam <= {BEAM_STEP_MAX_BEAM} expected (got {B}, {beam})')
        self.B, self.beam, self.BOS, self.EOS = B, beam, int(BOS), int(EOS)
        # a step at length 2 always runs and may finish a sequence of 3 tokens, whatever max_len says
        self.max_len = max(max_len, 4)
        if self.max_len > BEAM_STEP_MAX_LEN:
            raise CggError(f'BeamState: max_len must be <= {BEAM_STEP_MAX_LEN} (got {max_len})')
        i32 = dict(dtype=torch.int32, device=device)
        f = dict(dtype=float_dtype, device=device)
        self.seqs = torch.zeros((B, beam, self.max_len), **i32)
        self.seqs[:, 0, 0] = self.BOS
        self.weights = torch.zeros((B, beam), **f)
        self.nlive = torch.ones((B,), **i32)
        self.fin_seqs = torch.zeros((B, beam, self.max_len), **i32)
        self.fin_len = torch.zeros((B, beam), **i32)
        self.fin_score = torch.zeros((B, beam), **f)
        self.nfin = torch.zeros((B,), **i32)
        self.best_idx = torch.zeros((B,), **i32)
        self.done = torch.zeros((B,), **i32)
        self.ndone = torch.zeros((1,), **i32)
        # what the next decoder step reads: every slot starts from BOS and continues itself
        self.tokens = torch.full((B * beam,), self.BOS, dtype=torch.int64, device=device)
        self.parents = torch.arange(B * beam, dtype=torch.int64, device=device)
        self.ws = None

    def clone(self, device=None, float_dtype=None):
        """A deep copy, optionally on another device / with the float fields in another dtype."""
        o = object.__new__(BeamState)
        o.B, o.beam, o.BOS, o.EOS, o.max_len, o.ws = self.B, self.beam, self.BOS, self.EOS, self.max_len, None
        for k in self.FIELDS + ('tokens', 'parents'):
            t = getattr(self, k)
            t = t.to(device) if device is not None else t
            if float_dtype is not None and k in self.FLOAT_FIELDS:
                t = t.to(float_dtype)
            setattr(o, k, t.clone())
        return o


def beam_step(logits, state, length, alpha, max_len, first=False, passes=3):
    """One step of the batched caption search on the device (`cgg_beam_step`: two launches, no allocation after the first call on a
    state, no synchronisation). logits (L, B * beam, V) f32 contiguous; `state` a device `BeamState`, updated in place together with
    `state.tokens` / `state.parents`; `length` = the current length of the live sequences. The rule is
    `caption_search.beam_step_host`."""
    if not isinstance(state, BeamState):
        raise CggError(f'beam_step: state must be a BeamState (got {type(state).__name__})')
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise CggError('beam_step: logits must be a (L, B * beam, V) tensor')
    lp = dev_ptr(logits, 'beam_step: logits', torch.float32)
    L, rows, V = (int(v) for v in logits.shape)
    B, beam = state.B, state.beam
    if rows != B * beam:
        raise CggError(f'beam_step: logits has {rows} rows, the state {B} x {beam} slots')
    ptrs = []
    for k in ('seqs', 'weights', 'nlive', 'fin_seqs', 'fin_len', 'fin_score', 'nfin', 'best_idx', 'done', 'ndone', 'tokens', 'parents'):
        t = getattr(state, k)
        want = torch.float32 if k in BeamState.FLOAT_FIELDS else torch.int64 if k in ('tokens', 'parents') else torch.int32
        ptrs.append(dev_ptr(t, f'beam_step: state.{k}', want))
        if t.device != logits.device:
            raise CggError(f'beam_step: state.{k} ({t.device}) and logits ({logits.device}) live on different devices')
    need = int(_lib_().cgg_beam_step_workspace_bytes(B, beam, V))
    if state.ws is None or state.ws.numel() < need or state.ws.device != logits.device:
        state.ws = torch.empty(max(need, 4), dtype=torch.uint8, device=logits.device)
    with _timed('beam_step', bytes=float(logits.numel() * 4), shape=(L, B, beam, V)):
        _call('cgg_beam_step_passes', lp, L, B, beam, V, *ptrs, dev_ptr(state.ws), int(length), float(alpha), state.EOS, int(max_len),
              state.max_len, int(bool(first)), int(passes), stream_ptr(logits.device))
    return state


# ------------------------------------------------------------------------------------------------
# host side of the inference tail: COCO RLE of bit-packed masks (host function of the library, no device work)
# ------------------------------------------------------------------------------------------------
def rle_encode_bitmasks(bits, width, threads=8):
    """bits: HOST uint8 tensor / numpy array (n, H, row_bytes), pixel x in bit (x & 7) of byte (x >> 3) (what
    `instance_masks_picks(bitpack=True)` writes) -> list of n COCO RLE dicts {'size': [H, W], 'counts': bytes}."""
    import numpy as np
    arr = bits.numpy() if torch.is_tensor(bits) else np.asarray(bits)
    if arr.dtype != np.uint8 or arr.ndim != 3 or not arr.flags['C_CONTIGUOUS']:
        raise CggError('rle_encode_bitmasks: (n, H, row_bytes) contiguous uint8 host array expected')
    n, H, rb = arr.shape
    W = int(width)
    if n == 0:
        return []
    # ~2 KB per mask at 1024^2 with this benchmark's noisy masks: a too-small buffer encodes twice
    return _rle_strings('cgg_rle_encode_bitmasks', (ctypes.c_void_p(arr.ctypes.data), n, H, W, H * rb, rb, int(threads)),
                        n, H, W, max(1 << 16, n * 4096))


# ------------------------------------------------------------------------------------------------
# device side of the same encoding: run boundaries on the GPU (csrc/rle_device.hip), strings on the host
# ------------------------------------------------------------------------------------------------
def rle_cols_shape(H, width):
    """(padded columns, block-rows) of one mask's column-major plane in the workspace of `rle_transitions`."""
    return 64 * ((int(width) + 63) // 64), (int(H) + 63) // 64


def rle_transitions(bits, width, capacity=None, positions=None, offsets=None, ws=None):
    """bits: DEVICE uint8 (n, H, row_bytes), rows contiguous (stride(0) may exceed H * row_bytes), pixel x in bit (x & 7) of byte
    (x >> 3) -> (positions uint32 [capacity], offsets int64 [n + 1], ws uint8) on the device, on the current stream:
    the transitions of the column-major bit stream of every mask (`host_results.rle_transitions_host` states the rule).
    offsets is always complete; the positions of mask i are written iff offsets[i + 1] <= capacity. ws begins with the
    column-major planes: ws[:n * Wp * Hb * 8].view(int64).view(n, Wp, Hb) with (Wp, Hb) = rle_cols_shape(H, width).
    positions / offsets / ws may be handed in (reused buffers); no host read, no allocation then."""
    if not torch.is_tensor(bits) or bits.dtype != torch.uint8 or bits.dim() != 3:
        raise CggError('rle_transitions: (n, H, row_bytes) uint8 device tensor expected')
    pbits = dev_ptr(bits, 'rle_transitions: bits', torch.uint8, dense=False)
    n, H, rb = bits.shape
    W = int(width)
    if n > 0 and (bits.stride(2) != 1 or bits.stride(1) != rb or bits.stride(0) < H * rb):
        raise CggError(f'rle_transitions: rows must be contiguous and planes at least H * row_bytes apart (strides {bits.stride()})')
    dev = bits.device
    if positions is None:
        if capacity is None:
            raise CggError('rle_transitions: give `capacity` or a `positions` buffer')
        positions = torch.empty(max(int(capacity), 1), dtype=torch.int32, device=dev)
    cap = positions.numel() if capacity is None else int(capacity)
    if cap > positions.numel():
        raise CggError(f'rle_transitions: capacity {cap} exceeds the positions buffer ({positions.numel()})')
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if offsets.numel() < n + 1:
        raise CggError(f'rle_transitions: offsets has {offsets.numel()} elements, n + 1 = {n + 1} needed')
    need = int(_lib_().cgg_rle_transitions_workspace_bytes(n, H, W))
    if ws is None:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    if ws.numel() < need:
        raise CggError(f'rle_transitions: workspace of {ws.numel()} bytes, {need} needed')
    for t, name in ((positions, 'positions'), (offsets, 'offsets'), (ws, 'ws')):
        if t.device != dev:
            raise CggError(f'rle_transitions: {name} ({t.device}) and bits ({dev}) live on different devices')
    stride = bits.stride(0) if n > 0 else H * rb
    with _timed('rle_transitions', bytes=float(n * H * rb), shape=(n, H, W)):
        _call('cgg_rle_transitions', pbits, n, H, W, int(stride), rb, dev_ptr(ws, 'ws', torch.uint8),
              dev_ptr(positions, 'positions', torch.int32), cap, dev_ptr(offsets, 'offsets', torch.int64), stream_ptr(dev))
    return positions, offsets, ws


def _rle_strings(symbol, head, n, H, W, cap):
    """the n COCO RLE dicts of a host RLE entry point `symbol(*head, out, out_cap, out_offsets)`, called again with a buffer of the
    size it asked for when the first was too small"""
    import numpy as np
    offs = np.empty(n + 1, dtype=np.int64)
    while True:
        out = np.empty(cap, dtype=np.uint8)
        total = _call(symbol, *head, ctypes.c_void_p(out.ctypes.data), cap, ctypes.c_void_p(offs.ctypes.data), total=True)
        if total <= cap:
            break
        cap = int(total)
    raw = out[:total].tobytes()
    o = offs.tolist()
    return [dict(size=[H, W], counts=raw[o[i]:o[i + 1]]) for i in range(n)]


def rle_strings_from_transitions(positions, offsets, H, width):
    """HOST: positions (uint32 / int32 array, as `rle_transitions` wrote them) + offsets (int64 [n + 1]) -> list of n COCO RLE
    dicts, byte-identical to `rle_encode_bitmasks` on the same masks."""
    import numpy as np
    pos = positions.numpy() if torch.is_tensor(positions) else np.asarray(positions)
    off = offsets.numpy() if torch.is_tensor(offsets) else np.asarray(offsets)
    if pos.dtype not in (np.uint32, np.int32) or pos.ndim != 1 or not pos.flags['C_CONTIGUOUS']:
        raise CggError('rle_strings_from_transitions: contiguous 1-d uint32 host array of positions expected')
    if off.dtype != np.int64 or off.ndim != 1 or off.size < 1 or not off.flags['C_CONTIGUOUS']:
        raise CggError('rle_strings_from_transitions: contiguous int64 host array of n + 1 offsets expected')
    n = off.size - 1
    if n == 0:
        return []
    if int(off.max()) > pos.size:
        raise CggError(f'rle_strings_from_transitions: offsets reach {int(off.max())}, {pos.size} positions given')
    H, W = int(H), int(width)
    return _rle_strings('cgg_rle_strings_from_transitions', (ctypes.c_void_p(pos.ctypes.data), ctypes.c_void_p(off.ctypes.data), n, H, W),
                        n, H, W, max(1 << 12, 2 * int(off[-1] - off[0]) + 8 * n))


def rle_encode_colmajor(cols, H, width, threads=8):
    """HOST: cols (n, Wp, Hb) 64-bit words, the column-major planes at the head of `rle_transitions`' workspace ((Wp, Hb) =
    rle_cols_shape(H, width); bit r of cols[i, x, by] = pixel (by * 64 + r, x), bits beyond H or width zero) -> list of n COCO
    RLE dicts, byte-identical to `rle_encode_bitmasks` on the same masks."""
    import numpy as np
    arr = cols.numpy() if torch.is_tensor(cols) else np.asarray(cols)
    H, W = int(H), int(width)
    if arr.dtype not in (np.uint64, np.int64) or arr.ndim != 3 or not arr.flags['C_CONTIGUOUS'] or \
            tuple(arr.shape[1:]) != rle_cols_shape(H, W):
        raise CggError(f'rle_encode_colmajor: contiguous (n, {rle_cols_shape(H, W)[0]}, {rle_cols_shape(H, W)[1]}) 64-bit host '
                       'array expected')
    n = arr.shape[0]
    if n == 0:
        return []
    return _rle_strings('cgg_rle_encode_colmajor', (ctypes.c_void_p(arr.ctypes.data), n, H, W, int(threads)),
                        n, H, W, max(1 << 16, n * 4096))


# ------------------------------------------------------------------------------------------------
# drawing a result over its image on the device (csrc/paint.hip; paint.py states the rules in numpy)
# ------------------------------------------------------------------------------------------------
PAINT_MAX_MASKS = CONSTANTS['CGG_PAINT_MAX_MASKS']
PAINT_MAX_IDS = CONSTANTS['CGG_PAINT_MAX_IDS']
PAINT_MAX_IMAGE_BYTES = 1 << 31


def _u8_image_ok(img):
    return (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
            and img.is_contiguous() and 0 < img.numel() <= PAINT_MAX_IMAGE_BYTES)


def pack_bool_masks(masks):
    """DEVICE bool (n, H, W) -> bit-packed uint8 (n, H, ceil(W / 8)): pixel x in bit (x & 7) of byte (x >> 3), pad bits zero."""
    if not torch.is_tensor(masks) or masks.dtype != torch.bool or masks.dim() != 3:
        raise CggError('pack_bool_masks: (n, H, W) bool device tensor expected')
    n, H, W = masks.shape
    masks = masks.contiguous()
    rb = (W + 7) // 8
    bits = torch.empty((n, H, rb), dtype=torch.uint8, device=masks.device)
    if n * H > 0:
        _call('cgg_pack_bool_rows_u8', dev_ptr(masks.view(torch.uint8), 'masks', torch.uint8), n * H, W, rb, dev_ptr(bits),
              stream_ptr(masks.device))
    return bits


def paint_instances_ok(img, bits):
    """The gate of `paint_instances`: a contiguous (H, W, 3) uint8 device image of at most 2^31 bytes, and bit-packed masks
    (n <= PAINT_MAX_MASKS, H, row_bytes) on the same device with contiguous rows -- the layout `rle_transitions` reads."""
    if not _u8_image_ok(img) or not torch.is_tensor(bits) or bits.dtype != torch.uint8 or bits.dim() != 3:
        return False
    n, H, rb = bits.shape
    if bits.device != img.device or H != img.shape[0] or rb * 8 < img.shape[1] or n > PAINT_MAX_MASKS:
        return False
    return n == 0 or (bits.stride(2) == 1 and bits.stride(1) == rb and bits.stride(0) >= H * rb)


def paint_instances(img, bits, keep, colors, boxes=None, box_colors=None, alpha=0.8, thickness=2, edges=True, out=None):
    """img (H, W, 3) uint8, bits (n, H, row_bytes) uint8 bit-packed masks, keep (n) uint8, colors (n, 3) uint8, boxes (n, 4) int32
    with box_colors (n, 3) uint8 or None -- all on one device -> the painted image (a new tensor, or `out`, which may be `img`),
    equal to `paint.paint_instances_host` bit for bit. One launch on the current stream, no host read."""
    if not paint_instances_ok(img, bits):
        raise CggError('paint_instances: outside the kernel gate (contiguous (H, W, 3) uint8 device image of at most 2^31 bytes; '
                       f'(n <= {PAINT_MAX_MASKS}, H, row_bytes) uint8 masks with contiguous rows on the same device)')
    H, W, _ = img.shape
    n, _, rb = bits.shape
    dev = img.device
    if out is None:
        out = torch.empty_like(img)
    elif out.shape != img.shape or out.device != dev:
        raise CggError('paint_instances: out must have the image\'s shape and device')
    if (boxes is None) != (box_colors is None):
        raise CggError('paint_instances: boxes and box_colors go together')
    for t, name, shape in ((keep, 'keep', (n,)), (colors, 'colors', (n, 3)), (boxes, 'boxes', (n, 4)), (box_colors, 'box_colors', (n, 3))):
        if t is not None and (tuple(t.shape) != shape or t.device != dev):
            raise CggError(f'paint_instances: {name} must be {shape} on {dev} (got {tuple(t.shape)} on {t.device})')
    alpha = float(alpha)
    stride = bits.stride(0) if n > 0 else H * rb
    with _timed('paint_instances', bytes=float(n * H * rb + 2 * img.numel()), shape=(n, H, W)):
        _call('cgg_paint_instances_u8', dev_ptr(img, 'img', torch.uint8), dev_ptr(out, 'out', torch.uint8), H, W,
              dev_ptr(bits, 'bits', torch.uint8, dense=False) if n > 0 else None, n, int(stride), rb,
              dev_ptr(keep, 'keep', torch.uint8), dev_ptr(colors, 'colors', torch.uint8), dev_ptr(boxes, 'boxes', torch.int32),
              dev_ptr(box_colors, 'box_colors', torch.uint8), alpha, 1 - alpha, int(thickness), int(bool(edges)), stream_ptr(dev))
    return out


def label_components_ok(pan):
    """The gate of `label_components`: a contiguous (H, W) int32 device map with H * W < 2^31 (ids >= 0: the kernel reports a
    negative id in its status word, it cannot be seen here without a host read)."""
    return (torch.is_tensor(pan) and pan.is_cuda and pan.dtype == torch.int32 and pan.dim() == 2 and pan.is_contiguous()
            and 0 < pan.numel() < (1 << 31))


def label_components(pan, void, capacity=4096):
    """pan (H, W) int32 on the device -> (records int64 (capacity, 5), status int32 (2)) on the device, on the current stream, no host
    read: the 8-connected components of equal non-void id as `paint.components_host` lists them, [root, id, area, sum_x, sum_y],
    in no particular order. status[0] = number of components (records[:min(status[0], capacity)] are valid; more than `capacity`:
    overflow, the caller falls back to `components_host`), status[1] != 0: the records are not to be used (see cgg_hip.h)."""
    if not label_components_ok(pan):
        raise CggError('label_components: contiguous (H, W) int32 device tensor with H * W < 2^31 expected')
    H, W = pan.shape
    dev = pan.device
    cap = int(capacity)
    ws = torch.empty(max(int(_lib_().cgg_label_components_workspace_bytes(H, W)), 8), dtype=torch.uint8, device=dev)
    records = torch.empty((max(cap, 1), 5), dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    with _timed('label_components', bytes=float(pan.numel() * 4), shape=(H, W)):
        _call('cgg_label_components_i32', dev_ptr(pan, 'pan', torch.int32), H, W, int(void), dev_ptr(ws), dev_ptr(records), cap,
              dev_ptr(status), stream_ptr(dev))
    return records[:cap], status


def paint_panoptic_ok(img, pan, nids):
    return (_u8_image_ok(img) and torch.is_tensor(pan) and pan.dtype == torch.int32 and pan.device == img.device
            and tuple(pan.shape) == tuple(img.shape[:2]) and pan.is_contiguous() and 0 <= int(nids) <= PAINT_MAX_IDS)


def paint_panoptic(img, pan, ids, colors, alpha=0.8, edges=True, out=None):
    """img (H, W, 3) uint8, pan (H, W) int32, ids (k <= PAINT_MAX_IDS) int32 strictly ascending, colors (k, 3) uint8, all on one device -> the
    painted image, equal to `paint.paint_panoptic_host` bit for bit. One launch on the current stream, no host read."""
    k = int(ids.numel()) if torch.is_tensor(ids) else -1
    if k < 0 or not paint_panoptic_ok(img, pan, k):
        raise CggError('paint_panoptic: outside the kernel gate (contiguous (H, W, 3) uint8 device image of at most 2^31 bytes, (H, W) '
                       f'int32 map on the same device, at most {PAINT_MAX_IDS} ids)')
    dev = img.device
    if tuple(colors.shape) != (k, 3) or colors.device != dev or ids.device != dev:
        raise CggError(f'paint_panoptic: ids ({k}) and colors ({k}, 3) must live on {dev}')
    if out is None:
        out = torch.empty_like(img)
    elif out.shape != img.shape or out.device != dev:
        raise CggError('paint_panoptic: out must have the image\'s shape and device')
    H, W, _ = img.shape
    alpha = float(alpha)
    with _timed('paint_panoptic', bytes=float(pan.numel() * 4 + 2 * img.numel()), shape=(H, W, k)):
        _call('cgg_paint_panoptic_u8', dev_ptr(img, 'img', torch.uint8), dev_ptr(out, 'out', torch.uint8),
              dev_ptr(pan, 'pan', torch.int32), H, W, dev_ptr(ids, 'ids', torch.int32), dev_ptr(colors, 'colors', torch.uint8), k,
              alpha, 1 - alpha, int(bool(edges)), stream_ptr(dev))
    return out


# ------------------------------------------------------------------------------------------------
# COCO mask evaluation on the device (csrc/mask_eval.hip; mask_eval.py states the rules in numpy)
# ------------------------------------------------------------------------------------------------
MASK_EVAL_MAX_MASKS = CONSTANTS['CGG_MASK_EVAL_MAX_MASKS']
MASK_EVAL_MAX_THRS = CONSTANTS['CGG_MASK_EVAL_MAX_THRS']
MASK_EVAL_MAX_AREAS = CONSTANTS['CGG_MASK_EVAL_MAX_AREAS']
MASK_EVAL_MAX_CATS = CONSTANTS['CGG_MASK_EVAL_MAX_CATS']


def mask_eval_ok(D, G, H, W):
    """The gate of `mask_intersections` / `coco_match`: at most MASK_EVAL_MAX_MASKS masks on each side and H * W < 2^31 (the sums are int32).
    Shapes outside it take the host rule (`mask_eval.mask_intersections_host`, `mask_eval.evaluate_img_host`)."""
    return 0 <= int(D) <= MASK_EVAL_MAX_MASKS and 0 <= int(G) <= MASK_EVAL_MAX_MASKS and int(H) > 0 and int(W) > 0 \
        and int(H) * int(W) < (1 << 31)


def _bit_planes(bits, name):
    """(n, H, row_bytes, plane stride) of bit-packed device masks with contiguous rows"""
    if not torch.is_tensor(bits) or bits.dtype != torch.uint8 or bits.dim() != 3:
        raise CggError(f'{name}: (n, H, row_bytes) uint8 device tensor expected')
    n, H, rb = bits.shape
    if n > 0 and (bits.stride(2) != 1 or bits.stride(1) != rb or bits.stride(0) < H * rb):
        raise CggError(f'{name}: rows must be contiguous and planes at least H * row_bytes apart (strides {bits.stride()})')
    return n, H, rb, int(bits.stride(0)) if n > 0 else H * rb


def mask_intersections(det_bits, gt_bits, width, ws=None):
    """det_bits (D, H, row_bytes), gt_bits (G, H, row_bytes) DEVICE uint8 bit planes (rows contiguous, stride(0) may exceed
    H * row_bytes; pixel x in bit (x & 7) of byte (x >> 3), pad bits may hold anything) -> (inter int32 (D, G), area_d int32 (D,),
    area_g int32 (G,)) on the device, equal to `mask_eval.mask_intersections_host`. Two launches on the current stream, no host
    read; `ws` (uint8, cgg_mask_intersections_workspace_bytes) may be handed in."""
    D, H, rb, dstride = _bit_planes(det_bits, 'mask_intersections: det_bits')
    G, Hg, rbg, gstride = _bit_planes(gt_bits, 'mask_intersections: gt_bits')
    W = int(width)
    if Hg != H or rbg != rb or gt_bits.device != det_bits.device:
        raise CggError(f'mask_intersections: det_bits {tuple(det_bits.shape)} on {det_bits.device} and gt_bits {tuple(gt_bits.shape)} '
                       f'on {gt_bits.device} must share H, row_bytes and the device')
    if not mask_eval_ok(D, G, H, W):
        raise CggError(f'mask_intersections: outside the kernel gate (D={D}, G={G} <= {MASK_EVAL_MAX_MASKS}, H * W < 2^31)')
    dev = det_bits.device
    pd = dev_ptr(det_bits, 'mask_intersections: det_bits', torch.uint8, dense=False)
    pg = dev_ptr(gt_bits, 'mask_intersections: gt_bits', torch.uint8, dense=False)
    inter = torch.empty((D, G), dtype=torch.int32, device=dev)
    area_d = torch.empty(D, dtype=torch.int32, device=dev)
    area_g = torch.empty(G, dtype=torch.int32, device=dev)
    need = int(_lib_().cgg_mask_intersections_workspace_bytes(D, G, H, W))
    if ws is None:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    if ws.numel() < need or ws.device != dev:
        raise CggError(f'mask_intersections: workspace of {ws.numel()} bytes on {ws.device}, {need} on {dev} needed')
    with _timed('mask_intersections', bytes=float((D + G) * H * rb), shape=(D, G, H, W)):
        _call('cgg_mask_intersections_bits', pd if D else None, D, dstride, pg if G else None, G, gstride, H, W, rb,
              dev_ptr(ws, 'ws', torch.uint8), dev_ptr(inter, 'inter') if D * G else None, dev_ptr(area_d, 'area_d') if D else None,
              dev_ptr(area_g, 'area_g') if G else None, stream_ptr(dev))
    return inter, area_d, area_g


def _match_args(who, dev, D, G, cat_ids, area_rngs, iou_thrs, per_box, out):
    """What `coco_match` and `coco_match_boxes` check alike: the caps, the (D,) / (G,) operands `per_box` = ((tensor, name, n), ...)
    and the four outputs (allocated when `out` is None) -> (K, A, T, out)"""
    K, A, T = int(cat_ids.numel()), int(area_rngs.shape[0]), int(iou_thrs.numel())
    if tuple(area_rngs.shape) != (A, 2):
        raise CggError(f'{who}: area_rngs {tuple(area_rngs.shape)} must be (A, 2)')
    if D > MASK_EVAL_MAX_MASKS or G > MASK_EVAL_MAX_MASKS or T > MASK_EVAL_MAX_THRS or A > MASK_EVAL_MAX_AREAS or K > MASK_EVAL_MAX_CATS \
            or min(K, A, T) < 1:
        raise CggError(f'{who}: outside the kernel gate (D={D}, G={G} <= {MASK_EVAL_MAX_MASKS}, 1 <= T={T} <= {MASK_EVAL_MAX_THRS}, '
                       f'1 <= A={A} <= {MASK_EVAL_MAX_AREAS}, 1 <= K={K} <= {MASK_EVAL_MAX_CATS})')
    for t, name, n in per_box:
        if t.numel() != n or t.device != dev:
            raise CggError(f'{who}: {name} must have {n} elements on {dev} (got {t.numel()} on {t.device})')
    if out is None:
        out = (torch.empty((K, A, T, D), dtype=torch.int32, device=dev), torch.empty((K, A, T, D), dtype=torch.uint8, device=dev),
               torch.empty((K, A, G), dtype=torch.uint8, device=dev), torch.empty((K, 2), dtype=torch.int32, device=dev))
    for t, name, shape in zip(out, ('dt_match', 'dt_ignore', 'gt_ignore', 'counts'), ((K, A, T, D), (K, A, T, D), (K, A, G), (K, 2))):
        if tuple(t.shape) != shape or t.device != dev:
            raise CggError(f'{who}: {name} must be {shape} on {dev} (got {tuple(t.shape)} on {t.device})')
    return K, A, T, out


def coco_match(inter, area_d, area_g, det_order, det_cats, gt_cats, gt_crowd, gt_area, cat_ids, area_rngs, iou_thrs, max_det,
               class_agnostic, out=None):
    """The matching of `mask_eval.evaluate_img_host` for one image on the device, from the outputs of `mask_intersections`:
    det_order int32 (D,) (stable descending score order: `torch.sort(scores, descending=True, stable=True).indices`), det_cats
    int32 (D,), gt_cats int32 (G,), gt_crowd uint8 (G,), gt_area float64 (G,), cat_ids int32 (K,), area_rngs float64 (A, 2),
    iou_thrs float64 (T,) -> (dt_match int32 (K, A, T, D), dt_ignore uint8 (K, A, T, D), gt_ignore uint8 (K, A, G), counts int32
    (K, 2) = (D_k, G_k)); row (k, a, t) holds the category's D_k detections in score order, 0 past them. One launch on the current
    stream, no host read. `out`: the four tensors, preallocated."""
    D, G = int(area_d.numel()), int(area_g.numel())
    dev = area_d.device
    if tuple(inter.shape) != (D, G):
        raise CggError(f'coco_match: inter {tuple(inter.shape)} does not match D={D}, G={G}')
    K, A, T, out = _match_args('coco_match', dev, D, G, cat_ids, area_rngs, iou_thrs,
                               ((det_order, 'det_order', D), (det_cats, 'det_cats', D), (gt_cats, 'gt_cats', G),
                                (gt_crowd, 'gt_crowd', G), (gt_area, 'gt_area', G)), out)
    dt_match, dt_ignore, gt_ignore, counts = out

    def opt(t, name, dtype, n):
        return dev_ptr(t, f'coco_match: {name}', dtype) if n else None

    with _timed('coco_match', shape=(D, G, K, A, T)):
        _call('cgg_coco_match', opt(inter, 'inter', torch.int32, D * G), opt(area_d, 'area_d', torch.int32, D),
              opt(area_g, 'area_g', torch.int32, G), opt(det_order, 'det_order', torch.int32, D),
              opt(det_cats, 'det_cats', torch.int32, D), opt(gt_cats, 'gt_cats', torch.int32, G),
              opt(gt_crowd, 'gt_crowd', torch.uint8, G), opt(gt_area, 'gt_area', torch.float64, G),
              dev_ptr(cat_ids, 'coco_match: cat_ids', torch.int32), K, dev_ptr(area_rngs, 'coco_match: area_rngs', torch.float64), A,
              dev_ptr(iou_thrs, 'coco_match: iou_thrs', torch.float64), T, D, G, int(max_det), int(bool(class_agnostic)),
              opt(dt_match, 'dt_match', torch.int32, D), opt(dt_ignore, 'dt_ignore', torch.uint8, D),
              opt(gt_ignore, 'gt_ignore', torch.uint8, G), dev_ptr(counts, 'coco_match: counts', torch.int32), stream_ptr(dev))
    return dt_match, dt_ignore, gt_ignore, counts


def box_eval_ok(D, G):
    """The gate of `box_iou` / `coco_match_boxes`: at most MASK_EVAL_MAX_MASKS boxes on each side, the matcher's caps. Shapes outside it take the
    host rule (`mask_eval.box_iou_host`, `mask_eval.evaluate_img_host`)."""
    return 0 <= int(D) <= MASK_EVAL_MAX_MASKS and 0 <= int(G) <= MASK_EVAL_MAX_MASKS


def _boxes(det_boxes5, gt_xywh, gt_crowd, who):
    """(D, G, device) of det_boxes5 (D, 5) float32, gt_xywh (G, 4) float64 and gt_crowd (G,) uint8 on one device"""
    if not torch.is_tensor(det_boxes5) or det_boxes5.dim() != 2 or det_boxes5.shape[1] != 5:
        raise CggError(f'{who}: det_boxes5 must be a (D, 5) float32 device tensor (x0, y0, x1, y1, score)')
    if not torch.is_tensor(gt_xywh) or gt_xywh.dim() != 2 or gt_xywh.shape[1] != 4:
        raise CggError(f'{who}: gt_xywh must be a (G, 4) float64 device tensor (x, y, w, h)')
    D, G, dev = int(det_boxes5.shape[0]), int(gt_xywh.shape[0]), det_boxes5.device
    if gt_xywh.device != dev or not torch.is_tensor(gt_crowd) or gt_crowd.numel() != G or gt_crowd.device != dev:
        raise CggError(f'{who}: gt_xywh ({G}, 4) and gt_crowd ({G},) must live on {dev}')
    if not box_eval_ok(D, G):
        raise CggError(f'{who}: outside the kernel gate (D={D}, G={G} <= {MASK_EVAL_MAX_MASKS})')
    return D, G, dev


def box_iou(det_boxes5, gt_xywh, gt_crowd):
    """det_boxes5 (D, 5) float32 (x0, y0, x1, y1, score) as the results hold them, gt_xywh (G, 4) float64, gt_crowd (G,) uint8, all
    on one device -> (iou float64 (D, G), area_d float64 (D,)), equal to `mask_eval.box_iou_host` on
    `mask_eval.det_boxes_xywh_host(det_boxes5)` bit for bit, and that box's w * h. One launch on the current stream, no host read."""
    D, G, dev = _boxes(det_boxes5, gt_xywh, gt_crowd, 'box_iou')
    iou = torch.empty((D, G), dtype=torch.float64, device=dev)
    area_d = torch.empty(D, dtype=torch.float64, device=dev)
    with _timed('box_iou', bytes=float(20 * D + 33 * G + 8 * D * G + 8 * D), shape=(D, G)):
        _call('cgg_box_iou_f64', dev_ptr(det_boxes5, 'box_iou: det_boxes5', torch.float32) if D else None, D,
              dev_ptr(gt_xywh, 'box_iou: gt_xywh', torch.float64) if G else None,
              dev_ptr(gt_crowd, 'box_iou: gt_crowd', torch.uint8) if G else None, G, dev_ptr(iou, 'iou') if D * G else None,
              dev_ptr(area_d, 'area_d') if D else None, stream_ptr(dev))
    return iou, area_d


def coco_match_boxes(det_boxes5, gt_xywh, det_order, det_cats, gt_cats, gt_crowd, gt_area, cat_ids, area_rngs, iou_thrs, max_det,
                     class_agnostic, out=None):
    """`coco_match` on the box IoUs of `box_iou`, formed inside the matcher: det_boxes5 (D, 5) float32, gt_xywh (G, 4) float64 in
    place of inter / area_d / area_g (the detection's own area is its box's w * h); every other argument, the four outputs and
    `out=` as there. Equal to `mask_eval.evaluate_img_host` on `mask_eval.box_iou_host`. One launch on the current stream, no host
    read, no workspace."""
    D, G, dev = _boxes(det_boxes5, gt_xywh, gt_crowd, 'coco_match_boxes')
    K, A, T, out = _match_args('coco_match_boxes', dev, D, G, cat_ids, area_rngs, iou_thrs,
                               ((det_order, 'det_order', D), (det_cats, 'det_cats', D), (gt_cats, 'gt_cats', G),
                                (gt_area, 'gt_area', G)), out)
    dt_match, dt_ignore, gt_ignore, counts = out

    def opt(t, name, dtype, n):
        return dev_ptr(t, f'coco_match_boxes: {name}', dtype) if n else None

    with _timed('coco_match_boxes', shape=(D, G, K, A, T)):
        _call('cgg_coco_match_boxes', opt(det_boxes5, 'det_boxes5', torch.float32, D), opt(gt_xywh, 'gt_xywh', torch.float64, G),
              opt(det_order, 'det_order', torch.int32, D), opt(det_cats, 'det_cats', torch.int32, D),
              opt(gt_cats, 'gt_cats', torch.int32, G), opt(gt_crowd, 'gt_crowd', torch.uint8, G),
              opt(gt_area, 'gt_area', torch.float64, G), dev_ptr(cat_ids, 'coco_match_boxes: cat_ids', torch.int32), K,
              dev_ptr(area_rngs, 'coco_match_boxes: area_rngs', torch.float64), A,
              dev_ptr(iou_thrs, 'coco_match_boxes: iou_thrs', torch.float64), T, D, G, int(max_det), int(bool(class_agnostic)),
              opt(dt_match, 'dt_match', torch.int32, D), opt(dt_ignore, 'dt_ignore', torch.uint8, D),
              opt(gt_ignore, 'gt_ignore', torch.uint8, G), dev_ptr(counts, 'coco_match_boxes: counts', torch.int32), stream_ptr(dev))
    return dt_match, dt_ignore, gt_ignore, counts


# ------------------------------------------------------------------------------------------------
# Panoptic-quality evaluation on the device (csrc/pq_eval.hip; pq_eval.py states the rules in numpy)
# ------------------------------------------------------------------------------------------------
PQ_EVAL_MAX_SEGMENTS = CONSTANTS['CGG_PQ_EVAL_MAX_SEGMENTS']


def pq_hash_size(n):
    """entries of the kernel's id -> slot table for n ids: the power of two >= max(16, 2 n); an id starts probing at id % size"""
    s = 16
    while s < 2 * int(n):
        s *= 2
    return s


def pq_eval_lds_bytes(G, P):
    """LDS a workgroup of `pq_confusion` holds: the (G + 2) x (P + 1) int32 table and both id -> slot tables (-1 outside 0 .. 4096)"""
    return int(_lib_().cgg_pq_eval_lds_bytes(int(G), int(P)))


def pq_eval_ok(G, P, H, W, class0_is_thing=True):
    """The gate of `pq_confusion` / `pq_match`, host arithmetic only: the confusion table plus both id tables fit the dynamic-LDS
    limit, H * W < 2^31 (the counts are int32), and class 0 is a thing: were it stuff, its value 0 would collide with VOID after the
    relabelling of `pan_result_segments_host`, which the host rule follows literally and the device route does not try.
    Images outside it take the host rule (`pq_eval.pq_image_host`)."""
    G, P, H, W = int(G), int(P), int(H), int(W)
    if not (0 <= G <= PQ_EVAL_MAX_SEGMENTS and 0 <= P <= PQ_EVAL_MAX_SEGMENTS and H > 0 and W > 0 and H * W < (1 << 31)):
        return False
    return bool(class0_is_thing) and pq_eval_lds_bytes(G, P) <= int(_lib_().cgg_dynamic_lds_limit())


def _pq_table(table, n_kept, who):
    if table.dim() != 2 or table.shape[1] != 4 or n_kept.numel() != 1 or n_kept.device != table.device:
        raise CggError(f'{who}: table must be (P, 4) int32 and n_kept one int32 on its device (got {tuple(table.shape)}, {n_kept.numel()} '
                       f'on {n_kept.device})')
    P = int(table.shape[0])
    return P, (dev_ptr(table, f'{who}: table', torch.int32) if P else None), dev_ptr(n_kept, f'{who}: n_kept', torch.int32)


def pq_confusion(pan_pred, table, n_kept, pan_gt, gt_ids, num_classes, ws=None):
    """Confusion counts of one image on the device: pan_pred (H, W) int32; table (P, 4) int32 segment rows [value, category, area,
    query] with the device int32 n_kept of them valid (as `panoptic_fuse_batched` leaves them: n_kept is read on the device); pan_gt
    (H, W) int32 ids or (H, W, 3) uint8 RGB; gt_ids (G,) int32 -> int32 workspace whose first (G + 2) x (P + 1) cells are the table
    (row 0 VOID, rows 1 .. G the listed ids, row G + 1 any other id; column 0 void, column 1 + k table row k) followed by two status
    words. Two launches on the current stream, no host read. `pq_match` reads the workspace."""
    who = 'pq_confusion'
    dev = pan_pred.device
    if pan_pred.dim() != 2 or tuple(pan_gt.shape[:2]) != tuple(pan_pred.shape) or pan_gt.device != dev:
        raise CggError(f'{who}: pan_pred {tuple(pan_pred.shape)} on {dev} and pan_gt {tuple(pan_gt.shape)} on {pan_gt.device} must share '
                       'H, W and the device')
    H, W = int(pan_pred.shape[0]), int(pan_pred.shape[1])
    rgb = pan_gt.dim() == 3
    if (rgb and (pan_gt.shape[2] != 3 or pan_gt.dtype != torch.uint8)) or (not rgb and pan_gt.dtype != torch.int32):
        raise CggError(f'{who}: pan_gt must be (H, W) int32 or (H, W, 3) uint8 (got {pan_gt.dtype}, shape {tuple(pan_gt.shape)})')
    G = int(gt_ids.numel())
    P, ptable, pkept = _pq_table(table, n_kept, who)
    if not pq_eval_ok(G, P, H, W):
        raise CggError(f'{who}: outside the kernel gate (G={G}, P={P}: {pq_eval_lds_bytes(G, P)} bytes of LDS, H * W = {H * W})')
    need = int(_lib_().cgg_pq_confusion_workspace_bytes(G, P))
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
    if ws.numel() * 4 < need or ws.device != dev:
        raise CggError(f'{who}: workspace of {ws.numel() * 4} bytes on {ws.device}, {need} on {dev} needed')
    with _timed('pq_confusion', bytes=float(H * W * (4 + (3 if rgb else 4))), shape=(G, P, H, W)):
        _call('cgg_pq_confusion_i32', dev_ptr(pan_pred, f'{who}: pan_pred', torch.int32), dev_ptr(pan_gt, f'{who}: pan_gt'), int(rgb), H, W,
              dev_ptr(gt_ids, f'{who}: gt_ids', torch.int32) if G else None, G, ptable, pkept, P, int(num_classes),
              dev_ptr(ws, f'{who}: ws', torch.int32), stream_ptr(dev))
    return ws


def pq_match(ws, gt_cats, gt_crowd, gt_area, table, n_kept):
    """The matching of `pq_eval.pq_image_host` for one image on the device, from the workspace of `pq_confusion`: gt_cats int32 (G,)
    (category codes, compared with the table's category column as opaque integers), gt_crowd uint8 (G,), gt_area int32 (G,) ->
    (record, offs): ONE uint8 device buffer, so that one copy carries it, and name -> (byte offset, bytes) of status int32 (2,),
    gt_iou float64 (G,), gt_match int32 (G,), pred_area, pred_value, pred_cat int32 (P,), pred_flags uint8 (P,) (1 segment, 2 matched,
    4 ignored). One launch on the current stream, no host read."""
    who = 'pq_match'
    dev = ws.device
    G = int(gt_cats.numel())
    P, ptable, pkept = _pq_table(table, n_kept, who)
    if gt_crowd.numel() != G or gt_area.numel() != G or table.device != dev or gt_cats.device != dev:
        raise CggError(f'{who}: gt_cats, gt_crowd, gt_area must have {G} elements each, everything on {dev}')
    if pq_eval_lds_bytes(G, P) < 0 or ws.numel() * 4 < int(_lib_().cgg_pq_confusion_workspace_bytes(G, P)):
        raise CggError(f'{who}: workspace of {ws.numel() * 4} bytes does not hold the table of G={G}, P={P}')
    offs, total = {}, 0
    for name, nbytes in (('status', 8), ('gt_iou', 8 * G), ('gt_match', 4 * G), ('pred_area', 4 * P), ('pred_value', 4 * P),
                         ('pred_cat', 4 * P), ('pred_flags', P)):
        offs[name] = (total, nbytes)
        total += (nbytes + 7) & ~7
    rec = torch.empty(total, dtype=torch.uint8, device=dev)

    def part(name, dtype, n):
        o, nb = offs[name]
        return dev_ptr(rec[o:o + nb].view(dtype), f'{who}: {name}') if n else None

    with _timed('pq_match', shape=(G, P)):
        _call('cgg_pq_match', dev_ptr(ws, f'{who}: ws', torch.int32), dev_ptr(gt_cats, f'{who}: gt_cats', torch.int32) if G else None,
              dev_ptr(gt_crowd, f'{who}: gt_crowd', torch.uint8) if G else None,
              dev_ptr(gt_area, f'{who}: gt_area', torch.int32) if G else None, G, ptable, pkept, P, part('status', torch.int32, 2),
              part('gt_iou', torch.float64, G), part('gt_match', torch.int32, G), part('pred_area', torch.int32, P),
              part('pred_value', torch.int32, P), part('pred_cat', torch.int32, P), part('pred_flags', torch.uint8, P), stream_ptr(dev))
    return rec, offs


# ------------------------------------------------------------------------------------------------
# Caption metrics on the device (csrc/caption_eval.hip; caption_eval.py states the rules in plain Python)
# ------------------------------------------------------------------------------------------------
CAPTION_MAX_LEN = CONSTANTS['CGG_CAPTION_MAX_LEN']       # tokens of a sentence, in either token stream
CAPTION_MAX_REFS = CONSTANTS['CGG_CAPTION_MAX_REFS']     # references of an image
CAPTION_MAX_VOCAB = 65535                                # an n-gram key packs four 16-bit token ids, 0 is no token


def caption_eval_ok(V, max_len, max_refs):
    """The gate of the caption kernels, host arithmetic only: at most 65535 distinct tokens (the n-gram keys pack 16-bit ids), a
    longest sentence of at most CAPTION_MAX_LEN tokens in either stream and at most CAPTION_MAX_REFS references per image (both from
    the kernels' static LDS layout, see the header). A corpus outside it takes the rules of `caption_eval`, as a whole."""
    return 0 <= int(V) <= CAPTION_MAX_VOCAB and 0 <= int(max_len) <= CAPTION_MAX_LEN and 0 <= int(max_refs) <= CAPTION_MAX_REFS


def _caption_offsets(sent_off, img_off, who):
    N, S = int(img_off.numel()) - 1, int(sent_off.numel()) - 1
    if N < 0 or S < N:
        raise CggError(f'{who}: img_off must hold N + 1 and sent_off S + 1 >= N + 1 offsets (got {img_off.numel()} and {sent_off.numel()})')
    return N, S


def _caption_out(t, name, dtype, shape, dev, who):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise CggError(f'{who}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev} (got {t.dtype}, {tuple(t.shape)} on {t.device})')
    return t


def caption_bleu_lcs(words, sent_off, words_sp, sent_off_sp, img_off, bleu=None, lcs=None):
    """The integer parts of BLEU and ROUGE-L of an interned corpus (`caption_eval.intern_corpus_host`, its arrays on the device) ->
    (bleu int32 (N, 10): testlen, closest reference length, guess[4], correct[4] from the split() stream; lcs int32 (P,): the LCS
    length of every (hypothesis, reference) pair from the split(" ") stream). An image outside the kernel's caps is marked -1. One
    launch on the current stream, no host read."""
    who = 'caption_bleu_lcs'
    dev = img_off.device
    N, S = _caption_offsets(sent_off, img_off, who)
    if sent_off_sp.numel() != S + 1:
        raise CggError(f'{who}: sent_off_sp must hold the same {S + 1} offsets as sent_off (got {sent_off_sp.numel()})')
    W, Wsp = int(words.numel()), int(words_sp.numel())
    bleu = _caption_out(bleu, 'bleu', torch.int32, (N, 10), dev, who)
    lcs = _caption_out(lcs, 'lcs', torch.int32, (S - N,), dev, who)
    with _timed('caption_bleu_lcs', shape=(N, S, W, Wsp)):
        _call('cgg_caption_bleu_lcs_i32', dev_ptr(words, f'{who}: words', torch.int32) if W else None,
              dev_ptr(sent_off, f'{who}: sent_off', torch.int32), W, dev_ptr(words_sp, f'{who}: words_sp', torch.int32) if Wsp else None,
              dev_ptr(sent_off_sp, f'{who}: sent_off_sp', torch.int32), Wsp, dev_ptr(img_off, f'{who}: img_off', torch.int32), N, S,
              dev_ptr(bleu, f'{who}: bleu') if N else None, dev_ptr(lcs, f'{who}: lcs') if S > N else None, stream_ptr(dev))
    return bleu, lcs


def caption_ngram_keys(words, sent_off, img_off, keys=None, flags=None):
    """-> (keys int64 (W, 4): per word and order k the ids of words i .. i + k of its sentence packed 16 bits each, 0 where the
    sentence ends first; flags uint8 (W, 4): 1 iff the position is in a reference and no earlier position of its image's references
    has the same key -- so that the sum of the flags of a key is its document frequency). One launch, no host read."""
    who = 'caption_ngram_keys'
    dev = img_off.device
    N, S = _caption_offsets(sent_off, img_off, who)
    W = int(words.numel())
    keys = _caption_out(keys, 'keys', torch.int64, (W, 4), dev, who)
    flags = _caption_out(flags, 'flags', torch.uint8, (W, 4), dev, who)
    with _timed('caption_ngram_keys', shape=(N, S, W)):
        _call('cgg_caption_ngram_keys_i64', dev_ptr(words, f'{who}: words', torch.int32) if W else None,
              dev_ptr(sent_off, f'{who}: sent_off', torch.int32), W, dev_ptr(img_off, f'{who}: img_off', torch.int32), N, S,
              dev_ptr(keys, f'{who}: keys') if W else None, dev_ptr(flags, f'{who}: flags') if W else None, stream_ptr(dev))
    return keys, flags


def cider_sums(gids, df, idf_by_df, sent_off, img_off, norm2=None, num=None):
    """The ordered double sums of CIDEr (`caption_eval.cider_sums_host`): gids int32 (W, 4) an n-gram id per position and order, df
    int32 (U,) the document frequency of every id, idf_by_df float64 (N + 1,) the host-made table (`caption_eval.idf_table_host`) ->
    (norm2 float64 (S, 4), num float64 (P, 4)); an image outside the kernel's caps is marked -1.0. One launch, no host read."""
    who = 'cider_sums'
    dev = img_off.device
    N, S = _caption_offsets(sent_off, img_off, who)
    W, U = int(gids.shape[0]), int(df.numel())
    if gids.dim() != 2 or gids.shape[1] != 4 or idf_by_df.numel() != N + 1:
        raise CggError(f'{who}: gids must be (W, 4) and idf_by_df hold N + 1 = {N + 1} entries (got {tuple(gids.shape)}, {idf_by_df.numel()})')
    norm2 = _caption_out(norm2, 'norm2', torch.float64, (S, 4), dev, who)
    num = _caption_out(num, 'num', torch.float64, (S - N, 4), dev, who)
    with _timed('cider_sums', shape=(N, S, W, U)):
        _call('cgg_cider_sums_f64', dev_ptr(gids, f'{who}: gids', torch.int32) if W else None, dev_ptr(df, f'{who}: df', torch.int32) if U else None,
              U, dev_ptr(idf_by_df, f'{who}: idf_by_df', torch.float64), dev_ptr(sent_off, f'{who}: sent_off', torch.int32), W,
              dev_ptr(img_off, f'{who}: img_off', torch.int32), N, S, dev_ptr(norm2, f'{who}: norm2') if S else None,
              dev_ptr(num, f'{who}: num') if S > N else None, stream_ptr(dev))
    return norm2, num
