"""Device results -> host results for serving / evaluation.

The reference hands every mask to the host as its own (H, W) bool array (open_set/models/maskformer.py:205-208: ~300
`.cpu().numpy()` calls and 315 MB per 1024^2 image) and the evaluation path then run-length encodes each of them
(pycocotools `mask.encode` inside the dataset's `results2json`). `RleCollector` produces that END format directly:

  device   masks stay bit-packed ((n, H, W/8) uint8 from `cgg_instance_masks_picks(bitpack=1)`: 39 MB per image)
  copy     ONE asynchronous device->host copy per tensor into pinned staging buffers on a side stream, ordered after the
           producing stream by an event -- the GPU pipeline is never blocked by a pageable `.cpu()`
  host     `cgg_rle_encode_bitmasks` (C++ host threads of the extension) -> COCO RLE dicts, in a worker thread that
           overlaps the next batch's device work (ctypes releases the GIL)

`RleCollector(device_rle=True)` (opt-in) moves the first half of the encoding to the device. A run-length code is determined by
where the column-major bit stream changes value; finding those places is a bit transpose and a compaction:

  device   `cgg_rle_transitions` (csrc/rle_device.hip; `rle_transitions_host` below is its rule) on the copy stream, after the
           `ready` event, into buffers the slot owns: the transitions of every mask (uint32 positions, int64 offsets) and the
           column-major planes. `fut.copied` is recorded after these launches: nothing reads the caller's tensors afterwards
  copy     the offsets and `run_capacity` positions per tensor (default 2048 per mask: 2.4 MB per 300-mask image, not 39 MB)
  host     `cgg_rle_strings_from_transitions`: delta coding and 5-bit groups, per run. The masks of a tensor from the first one
           whose positions did not fit are encoded from their column-major planes in the slot's workspace instead (one further
           copy of those planes, `cgg_rle_encode_colmajor`): no batch raises, no result differs
Tensors that are not bit-packed take the path above unchanged.

Result per image: {eval_type: (bbox_results, segm_results)} with the reference's per-class list layout
(`bbox2result` arrays; `segm_results[label]` = list of {'size': [H, W], 'counts': bytes}), i.e. what
`results2json` would build from the reference's arrays.
"""
import concurrent.futures as cf

import numpy as np
import torch

from . import ops


class RleCollector:

    RUNS_PER_MASK = 2048      # default `run_capacity` = this many transitions per mask of the tensor

    def __init__(self, device, num_classes, depth=3, rle_threads=None, device_rle=False, run_capacity=None):
        """num_classes: {eval_type: number of classes} (the fusion head's all / novel / base class counts).

        device_rle=True: the run boundaries of every bit-packed mask tensor are found on the device (`ops.rle_transitions`,
        on the copy stream) and only they are copied; the worker turns them into the counts strings. The results are the same
        dicts, byte for byte. run_capacity: the number of positions the device may write PER TENSOR (an eval type's masks of
        one image share it); the whole buffer is copied, so it is also the copy's size. Default: 2048 per mask of the tensor,
        i.e. 8 KB per mask and 2.4 MB per 300-mask image whatever its size, instead of the 39 MB of the planes of a 1024^2
        image (a trained model's masks have a few hundred transitions each: 0.5-2 KB of RLE). The masks of a tensor are
        written in order while they fit: from the first one that would pass the capacity on, the tensor's masks are encoded
        by the worker from their column-major planes in the slot's workspace (one further copy of those planes,
        `ops.rle_encode_colmajor`). No batch raises and no result differs."""
        self.device = torch.device(device)
        self.num_classes = dict(num_classes)
        self.depth = depth
        self.device_rle = bool(device_rle)
        self.run_capacity = None if run_capacity is None else int(run_capacity)
        if self.run_capacity is not None and self.run_capacity < 0:
            raise ValueError(f'run_capacity={run_capacity}: a number of positions (>= 0) expected')
        import os
        from . import runtime
        # the encoder's cost is per RUN; `depth` batches are encoded concurrently, each on this many host threads. The budget is
        # the CPUs the process may really use (cgroup quota, not `nproc`): oversubscribing it gets every thread throttled
        self.rle_threads = rle_threads or int(os.environ.get('CGG_RLE_THREADS', 0)) or \
            max(2, min(16, (runtime.effective_cpu_count() - 2) // max(depth, 1)))
        self.copy_stream = torch.cuda.Stream(self.device)
        self.fallback_stream = torch.cuda.Stream(self.device) if self.device_rle else None
        self.pool = cf.ThreadPoolExecutor(max_workers=depth)
        self._slots = [dict(buffers={}, event=None, future=None) for _ in range(depth)]
        self._n = 0
        # what left the device and how (read by measurements; masks / fallback_masks count device-mode tensors only)
        self.stats = dict(d2h_bytes=0, masks=0, fallback_masks=0)

    def _pinned(self, slot, key, like):
        buf = slot['buffers'].get(key)
        if buf is None or buf.shape != like.shape or buf.dtype != like.dtype:
            buf = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
            slot['buffers'][key] = buf
        return buf

    def _device_buffer(self, slot, key, numel, dtype, device):
        buf = slot['buffers'].get(key)
        if buf is None or buf.numel() < numel or buf.device != device:
            buf = torch.empty(max(int(numel), 2), dtype=dtype, device=device)
            slot['buffers'][key] = buf
        return buf

    def _takes_device_path(self, masks):
        """bit-packed planes on this device that `ops.rle_transitions` reads in place"""
        n, H, rb = masks.shape if masks.dim() == 3 else (0, 0, 0)
        mine = masks.is_cuda and (self.device.index is None or masks.device.index == self.device.index)
        return self.device_rle and masks.dtype == torch.uint8 and masks.dim() == 3 and mine and \
            H > 0 and rb > 0 and (n == 0 or (masks.stride(2) == 1 and masks.stride(1) == rb and masks.stride(0) >= H * rb))

    def submit(self, results, width=None):
        """results: list (one per image) of {eval_type: (labels, bboxes (n, 5), masks (n, H, W/8) uint8)} DEVICE tensors
        (`simple_test(..., device_results=True, mask_bits=True)`). Returns a future -> list of host result dicts.
        The device tensors may be overwritten once `wait_copied(ticket)` returned (ticket = the future's `.ticket`)."""
        slot = self._slots[self._n % self.depth]
        if slot['future'] is not None:
            slot['future'].result()                       # the slot's previous batch has left its pinned buffers
        self._n += 1
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        staged, nbytes = [], 0
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            on_device = []
            for i, res in enumerate(results):
                per = {}
                for key, val in res.items():
                    if not (isinstance(val, (tuple, list)) and len(val) == 3 and torch.is_tensor(val[2])):
                        continue
                    labels, bboxes, masks = val
                    packed = masks.dtype != torch.bool
                    if not packed:                      # shapes outside the bit-packing kernel: packed on the host below
                        masks = masks.view(torch.uint8)
                    w_px = int(width) if width is not None else masks.shape[-1] * (8 if packed else 1)
                    hl = self._pinned(slot, (i, key, 'l'), labels)
                    hb = self._pinned(slot, (i, key, 'b'), bboxes)
                    hl.copy_(labels, non_blocking=True)
                    hb.copy_(bboxes, non_blocking=True)
                    nbytes += hl.numel() * hl.element_size() + hb.numel() * hb.element_size()
                    if packed and self._takes_device_path(masks) and masks.shape[1] * w_px < 2 ** 31:
                        n, H, _ = masks.shape
                        cap = self.run_capacity if self.run_capacity is not None else self.RUNS_PER_MASK * n
                        need = int(ops._lib_().cgg_rle_transitions_workspace_bytes(n, H, w_px))
                        ws = self._device_buffer(slot, (i, key, 'ws'), max(need, 8), torch.uint8, masks.device)
                        pos = self._device_buffer(slot, (i, key, 'pos'), cap, torch.int32, masks.device)
                        off = self._device_buffer(slot, (i, key, 'off'), n + 1, torch.int64, masks.device)
                        ops.rle_transitions(masks, w_px, capacity=cap, positions=pos, offsets=off, ws=ws)
                        on_device.append((i, key, n, cap, pos, off))
                        per[key] = (hl, hb, None, w_px, dict(n=n, H=H, cap=cap, ws=ws, slot=slot, tag=(i, key)))
                    else:
                        hm = self._pinned(slot, (i, key, 'm'), masks)
                        hm.copy_(masks, non_blocking=True)
                        nbytes += hm.numel() * hm.element_size()
                        per[key] = (hl, hb, hm, w_px, packed)
                staged.append(per)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
            copied = done
            if on_device:
                # nothing reads the caller's tensors past this point: `copied` is recorded after the kernels, the transitions
                # leave from the slot's own buffers
                for i, key, n, cap, pos, off in on_device:
                    hp = self._pinned(slot, (i, key, 'hp'), pos[:max(cap, 1)])
                    ho = self._pinned(slot, (i, key, 'ho'), off[:n + 1])
                    ho.copy_(off[:n + 1], non_blocking=True)
                    if cap > 0:
                        hp.copy_(pos[:cap], non_blocking=True)
                    nbytes += ho.numel() * 8 + cap * 4
                    staged[i][key][4].update(hp=hp, ho=ho)
                done = torch.cuda.Event()
                done.record(self.copy_stream)
        self.stats['d2h_bytes'] += nbytes
        slot['event'] = done
        fut = self.pool.submit(self._encode, staged, done)
        fut.copied = copied
        slot['future'] = fut
        return fut

    @staticmethod
    def wait_copied(fut):
        """Host-side wait until the batch's device tensors have been copied out (they may then be overwritten)."""
        fut.copied.synchronize()

    def _strings_from_device(self, d, W):
        """device mode, worker side: the strings of one tensor from its transitions; the masks past the capacity from their
        column-major planes, which are still in the slot's workspace (the slot is reused only after this future resolved)"""
        n, H, cap = d['n'], d['H'], d['cap']
        offs = d['ho'].numpy()
        k = int(np.searchsorted(offs[1:], cap, side='right'))           # masks 0 .. k - 1 were written
        pos = d['hp'].numpy().view(np.uint32)
        rles = ops.rle_strings_from_transitions(pos, np.ascontiguousarray(offs[:k + 1]), H, W) if k else []
        self.stats['masks'] += n
        if k < n:
            Wp, Hb = ops.rle_cols_shape(H, W)
            words = d['ws'][:n * Wp * Hb * 8].view(torch.int64).view(n, Wp, Hb)
            hc = d['slot']['buffers'].get(d['tag'] + ('hc',))
            if hc is None or hc.shape != words.shape:
                hc = torch.empty(words.shape, dtype=torch.int64, pin_memory=True)
                d['slot']['buffers'][d['tag'] + ('hc',)] = hc
            with torch.cuda.stream(self.fallback_stream):
                hc[:n - k].copy_(words[k:], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.fallback_stream)
            ev.synchronize()
            self.stats['d2h_bytes'] += (n - k) * Wp * Hb * 8
            self.stats['fallback_masks'] += n - k
            rles += ops.rle_encode_colmajor(hc[:n - k], H, W, threads=self.rle_threads)
        return rles

    def _encode(self, staged, done):
        done.synchronize()
        out = []
        for per in staged:
            res = {}
            for key, (hl, hb, hm, W, packed) in per.items():
                labels = hl.numpy().astype(np.int64)
                bboxes = hb.numpy().copy()
                if hm is None:
                    rles = self._strings_from_device(packed, W)
                else:
                    bits = hm if packed else np.packbits(hm.numpy(), axis=-1, bitorder='little')
                    rles = ops.rle_encode_bitmasks(bits, W, threads=self.rle_threads)
                ncls = int(self.num_classes[key])
                bbox_results = [bboxes[labels == c, :] for c in range(ncls)]
                segm = [[] for _ in range(ncls)]
                for lab, r in zip(labels.tolist(), rles):
                    segm[lab].append(r)
                res[key] = (bbox_results, segm)
            out.append(res)
        return out

    def close(self):
        self.pool.shutdown(wait=True)


def rle_transitions_host(bits, width):
    """The rule `ops.rle_transitions` (csrc/rle_device.hip) must equal exactly, in numpy.

    bits (n, H, row_bytes) uint8, pixel x of a row = bit (x & 7) of byte (x >> 3); only the first `width` pixels of a row
    count, pad bits may hold anything. With the column-major stream p = x * H + y, v(p) the pixel and v(-1) = 0, position p
    is a transition iff v(p) != v(p - 1): the bottom pixel of column x precedes the top pixel of column x + 1, and a mask whose
    pixel (0, 0) is set has a transition at 0. -> (positions uint32, ascending per mask, packed mask after mask;
    offsets int64 [n + 1]). The COCO counts of mask i are then [t0, t1 - t0, ..., H * W - t_last], or [H * W] for an empty
    mask. H * W < 2**31."""
    bits = np.asarray(bits)
    if bits.dtype != np.uint8 or bits.ndim != 3:
        raise ValueError('rle_transitions_host: (n, H, row_bytes) uint8 array expected')
    n, H, rb = bits.shape
    W = int(width)
    if not (0 < W <= rb * 8) or H <= 0 or H * W >= 2 ** 31:
        raise ValueError(f'rle_transitions_host: H={H}, width={W}, row_bytes={rb}')
    px = np.unpackbits(bits, axis=-1, bitorder='little')[:, :, :W]
    v = px.transpose(0, 2, 1).reshape(n, W * H)
    before = np.concatenate([np.zeros((n, 1), np.uint8), v[:, :-1]], axis=1)
    which, where = np.nonzero(v != before)                 # row-major: ascending per mask, mask after mask
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(which, minlength=n), out=offsets[1:])
    return where.astype(np.uint32), offsets


def fusion_class_counts(fusion_head):
    return dict(all_results=getattr(fusion_head, 'all_classes', None), novel_results=getattr(fusion_head, 'novel_classes', None),
                base_results=getattr(fusion_head, 'base_classes', None))


def rle_to_mask(rle):
    """Decoder of the COCO counts string (tests / consumers without pycocotools): -> (H, W) bool."""
    H, W = rle['size']
    s = rle['counts']
    counts, i, p = [], 0, 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if i > 2:
            x += counts[i - 2]
        counts.append(x)
        i += 1
    flat = np.zeros(H * W, dtype=bool)
    pos, v = 0, False
    for c in counts:
        if v:
            flat[pos:pos + c] = True
        pos += c
        v = not v
    return flat.reshape((W, H)).T
