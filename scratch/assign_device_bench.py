"""Device Hungarian solver against the host path it replaces (-> profiles/assign_device_ab.txt).

160 problems (16 images x 10 layers) at Q = 100: G drawn 1..20 per image, as synthetic.train_batch(max_inst=20) gives, and the
worst case G = 100. Device: ONE launch of cgg_lsap_device_f32 with the label / weight epilogue, timed with events after warm-up.
Host: what `_targets_batched` does with CGG_DEVICE_ASSIGN=0 after the costs exist -- D2H of the cost matrices into pinned memory,
ops.linear_sum_assignment_batch, the Python / numpy target loop, the H2D of labels / weights / index table -- as wall time from the
copy's enqueue to the last upload's completion. Indices are compared once.

    python scratch/assign_device_bench.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cgg_amd  # noqa: E402,F401
from cgg_amd import ops  # noqa: E402


def problems(Q, Gs, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, Q, G, generator=g) * 4 - 2 for G in Gs]          # per image: (n, Q, G)


def device_side(costs, Q, n, dev, reps):
    B = len(costs)
    Gs = [int(c.shape[2]) for c in costs]
    m = [min(Q, G) for G in Gs]
    K = sum(m)
    table, coff, loff, slot, lds = [], 0, 0, 0, 0
    for b, G in enumerate(Gs):
        table.extend((coff + li * Q * G, Q, G, li * K + slot, (li * B + b) * Q, loff) for li in range(n))
        coff += n * Q * G
        lds = max(lds, ops.lsap_device_lds_bytes(Q, G))
        slot += m[b]
        loff += G
    flat = torch.cat([c.reshape(-1) for c in costs]).to(dev)
    desc = torch.tensor(table, dtype=torch.int64).to(dev)
    gt = torch.randint(0, 80, (loff,), device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    q = torch.zeros(n * K, dtype=torch.int64, device=dev)
    g = torch.zeros(n * K, dtype=torch.int64, device=dev)
    labels = torch.full((n, B, Q), 80, dtype=torch.int64, device=dev)
    weights = torch.zeros((n, B, Q), dtype=torch.float32, device=dev)
    times = []
    for it in range(reps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.lsap_device_launch(flat, desc, lds, q, g, status, gt_labels=gt, labels=labels, weights=weights)
        e.record()
        e.synchronize()
        if it >= 3:
            times.append(s.elapsed_time(e))
    assert status.tolist() == [0, 0]
    return flat, q.cpu().view(n, K), g.cpu().view(n, K), float(np.median(times)), float(np.max(times))


def host_side(flat_dev, costs, Q, n, dev, reps):
    B = len(costs)
    Gs = [int(c.shape[2]) for c in costs]
    gl_host = [np.random.RandomState(b).randint(0, 80, (G,)) for b, G in enumerate(Gs)]
    pinned = torch.empty(flat_dev.shape, dtype=flat_dev.dtype, pin_memory=True)
    times, pairs = [], None
    for it in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(flat_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        mats, off = [], 0
        for G in Gs:
            cm = pinned[off:off + n * Q * G].view(n, Q, G)
            off += n * Q * G
            mats.extend(cm[li] for li in range(n))
        solved = iter(ops.linear_sum_assignment_batch(mats))
        labels_np = np.full((n, B, Q), 80, dtype=np.int64)
        weights_np = np.zeros((n, B, Q), dtype=np.float32)
        pos = [[[] for _ in range(n)] for _ in range(4)]
        for b, G in enumerate(Gs):
            for li in range(n):
                rows, cols = (t.numpy() for t in next(solved))
                order = np.argsort(rows)
                rows, cols = rows[order], cols[order]
                labels_np[li, b, rows] = gl_host[b][cols]
                weights_np[li, b, rows] = 1.0
                pos[0][li].extend([b] * len(rows))
                pos[1][li].extend(rows.tolist())
                pos[2][li].extend(cols.tolist())
                pos[3][li].extend(range(len(rows)))
        torch.from_numpy(labels_np).to(dev, non_blocking=True)
        torch.from_numpy(weights_np).to(dev, non_blocking=True)
        idx = np.array([sum(p, []) for p in pos], dtype=np.int64).reshape(4, -1)
        torch.from_numpy(idx).to(dev, non_blocking=True)
        torch.cuda.synchronize()
        if it >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
        pairs = (pos[1], pos[2])
    return pairs, float(np.median(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    Q, n, B = 100, 10, 16
    g = torch.Generator().manual_seed(3)
    drawn = [int(torch.randint(1, 21, (1,), generator=g)) for _ in range(B)]
    for name, Gs in (('G drawn 1..20', drawn), ('G = 100 (worst case)', [100] * B)):
        costs = problems(Q, Gs, n, 7)
        flat, q, gg, d_med, d_max = device_side(costs, Q, n, dev, args.reps)
        (hq, hg), h_med, h_max = host_side(flat, costs, Q, n, dev, args.reps)
        same = all(q[li].tolist() == hq[li] and gg[li].tolist() == hg[li] for li in range(n))
        print(f'{n * B} problems, Q = {Q}, {name} (sum G = {sum(Gs)}): device launch {d_med:.3f} ms median ({d_max:.3f} max), '
              f'host path {h_med:.3f} ms median ({h_max:.3f} max) wall, indices equal: {same}', flush=True)


if __name__ == '__main__':
    main()
