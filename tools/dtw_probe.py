#!/usr/bin/env python
"""Times the DTW alignment of csrc/dtw.hip with HIP events and prints the figures of DESIGN.md section 6 ("DTW alignment"): the three
device phases of ptts_dtw_align_batch one by one (local costs, wavefront, backtrack with the reversal: the `phases` argument runs
a subset of the launches on what the last call left in the workspace) and the whole call, each the median of --reps launches after
3 warm-up launches, for

    batch   eight pairs of 400 to 700 frames a side in ONE call (time-warped copies of a random walk plus noise, D = 65)
    long    one 2000 x 2000 pair

beside the host restatement's time for the same pairs (numpy local costs column by column in fp64, then the dynamic programme and
the backtrack in Python loops, as tests/test_dtw.py states them; run once), and the largest relative difference of the device's
costs from the restatement's.

    python tools/dtw_probe.py [--reps 20] [--no-host]
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 65
SCALE = 20.0 / np.log(10.0)


def warped_pair(rng, Tg, Tr, exponent, noise=0.05):
    R = np.cumsum(rng.randn(Tr, D) * 0.1, axis=0)
    t = (np.arange(Tg) / (Tg - 1.0)) ** exponent * (Tr - 1)
    lo = np.minimum(np.floor(t).astype(int), Tr - 2)
    w = (t - lo)[:, None]
    return ((1 - w) * R[lo] + w * R[lo + 1] + noise * rng.randn(Tg, D)).astype(np.float32), R.astype(np.float32)


def host_align(G, R):
    """The restatement: (cost, path length)."""
    G, R = G.astype(np.float64), R.astype(np.float64)
    acc = np.zeros((G.shape[0], R.shape[0]))
    for d in range(D):
        t = SCALE * (G[:, d][:, None] - R[:, d][None, :])
        acc = acc + t * t
    C = np.sqrt(acc).tolist()
    Tg, Tr = len(C), len(C[0])
    A = [[0.0] * Tr for _ in range(Tg)]
    P = [[3] * Tr for _ in range(Tg)]
    for i in range(Tg):
        Ai, Ci, Pi, Au = A[i], C[i], P[i], A[i - 1] if i > 0 else None
        for j in range(Tr):
            best, frm = None, 3
            if i > 0 and j > 0:
                best, frm = Au[j - 1], 0
            if i > 0 and (best is None or Au[j] < best):
                best, frm = Au[j], 1
            if j > 0 and (best is None or Ai[j - 1] < best):
                best, frm = Ai[j - 1], 2
            Ai[j] = Ci[j] if best is None else Ci[j] + best
            Pi[j] = frm
    i, j, n = Tg - 1, Tr - 1, 1
    while (i, j) != (0, 0):
        frm = P[i][j]
        if frm != 2: i -= 1
        if frm != 1: j -= 1
        n += 1
    return A[-1][-1], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'dtw_probe needs the GPU'
    rng = np.random.RandomState(0)
    sides = [(400, 430), (460, 400), (520, 560), (600, 540), (640, 700), (700, 650), (480, 610), (570, 450)]
    sets = (('batch', [warped_pair(rng, tg, tr, 1.0 + 0.05 * k) for k, (tg, tr) in enumerate(sides)]),
            ('long', [warped_pair(rng, 2000, 2000, 1.2)]))
    phases = (('costs', _hip._define('PTTS_DTW_PHASE_COSTS')), ('wavefront', _hip._define('PTTS_DTW_PHASE_WAVEFRONT')),
              ('backtrack', _hip._define('PTTS_DTW_PHASE_BACKTRACK')), ('all', _hip._define('PTTS_DTW_PHASE_ALL')))
    res = {'D': D, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'max_frames': ops.dtw_max_frames()}
    for label, pairs in sets:
        G = torch.from_numpy(np.concatenate([g for g, _ in pairs])).cuda()
        R = torch.from_numpy(np.concatenate([r for _, r in pairs])).cuda()
        gl, rl = [g.shape[0] for g, _ in pairs], [r.shape[0] for _, r in pairs]
        go, ro = ops.packed_offsets(gl, G.device), ops.packed_offsets(rl, G.device)
        times = {name: [] for name, _ in phases}
        for rep in range(3 + args.reps):
            with _hip.KernelTimer() as kt:
                for name, mask in phases:
                    out = ops.dtw_align(G, R, go, ro, scale=SCALE, phases=mask)
            if rep >= 3:
                for (name, _), (_, _, ms) in zip(phases, kt.durations_ms()):
                    times[name].append(ms * 1e-3)
        cells = sum(g * r for g, r in zip(gl, rl))
        entry = {'pairs': len(pairs), 'sides': list(zip(gl, rl)), 'cells': cells,
                 'path_lengths': out.lengths.cpu().numpy().tolist()}
        for name, ts in times.items():
            entry[name + '_s'] = float(np.median(ts))
        entry['cells_per_s'] = cells / entry['all_s']
        if not args.no_host:
            t0 = time.perf_counter()
            want = [host_align(g, r) for g, r in pairs]
            entry['host_restatement_s'] = time.perf_counter() - t0
            entry['host_over_device'] = entry['host_restatement_s'] / entry['all_s']
            cost = out.cost.cpu().numpy()
            entry['cost_largest_relative_difference'] = float(max(abs(c - w[0]) / w[0] for c, w in zip(cost, want)))
            entry['path_lengths_equal'] = [w[1] for w in want] == entry['path_lengths']
        res[label] = entry
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
