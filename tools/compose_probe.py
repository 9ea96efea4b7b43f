#!/usr/bin/env python
"""Times the three launches of csrc/compose.hip with HIP events at a corpus-like size and prints rows/s and the achieved
fraction of the HBM figure bench.py's roofline uses (8 TB/s).

Default size: 1 000 utterances of 450..750 frames (~600 000 rows), D = 163 raw columns (lf0 + 129 spec + 33 noise), two windows
(K = 3, 489 composed columns), the first 900 utterances counting for the statistics.  Algorithmic bytes per launch:
    compose_windows    4 R D read + 4 R K D written
    compose_sqdev      4 R' K D read (R' rows of the statistics utterances)
    compose_normalise  4 R K D read + 4 R K D written (in place)
For scale it also times a device-to-device copy of the composed rows on the same box (what a bandwidth-bound kernel can hope
for) and the numpy restatement of the same work on the host (windows per column through scipy.signal.convolve, fp64 statistics,
fp32 normalisation) over a sample of the utterances, on the threads the environment allows (OMP_NUM_THREADS, 16 by default).

    python tools/compose_probe.py [--utts 1000] [--D 163] [--wins 2] [--reps 20] [--host-utts 40]
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM_GBPS = 8000.0          # the figure of bench.py's roofline
WINS = [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]


def timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup): fn()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    return float(np.median(times))


def host_restatement(Y, offs, wins, nstat):
    """The reference's three sweeps in numpy over utterances [offs[i], offs[i+1]) of Y (fp32 [R,D])."""
    import scipy.signal
    comp, sums, n = [], None, 0
    for i in range(len(offs) - 1):
        y = Y[offs[i]:offs[i + 1]]
        streams = [y]
        for w in wins:
            yw = np.ones(y.shape)
            for d in range(y.shape[1]):
                yw[1:-1, d] = -scipy.signal.convolve(y[:, d], w)[2:-2]
            yw[0], yw[-1] = yw[1], yw[-2]
            streams.append(yw)
        c = np.hstack(streams)
        if i < nstat:
            sums = c.sum(axis=0) if sums is None else sums + c.sum(axis=0)
            n += c.shape[0]
        comp.append(c.astype(np.float32))
    mean = sums / n
    sq = sum(((c - mean) ** 2).sum(axis=0) for c in comp[:nstat])
    std = np.sqrt(sq / (n - 1)).astype(np.float32)
    m32 = mean.astype(np.float32)
    return [(c - m32) / std for c in comp]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=1000)
    ap.add_argument('--D', type=int, default=163)
    ap.add_argument('--wins', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-utts', type=int, default=40)
    a = ap.parse_args()
    import torch
    from percivaltts_amd import ops
    assert torch.cuda.is_available(), 'compose_probe needs the device'
    rng = np.random.RandomState(0)
    lens = rng.randint(450, 751, size=a.utts)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    R, D, wins = int(offs[-1]), a.D, WINS[:a.wins]
    K = 1 + len(wins)
    nstat = int(0.9 * a.utts)
    Rstat = int(offs[nstat])
    Y = rng.randn(R, D).astype(np.float32)
    y, offs_d = torch.from_numpy(Y).cuda(), torch.from_numpy(offs).cuda()
    out = torch.empty(R, K * D, dtype=torch.float32, device='cuda')
    stats = ops.compose_stats_buffers(K * D, 'cuda')
    t_win = timed(lambda: ops.compose_windows(y, offs_d, wins, stats=stats, n_stat_utts=nstat, out=out), a.reps)
    stats = ops.compose_stats_buffers(K * D, 'cuda')
    ops.compose_windows(y, offs_d, wins, stats=stats, n_stat_utts=nstat, out=out)
    mean = stats[2] / Rstat
    sq = torch.zeros(K * D, dtype=torch.float64, device='cuda')
    t_sq = timed(lambda: ops.compose_sqdev(out, offs_d, mean, sq, nstat), a.reps)
    sq.zero_()
    ops.compose_sqdev(out, offs_d, mean, sq, nstat)
    std = torch.sqrt(sq / (Rstat - 1)).float()
    m32 = mean.float()
    norm = torch.empty_like(out)
    t_norm = timed(lambda: ops.compose_normalise(out, m32, std, out=norm), a.reps)
    t_copy = timed(lambda: norm.copy_(out), a.reps)
    rows = []
    for name, t, nbytes, r in (('compose_windows', t_win, 4.0 * R * D + 4.0 * R * K * D, R), ('compose_sqdev', t_sq, 4.0 * Rstat * K * D, Rstat),
                               ('compose_normalise', t_norm, 8.0 * R * K * D, R), ('device copy of the composed rows', t_copy, 8.0 * R * K * D, R)):
        rows.append(dict(launch=name, ms=t * 1e3, rows_per_s=r / t, GBps=nbytes / t / 1e9, frac_of_hbm_peak=nbytes / t / 1e9 / PEAK_HBM_GBPS))
        print('{:34s} {:8.3f} ms  {:10.3e} rows/s  {:8.1f} GB/s  {:.3f} of {:.0f} GB/s'.format(
            name, t * 1e3, r / t, nbytes / t / 1e9, nbytes / t / 1e9 / PEAK_HBM_GBPS, PEAK_HBM_GBPS))
    hu = min(a.host_utts, a.utts)
    t0 = time.time()
    host_restatement(Y, offs[:hu + 1], wins, max(2, int(0.9 * hu)))
    t_host = time.time() - t0
    host_rows = int(offs[hu])
    dev_total = t_win + t_sq + t_norm
    print('host numpy restatement: {} utterances ({} rows) in {:.2f} s = {:.3e} rows/s on {} threads; the three launches together: {:.3e} rows/s'.format(
        hu, host_rows, t_host, host_rows / t_host, os.environ.get('OMP_NUM_THREADS', '16'), R / dev_total))
    print(json.dumps(dict(R=R, D=D, K=K, utts=a.utts, stat_utts=nstat, launches=rows,
                          host=dict(utts=hu, rows=host_rows, seconds=t_host, rows_per_s=host_rows / t_host))))


if __name__ == '__main__':
    main()
