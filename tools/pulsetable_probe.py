#!/usr/bin/env python
"""Times the pulse table on the device (csrc/pulsetable.hip) and what it buys, and prints the figures of DESIGN.md section 6: the
HIP-event times of ptts_pulse_walk and ptts_pulse_rows for a batch of utterances, and the wall time (a device synchronise on both
sides) of a loop of synthesis_device calls, one per utterance with its pulse table built on the host, beside one
synthesis_device_batch call over the same utterances; median and p10 / p90 of --reps repetitions after 3 warm-ups, both in this
process on the same box.  synthesis_device is the per-utterance path as it was before the batched one existed.

Default size: 8 utterances of T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, 65 spectral and 25 noise bands, seeded f0
contours around 170 + 60 sin(i / 7) Hz; the WORLD form has voiced and unvoiced stretches of --stretch frames in turn.

    python tools/pulsetable_probe.py [--utts 8] [--frames 1000] [--fs 32000] [--dftlen 4096] [--nb 25] [--stretch 50] [--reps 20]
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005
NSPEC = 65


def spread(ts):
    return {'median_s': float(np.median(ts)), 'p10_s': float(np.percentile(ts, 10)), 'p90_s': float(np.percentile(ts, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--nb', type=int, default=25)
    ap.add_argument('--stretch', type=int, default=50)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops, vocoders
    assert torch.cuda.is_available(), 'pulsetable_probe needs the GPU'
    B, T, fs, L, nb = args.utts, args.frames, args.fs, args.dftlen, args.nb
    rng = np.random.RandomState(0)
    i = np.arange(T)
    f0s = [(170.0 + rng.uniform(-20, 20) + 60.0 * np.sin(i / 7.0 + rng.uniform(0, 6.28))).astype(np.float32) for _ in range(B)]
    voiced = (i // args.stretch) % 2 == 0
    res = {'utterances': B, 'frames': T, 'fs': fs, 'dftlen': L, 'nb': nb, 'stretch': args.stretch, 'reps': args.reps,
           'seconds_of_speech': B * SHIFT * (T - 1), 'device': torch.cuda.get_device_name(0)}

    for key in ('pml', 'world'):
        if key == 'pml':
            voc = vocoders.VocoderPML(fs, SHIFT, NSPEC, nb, dftlen=L)
            tail = lambda: [np.clip(np.linspace(0.0, 1.0, nb)[None, :] + rng.randn(T, nb) * 0.2, 0, 1)]
        else:
            voc = vocoders.VocoderWORLDDevice(fs, SHIFT, NSPEC, nb, dftlen=L)
            tail = lambda: [np.clip(np.linspace(-30.0, 0.0, nb)[None, :] + rng.randn(T, nb) * 4.0, -60.0, 3.0),
                            voiced.astype(np.float64)[:, None]]
        CMPs = []
        for f0 in f0s:
            fw = rng.uniform(-6.0, -3.0, size=(T, 1)) + np.cumsum(rng.randn(T, NSPEC) * 0.3, axis=1)
            cmp_ = np.concatenate([np.log(f0.astype(np.float64))[:, None], fw] + tail(), axis=1).astype(np.float32)
            CMPs.append(torch.from_numpy(cmp_).cuda())

        # the two table kernels alone
        f0_d = torch.exp(torch.cat([c[:, 0] for c in CMPs])).contiguous()
        voiced_d = torch.cat([c[:, -1] >= 0.5 for c in CMPs]) if key == 'world' else None
        launches = {}
        for rep in range(3 + args.reps):
            with _hip.KernelTimer() as kt:
                table = ops.pulse_table_device(f0_d, [T] * B, SHIFT, fs, L, voiced=voiced_d)
            if rep >= 3:
                for name, _, ms in kt.durations_ms():
                    launches.setdefault(name, []).append(ms * 1e-3)
        out = {'pulses': table.P, 'pulse_slots_per_utterance': table.cap, 'largest_window': table.W}
        for name, ts in launches.items():
            out[name] = spread(ts)
        out['ptts_pulse_walk']['s_per_pulse_of_the_longest_utterance'] = out['ptts_pulse_walk']['median_s'] / int(table.counts.max())

        # the per-utterance loop beside the batch
        loop, batch = [], []
        for rep in range(3 + args.reps):
            ops.rng_seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = [voc.synthesis_device(c) for c in CMPs]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ops.rng_seed(rep)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            got = voc.synthesis_device_batch(CMPs)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if rep >= 3:
                loop.append(t1 - t0)
                batch.append(t3 - t2)
        out['same_bytes'] = all(np.array_equal(g, w) for g, w in zip(got, want))
        out['synthesis_device_loop'], out['synthesis_device_batch'] = spread(loop), spread(batch)
        out['loop_median_over_batch_median'] = out['synthesis_device_loop']['median_s'] / out['synthesis_device_batch']['median_s']
        out['batch_p90_below_loop_p10'] = out['synthesis_device_batch']['p90_s'] < out['synthesis_device_loop']['p10_s']

        # where the loop's time goes: the host table of one utterance
        f0_h = f0_d[:T].cpu().numpy()
        t0 = time.perf_counter()
        if key == 'world':
            ops.world_pulse_table(f0_h, voiced, SHIFT, fs, int(round(SHIFT * (T - 1) * fs)), L)
        else:
            ops.pulse_table(f0_h, SHIFT, fs, int(round(SHIFT * (T - 1) * fs)), L)
        out['host_table_of_one_utterance_s'] = time.perf_counter() - t0
        res[key] = out
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
