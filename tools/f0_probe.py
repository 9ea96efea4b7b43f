#!/usr/bin/env python
"""Times the two launches of csrc/f0.hip with HIP events for one utterance and prints the figures of DESIGN.md section 6:
ptts_f0_candidates and ptts_f0_viterbi, and in the same run ptts_frame_harmonics as the yardstick (median of --reps launches after 3
warm-up launches; the window table is built before the first timed launch), beside the estimate's voicing and pitch errors against
the track the waveform was synthesised from.

Default size, that of tools/analysis_probe.py: T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, f0 = 170 + 60 sin(i / 7) Hz
searched in 70 .. 600 Hz; the waveform comes from ops.pulse_synthesis on a smooth envelope with the noise mask set above fs / 5.

    python tools/f0_probe.py [--frames 1000] [--fs 32000] [--dftlen 4096] [--f0min 70] [--f0max 600] [--ncand 8] [--reps 20]
"""
from __future__ import print_function

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--f0min', type=float, default=70.0)
    ap.add_argument('--f0max', type=float, default=600.0)
    ap.add_argument('--ncand', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'f0_probe needs the GPU'
    T, fs, L = args.frames, args.fs, args.dftlen
    K = L // 2 + 1
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    fw = (rng.uniform(-6.0, -3.0) + np.cumsum(rng.randn(2, 65) * 0.3, axis=1))
    x = np.linspace(0, 1, T)[:, None]
    fw = ((1 - x) * fw[0] + x * fw[1]).astype(np.float32)                   # a slow morph between two smooth envelopes
    spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
    mask = torch.from_numpy(np.tile((np.arange(K) * fs / L >= fs / 5.0).astype(np.float32), (T, 1))).cuda()
    tab = ops.pulse_table(f0, SHIFT, fs, wavlen, L)
    wav = ops.pulse_synthesis(spec, mask, tab, torch.from_numpy(rng.randn(wavlen).astype(np.float32)).cuda(), fs, L, wavlen)
    hw, lmin, lmax = ops.f0_check(L, fs, SHIFT, args.f0min, args.f0max)
    hcap = ops.analysis_check(L, fs, SHIFT, args.f0min, args.f0max)
    assert ops.f0_frame_count(wavlen, SHIFT, fs) == T
    w64 = wav.to(torch.float64)
    gpeak = float((w64 - w64.mean()).abs().max().item())
    f0_d = torch.from_numpy(ops.f0_track(f0, args.f0min, args.f0max, fs, SHIFT, L, wavlen=wavlen)).cuda()

    per_launch = {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kt:
            freq, strength, n, lag = ops.f0_candidates(wav, T, SHIFT, fs, L, args.f0min, args.f0max, gpeak, ncand=args.ncand)
            est = ops.f0_viterbi(freq, strength, n, SHIFT)
            ops.frame_harmonics(wav, f0_d, SHIFT, fs, L, hcap, log=True)
        if rep >= 3:
            for name, _, ms in kt.durations_ms():
                per_launch.setdefault(name, []).append(ms * 1e-3)
    res = {'frames': T, 'fs': fs, 'dftlen': L, 'f0_min': args.f0min, 'f0_max': args.f0max, 'ncand': args.ncand, 'window': 2 * hw + 1,
           'lags': [lmin, lmax], 'wavlen': wavlen, 'seconds_of_speech': wavlen / fs, 'device': torch.cuda.get_device_name(0),
           'reps': args.reps}
    for name, ts in per_launch.items():
        res[name] = {'s': float(np.median(ts)), 'frames_per_s': T / float(np.median(ts))}
    res['candidates_over_frame_harmonics'] = res['ptts_f0_candidates']['s'] / res['ptts_frame_harmonics']['s']

    est = est.cpu().numpy()
    inner = np.arange(4, T - 4)
    voiced = est[inner] > 0
    rel = np.abs(est[inner][voiced].astype(np.float64) / f0[inner][voiced] - 1.0)
    res['voiced_share'] = float(voiced.mean())
    res['relative_error_mean'], res['relative_error_max'] = float(rel.mean()), float(rel.max())
    res['gross_errors'] = int((rel > 0.2).sum())
    res['candidates_mean'] = float(n.cpu().numpy().mean())
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
