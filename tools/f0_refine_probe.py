#!/usr/bin/env python
"""Times ptts_f0_refine with HIP events next to the estimator it follows, ptts_f0_candidates + ptts_f0_viterbi, on one utterance, and
prints the figures of DESIGN.md section 6 (median of --reps launches after 3 warm-up launches; the estimator's window table is built
before the first timed launch), beside the relative error of the estimated and of the refined track against the track the waveform
was made from.

Default sizes: T = 2000 frames of 5 ms at fs = 16 000 (dftlen 2048) and at fs = 32 000 (dftlen 4096), searched in 70 .. 600 Hz.  The
waveform is a frequency-modulated harmonic sum, f(t) = 170 + 60 sin(2 pi 1.5 t), harmonics up to 0.45 fs at 240 Hz with amplitude
0.8^h and seeded random phases, plus white noise 40 dB below the first harmonic.

    python tools/f0_refine_probe.py [--frames 2000] [--f0min 70] [--f0max 600] [--ncand 8] [--reps 20]
"""
from __future__ import print_function

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005
SHAPES = ((16000.0, 2048), (32000.0, 4096))


def fm_signal(fs, T, seed=0):
    N = int(np.floor((T - 1) * SHIFT * fs + 0.5)) + 1
    f = 170.0 + 60.0 * np.sin(2 * np.pi * 1.5 * np.arange(N) / fs)
    phase = 2 * np.pi * np.cumsum(f) / fs
    rng = np.random.RandomState(seed)
    nh = int(0.45 * fs / 240.0)
    phi = rng.uniform(0, 2 * np.pi, size=nh)
    wav = 0.1 * sum(0.8 ** h * np.cos(h * phase + phi[h - 1]) for h in range(1, nh + 1)) + 0.0008 * rng.randn(N)
    exact = f[np.floor(np.arange(T) * SHIFT * fs + 0.5).astype(np.int64)]
    return wav.astype(np.float32), exact


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--f0min', type=float, default=70.0)
    ap.add_argument('--f0max', type=float, default=600.0)
    ap.add_argument('--ncand', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'f0_refine_probe needs the GPU'
    T = args.frames
    for fs, L in SHAPES:
        wav_h, exact = fm_signal(fs, T)
        wav = torch.from_numpy(wav_h).cuda()
        assert ops.f0_frame_count(wav.numel(), SHIFT, fs) == T
        hw, lmin, lmax = ops.f0_check(L, fs, SHIFT, args.f0min, args.f0max)
        w64 = wav.to(torch.float64)
        gpeak = float((w64 - w64.mean()).abs().max().item())
        per_launch = {}
        for rep in range(3 + args.reps):
            with _hip.KernelTimer() as kt:
                freq, strength, n, lag = ops.f0_candidates(wav, T, SHIFT, fs, L, args.f0min, args.f0max, gpeak, ncand=args.ncand)
                est = ops.f0_viterbi(freq, strength, n, SHIFT)
                refined, status = ops.f0_refine(wav, est, SHIFT, fs, args.f0min, args.f0max, want_status=True)
            if rep >= 3:
                for name, _, ms in kt.durations_ms():
                    per_launch.setdefault(name, []).append(ms * 1e-3)
        res = {'frames': T, 'fs': fs, 'dftlen': L, 'f0_min': args.f0min, 'f0_max': args.f0max, 'ncand': args.ncand,
               'estimator_window': 2 * hw + 1, 'refine_window_at_170Hz': 2 * int(np.floor(1.5 * fs / 170.0 + 0.5)) + 1,
               'seconds_of_speech': wav.numel() / fs, 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
        for name, ts in per_launch.items():
            res[name] = {'s': float(np.median(ts)), 'min_s': float(np.min(ts)), 'max_s': float(np.max(ts)), 'frames_per_s': T / float(np.median(ts))}
        res['estimator_s'] = res['ptts_f0_candidates']['s'] + res['ptts_f0_viterbi']['s']
        res['refine_over_estimator'] = res['ptts_f0_refine']['s'] / res['estimator_s']
        est = est.cpu().numpy()
        sel = (status == 1) & (np.arange(T) >= 4) & (np.arange(T) < T - 4)
        res['frames_refined'] = int((status == 1).sum())
        res['status_counts'] = np.bincount(status, minlength=4).tolist()
        res['relative_error_estimated'] = float(np.abs(est[sel].astype(np.float64) / exact[sel] - 1.0).mean())
        res['relative_error_refined'] = float(np.abs(refined[sel].astype(np.float64) / exact[sel] - 1.0).mean())
        print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
