#!/usr/bin/env python
"""Times the two launches of csrc/preproc.hip with HIP events and prints the figures of DESIGN.md section 6: ptts_resample and
ptts_highpass_zerophase for one utterance and for a batch of --batch utterances in one launch (median of --reps launches after 3
warm-up launches; the resampler's table is built before the first timed launch), beside the host's scipy time for the same work
(scipy.signal.resample_poly with its own filter, then sosfiltfilt of the same sections) and the largest difference between the
device's high-pass and scipy's on the same input.

Default size: the waveform of tools/f0_probe.py (T = 1000 frames of 5 ms, f0 = 170 + 60 sin(i / 7) Hz, a smooth envelope with noise
above fs / 5) synthesised at 48 000 Hz, resampled to 32 000 Hz, then high-passed at 70 Hz.

    python tools/preproc_probe.py [--frames 1000] [--fs-in 48000] [--fs-out 32000] [--fc 70] [--batch 64] [--reps 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs-in', type=int, default=48000)
    ap.add_argument('--fs-out', type=int, default=32000)
    ap.add_argument('--fc', type=float, default=70.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from scipy import signal as sig
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'preproc_probe needs the GPU'
    T, fs, L = args.frames, float(args.fs_in), args.dftlen
    K = L // 2 + 1
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    fw = (rng.uniform(-6.0, -3.0) + np.cumsum(rng.randn(2, 65) * 0.3, axis=1))
    x = np.linspace(0, 1, T)[:, None]
    fw = ((1 - x) * fw[0] + x * fw[1]).astype(np.float32)
    spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
    mask = torch.from_numpy(np.tile((np.arange(K) * fs / L >= fs / 5.0).astype(np.float32), (T, 1))).cuda()
    tab = ops.pulse_table(f0, SHIFT, fs, wavlen, L)
    wav = ops.pulse_synthesis(spec, mask, tab, torch.from_numpy(rng.randn(wavlen).astype(np.float32)).cuda(), fs, L, wavlen)
    wav = wav + 0.05                                            # the offset the filter is there to remove

    up, down, hw = ops.preproc_check(args.fs_in, args.fs_out, args.fc)
    chunk, tile = ops.highpass_tile()
    res = {'frames': T, 'fs_in': args.fs_in, 'fs_out': args.fs_out, 'fc': args.fc, 'up': up, 'down': down, 'taps': 2 * hw,
           'chunk': chunk, 'tile': tile, 'samples_in': wavlen, 'seconds_of_speech': wavlen / fs, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}
    for label, n in (('one', 1), ('batch', args.batch)):
        wavs = wav if n == 1 else [wav] * n
        per_launch = {}
        for rep in range(3 + args.reps):
            with _hip.KernelTimer() as kt:
                low = ops.resample(wavs, args.fs_in, args.fs_out)
                out = ops.highpass_zerophase(low, args.fs_out, args.fc)
            if rep >= 3:
                for name, _, ms in kt.durations_ms():
                    per_launch.setdefault(name, []).append(ms * 1e-3)
        speech = n * wavlen / fs
        res[label] = {'utterances': n, 'seconds_of_speech': speech}
        for name, ts in per_launch.items():
            res[label][name] = {'s': float(np.median(ts)), 'times_real_time': speech / float(np.median(ts))}
    low1 = low[0] if isinstance(low, list) else low
    out1 = out[0] if isinstance(out, list) else out
    res['samples_out'] = low1.numel()

    host = wav.cpu().numpy().astype(np.float64)
    sos = sig.butter(4, args.fc / (args.fs_out / 2.0), 'high', output='sos')
    ts_r, ts_f = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        low_h = sig.resample_poly(host, up, down)
        t1 = time.perf_counter()
        sig.sosfiltfilt(sos, low_h, padtype='odd', padlen=ops.HIGHPASS_PADLEN)
        t2 = time.perf_counter()
        ts_r.append(t1 - t0)
        ts_f.append(t2 - t1)
    res['scipy_one'] = {'resample_poly_s': float(np.median(ts_r)), 'sosfiltfilt_s': float(np.median(ts_f))}
    want = sig.sosfiltfilt(sos, low1.cpu().numpy().astype(np.float64), padtype='odd', padlen=ops.HIGHPASS_PADLEN)
    res['highpass_against_sosfiltfilt'] = {'largest_difference': float(np.abs(out1.cpu().numpy() - want).max()),
                                           'peak': float(np.abs(want).max()), 'mean_in': float(low1.mean().item()),
                                           'mean_out': float(out1.mean().item())}
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
