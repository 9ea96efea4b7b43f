#!/usr/bin/env python
"""Times the three launches of csrc/pulsesynth.hip with HIP events for one utterance and prints the figures of DESIGN.md
section 6: ptts_noise_mask, ptts_pulse_segments and ptts_pulse_overlap_add (median of --reps launches after 3 warm-up launches),
beside the wall time of the same synthesis restated with numpy's FFTs in fp64 on the host (on the threads the environment
allows), and the largest difference between the two waveforms.

Default size: T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, nb = 25 noise-mask bands, f0 = 170 + 60 sin(i / 7) Hz.

    python tools/pulsesynth_probe.py [--frames 1000] [--fs 32000] [--dftlen 4096] [--nb 25] [--reps 20]
"""
from __future__ import print_function

import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005


def host_synthesis(spec, mask, g, tab, fs, L, wavlen):
    """The definition of DESIGN.md section 3 in numpy fp64, one pulse after the other."""
    K = L // 2 + 1
    k = np.arange(K)
    d = int(math.floor(0.001 * fs + 0.5))
    hann = np.hanning(2 * d + 1)[:d + 1]
    wav = np.zeros(wavlen)
    spec, mask, g = spec.astype(np.float64), mask.astype(np.float64), g.astype(np.float64)
    tank = np.tan(np.pi * k[1:] / L)
    for n in range(len(tab['start'])):
        start, winlen, lb, rb, fr = (int(tab[key][n]) for key in ('start', 'winlen', 'lb', 'rb', 'fr'))
        hp = np.zeros(K)
        hp[1:] = (1.0 + (np.tan(np.pi * 0.5 * tab['f0'][n] / fs) / tank) ** 8) ** -0.5
        c = np.fft.irfft(np.log(np.maximum(spec[fr] * hp, 1e-10)), L)
        c[1:L // 2] *= 2
        c[L // 2 + 1:] = 0
        E = np.exp(np.fft.rfft(c))
        D = np.exp(-2j * np.pi * tab['delay'][n] * k / L)
        x = np.zeros(L)
        if rb > lb:
            s = g[lb:rb].copy()
            if rb - lb >= 2 * (d + 1):
                s[:d + 1] *= hann
                s[rb - lb - d - 1:] *= hann[::-1]
            x[lb - start:rb - start] = s
        N = np.fft.rfft(x)
        p = np.abs(N) ** 2
        e = (p[0] + p[-1] + 2 * p[1:-1].sum()) / L
        if e > 0: N = N / np.sqrt(e)
        S = E * ((1 - mask[fr]) * D + mask[fr] * N)
        S[0], S[-1] = S[0].real, S[-1].real
        seg = np.fft.irfft(S, L)[:winlen]
        a, b = max(start, 0), min(start + winlen, wavlen)
        if b > a: wav[a:b] += seg[a - start:b - start]
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--nb', type=int, default=25)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'pulsesynth_probe needs the GPU'
    T, fs, L, nb = args.frames, args.fs, args.dftlen, args.nb
    K = L // 2 + 1
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    fw = (rng.uniform(-6.0, -3.0, size=(T, 1)) + np.cumsum(rng.randn(T, 65) * 0.3, axis=1)).astype(np.float32)
    nmb = np.clip(np.linspace(0.0, 1.0, nb)[None, :] + rng.randn(T, nb) * 0.2, 0, 1).astype(np.float32)
    g = rng.randn(wavlen).astype(np.float32)
    spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
    nmb_d, f0_d, g_d = torch.from_numpy(nmb).cuda(), torch.from_numpy(f0).cuda(), torch.from_numpy(g).cuda()
    tab = ops.pulse_table(f0, SHIFT, fs, wavlen, L)
    P = len(tab['start'])

    per_launch = {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kt:
            mask = ops.noise_mask(nmb_d, f0_d, fs, L)
            wav = ops.pulse_synthesis(spec, mask, tab, g_d, fs, L, wavlen)
        if rep >= 3:
            for name, _, ms in kt.durations_ms():
                per_launch.setdefault(name, []).append(ms * 1e-3)
    res = {'frames': T, 'fs': fs, 'dftlen': L, 'nb': nb, 'pulses': P, 'wavlen': wavlen, 'seconds_of_speech': wavlen / fs,
           'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    for name, ts in per_launch.items():
        res[name] = {'s': float(np.median(ts))}
    res['ptts_pulse_segments']['pulses_per_s'] = P / res['ptts_pulse_segments']['s']
    res['device_total_s'] = sum(res[name]['s'] for name in per_launch)

    t0 = time.time()
    want = host_synthesis(spec.cpu().numpy(), mask.cpu().numpy(), g, tab, fs, L, wavlen)
    th = time.time() - t0
    res['host_fp64'] = {'s': th, 'pulses_per_s': P / th, 'threads': int(os.environ.get('OMP_NUM_THREADS', '16'))}
    res['max_abs_difference'] = float(np.abs(wav.cpu().numpy().astype(np.float64) - want).max())
    res['max_abs_wav'] = float(np.abs(want).max())
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
