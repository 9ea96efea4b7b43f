#!/usr/bin/env python
"""Times the launches of csrc/worldsynth.hip with HIP events for one utterance and, in the same run on the same box, the PML
synthesiser's launches (csrc/pulsesynth.hip) for that utterance, and prints the figures of DESIGN.md section 6: ptts_aper_rows,
ptts_world_segments and its ptts_pulse_overlap_add beside ptts_noise_mask, ptts_pulse_segments and its overlap-add (median of
--reps launches after 3 warm-up launches), the wall time of the WORLD definition restated with numpy's FFTs in fp64 on the host,
and the largest difference between that waveform and the device's.

Default size: T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, 25 bands, f0 = 170 + 60 sin(i / 7) Hz, voiced and unvoiced
stretches of --stretch frames in turn (half the frames voiced).  The PML synthesiser has no voicing decision: it lays its pulses at
f0 throughout.

    python tools/worldsynth_probe.py [--frames 1000] [--fs 32000] [--dftlen 4096] [--nb 25] [--stretch 50] [--reps 20]
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


def minphase(la, L):
    c = np.fft.irfft(la, L)
    c[1:L // 2] *= 2
    c[L // 2 + 1:] = 0
    return np.exp(np.fft.rfft(c))


def host_synthesis(spec, aper, g, tab, fs, L, wavlen):
    """The definition of DESIGN.md section 3 in numpy fp64, one pulse after the other."""
    K = L // 2 + 1
    k = np.arange(K)
    d = int(math.floor(0.001 * fs + 0.5))
    hann = np.hanning(2 * d + 1)[:d + 1]
    wav = np.zeros(wavlen)
    spec, aper, g = spec.astype(np.float64), aper.astype(np.float64), g.astype(np.float64)
    tank = np.tan(np.pi * k[1:] / L)
    for n in range(len(tab['start'])):
        start, winlen, lb, rb, i0, i1, v = (int(tab[key][n]) for key in ('start', 'winlen', 'lb', 'rb', 'i0', 'i1', 'v'))
        w = tab['w'][n]
        s = (1 - w) * spec[i0] + w * spec[i1]
        a = (1 - w) * aper[i0] + w * aper[i1]
        x = np.zeros(L)
        if rb > lb:
            q = g[lb:rb].copy()
            if rb - lb >= 2 * (d + 1):
                q[:d + 1] *= hann
                q[rb - lb - d - 1:] *= hann[::-1]
            x[lb - start:rb - start] = q
        N = np.fft.rfft(x)
        p = np.abs(N) ** 2
        e = (p[0] + p[-1] + 2 * p[1:-1].sum()) / L
        if e > 0: N = N / np.sqrt(e)
        S = minphase(np.log(np.maximum(s * a, 1e-10)), L) * N
        if v:
            hp = np.zeros(K)
            hp[1:] = (1.0 + (np.tan(np.pi * 0.5 * tab['f0'][n] / fs) / tank) ** 8) ** -0.5
            S = S + minphase(np.log(np.maximum(s * np.sqrt(1 - a * a) * hp, 1e-10)), L) * np.exp(-2j * np.pi * tab['delay'][n] * k / L)
        S[0], S[-1] = S[0].real, S[-1].real
        seg = np.fft.irfft(S, L)[:winlen]
        a0, b0 = max(start, 0), min(start + winlen, wavlen)
        if b0 > a0: wav[a0:b0] += seg[a0 - start:b0 - start]
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--nb', type=int, default=25)
    ap.add_argument('--stretch', type=int, default=50)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'worldsynth_probe needs the GPU'
    T, fs, L, nb = args.frames, args.fs, args.dftlen, args.nb
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    voiced = (np.arange(T) // args.stretch) % 2 == 0
    fw = (rng.uniform(-6.0, -3.0, size=(T, 1)) + np.cumsum(rng.randn(T, 65) * 0.3, axis=1)).astype(np.float32)
    aper_db = np.clip(np.linspace(-30.0, 0.0, nb)[None, :] + rng.randn(T, nb) * 4.0, -60.0, 3.0).astype(np.float32)
    nmb = np.clip(np.linspace(0.0, 1.0, nb)[None, :] + rng.randn(T, nb) * 0.2, 0, 1).astype(np.float32)
    g = rng.randn(wavlen).astype(np.float32)
    spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
    db_d, nmb_d, f0_d, g_d = (torch.from_numpy(x).cuda() for x in (aper_db, nmb, f0, g))
    vuv_d = torch.from_numpy(voiced.astype(np.float32)).cuda()
    wtab = ops.world_pulse_table(f0, voiced, SHIFT, fs, wavlen, L)
    ptab = ops.pulse_table(f0, SHIFT, fs, wavlen, L)

    world, pml = {}, {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kw:
            aper = ops.aper_rows(db_d, vuv_d, fs, L)
            wav = ops.world_synthesis(spec, aper, wtab, g_d, fs, L, wavlen)
        with _hip.KernelTimer() as kp:
            mask = ops.noise_mask(nmb_d, f0_d, fs, L)
            ops.pulse_synthesis(spec, mask, ptab, g_d, fs, L, wavlen)
        if rep >= 3:
            for into, kt in ((world, kw), (pml, kp)):
                for name, _, ms in kt.durations_ms():
                    into.setdefault(name, []).append(ms * 1e-3)
    Pw, Pp = len(wtab['start']), len(ptab['start'])
    res = {'frames': T, 'fs': fs, 'dftlen': L, 'nb': nb, 'stretch': args.stretch, 'wavlen': wavlen, 'seconds_of_speech': wavlen / fs,
           'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'world': {'pulses': Pw, 'voiced_pulses': int(wtab['v'].sum()), 'unvoiced_pulses': int(Pw - wtab['v'].sum())},
           'pml': {'pulses': Pp}}
    for key, per_launch in (('world', world), ('pml', pml)):
        for name, ts in per_launch.items():
            res[key][name] = {'s': float(np.median(ts))}
        res[key]['device_total_s'] = sum(float(np.median(ts)) for ts in per_launch.values())
    ws, ps = res['world']['ptts_world_segments'], res['pml']['ptts_pulse_segments']
    ws['pulses_per_s'], ps['pulses_per_s'] = Pw / ws['s'], Pp / ps['s']
    res['world_segments_over_pulse_segments'] = ws['s'] / ps['s']

    t0 = time.time()
    want = host_synthesis(spec.cpu().numpy(), aper.cpu().numpy(), g, wtab, fs, L, wavlen)
    th = time.time() - t0
    res['host_fp64'] = {'s': th, 'pulses_per_s': Pw / th, 'threads': int(os.environ.get('OMP_NUM_THREADS', '16'))}
    res['max_abs_difference'] = float(np.abs(wav.cpu().numpy().astype(np.float64) - want).max())
    res['max_abs_wav'] = float(np.abs(want).max())
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
