#!/usr/bin/env python
"""Times the three launches of csrc/analysis.hip with HIP events for one utterance and prints the figures of DESIGN.md section 6:
ptts_frame_harmonics, ptts_phase_coherence and ptts_fwbnd_compress (median of --reps launches after 3 warm-up launches; the two band
tables are built before the first timed launch), beside the wall time of the frame spectra alone with numpy's FFTs in fp64 on the
host, and the envelope's rms error in dB against the one the waveform was synthesised from.

Default size: T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, 129 spectral and 33 noise-mask bands, f0 = 170 + 60 sin(i / 7) Hz;
the waveform comes from ops.pulse_synthesis on a smooth envelope with the noise mask set above fs / 5.

    python tools/analysis_probe.py [--frames 1000] [--fs 32000] [--dftlen 4096] [--spec 129] [--nm 33] [--reps 20]
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
F0_MIN, F0_MAX = 100.0, 400.0


def host_frame_spectra(wav, f0, fs, L):
    """The windowed, zero-phase frame spectra of DESIGN.md section 3 in numpy fp64, one frame after the other."""
    N = len(wav)
    out = np.zeros((len(f0), L // 2 + 1))
    for i in range(len(f0)):
        c, hw = int(math.floor(i * SHIFT * fs + 0.5)), int(1.5 * fs / float(f0[i]))
        w = np.blackman(2 * hw + 1)
        w /= w.sum()
        x = np.zeros(L)
        lo, hi = max(c - hw, 0), min(c + hw + 1, N)
        if hi > lo:
            seg = wav[lo:hi] * w[lo - c + hw:hi - c + hw]
            x[(np.arange(lo, hi) - c) % L] = seg
        out[i] = np.abs(np.fft.rfft(x))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--spec', type=int, default=129)
    ap.add_argument('--nm', type=int, default=33)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'analysis_probe needs the GPU'
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
    hcap = ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    f0_d = torch.from_numpy(ops.f0_track(f0, F0_MIN, F0_MAX, fs, SHIFT, L, wavlen=wavlen)).cuda()

    per_launch = {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kt:
            lspec, u = ops.frame_harmonics(wav, f0_d, SHIFT, fs, L, hcap, log=True)
            R, nm = ops.phase_coherence(u, f0_d, SHIFT, fs, L, args.nm)
            bands = ops.fwbnd_compress(lspec, fs, args.spec, mode='lsq', log=True)
        if rep >= 3:
            for name, _, ms in kt.durations_ms():
                per_launch.setdefault(name, []).append(ms * 1e-3)
    res = {'frames': T, 'fs': fs, 'dftlen': L, 'spec_bands': args.spec, 'nm_bands': args.nm, 'hcap': hcap, 'wavlen': wavlen,
           'seconds_of_speech': wavlen / fs, 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    for name, ts in per_launch.items():
        res[name] = {'s': float(np.median(ts))}
    res['ptts_frame_harmonics']['frames_per_s'] = T / res['ptts_frame_harmonics']['s']
    res['device_total_s'] = sum(res[name]['s'] for name in per_launch)

    t0 = time.time()
    host_frame_spectra(wav.cpu().numpy().astype(np.float64), f0, fs, L)
    th = time.time() - t0
    res['host_fp64_frame_spectra'] = {'s': th, 'frames_per_s': T / th, 'threads': int(os.environ.get('OMP_NUM_THREADS', '16'))}

    # the envelope against the one the waveform was made from: interior frames, bins of [f0, fs/5 - f0)
    got, want = lspec.cpu().numpy().astype(np.float64), np.log(spec.cpu().numpy().astype(np.float64))
    f = np.arange(K) * fs / L
    err = [(20.0 / math.log(10.0)) * (got[i] - want[i])[(f >= f0[i]) & (f < fs / 5.0 - f0[i])] for i in range(4, T - 4)]
    res['envelope_rms_db'] = float(np.sqrt(np.mean(np.concatenate(err) ** 2)))
    nmv = nm.cpu().numpy()[4:T - 4]
    res['nm_first_band_mean'], res['nm_last_band_mean'] = float(nmv[:, 0].mean()), float(nmv[:, -1].mean())
    res['bands_finite'] = bool(np.isfinite(bands.cpu().numpy()).all())
    res['R_min'] = float(R.min())
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
