#!/usr/bin/env python
"""Times the two launches of csrc/worldanalysis.hip with HIP events for one utterance and prints the figures of DESIGN.md section 6:
ptts_world_envelope and ptts_world_aperiodicity (median of --reps launches after 3 warm-up launches; the band table is built before
the first timed launch), beside ptts_frame_harmonics of csrc/analysis.hip on the same waveform in the same run as the yardstick
(one transform a frame against three and two), and how well the parameters the waveform was synthesised from come back.

Default size: T = 1000 frames of 5 ms, fs = 32 000 (a waveform of 159 840 samples), dftlen = 4096, 5 aperiodicity bands,
f0 = 170 + 30 sin(i / 40) Hz, every tenth stretch of ten frames unvoiced; the waveform comes from ops.world_synthesis on a smooth
envelope with the bands at -30 / -24 / -14 / -8 / -3 dB.

    python tools/worldanalysis_probe.py [--frames 1000] [--fs 32000] [--dftlen 4096] [--aper 5] [--reps 20]
"""
from __future__ import print_function

import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005
F0_MIN, F0_MAX = 100.0, 400.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--aper', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'worldanalysis_probe needs the GPU'
    T, fs, L, nb = args.frames, args.fs, args.dftlen, args.aper
    K = L // 2 + 1
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    f0 = (170.0 + 30.0 * np.sin(np.arange(T) / 40.0)).astype(np.float32)
    voiced = (np.arange(T) // 10) % 10 != 9
    fw = (rng.uniform(-6.0, -3.0) + np.cumsum(rng.randn(2, 65) * 0.3, axis=1))
    x = np.linspace(0, 1, T)[:, None]
    fw = ((1 - x) * fw[0] + x * fw[1]).astype(np.float32)                   # a slow morph between two smooth envelopes
    spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
    bands = np.linspace(-30.0, -3.0, nb) if nb != 5 else np.array([-30.0, -24.0, -14.0, -8.0, -3.0])
    aper_db = torch.from_numpy(np.tile(bands.astype(np.float32), (T, 1))).cuda()
    vuv = torch.from_numpy(voiced.astype(np.float32)).cuda()
    tab = ops.world_pulse_table(f0, voiced, SHIFT, fs, wavlen, L)
    wav = ops.world_synthesis(spec, ops.aper_rows(aper_db, vuv, fs, L), tab, torch.from_numpy(rng.randn(wavlen).astype(np.float32)).cuda(),
                              fs, L, wavlen)
    ops.world_analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    hcap = ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    f0_d = torch.from_numpy(f0).cuda()
    rate_d = torch.from_numpy(np.where(voiced, f0, np.float32(ops.WORLD_UNVOICED_RATE)).astype(np.float32)).cuda()

    per_launch = {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kt:
            lspec = ops.world_envelope(wav, rate_d, SHIFT, fs, L, log=True)
            aper = ops.world_aperiodicity(wav, f0_d, vuv, SHIFT, fs, L, nb)
            ops.frame_harmonics(wav, f0_d, SHIFT, fs, L, hcap, log=True)
        if rep >= 3:
            for name, _, ms in kt.durations_ms():
                per_launch.setdefault(name, []).append(ms * 1e-3)
    res = {'frames': T, 'voiced_frames': int(voiced.sum()), 'fs': fs, 'dftlen': L, 'aper_bands': nb, 'wavlen': wavlen,
           'seconds_of_speech': wavlen / fs, 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    for name, ts in per_launch.items():
        res[name] = {'s': float(np.median(ts)), 'frames_per_s': T / float(np.median(ts))}
    yard = res['ptts_frame_harmonics']['s']
    for name in ('ptts_world_envelope', 'ptts_world_aperiodicity'):
        res[name]['times_frame_harmonics'] = res[name]['s'] / yard

    # what went in against what came out: interior voiced frames, the envelope at and above f0
    got, want = lspec.cpu().numpy().astype(np.float64), np.log(spec.cpu().numpy().astype(np.float64))
    f = np.arange(K) * fs / L
    inner = [i for i in range(20, T - 20) if voiced[i - 2:i + 3].all()]
    err = np.concatenate([(20.0 / math.log(10.0)) * (got[i] - want[i])[f >= f0[i]] for i in inner])
    res['envelope_rms_db'], res['envelope_mean_db'] = float(np.sqrt(np.mean(err ** 2))), float(err.mean())
    a = aper.cpu().numpy()
    res['aper_band_medians_db'] = [float(v) for v in np.median(a[inner], axis=0)]
    res['aper_bands_in_db'] = [float(v) for v in bands]
    res['unvoiced_rows_zero'] = bool((a[~voiced] == 0).all())
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
