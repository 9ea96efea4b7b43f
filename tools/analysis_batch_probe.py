#!/usr/bin/env python
"""Times the waveform analysis over a batch of utterances and prints the figures of DESIGN.md section 6, "Waveform analysis,
utterances in batches"; median and p10 / p90 of --reps repetitions after 3 warm-ups, both sides in this process on the same box:

(a) the wall time (a device synchronise on both sides) of a loop of analysis_device calls, one per utterance, beside one
    analysis_device_batch call over the same utterances, for both vocoders, with the tracks given and with f0s=None;
    analysis_device is the per-utterance path as it was before the batched one existed;
(b) the HIP-event time of ptts_f0_viterbi_batch over the batch beside ptts_f0_viterbi over one of its utterances;
(c) the HIP-event time of each batched frame kernel beside the sum of the launches of its single form, one per utterance.

Default size: 8 utterances of T = 1000 frames of 5 ms, fs = 32 000, dftlen = 4096, 129 spectral and 33 noise bands, synthesised as
in tools/analysis_probe.py (ops.pulse_synthesis on a smooth envelope with the noise mask set above fs / 5), each with its own f0
contour around 170 + 60 sin(i / 7) Hz.

    python tools/analysis_batch_probe.py [--utts 8] [--frames 1000] [--fs 32000] [--dftlen 4096] [--spec 129] [--nm 33] [--reps 20]
"""
from __future__ import print_function

import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIFT = 0.005
F0_MIN, F0_MAX = 100.0, 400.0


def spread(ts):
    return {'median_s': float(np.median(ts)), 'p10_s': float(np.percentile(ts, 10)), 'p90_s': float(np.percentile(ts, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--spec', type=int, default=129)
    ap.add_argument('--nm', type=int, default=33)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops, vocoders
    assert torch.cuda.is_available(), 'analysis_batch_probe needs the GPU'
    B, T, fs, L = args.utts, args.frames, args.fs, args.dftlen
    K = L // 2 + 1
    wavlen = int(round(SHIFT * (T - 1) * fs))
    rng = np.random.RandomState(0)
    mask = torch.from_numpy(np.tile((np.arange(K) * fs / L >= fs / 5.0).astype(np.float32), (T, 1))).cuda()
    x = np.linspace(0, 1, T)[:, None]
    wavs, f0s = [], []
    for b in range(B):
        f0 = (170.0 + rng.uniform(-20, 20) + 60.0 * np.sin(np.arange(T) / 7.0 + rng.uniform(0, 6.28))).astype(np.float32)
        fw = rng.uniform(-6.0, -3.0) + np.cumsum(rng.randn(2, 65) * 0.3, axis=1)
        fw = ((1 - x) * fw[0] + x * fw[1]).astype(np.float32)
        spec = ops.fwbnd2spec(torch.from_numpy(fw).cuda(), fs, dftlen=L)
        tab = ops.pulse_table(f0, SHIFT, fs, wavlen, L)
        g = torch.from_numpy(rng.randn(wavlen).astype(np.float32)).cuda()
        wavs.append(ops.pulse_synthesis(spec, mask, tab, g, fs, L, wavlen).cpu().numpy())
        f0[rng.randint(100, T - 100):][:20] = 0.0               # an unvoiced stretch of 0.1 s
        f0s.append(f0)
    res = {'utterances': B, 'frames': T, 'fs': fs, 'dftlen': L, 'spec_bands': args.spec, 'nm_bands': args.nm, 'reps': args.reps,
           'seconds_of_speech': B * wavlen / fs, 'device': torch.cuda.get_device_name(0)}

    # (a) the per-utterance loop beside the batch
    quiet = io.StringIO()
    for key in ('pml', 'world'):
        voc = (vocoders.VocoderPML(fs, SHIFT, args.spec, args.nm, dftlen=L) if key == 'pml'
               else vocoders.VocoderWORLDAnalysisDevice(fs, SHIFT, args.spec, args.nm, dftlen=L))
        for how, tracks in (('tracks_given', f0s), ('tracks_estimated', None)):
            loop, batch = [], []
            for rep in range(3 + args.reps):
                with contextlib.redirect_stdout(quiet):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    want = [voc.analysis_device(w, None if tracks is None else tracks[b], F0_MIN, F0_MAX) for b, w in enumerate(wavs)]
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    got = voc.analysis_device_batch(wavs, tracks, F0_MIN, F0_MAX)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                if rep >= 3:
                    loop.append(t1 - t0)
                    batch.append(t2 - t1)
            out = {'analysis_device_loop': spread(loop), 'analysis_device_batch': spread(batch),
                   'same_bytes': all(np.array_equal(g, w) for g, w in zip(got, want))}
            out['loop_median_over_batch_median'] = out['analysis_device_loop']['median_s'] / out['analysis_device_batch']['median_s']
            out['batch_p90_below_loop_p10'] = out['analysis_device_batch']['p90_s'] < out['analysis_device_loop']['p10_s']
            res[key + '_' + how] = out

    # (b), (c) the kernels: the batched launch beside the launches of the single form
    dev = torch.device('cuda')
    wav = torch.from_numpy(np.concatenate(wavs)).to(dev)
    wl = ops.packed_offsets([len(w) for w in wavs], dev)
    est, fo = ops.f0_estimate_batch(wav, wl, SHIFT, fs, L, F0_MIN, F0_MAX)
    track, vuv, oo = ops.f0_track_device(est, fo, wl, F0_MIN, F0_MAX, fs, SHIFT, L)
    rate = torch.where(vuv > 0, track, torch.full_like(track, ops.WORLD_UNVOICED_RATE))
    hcap = ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    ws, ts_, vs, rs = wav.split(wl.lengths), track.split(oo.lengths), vuv.split(oo.lengths), rate.split(oo.lengths)
    ws, ts_, vs, rs = [[t.contiguous() for t in xs] for xs in (ws, ts_, vs, rs)]
    gpeak = ops.wave_peak(wav, wl)
    gp = [float(v) for v in gpeak.cpu().numpy()]
    batched, single = {}, {}
    for rep in range(3 + args.reps):
        with _hip.KernelTimer() as kt:
            freq, strength, n, _ = ops.f0_candidates_batch(wav, wl, fo, SHIFT, fs, L, F0_MIN, F0_MAX, gpeak)
            ops.f0_viterbi_batch(freq, strength, n, fo, SHIFT)
            ops.f0_refine_batch(wav, wl, est, fo, SHIFT, fs, F0_MIN, F0_MAX)
            ops.f0_track_device(est, fo, wl, F0_MIN, F0_MAX, fs, SHIFT, L)
            ops.wave_peak(wav, wl)
            _, u = ops.frame_harmonics_batch(wav, wl, track, oo, SHIFT, fs, L, hcap, log=True)
            ops.phase_coherence_batch(u, track, oo, SHIFT, fs, L, args.nm)
            ops.world_envelope_batch(wav, wl, rate, oo, SHIFT, fs, L, log=True)
            ops.world_aperiodicity_batch(wav, wl, track, vuv, oo, SHIFT, fs, L, args.nm)
        if rep >= 3:
            for name, _, ms in kt.durations_ms():
                batched.setdefault(name, []).append(ms * 1e-3)
        with _hip.KernelTimer() as kt:
            for b in range(B):
                c = ops.f0_candidates(ws[b], fo.lengths[b], SHIFT, fs, L, F0_MIN, F0_MAX, gp[b])
                ops.f0_viterbi(c[0], c[1], c[2], SHIFT)
                ops.f0_refine(ws[b], est[fo.off[b]:fo.off[b + 1]], SHIFT, fs, F0_MIN, F0_MAX)
                _, ub = ops.frame_harmonics(ws[b], ts_[b], SHIFT, fs, L, hcap, log=True)
                ops.phase_coherence(ub, ts_[b], SHIFT, fs, L, args.nm)
                ops.world_envelope(ws[b], rs[b], SHIFT, fs, L, log=True)
                ops.world_aperiodicity(ws[b], ts_[b], vs[b], SHIFT, fs, L, args.nm)
        if rep >= 3:
            sums = {}
            for name, _, ms in kt.durations_ms():
                sums.setdefault(name, []).append(ms * 1e-3)
            for name, v in sums.items():
                single.setdefault(name, []).append(v)
    kernels = {}
    for name, ts in sorted(batched.items()):
        kernels[name] = {'batch': spread(ts)}
        one = name[:-len('_batch')] if name.endswith('_batch') else None
        if one in single:
            per_rep = np.array(single[one])                     # [reps, B]
            kernels[name]['single_launches_summed'] = spread(per_rep.sum(axis=1))
            kernels[name]['single_launch_of_one_utterance'] = spread(per_rep[:, 0])
            kernels[name]['batch_over_summed'] = kernels[name]['batch']['median_s'] / kernels[name]['single_launches_summed']['median_s']
            kernels[name]['batch_over_one_utterance'] = (kernels[name]['batch']['median_s'] /
                                                         kernels[name]['single_launch_of_one_utterance']['median_s'])
    res['kernels'] = kernels
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
