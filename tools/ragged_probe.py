#!/usr/bin/env python
"""Times generation with the network run utterance by utterance beside the ragged batch (ModelTTS.predict_device_batch,
generate_params(predict_batched=True)) and prints the figures of DESIGN.md section 6, "Ragged inference".

The model is the BASELINE architecture (DCNNF0SpecNoiseFeatures, H = 256, ctx 601, one context Conv1D of 21, 8 x Conv2D(4, 5x5),
VocoderPML 65 + 20) with its initial weights; the corpus is --utts synthetic utterances of 400 to 700 frames (seeded).  For each
batch_size of --sizes, --reps repetitions after 3 warm-ups, the two sides alternating in this process:

(a) the prediction loop alone between HIP events: predict_device per utterance (the path as it was before the batched one existed)
    beside predict_device_batch per group of batch_size;
(b) generate_params(do_objmeas=False, no specdir, no wavdir) as wall time around a device synchronise, both ways;
(c) in a pass of its own under KernelTimer (its events slow the host: not the pass the times above come from), the share of the
    BLSTM recurrence (ptts_lstm_fwd / ptts_lstm_fwd_ragged) in the summed kernel time of the prediction.

    python tools/ragged_probe.py [--utts 8] [--sizes 1,4,8] [--reps 10]
"""
from __future__ import print_function

import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX, SPEC, NM = 601, 65, 20


def spread(ts):
    return {'median_s': float(np.median(ts)), 'p10_s': float(np.percentile(ts, 10)), 'p90_s': float(np.percentile(ts, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=8)
    ap.add_argument('--sizes', default='1,4,8')
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()

    import torch
    import percivaltts_amd
    from percivaltts_amd import _hip, modeltts_common, vocoders
    assert torch.cuda.is_available(), 'ragged_probe needs the GPU'
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 256; cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 21
    cfg.arch_gen_nbcnnlayers = 8; cfg.arch_gen_nbfilters = 4; cfg.arch_gen_winlen = 5; cfg.arch_spec_freqlen = 5
    voc = vocoders.VocoderPML(16000, 0.005, SPEC, NM)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        mod = modeltts_common.DCNNF0SpecNoiseFeatures(CTX, voc, cfg)
    nout = voc.featuressize()
    rng = np.random.RandomState(0)
    lens = [int(n) for n in rng.randint(400, 701, size=args.utts)]
    xs = [(rng.rand(n, CTX) * 2 - 1).astype(np.float32) for n in lens]
    res = {'utterances': args.utts, 'lengths': lens, 'frames': int(sum(lens)), 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'sizes': {}}

    tmp = tempfile.mkdtemp(prefix='ragged_probe_')
    os.makedirs(os.path.join(tmp, 'lab')); os.makedirs(os.path.join(tmp, 'cmp'))
    fids = ['utt_{:02d}'.format(i) for i in range(args.utts)]
    for fid, x in zip(fids, xs):
        x.tofile(os.path.join(tmp, 'lab', fid + '.lab'))
    np.zeros(nout, dtype=np.float32).tofile(os.path.join(tmp, 'cmp', 'mean4norm.dat'))
    np.ones(nout, dtype=np.float32).tofile(os.path.join(tmp, 'cmp', 'std4norm.dat'))
    inpath = os.path.join(tmp, 'lab') + '/*.lab:(-1,{})'.format(CTX)
    outpath = os.path.join(tmp, 'cmp') + '/*.cmp:(-1,{})'.format(nout)

    def groups(bs):
        return [list(range(v0, min(v0 + bs, args.utts))) for v0 in range(0, args.utts, bs)]

    def predict_one(bs):
        return [mod.predict_device(xs[i][None])[0] for g in groups(bs) for i in g]

    def predict_bat(bs):
        return [y for g in groups(bs) for y in mod.predict_device_batch([xs[i] for i in g])]

    def events(fn, bs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn(bs)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e-3, out

    def wall(batched, bs, sub):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            mod.generate_params(inpath, outpath, fids, os.path.join(tmp, sub), do_objmeas=False, batch_size=bs,
                                predict_batched=batched)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for bs in [int(v) for v in args.sizes.split(',')]:
        one, bat, gone, gbat = [], [], [], []
        for rep in range(3 + args.reps):
            t_one, y_one = events(predict_one, bs)
            t_bat, y_bat = events(predict_bat, bs)
            w_one, w_bat = wall(False, bs, 'one'), wall(True, bs, 'bat')
            if rep >= 3:
                one.append(t_one); bat.append(t_bat); gone.append(w_one); gbat.append(w_bat)
        worst = max(float((a - b).abs().max()) for a, b in zip(y_one, y_bat))
        out = {'predict_one_by_one': spread(one), 'predict_batched': spread(bat),
               'generate_params_one_by_one': spread(gone), 'generate_params_batched': spread(gbat),
               'worst_abs_difference_of_the_outputs': worst}
        out['utterances_per_s_one_by_one'] = args.utts / out['predict_one_by_one']['median_s']
        out['utterances_per_s_batched'] = args.utts / out['predict_batched']['median_s']
        out['one_by_one_median_over_batched_median'] = out['predict_one_by_one']['median_s'] / out['predict_batched']['median_s']
        out['batched_p90_below_one_by_one_p10'] = out['predict_batched']['p90_s'] < out['predict_one_by_one']['p10_s']
        # (c) kernel time by entry point, a pass of its own
        for key, fn in (('one_by_one', predict_one), ('batched', predict_bat)):
            with _hip.KernelTimer() as kt:
                fn(bs)
            torch.cuda.synchronize()
            tot, rec = 0.0, 0.0
            for name, _, ms in kt.durations_ms():
                tot += ms
                if name in ('ptts_lstm_fwd', 'ptts_lstm_fwd_ragged'):
                    rec += ms
            out['kernel_time_' + key] = {'all_entry_points_ms': tot, 'blstm_recurrence_ms': rec, 'blstm_share': rec / tot if tot else None}
        res['sizes'][str(bs)] = out
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
