#!/usr/bin/env python
"""Times OptimizerTTSWGAN.update_validation_cost one utterance at a time (cfg.train_validation_batch_size = None, the path as it
was before the batched one existed) beside the ragged batches (train_validation_batch_size = 1, 4, 8, with and without sorting by
length) and prints the figures of DESIGN.md section 6, "Batched validation".

The model is the BASELINE architecture (DCNNF0SpecNoiseFeatures, H = 256, ctx 601, one context Conv1D of 21, 8 x Conv2D(4, 5x5),
VocoderPML 65 + 20) and its critic with their initial weights under a WLSWGAN optimiser after prepare(); the validation set is
--utts synthetic utterances of 400 to 700 frames (seeded: the set of tools/ragged_probe.py).  One process, the sides alternating
in every repetition; --reps repetitions after 3 warm-ups; wall time of update_validation_cost around a device synchronise, median
(p10 - p90).  In a pass of its own under KernelTimer (its events slow the host: not the pass the times come from) the summed
kernel time is split into the BLSTM recurrence, the critic's penalty passes (everything between ptts_gp_interpolate and
ptts_gp_sqnorm: the three forwards and the backward-data pass), the cost kernels (row masks, means, least squares, penalty) and
the rest (the generator's other layers; one by one also the generator cost's own critic forward).

    python tools/validation_probe.py [--utts 8] [--sizes 1,4,8] [--reps 10]
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

CTX, SPEC, NM = 601, 65, 20
COST_KERNELS = ('ptts_affine_act_rows', 'ptts_affine_act_rows_bwd', 'ptts_rows_mean', 'ptts_wlse_rows', 'ptts_gp_penalty_rows',
                'ptts_gp_sqnorm', 'ptts_gp_penalty', 'ptts_gp_interpolate', 'ptts_mean_scaled', 'ptts_wlse_fwd')
COSTS = ('model_rmse_validation', 'model_validation', 'critic_training', 'critic_validation', 'critic_validation_ltm')


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
    from percivaltts_amd import _hip, data, modeltts_common, networks_critic, optimizertts_wgan, vocoders
    assert torch.cuda.is_available(), 'validation_probe needs the GPU'
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 256; cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 21
    cfg.arch_gen_nbcnnlayers = 8; cfg.arch_gen_nbfilters = 4; cfg.arch_gen_winlen = 5; cfg.arch_spec_freqlen = 5
    cfg.train_wgan_critic_LSWGANtransidx = 30.0
    voc = vocoders.VocoderPML(16000, 0.005, SPEC, NM)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        mod = modeltts_common.DCNNF0SpecNoiseFeatures(CTX, voc, cfg)
        crit = networks_critic.Critic(voc, CTX, cfg)
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
    nout = voc.featuressize()
    rng = np.random.RandomState(0)
    lens = [int(n) for n in rng.randint(400, 701, size=args.utts)]
    Xv = [(rng.rand(n, CTX) * 2 - 1).astype(np.float32) for n in lens]
    Yv = [rng.randn(n, nout).astype(np.float32) for n in lens]
    opt.validation_alphas = rng.rand(args.utts).astype(np.float32)       # the same penalty samples on every side
    sides = [('one_by_one', None, True)]
    for bs in [int(v) for v in args.sizes.split(',')]:
        sides += [('batch_{}_sorted'.format(bs), bs, True), ('batch_{}_input_order'.format(bs), bs, False)]
    res = {'utterances': args.utts, 'lengths': lens, 'frames': int(sum(lens)), 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'sides': {}}

    def run(bs, sort):
        opt.cfg.train_validation_batch_size, opt.cfg.train_validation_sort_by_length = bs, sort
        opt.costs_tra_critic_batches.append_device(torch.ones((), device='cuda'))
        costs = {k: [] for k in COSTS}
        with contextlib.redirect_stdout(quiet):
            opt.update_validation_cost(costs, Xv, Yv)
        return costs

    times = {name: [] for name, _, _ in sides}
    costs = {}
    for rep in range(3 + args.reps):
        for name, bs, sort in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            costs[name] = run(bs, sort)
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append(time.perf_counter() - t0)
    base = spread(times['one_by_one'])
    for name, bs, sort in sides:
        out = spread(times[name])
        out['one_by_one_median_over_this_median'] = base['median_s'] / out['median_s']
        out['p90_below_one_by_one_p10'] = out['p90_s'] < base['p10_s']
        out['costs'] = {k: float(costs[name][k][0]) for k in COSTS}
        out['padded_frames'] = 0 if bs is None else int(data._padding(lens, data.length_groups(lens, bs, sort=sort)))
        with _hip.KernelTimer() as kt:          # kernel time by kind, a pass of its own
            run(bs, sort)
        torch.cuda.synchronize()
        split = {'blstm_recurrence_ms': 0.0, 'critic_penalty_passes_ms': 0.0, 'cost_kernels_ms': 0.0, 'rest_ms': 0.0}
        in_critic = False
        for kname, _, ms in kt.durations_ms():
            if kname == 'ptts_gp_interpolate': in_critic = True
            if kname == 'ptts_gp_sqnorm': in_critic = False
            if kname in ('ptts_lstm_fwd', 'ptts_lstm_fwd_ragged'): split['blstm_recurrence_ms'] += ms
            elif kname in COST_KERNELS: split['cost_kernels_ms'] += ms
            elif in_critic: split['critic_penalty_passes_ms'] += ms
            else: split['rest_ms'] += ms
        split['launches'] = len(kt.records)
        out['kernel_time'] = split
        res['sides'][name] = out
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
