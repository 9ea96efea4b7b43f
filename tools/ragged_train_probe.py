#!/usr/bin/env python
"""Real frames per second of the WGAN training step with and without masked training, the figures of DESIGN.md section 6,
"Ragged training", as one JSON document.

A synthetic corpus of --utts cropped utterances whose lengths are spread evenly over 150 to 900 frames (seeded; 601 context
columns, 86 output columns) is made resident on the device (data.DeviceCorpus.from_utterances).  Batches of --batch utterances,
lengthmax 400, the BASELINE architecture (H = 256, 8 x 4 conv layers, WLSWGAN).  Three cases, each through
OptimizerTTSWGAN.device_step on the batches the training loop would cut:

  randshift           the yardstick: the window of a batch is its shortest row (capped by lengthmax), every frame real; T changes
                      from batch to batch, so the step stays in its eager or freshly tuned form as the loop would have it
  randshiftpad        T = lengthmax for every batch, rows shorter than that zero-padded, the masked step
  randshiftpad_full   the same on a corpus whose rows are all at least lengthmax long: every row full -- the price of the masks
                      and of the eager steps, against 'randshift_full', the dense step on the same batches

A frame is real if it lies in front of its row's length.  Timing: per case --warmup steps, then the cases ALTERNATE in rounds of
--steps steps (one generator step per ten batches at these update counts; 200 steps of 4 to 7 ms: a window of about a second),
each round between two device events behind a synchronise.  The window holds what the training loop does per batch: the window plan
on the host, the ptts_batch_windows gather and the step; under 'randshift' it also holds the first launches of every T that has not
come before (T changes with the batch's shortest row, so no warm-up covers them: that is the case being measured).
frames/s = real frames of the round / its time; median, p10 and p90 over --rounds rounds.

--critic chain: the critic form instead -- two cases on the spread corpus, the same batches and lengths (same seed), alternating
as above: 'randshiftpad' (the masked step, fp32 layer-wise critic) and 'randshiftpad_chain' (the masked step with
cfg.arch_critic_bf16 = 'chain': the Conv2D stack on the per-row chain kernels).

    python tools/ragged_train_probe.py [--utts 256] [--batch 64] [--steps 200] [--rounds 5] [--warmup 20] [--critic fp32|chain]
"""
from __future__ import print_function

import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX, SPEC, NM = 601, 65, 20
OUT = 1 + SPEC + NM
LENGTHMAX = 400


def spread(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {'median': float(np.median(ts)), 'p10': float(np.percentile(ts, 10)), 'p90': float(np.percentile(ts, 90)), 'count': int(ts.size)}


def make_corpus(nutts, lo, hi, seed):
    from percivaltts_amd import data
    rng = np.random.RandomState(seed)
    lens = rng.permutation(np.linspace(lo, hi, nutts).astype(int))
    Xs = [(rng.rand(n, CTX) * 2 - 1).astype(np.float32) for n in lens]
    Ys = [rng.randn(n, OUT).astype(np.float32) for n in lens]
    Ws = [np.ones((n, 1), dtype=np.float32) for n in lens]
    return data.DeviceCorpus.from_utterances(Xs, Ys, Ws), lens


def make_optimiser(batch, padtype, critic=None):
    import torch
    import percivaltts_amd
    from percivaltts_amd import modeltts_common, networks_critic, optimizertts_wgan, vocoders
    np.random.seed(123); torch.manual_seed(123)
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 256; cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 21
    cfg.arch_gen_nbcnnlayers = 8; cfg.arch_gen_nbfilters = 4; cfg.arch_gen_winlen = 5; cfg.arch_spec_freqlen = 5
    cfg.train_batch_size = batch; cfg.train_batch_lengthmax = LENGTHMAX; cfg.train_batch_padtype = padtype
    if critic == 'chain':
        cfg.arch_critic_bf16 = 'chain'
    voc = vocoders.VocoderPML(16000, 0.005, SPEC, NM)
    mod = modeltts_common.DCNNF0SpecNoiseFeatures(CTX, voc, cfg)
    crit = networks_critic.Critic(voc, CTX, cfg)
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    opt.generator_updates = 0
    return opt


class Case(object):
    def __init__(self, name, corpus, batch, padtype, seed, critic=None):
        self.name, self.corpus, self.batch, self.padtype = name, corpus, batch, padtype
        self.masked = padtype == 'randshiftpad'
        self.opt = make_optimiser(batch, padtype, critic)
        self.rng = np.random.RandomState(seed)
        self.batchid = 0
        self.rates, self.frames, self.ms = [], [], []

    def steps(self, k):
        """k training steps; returns the real frames they trained on"""
        real = 0
        for _ in range(k):
            ids = self.rng.permutation(len(self.corpus))[:self.batch]
            X, Y, n = self.corpus.batch(ids, None, LENGTHMAX, self.padtype, want_lengths=True)
            real += int(n.sum())
            if self.masked:
                self.opt.device_step(self.batchid, X, Y, lengths=n)
            else:
                self.opt.device_step(self.batchid, X, Y)
            self.batchid += 1
        return real

    def timed_round(self, k):
        import torch
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        real = self.steps(k)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e)
        self.rates.append(real / (ms * 1e-3)); self.frames.append(real / float(k)); self.ms.append(ms / k)

    def result(self):
        return {'padtype': self.padtype, 'real_frames_per_s': spread(self.rates), 'real_frames_per_batch': spread(self.frames),
                'ms_per_step': spread(self.ms), 'frames_in_a_batch_tensor': 'B x T of that batch' if not self.masked else self.batch * LENGTHMAX}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--critic', choices=['fp32', 'chain'], default='fp32', help="'chain': the masked step with the bf16 chain critic against the masked fp32 one")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), 'ragged_train_probe needs the GPU'
    quiet = io.StringIO()
    try:
        with contextlib.redirect_stdout(quiet):
            spread_corpus, lens = make_corpus(args.utts, 150, 900, seed=0)
            full_corpus, _ = make_corpus(args.utts, LENGTHMAX, 900, seed=1)
            if args.critic == 'chain':
                cases = [Case('randshiftpad', spread_corpus, args.batch, 'randshiftpad', 10),
                         Case('randshiftpad_chain', spread_corpus, args.batch, 'randshiftpad', 10, critic='chain')]
            else:
                cases = [Case('randshift', spread_corpus, args.batch, 'randshift', 10),
                         Case('randshiftpad', spread_corpus, args.batch, 'randshiftpad', 10),
                         Case('randshift_full', full_corpus, args.batch, 'randshift', 11),
                         Case('randshiftpad_full', full_corpus, args.batch, 'randshiftpad', 11)]
            for c in cases:
                c.steps(args.warmup)
            for _ in range(args.rounds):
                for c in cases:                       # the cases alternate: what else runs on the machine hits them alike
                    c.timed_round(args.steps)
    except BaseException:
        sys.stderr.write(quiet.getvalue()[-4000:])
        raise
    res = {'device': torch.cuda.get_device_name(0), 'utterances': args.utts, 'cropped_lengths': [int(lens.min()), int(lens.max())],
           'batch': args.batch, 'lengthmax': LENGTHMAX, 'steps_per_round': args.steps, 'rounds': args.rounds, 'critic': args.critic,
           'cases': dict((c.name, c.result()) for c in cases)}
    base = res['cases'][cases[0].name]['real_frames_per_s']['median']
    for c in cases:
        res['cases'][c.name]['over_' + cases[0].name] = res['cases'][c.name]['real_frames_per_s']['median'] / base
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
