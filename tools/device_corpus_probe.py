#!/usr/bin/env python
"""Times the training loop's batch feed both ways -- load_inoutset per batch (the host loader) against the training set resident
on the device (data.DeviceCorpus, cfg.train_data_on_device) -- and prints the figures of DESIGN.md section 6, "Resident training
set", as one JSON document.

The corpus is synthetic and written under a temporary directory: --utts utterances of 500 to 900 frames (seeded), 601 context
columns, 86 output columns, one time-weight column with 20 silent frames at either end.  Batches of --batch utterances,
lengthmax 400, 'randshift', cropmode 'begendbigger' (the training defaults).

  1 host_loader   wall time of one load_inoutset call on a shuffled batch, files in the page cache; --reps calls after 3 warm-ups.
  2 gather        the kernel alone: --launches ptts_batch_windows launches back to back between two HIP events (8 window plans in
                  turn, tables already on the device), per launch, and the bytes/s of the bytes it reads plus the bytes it writes;
                  beside it the wall time of a whole DeviceCorpus.batch call (plan, checks, table upload, launch).
  3 copy          Tensor.copy_ of a tensor with the gather's destination byte count, timed the same way, alternating with 2.
  4 loop          OptimizerTTSWGAN.train over --epochs epochs with the BASELINE model (H = 256), switch off and on, same seeds:
                  per epoch its wall time (with the validation sweep and the checkpoints), the time inside train_on_batch, the
                  time inside the loader's calls (what the epoch line prints as train: and load:) and the stall -- the time the
                  loop spent between two train_on_batch calls, waiting for its next batch.

    python tools/device_corpus_probe.py [--utts 256] [--batch 64] [--reps 20] [--launches 200] [--epochs 4] [--skip-loop]
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
OUT = 1 + SPEC + NM
LENGTHMAX, PADTYPE, CROPMODE = 400, 'randshift', 'begendbigger'


def spread(ts, scale=1.0):
    ts = np.asarray(ts, dtype=np.float64) * scale
    return {'median': float(np.median(ts)), 'p10': float(np.percentile(ts, 10)), 'p90': float(np.percentile(ts, 90)), 'count': int(ts.size)}


def make_corpus(root, nutts, seed=0):
    rng = np.random.RandomState(seed)
    fids = ['syn_{:04d}'.format(i) for i in range(nutts)]
    for sub in ('lab', 'cmp', 'w'):
        os.makedirs(os.path.join(root, sub))
    for fid in fids:
        n = int(rng.randint(500, 901))
        (rng.rand(n, CTX) * 2 - 1).astype(np.float32).tofile(os.path.join(root, 'lab', fid + '.lab'))
        rng.randn(n, OUT).astype(np.float32).tofile(os.path.join(root, 'cmp', fid + '.cmp'))
        w = np.ones((n, 1), dtype=np.float32)
        w[:20] = 0.0; w[-20:] = 0.0
        w.tofile(os.path.join(root, 'w', fid + '.w'))
    return (os.path.join(root, 'lab', '*.lab') + ':(-1,{})'.format(CTX), os.path.join(root, 'cmp', '*.cmp') + ':(-1,{})'.format(OUT),
            os.path.join(root, 'w', '*.w') + ':(-1,1)', fids)


def host_loader(paths, fids, batch, reps):
    from percivaltts_amd import data
    indir, outdir, wdir = paths
    rng = np.random.RandomState(1)
    ts = []
    for rep in range(3 + reps):
        ids = [fids[i] for i in rng.permutation(len(fids))[:batch]]
        t0 = time.perf_counter()
        data.load_inoutset(indir, outdir, wdir, ids, lengthmax=LENGTHMAX, maskpadtype=PADTYPE, cropmode=CROPMODE)
        if rep >= 3:
            ts.append(time.perf_counter() - t0)
    return spread(ts, 1e3)


def gather_and_copy(corpus, batch, launches, reps):
    import torch
    from percivaltts_amd import _hip
    from percivaltts_amd._hip import call, ptr, stream
    dev = corpus.device
    rng = np.random.RandomState(2)
    plans, read_bytes = [], []
    for _ in range(8):
        ids = rng.permutation(len(corpus))[:batch]
        T, utt, shift, n = corpus.plan(ids, None, LENGTHMAX, PADTYPE)
        plans.append((T, torch.from_numpy(np.stack((utt, shift, n))).to(dev)))
        read_bytes.append(4 * int(n.sum()) * (CTX + OUT))
    assert all(p[0] == LENGTHMAX for p in plans)
    X = torch.empty((batch, LENGTHMAX, CTX), dtype=torch.float32, device=dev)
    Y = torch.empty((batch, LENGTHMAX, OUT), dtype=torch.float32, device=dev)
    written = 4 * (X.numel() + Y.numel())
    moved = written + float(np.mean(read_bytes))
    a = torch.randn(written // 4, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)

    def gather(i):
        tab = plans[i % len(plans)][1]
        call('ptts_batch_windows', ptr(corpus.X), ptr(corpus.Y), None, ptr(X), ptr(Y), None, CTX, OUT, 0, 2, ptr(corpus._row_off_dev),
             len(corpus), ptr(tab[0]), ptr(tab[1]), ptr(tab[2]), batch, LENGTHMAX, stream())

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for i in range(launches):
            fn(i)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / launches          # us per launch

    tg, tc = [], []
    for rep in range(2 + reps):                            # the two sides alternate; two warm-up rounds
        g, c = timed(gather), timed(lambda i: b.copy_(a))
        if rep >= 2:
            tg.append(g); tc.append(c)
    # the whole call as the training loop makes it
    tcall = []
    for rep in range(3 + 50):
        ids = rng.permutation(len(corpus))[:batch]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        corpus.batch(ids, None, LENGTHMAX, PADTYPE)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if rep >= 3:
            tcall.append((t1 - t0, time.perf_counter() - t0))
    out_g, out_c = spread(tg), spread(tc)
    out_g.update({'unit': 'us per launch', 'launches_per_window': launches, 'bytes_read': float(np.mean(read_bytes)), 'bytes_written': written,
                  'gbytes_per_s': moved / (out_g['median'] * 1e-6) / 1e9})
    out_c.update({'unit': 'us per launch', 'launches_per_window': launches, 'bytes_read': written, 'bytes_written': written,
                  'gbytes_per_s': 2.0 * written / (out_c['median'] * 1e-6) / 1e9})
    out_g['over_copy'] = out_g['median'] / out_c['median']
    return out_g, out_c, {'host_enqueue_ms': spread([t[0] for t in tcall], 1e3), 'until_done_ms': spread([t[1] for t in tcall], 1e3)}


def loop(paths, fids, batch, epochs, on_device, workdir):
    import torch
    import percivaltts_amd
    from percivaltts_amd import data, modeltts_common, networks_critic, optimizertts_wgan, vocoders
    indir, outdir, wdir = paths
    np.random.seed(123); torch.manual_seed(123)
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 256; cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 21
    cfg.arch_gen_nbcnnlayers = 8; cfg.arch_gen_nbfilters = 4; cfg.arch_gen_winlen = 5; cfg.arch_spec_freqlen = 5
    cfg.train_batch_size = batch; cfg.train_batch_lengthmax = LENGTHMAX
    cfg.train_min_nbepochs = 1; cfg.train_max_nbepochs = epochs; cfg.train_cancel_nodecepochs = 10 * epochs
    cfg.train_nbepochs_scalewdata = False
    cfg.train_data_on_device = bool(on_device)
    voc = vocoders.VocoderPML(16000, 0.005, SPEC, NM)
    mod = modeltts_common.DCNNF0SpecNoiseFeatures(CTX, voc, cfg)
    crit = networks_critic.Critic(voc, CTX, cfg)
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    marks = {'train': [], 'load': []}              # (start, end) of every train_on_batch and of every loader call

    def clocked(fn, key):
        def f(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                marks[key].append((t0, time.perf_counter()))
        return f
    opt.train_on_batch = clocked(opt.train_on_batch, 'train')
    real = (data.load_inoutset, data.DeviceCorpus.batch)
    data.load_inoutset = clocked(real[0], 'load')
    data.DeviceCorpus.batch = clocked(real[1], 'load')
    os.makedirs(workdir)
    t_start = time.perf_counter()
    try:
        opt.train(indir, outdir, wdir, fids[:-4], fids[-4:], os.path.join(workdir, 'model.h5'))
        torch.cuda.synchronize()
    finally:
        data.load_inoutset, data.DeviceCorpus.batch = real
    total = time.perf_counter() - t_start
    import pickle
    with open(os.path.join(workdir, 'model-trainingstate-last.h5.model.cfgextras.pkl'), 'rb') as f:
        _, extras, _ = pickle.load(f)
    nb = (len(fids) - 4) // batch
    per_epoch = []
    for ep in range(epochs):
        tr = marks['train'][ep * nb:(ep + 1) * nb]
        ld = marks['load'][ep * nb:(ep + 1) * nb]
        per_epoch.append({'epoch_s': float(extras['epochs_durs'][ep]), 'train_s': sum(e - s for s, e in tr), 'load_s': sum(e - s for s, e in ld),
                          'stall_s': sum(tr[i + 1][0] - tr[i][1] for i in range(len(tr) - 1)), 'batch_loop_s': tr[-1][1] - tr[0][0]})
    assert len(marks['train']) == len(marks['load']) == nb * epochs
    return {'train_data_on_device': bool(on_device), 'batches_per_epoch': nb, 'epochs': per_epoch, 'whole_run_s': total,
            'cost_tra': [float(c) for c in extras['costs']['model_training']]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--skip-loop', action='store_true')
    args = ap.parse_args()

    import torch
    from percivaltts_amd import data
    assert torch.cuda.is_available(), 'device_corpus_probe needs the GPU'
    root = tempfile.mkdtemp(prefix='ptts_corpus_probe_')
    res = {'device': torch.cuda.get_device_name(0), 'utterances': args.utts, 'batch': args.batch, 'lengthmax': LENGTHMAX,
           'columns': [CTX, OUT, 1]}
    try:
        indir, outdir, wdir, allfids = make_corpus(root, args.utts + 4)          # the last four: the loop's validation set
        paths, fids = (indir, outdir, wdir), allfids[:args.utts]
        res['host_loader_ms_per_batch'] = host_loader(paths, fids, args.batch, args.reps)
        t0 = time.perf_counter()
        corpus = data.DeviceCorpus(indir, outdir, wdir, fids, cropmode=CROPMODE)
        torch.cuda.synchronize()
        res['corpus'] = {'build_s': time.perf_counter() - t0, 'bytes': corpus.nbytes, 'frames_kept': int(corpus.row_off[-1])}
        res['gather'], res['copy'], res['corpus_batch_call'] = gather_and_copy(corpus, args.batch, args.launches, args.reps)
        del corpus
        torch.cuda.empty_cache()
        if not args.skip_loop:
            quiet = io.StringIO()
            res['loop'] = []
            for k, on in enumerate((False, True)):
                try:
                    with contextlib.redirect_stdout(quiet):
                        res['loop'].append(loop(paths, allfids, args.batch, args.epochs, on, os.path.join(root, 'run{}'.format(k))))
                except BaseException:
                    sys.stderr.write(quiet.getvalue()[-4000:])
                    raise
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
