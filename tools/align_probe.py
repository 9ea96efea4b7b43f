#!/usr/bin/env python
"""Times the forced alignment of csrc/align.hip with HIP events and prints the figures of DESIGN.md section 6 ("Forced alignment"):

    batch   eight utterances of 400 to 700 frames with about 40 phones (200 chain states) in ONE ptts_align_viterbi_batch call,
            D = 60: the three device phases one by one (emissions, time loop, backtrack: the `phases` argument runs a subset of the
            launches on what the last call left in the workspace) and the whole call, each the median of --reps launches after
            3 warm-up launches; ptts_align_accumulate and ptts_align_update for the same batch
    train   one full ops.forced_align_train run on a synthetic corpus (--utts utterances of the same kind, 40 models x 5 states),
            a host clock around the call, which ends in a download

beside the fp64 host restatement's time for the same work (numpy emissions column by column, the recurrence vectorised over the
states, the backtrack, accumulate, update and the loop, as tests/test_forced_align.py states them; run once), and whether the
device's durations equal the restatement's.

    python tools/align_probe.py [--reps 20] [--utts 32] [--no-host]
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, MODELS, S = 60, 40, 5


def utterance(rng, means, phones, lo, hi):
    chain = (rng.randint(0, MODELS, size=phones)[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    dur = rng.randint(lo, hi + 1, size=chain.size)
    X = means[np.repeat(chain, dur)] + rng.randn(int(dur.sum()), D)
    return X.astype(np.float32), chain


def host_emissions(X, chain, mu, w, g):
    x = X.astype(np.float64)
    acc = np.zeros((x.shape[0], chain.size))
    for d in range(D):
        t = x[:, d][:, None] - mu[chain, d][None, :]
        acc = acc + (t * t) * w[chain, d][None, :]
    return -0.5 * (acc + g[chain][None, :])


def host_viterbi(E):
    T, N = E.shape
    V = np.full(N, -np.inf)
    V[0] = E[0, 0]
    take = np.zeros((T, N), dtype=bool)
    for t in range(1, T):
        adv = np.concatenate([[-np.inf], V[:-1]])
        take[t] = adv > V
        V = E[t] + np.where(take[t], adv, V)
    state, n = np.zeros(T, dtype=np.int64), N - 1
    for t in range(T - 1, -1, -1):
        state[t] = n
        if t > 0 and take[t, n]:
            n -= 1
    return np.bincount(state, minlength=N), state, V[N - 1]


def host_reestimate(Xs, chains, durs, Q, floor, mu, w, g, min_count=2):
    count, s1, s2 = np.zeros(Q, np.int64), np.zeros((Q, D)), np.zeros((Q, D))
    for X, chain, dur in zip(Xs, chains, durs):
        q = np.repeat(chain, dur)
        x = X.astype(np.float64)
        np.add.at(count, q, 1)
        np.add.at(s1, q, x)
        np.add.at(s2, q, x * x)
    ok = count >= min_count
    m = s1[ok] / count[ok, None]
    var = np.maximum(s2[ok] / count[ok, None] - m * m, floor[None, :])
    mu[ok], w[ok] = m, 1.0 / var
    total = np.zeros(int(ok.sum()))
    for d in range(D):
        total = total + np.log(var[:, d])
    g[ok] = total


def host_train(Xs, chains, Q, n_iter):
    x = np.concatenate(Xs).astype(np.float64)
    floor = 0.01 * ((x - x.mean(axis=0)) ** 2).mean(axis=0)
    mu, w, g = np.zeros((Q, D)), np.ones((Q, D)), np.zeros(Q)
    durs = []
    for X, c in zip(Xs, chains):
        n = np.arange(c.size, dtype=np.int64)
        durs.append((n + 1) * X.shape[0] // c.size - n * X.shape[0] // c.size)
    host_reestimate(Xs, chains, durs, Q, floor, mu, w, g)
    prev, its = [np.repeat(np.arange(len(d)), d) for d in durs], 0
    for _ in range(n_iter):
        res = [host_viterbi(host_emissions(X, c, mu, w, g)) for X, c in zip(Xs, chains)]
        its += 1
        changed = sum(int((r[1] != p).sum()) for r, p in zip(res, prev))
        durs, prev = [r[0] for r in res], [r[1] for r in res]
        if changed == 0:
            break
        host_reestimate(Xs, chains, durs, Q, floor, mu, w, g)
    return durs, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--utts', type=int, default=32)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()

    import torch
    from percivaltts_amd import _hip, ops
    assert torch.cuda.is_available(), 'align_probe needs the GPU'
    rng = np.random.RandomState(0)
    Q = MODELS * S
    means = rng.randint(-8, 9, size=(Q, D)).astype(np.float64)
    res = {'D': D, 'Q': Q, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'max_states': ops.align_max_states()}

    # ---- one batch, phase by phase ----
    batch = [utterance(rng, means, 40, 1, hi) for hi in (3, 3, 4, 4, 4, 5, 5, 6)]
    fl, sl = [x.shape[0] for x, _ in batch], [c.size for _, c in batch]
    X = torch.from_numpy(np.concatenate([x for x, _ in batch])).cuda()
    gauss = torch.from_numpy(np.concatenate([c for _, c in batch]).astype(np.int32)).cuda()
    fo, so = ops.packed_offsets(fl, X.device), ops.packed_offsets(sl, X.device)
    mu, w, g = (torch.from_numpy(a).cuda() for a in (means, np.ones((Q, D)), np.zeros(Q)))
    occ, occ_off = (torch.from_numpy(a).cuda() for a in ops.align_occurrences(gauss.cpu().numpy(), Q))
    floor = torch.full((D,), 0.01, dtype=torch.float64, device=X.device)
    phases = (('emissions', _hip._define('PTTS_ALIGN_PHASE_EMISSIONS')), ('time_loop', _hip._define('PTTS_ALIGN_PHASE_TIME_LOOP')),
              ('backtrack', _hip._define('PTTS_ALIGN_PHASE_BACKTRACK')), ('all', _hip._define('PTTS_ALIGN_PHASE_ALL')))
    names = [n for n, _ in phases] + ['accumulate', 'update']
    times = {n: [] for n in names}
    info = torch.zeros(len(batch), dtype=torch.int32, device=X.device)
    for rep in range(3 + args.reps):
        m2 = [t.clone() for t in (mu, w, g)]
        with _hip.KernelTimer() as kt:
            for _, mask in phases:
                out = ops.align_viterbi(X, fo, gauss, so, mu, w, g, phases=mask, info=info)
            sums = ops.align_accumulate(X, fo, gauss, so, out.dur, occ, occ_off, Q)
            ops.align_update(*sums, floor, *m2)
        if rep >= 3:
            for n, (_, _, ms) in zip(names, kt.durations_ms()):
                times[n].append(ms * 1e-3)
    cells = sum(t * n for t, n in zip(fl, sl))
    entry = {'utterances': len(batch), 'frames': fl, 'states': sl, 'cells': cells, 'flags': info.cpu().numpy().tolist()}
    for n, ts in times.items():
        entry[n + '_s'] = float(np.median(ts))
    entry['emission_gflops'] = 4.0 * cells * D / entry['emissions_s'] * 1e-9     # a difference, two products and a sum per column
    entry['time_loop_us_per_frame'] = entry['time_loop_s'] / max(fl) * 1e6     # the waves run side by side: the longest utterance
    if not args.no_host:
        t0 = time.perf_counter()
        want = [host_viterbi(host_emissions(x, c, means, np.ones((Q, D)), np.zeros(Q))) for x, c in batch]
        entry['host_restatement_s'] = time.perf_counter() - t0
        entry['host_over_device'] = entry['host_restatement_s'] / entry['all_s']
        entry['dur_equal'] = bool((out.dur.cpu().numpy() == np.concatenate([r[0] for r in want])).all())
        score = out.score.cpu().numpy()
        entry['score_largest_relative_difference'] = float(max(abs(s - r[2]) / abs(r[2]) for s, r in zip(score, want)))
    res['batch'] = entry

    # ---- one training run ----
    corpus = [utterance(rng, means, 40, 1, 3 + u % 4) for u in range(args.utts)]
    Xs, chains = [x for x, _ in corpus], [c for _, c in corpus]
    Xc = torch.from_numpy(np.concatenate(Xs)).cuda()
    lens = [x.shape[0] for x in Xs]
    ops.forced_align_train(Xc, lens, chains, Q, n_iter=1)                       # warm-up: code objects, the workspace
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model, dur, hist = ops.forced_align_train(Xc, lens, chains, Q)
    dur = dur.cpu().numpy()
    entry = {'utterances': len(corpus), 'frames': int(sum(lens)), 'device_s': time.perf_counter() - t0, 'alignments': len(hist) - 1,
             'changed': [h[1] for h in hist], 'kept': [h[2] for h in hist], 'floored': [h[3] for h in hist], 'total': [h[0] for h in hist[1:]]}
    entry['device_s_per_alignment'] = entry['device_s'] / max(1, entry['alignments'])
    if not args.no_host:
        t0 = time.perf_counter()
        hdurs, its = host_train(Xs, chains, Q, 20)
        entry['host_restatement_s'] = time.perf_counter() - t0
        entry['host_alignments'] = its
        entry['host_over_device'] = entry['host_restatement_s'] / entry['device_s']
        entry['dur_equal'] = bool(its == entry['alignments'] and (dur == np.concatenate(hdurs)).all())
    res['train'] = entry
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
