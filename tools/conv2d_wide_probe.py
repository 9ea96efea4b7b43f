"""Wide and non-square Conv2D layers at [64,400,65]: device time of the forward, the backward (dx + dW + dbias) and the
second-order sweep (masked forward + dW) of one layer with a LeakyReLU input, with the wide tier (csrc/conv2d_wide.hip) on and
off -- off: the generic kernels of csrc/conv2d.hip.  Only ops.conv2d, autograd and _hip.KernelTimer: on a tree without the wide
tier both legs are the generic kernels.  The 4 -> 4 5x5 layer (its own matrix-core kernels, either leg) is timed for scale.

    python tools/conv2d_wide_probe.py [--reps 50] [--json out.json]

A pass's time is the sum of its C-ABI calls between device events (the grouped reduction of the partial rows included); the legs
alternate repetition by repetition in one process.  Share of peak: algorithmic flops against the fp32 matrix peak (157.3 TFLOP/s)
or algorithmic bytes against HBM (8.0 TB/s spec), whichever bounds the pass (MI355X)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from percivaltts_amd import ops, _hip

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
B, T, F = 64, 400, 65
SHAPES = [
    # name, Cin, Cout, KT, KF, dil, causal
    ('1->8 5x5', 1, 8, 5, 5, 1, False), ('8->8 5x5', 8, 8, 5, 5, 1, False), ('8->1 5x5', 8, 1, 5, 5, 1, False),
    ('16->16 5x5', 16, 16, 5, 5, 1, False), ('4->4 5x3', 4, 4, 5, 3, 1, False), ('8->8 5x5 dil 2 causal', 8, 8, 5, 5, 2, True),
    ('4->4 5x5 (scale)', 4, 4, 5, 5, 1, False),
]


def switch(on):
    if hasattr(ops, 'conv2d_wide'):
        ops.conv2d_wide(on)


def timed(fn):
    with _hip.KernelTimer() as kt:
        fn()
    return sum(ms for _, _, ms in kt.durations_ms()) * 1e3          # us


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    return q(0.5), q(0.1), q(0.9)


def layer(name, Cin, Cout, KT, KF, dil, causal, reps, warm):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, F, Cin, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(KT, KF, Cin, Cout, generator=g) * 0.2).cuda().requires_grad_(True)
    b = torch.randn(Cout, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(B, T, F, Cout, generator=g).cuda()
    u = torch.randn(B, T, F, Cin, generator=g).cuda()
    R = torch.randn(B, T, F, Cout, generator=g).cuda().requires_grad_(True)
    pad = ops.PAD_CAUSAL if causal else ops.PAD_SAME
    conv = lambda: ops.conv2d(ops.Lazy(x, lrelu=True), w, b, dil_t=dil, pad_mode=pad)

    def fwd():
        with torch.no_grad():
            return timed(conv)

    def bwd():
        y = conv()
        t = timed(lambda: y.backward(dy))
        x.grad = w.grad = b.grad = None
        return t

    def sweep():
        y = conv()
        with ops.input_grad_only():
            gx = torch.autograd.grad(y, x, grad_outputs=R, create_graph=True)[0]
        t = timed(lambda: gx.backward(u))
        w.grad = R.grad = b.grad = x.grad = None
        return t

    mac = B * T * F * KT * KF * Cin * Cout
    px = 4 * B * T * F
    work = {'forward': (2 * mac, px * (Cin + Cout)), 'backward': (4 * mac, px * (2 * Cin + Cout)),
            'second-order sweep': (4 * mac, px * (2 * Cin + 2 * Cout))}
    rows = []
    for pname, fn in (('forward', fwd), ('backward', bwd), ('second-order sweep', sweep)):
        legs = {True: [], False: []}
        for i in range(warm + reps):
            for on in (True, False):
                switch(on)
                t = fn()
                if i >= warm:
                    legs[on].append(t)
        switch(None)
        on_s, off_s = stats(legs[True]), stats(legs[False])
        flops, nbytes = work[pname]
        bound = 'matrix' if flops / PEAK_FLOPS >= nbytes / PEAK_BYTES else 'HBM'
        floor_us = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e6
        rows.append(dict(shape=name, **{'pass': pname}, on_us=on_s, off_us=off_s, ratio=off_s[0] / on_s[0], gflop=flops / 1e9,
                         mbytes=nbytes / 1e6, bound=bound, share_on=floor_us / on_s[0], share_off=floor_us / off_s[0]))
        r = rows[-1]
        print('{:<24s} {:<19s} on {:9.1f} us [{:.1f}-{:.1f}]  off {:10.1f} us [{:.1f}-{:.1f}]  x{:6.2f}  {:7.2f} GFLOP {:7.1f} MB  '
              '{} bound: {:5.1f} % of peak on, {:5.2f} % off'.format(name, pname, on_s[0], on_s[1], on_s[2], off_s[0], off_s[1], off_s[2],
                                                                   r['ratio'], r['gflop'], r['mbytes'], bound, 100 * r['share_on'],
                                                                   100 * r['share_off']), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--only', default=None, help='substring of a shape name')
    a = ap.parse_args()
    assert a.reps >= 1
    print('wide tier: {}'.format('present' if hasattr(ops, 'conv2d_wide') else 'absent (both legs are the generic kernels)'))
    rows = []
    for s in SHAPES:
        if a.only is None or a.only in s[0]:
            rows += layer(*s, reps=a.reps, warm=a.warmup)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
