"""Ragged inference, the rule itself (CPU, float64): a zero-padded batch [B, Tmax, ctx] with a length per row gives, on each
row's real frames, what that utterance gives alone, PROVIDED every layer that reads across time sees zeros at t >= len: the
convolutions get their input with those rows zeroed (what 'same' padding shows a lone utterance) and the recurrence walks each
row over its own length.  Per-frame layers (Dense, BatchNorm in inference, LeakyReLU, sigmoid) need nothing.

`ragged_generator_forward` restates the generator's inference forward under that rule from the oracle's own primitives; it must
equal the oracle's lone forward to the bounds tests/test_golden.py uses for generator_forward (rtol 1e-10 / atol 1e-12).  The
second test shows the inputs have teeth: the same padded batches through the oracle WITHOUT the rule miss the lone result by more
than 100 times the bound of the GPU tests (tests/test_ragged_gpu.py: rtol 5e-4, atol 5e-5), in the f0 column and in the
spectral columns of every utterance shorter than Tmax -- random_weights(bn_noise=True) gives non-zero BatchNorm shifts, so the
pad rows are non-zero after the first layer.

One exception is structural, not a matter of seeds: in 'gated_dilated' every Conv2D is causal, and its one context Conv1D reads
the zero-padded input itself, so nothing on the way to the spectral columns ever looks across the end of a row.  There the
spectral columns of the unmasked batch EQUAL the lone ones, which is asserted; its f0 column (the backward LSTM direction) has
the teeth, and the spectral teeth of a gated stack are shown on 'gated', the same layers with symmetric padding.  The input
seed (8) is one at which every padded utterance of all three geometries clears the factor 100."""
import functools

import pytest
import torch

from oracle import percival_oracle as O

import test_model_gpu as tm                                     # GEOMS only: nothing of it runs here

GPU_RTOL, GPU_ATOL = 5e-4, 5e-5                                 # tests/test_model_gpu.py's bound for predict


def arch(geom):
    g = tm.GEOMS[geom]
    return O.Arch(g['ctx'], g['spec'], g['nm'], g['H'], g['nctx'], g['kctx'], g['L'], g['C'], g['kt'], g['kf'],
                  gen_gated=bool(g.get('gated')), gen_dilations=g.get('dils'), gen_causal=bool(g.get('causal', False)))


def lengths_of(geom):
    T = tm.GEOMS[geom]['T']
    return [T, T - 1, 3, 1]


@functools.lru_cache(maxsize=None)
def batch(geom, seed=8):
    """(arch, weights, utterances [T_i, ctx], zero-padded batch [4, Tmax, ctx], lengths); float64, shared, nobody writes to it."""
    a = arch(geom)
    gw = O.random_weights(O.generator_weight_shapes(a), seed=11, bn_noise=True)
    gen = torch.Generator().manual_seed(seed)
    lens = lengths_of(geom)
    xs = [torch.rand(n, a.ctxsize, generator=gen, dtype=torch.float64) * 2 - 1 for n in lens]
    xpad = torch.zeros(len(lens), max(lens), a.ctxsize, dtype=torch.float64)
    for i, x in enumerate(xs):
        xpad[i, :lens[i]] = x
    return a, gw, xs, xpad, lens


@functools.lru_cache(maxsize=None)
def lone(geom):
    """The oracle's forward of each utterance alone."""
    a, gw, xs, _, _ = batch(geom)
    with torch.no_grad():
        return [O.generator_forward(gw, a, x[None], training=False)[0] for x in xs]


def zero_pad_rows(x, lens):
    y = x.clone()
    for i, n in enumerate(lens):
        y[i, n:] = 0
    return y


def ragged_generator_forward(weights, a, ctx, lens):
    """oracle.generator_forward(training=False) under the masking rule: rows t >= len zeroed in front of every convolution, the
    BLSTM run per row over its own length, the result's pad rows zeroed."""
    take = O._Take(weights)
    B, T = ctx.shape[0], ctx.shape[1]
    m = lambda x: zero_pad_rows(x, lens)

    def bnl(x):
        g, bt, mm, mv = take(4)
        return O.lrelu(O.BN(g, bt, mm, mv)(x, False))

    h = ctx
    for _ in range(a.nctx):
        h = bnl(O.conv1d_ntc(m(h), take()))
    for _ in range(2):
        h = bnl(O.dense(h, take()))
    W, U, b = take(3)
    f0 = h.new_zeros(B, T, 2 * a.H)
    for i, n in enumerate(lens):
        f0[i, :n] = O.blstm(h[i:i + 1, :n], W, U, b)[0]
    w, b = take(2)
    f0 = O.dense(f0, w, b)
    w, b = take(2)
    s = O.dense(h, w, b).reshape(B, T, a.specsize, 1)
    for li in range(a.L):
        if a.gated:
            dil = a.dilations[li % len(a.dilations)] if a.dilations else 1
            wa, wb = take(2)
            s = bnl(O.pgcnn2d_product(m(s), wa, wb, dil, a.causal))
        else:
            s = bnl(O.conv2d_nhwc(m(s), take()))
    w, b = take(2)
    s = O.conv2d_nhwc(m(s), w, b, causal=bool(a.gated and a.causal)).reshape(B, T, a.specsize)
    n_ = h
    for _ in range(a.L // 2):
        n_ = bnl(O.dense(n_, take()))
    w, b = take(2)
    n_ = torch.sigmoid(O.dense(n_, w, b))
    take.done()
    return m(torch.cat([f0, s, n_], dim=-1))


@pytest.mark.parametrize('geom', ['test', 'gated_dilated'])
def test_the_rule_is_sufficient(geom):
    a, gw, xs, xpad, lens = batch(geom)
    assert lens == [xpad.shape[1], xpad.shape[1] - 1, 3, 1]
    with torch.no_grad():
        got = ragged_generator_forward(gw, a, xpad, lens)
    for i, (n, want) in enumerate(zip(lens, lone(geom))):
        err = float((got[i, :n] - want).abs().max())
        print('{} utterance {} (T = {}): worst |err| {:.3e}'.format(geom, i, n, err))
        torch.testing.assert_close(got[i, :n], want, rtol=1e-10, atol=1e-12)
        assert float(got[i, n:].abs().sum()) == 0.0


@pytest.mark.parametrize('geom', ['test', 'gated_dilated', 'gated'])
def test_the_inputs_have_teeth(geom):
    """Without the rule the padded batch is wrong by more than 100 x the GPU bound on every padded utterance."""
    a, gw, xs, xpad, lens = batch(geom)
    with torch.no_grad():
        got = O.generator_forward(gw, a, xpad, training=False)
    spec = slice(1, 1 + a.specsize)
    for i, (n, want) in enumerate(zip(lens, lone(geom))):
        excess = (got[i, :n] - want).abs() / (GPU_ATOL + GPU_RTOL * want.abs())
        f0x, spx = float(excess[:, 0].max()), float(excess[:, spec].max())
        print('{} utterance {} (T = {}): worst error / GPU bound, f0 {:.1f}, spectrum {:.1f}'.format(geom, i, n, f0x, spx))
        if n == xpad.shape[1]:
            assert f0x < 1e-6 and spx < 1e-6                     # no padding: the same computation
        else:
            assert f0x > 100.0, 'f0 of utterance {} only {:.1f} x the GPU bound'.format(i, f0x)
            if a.gated and a.causal and a.nctx == 1:
                assert spx < 1e-6                               # no layer of this branch reads across the row's end
            else:
                assert spx > 100.0, 'spectrum of utterance {} only {:.1f} x the GPU bound'.format(i, spx)
