"""Evaluation costs on a ragged batch, the rule itself (CPU, float64): the critic and its gradient penalty on a zero-padded batch
[B, Tmax, ...] with a length per row give each utterance's own costs, PROVIDED every convolution of the critic reads its input
with the frames t >= len zeroed, the result is masked the same way, and every mean runs over the row's real frames only.  The
backward of a masked input is the masked gradient, so d sum_{t<len} D(x^)_b / d x^_b is the lone utterance's gradient on its
real frames and exactly zero behind them: the norm over [Tmax, spec] is the lone norm.

`ragged_critic_forward` restates oracle.critic_forward under that rule from the oracle's own primitives.  Per row, the two
Wasserstein means, the gradient norm of D(x^) (torch.autograd.grad) and the weighted least-squares term must equal
O.critic_step_loss(..., training=False) and O.generator_step_loss(..., training=False) of that utterance alone to 1e-10
relative.  The second test shows the batch has teeth: the same padded batch WITHOUT the masks (the means still over the real
frames only, so only what the convolutions and the recurrence read across a row's end is wrong) misses EVERY cost of every
padded utterance by more than 1e-6 relative, four orders of magnitude above the 1e-10 the rule is held to, and the penalty, the
gradient norm and the critic's total by more than 10 times the bound of the GPU tests (tests/test_validation_batched_gpu.py:
rtol 5e-4, atol 1e-5), so that a device path without the masks cannot pass there.

This file defines the target of the batched validation costs.  It tests the oracle against itself, so it passes on the code
before that feature as well: by design."""
import functools

import pytest
import torch

from oracle import percival_oracle as O

import test_model_gpu as tm                                     # GEOMS only: nothing of it runs here
import test_ragged_rule as rr                                   # ragged_generator_forward, zero_pad_rows: the generator's rule

TMAX = 12
GPU_RTOL, GPU_ATOL = 5e-4, 1e-5
TRANSIDX = 30.0


def ragged_critic_forward(weights, a, features, ctx, lens):
    """oracle.critic_forward under the masking rule: rows t >= len zeroed in front of every convolution and in the result."""
    take = O._Take(weights)
    B, T = features.shape[0], features.shape[1]
    m = lambda x: rr.zero_pad_rows(x, lens)
    h = features[:, :, 1:1 + a.specsize].reshape(B, T, a.specsize, 1)
    assert a.L > 0
    for li in range(a.L):
        w, b = take(2)
        h = O.lrelu(O.conv2d_nhwc(m(h), w, b))
    h = h.reshape(B, T, a.specsize * a.C)
    c = ctx
    for _ in range(a.nctx):
        w, b = take(2)
        c = O.lrelu(O.conv1d_ntc(m(c), w, b))
    for _ in range(2):
        w, b = take(2)
        c = O.lrelu(O.dense(c, w, b))
    p = torch.cat([h, c], dim=-1)
    for _ in range(3):
        w, b = take(2)
        p = O.lrelu(O.dense(p, w, b))
    w, b = take(2)
    out = O.dense(p, w, b)
    take.done()
    return m(out)


def rows_mean(v, lens):
    return torch.stack([v[i, :n].mean() for i, n in enumerate(lens)])


@functools.lru_cache(maxsize=None)
def case(lens):
    """(arch, generator weights, critic weights, utterances X_i, Y_i, alphas, w_ls, wgan weight); float64, shared, nobody writes."""
    a = rr.arch('test')
    gw = O.random_weights(O.generator_weight_shapes(a), seed=11, bn_noise=True)
    cw = O.random_weights(O.critic_weight_shapes(a), seed=12)
    gen = torch.Generator().manual_seed(21)
    xs = [torch.rand(n, a.ctxsize, generator=gen, dtype=torch.float64) * 2 - 1 for n in lens]
    ys = [torch.randn(n, a.outsize, generator=gen, dtype=torch.float64) for n in lens]
    al = torch.rand(len(lens), generator=gen, dtype=torch.float64)
    w_ls, ww = O.wls_weights(a.specsize, a.noisesize, 0, 0.25, TRANSIDX)
    return a, gw, cw, xs, ys, al, torch.tensor(w_ls), ww


@functools.lru_cache(maxsize=None)
def lone(lens):
    """Every cost of each utterance alone, from the oracle's own evaluation-mode losses."""
    a, gw, cw, xs, ys, al, w_ls, ww = case(lens)
    out = []
    for i in range(len(lens)):
        total, parts = O.critic_step_loss(cw, gw, a, xs[i][None], ys[i][None], al[i:i + 1], gp_lambda=10.0, training=False)
        gtot, gparts = O.generator_step_loss(cw, gw, a, xs[i][None], ys[i][None], 'WLSWGAN', w_ls, ww, training=False)
        g = parts['g'].detach()
        out.append({'l_valid': parts['valid'].detach(), 'l_fake': parts['fake'].detach(), 'gp': parts['gp'].detach(),
                    'norm': torch.sqrt((g * g).sum()), 'critic_total': total.detach(), 'gen_wgan': gparts['wgan'].detach(),
                    'gen_ls': gparts['ls'].detach(), 'gen_total': gtot.detach()})
    return out


def pad(ts, T):
    out = ts[0].new_zeros(len(ts), T, ts[0].shape[1])
    for i, t in enumerate(ts):
        out[i, :t.shape[0]] = t
    return out


def batched(lens, masked):
    """The same costs per row off ONE padded batch; `masked`: under the rule, else through the oracle's plain forwards."""
    a, gw, cw, xs, ys, al, w_ls, ww = case(lens)
    lens = list(lens)
    X, Y = pad(xs, TMAX), pad(ys, TMAX)
    with torch.no_grad():
        pred = rr.ragged_generator_forward(gw, a, X, lens) if masked else O.generator_forward(gw, a, X, training=False)
    D = (lambda f: ragged_critic_forward(cw, a, f, X, lens)) if masked else (lambda f: O.critic_forward(cw, a, f, X))
    x_hat = O.random_weighted_average(Y, pred, al).detach().requires_grad_(True)
    valid, fake_v, v_hat = D(Y), D(pred), D(x_hat)
    g = torch.autograd.grad(v_hat.sum(), x_hat)[0]
    norm = torch.sqrt((g * g).sum(dim=(1, 2)))
    l_valid, l_fake = -rows_mean(valid.detach(), lens), rows_mean(fake_v.detach(), lens)
    gp = (1 - norm) ** 2
    gen_ls = torch.stack([(((Y[i, :n] - pred[i, :n]) ** 2) * w_ls).mean() for i, n in enumerate(lens)])
    return {'l_valid': l_valid, 'l_fake': l_fake, 'gp': gp, 'norm': norm, 'critic_total': l_valid + l_fake + 10.0 * gp,
            'gen_wgan': -l_fake, 'gen_ls': gen_ls, 'gen_total': ww * -l_fake + gen_ls}, g


LENGTHS = [(11, 1, 12), (2, 12)]        # (2, 12): shorter than half a window


@pytest.mark.parametrize('lens', LENGTHS)
def test_the_rule_is_sufficient(lens):
    assert max(lens) == TMAX
    got, g = batched(lens, masked=True)
    for i, (n, want) in enumerate(zip(lens, lone(lens))):
        assert float(g[i, n:].abs().sum()) == 0.0, 'gradient behind the end of utterance {}'.format(i)
        for k, w in want.items():
            rel = float((got[k][i] - w).abs() / w.abs())
            print('lengths {} utterance {} (T = {}) {}: {:+.12e}, relative error {:.2e}'.format(lens, i, n, k, float(w), rel))
            assert rel <= 1e-10, '{} of utterance {}: {} against {}'.format(k, i, float(got[k][i]), float(w))


@pytest.mark.parametrize('lens', LENGTHS)
def test_the_batch_has_teeth(lens):
    """Without the masks every cost of every padded utterance is wrong, the penalty by more than 10 x the GPU bound."""
    got, _ = batched(lens, masked=False)
    for i, (n, want) in enumerate(zip(lens, lone(lens))):
        excess = {k: float((got[k][i] - w).abs() / (GPU_ATOL + GPU_RTOL * w.abs())) for k, w in want.items()}
        print('lengths {} utterance {} (T = {}): error / GPU bound {}'.format(
            lens, i, n, ', '.join('{} {:.1f}'.format(k, v) for k, v in excess.items())))
        if n == TMAX:
            assert max(excess.values()) < 1e-6                   # no padding: the same computation
        else:
            for k, w in want.items():
                rel = float((got[k][i] - w).abs() / w.abs())
                assert rel > 1e-6, '{} of utterance {} misses by {:.1e} relative only'.format(k, i, rel)
            for k in ('gp', 'norm', 'critic_total'):
                assert excess[k] > 10.0, '{} of utterance {} only {:.1f} x the GPU bound'.format(k, i, excess[k])
