"""Masked training, the rule itself (CPU, float64): a zero-padded batch X [B,T,ctx], Y [B,T,out] with n[b] real frames per row,
N = sum_b n[b].  The generator's TRAINING forward under the rule is tests/test_ragged_rule.py's masking (zeros at t >= n[b] in
front of every convolution, the BLSTM over each row's own length, the outputs masked once) plus BatchNormalization whose mean and
biased variance are taken over the real frames only (count N for [B,T,C], N*F for [B,T,F,C]; the moving statistics updated from
them, Bessel factor count / (count - 1) on the 4-D maps); the least-squares cost is sum_{b, t<n[b], d} (Y - pred)^2 w[d] / (N out).

`ragged_train_generator_forward` and `masked_lse` restate that from the oracle's primitives and a masked BatchNorm written here;
tests/test_ragged_train_gpu.py compares the device against them.

Sufficiency: with each layer's pooled statistics fed back as fixed affines, every utterance run ALONE gives the batch's real
frames (rtol 1e-10 / atol 1e-12), and the batch cost is the n[b]/N-weighted sum of the lone costs: what the rule computes on row
b is the network applied to utterance b with the batch's statistics.  With all n[b] = T the rule is the oracle's own training
forward and cost.

The critic (it has no BatchNormalization) under the rule is the masking alone, and the costs are `masked_critic_step_loss` and
`masked_generator_step_loss`: Wasserstein terms sign * sum_{b, t<n[b]} D / N, the penalty unchanged (per-sample norm over [T, out], whose
pad frames hold exact zeros, mean over B).  For a given fake sample the critic's cost and EVERY weight gradient equal the sums of the
lone ones -- the Wasserstein terms weighted n[b]/N, the penalties 1/B -- at the same bound, and the gradient with respect to x^ is
exactly zero on pad frames.

These tests restate the oracle and touch no code of the package, so they pass with or without the feature: they are the float64
reference the device tests (tests/test_ragged_train_gpu.py, which do fail without it) compare against, and the proof that it is the right one.

Teeth: the same padded batch through the unmasked oracle in training mode misses the cost and at least one weight gradient by more
than 100 times the GPU bounds (cost rtol 5e-4 / atol 1e-5; gradients rtol 2e-3 / atol 5e-5 gmax + 1e-6, those of
tests/test_model_gpu.py::test_critic_and_generator_steps).  Input seed 8, as in tests/test_ragged_rule.py; both geometries clear
the factor there."""
import functools

import pytest
import torch

from oracle import percival_oracle as O

import test_model_gpu as tm                                     # GEOMS only: nothing of it runs here
import test_ragged_rule as rr

GEOMS = ['test', 'nocnn']
LOSS_TOL = (5e-4, 1e-5)
GRAD_RTOL, GRAD_ATOL_REL, GRAD_ATOL = 2e-3, 5e-5, 1e-6


def frame_mask(x, lens):
    m = x.new_zeros(x.shape[0], x.shape[1])
    for i, n in enumerate(lens):
        m[i, :n] = 1
    return m.view(x.shape[0], x.shape[1], *([1] * (x.dim() - 2)))


def masked_bn(x, lens, gamma, beta, mm, mv, update=False, unbiased_moving=False, stats=None, record=None):
    """BatchNormalization in training mode over the real frames of x [B,T,..,C]; `stats` = (mean, var): these instead (a fixed
    affine); `record`: a list that receives (mean, var)."""
    C = x.shape[-1]
    if stats is None:
        m = frame_mask(x, lens)
        count = sum(lens) * (x[0, 0].numel() // C)
        if count < 2:
            raise ValueError('BatchNormalization over {} value per channel'.format(count))
        mean = (x * m).reshape(-1, C).sum(0) / count
        var = (((x - mean) * m) ** 2).reshape(-1, C).sum(0) / count
        if update:
            with torch.no_grad():
                mm.mul_(O.BN_MOMENTUM).add_((1 - O.BN_MOMENTUM) * mean)
                mv.mul_(O.BN_MOMENTUM).add_((1 - O.BN_MOMENTUM) * (var * count / (count - 1) if unbiased_moving else var))
    else:
        mean, var = stats
    if record is not None:
        record.append((mean.detach(), var.detach()))
    return gamma * (x - mean) / torch.sqrt(var + O.BN_EPS) + beta


def ragged_train_generator_forward(weights, a, ctx, lens, update_moving=False, stats=None, record=None):
    """oracle.generator_forward(training=True) under the rule.  `stats`: one (mean, var) per BatchNormalization layer, in the
    order the layers run, used as fixed affines; `record` collects what each layer used."""
    take = O._Take(weights)
    B, T = ctx.shape[0], ctx.shape[1]
    m = lambda x: rr.zero_pad_rows(x, lens)
    stats = list(stats) if stats is not None else None

    def bnl(x, fused4d=False):
        g, bt, mm, mv = take(4)
        return O.lrelu(masked_bn(x, lens, g, bt, mm, mv, update_moving, fused4d, stats.pop(0) if stats is not None else None, record))

    h = ctx
    for _ in range(a.nctx):
        h = bnl(O.conv1d_ntc(m(h), take()))
    for _ in range(2):
        h = bnl(O.dense(h, take()))
    W, U, b = take(3)
    f0 = torch.cat([torch.cat([O.blstm(h[i:i + 1, :n], W, U, b), h.new_zeros(1, T - n, 2 * a.H)], dim=1) for i, n in enumerate(lens)])
    w, b = take(2)
    f0 = O.dense(f0, w, b)
    w, b = take(2)
    s = O.dense(h, w, b).reshape(B, T, a.specsize, 1)
    for li in range(a.L):
        if a.gated:
            dil = a.dilations[li % len(a.dilations)] if a.dilations else 1
            wa, wb = take(2)
            s = bnl(O.pgcnn2d_product(m(s), wa, wb, dil, a.causal), fused4d=True)
        else:
            s = bnl(O.conv2d_nhwc(m(s), take()), fused4d=True)
    w, b = take(2)
    s = O.conv2d_nhwc(m(s), w, b, causal=bool(a.gated and a.causal)).reshape(B, T, a.specsize)
    n_ = h
    for _ in range(a.L // 2):
        n_ = bnl(O.dense(n_, take()))
    w, b = take(2)
    n_ = torch.sigmoid(O.dense(n_, w, b))
    take.done()
    return m(torch.cat([f0, s, n_], dim=-1))


def masked_lse(y, pred, w, lens):
    """sum_{b, t<n[b], d} (y - pred)^2 w[d] / (N D)"""
    return (((y - pred) ** 2) * w * frame_mask(y, lens)).sum() / (sum(lens) * y.shape[-1])


@functools.lru_cache(maxsize=None)
def train_batch(geom, seed=8):
    """(arch, weights, zero-padded X, zero-padded Y, cost weights w [out], lengths); float64, shared, nobody writes to it."""
    a, gw, xs, xpad, lens = rr.batch(geom, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    Y = rr.zero_pad_rows(torch.randn(len(lens), max(lens), a.outsize, generator=gen, dtype=torch.float64), lens)
    w = torch.rand(a.outsize, generator=gen, dtype=torch.float64) + 0.5
    return a, gw, xpad, Y, w, lens


def cost_and_gradients(geom, masked):
    a, gw, X, Y, w, lens = train_batch(geom)
    ws = [t.clone().requires_grad_(t.is_floating_point()) for t in gw]
    if masked:
        loss = masked_lse(Y, ragged_train_generator_forward(ws, a, X, lens), w, lens)
    else:
        loss = O.specweighted_lse_loss(Y, O.generator_forward(ws, a, X, training=True), w)
    grads = torch.autograd.grad(loss, [t for t in ws if t.requires_grad], allow_unused=True)
    return loss.detach(), [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, [t for t in ws if t.requires_grad])]


@pytest.mark.parametrize('geom', GEOMS)
def test_the_rule_is_sufficient(geom):
    a, gw, X, Y, w, lens = train_batch(geom)
    assert lens == [X.shape[1], X.shape[1] - 1, 3, 1]
    N = sum(lens)
    with torch.no_grad():
        record = []
        got = ragged_train_generator_forward([t.clone() for t in gw], a, X, lens, record=record)
        total = masked_lse(Y, got, w, lens)
        lone_sum = 0.0
        for i, n in enumerate(lens):
            alone = ragged_train_generator_forward([t.clone() for t in gw], a, X[i:i + 1, :n], [n], stats=record)
            torch.testing.assert_close(got[i, :n], alone[0], rtol=1e-10, atol=1e-12)
            assert float(got[i, n:].abs().sum()) == 0.0
            lone_sum = lone_sum + n / N * O.specweighted_lse_loss(Y[i:i + 1, :n], alone, w)
        torch.testing.assert_close(total, lone_sum, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('geom', GEOMS)
def test_full_lengths_are_the_oracles_training_forward(geom):
    a, gw, X, Y, w, _ = train_batch(geom)
    B, T = X.shape[0], X.shape[1]
    g = torch.Generator().manual_seed(3)
    X = torch.rand(X.shape, generator=g, dtype=torch.float64) * 2 - 1
    Y = torch.randn(Y.shape, generator=g, dtype=torch.float64)
    wa, wb = [t.clone() for t in gw], [t.clone() for t in gw]
    with torch.no_grad():
        got = ragged_train_generator_forward(wa, a, X, [T] * B, update_moving=True)
        want = O.generator_forward(wb, a, X, training=True, update_moving=True)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12)
    for p, q in zip(wa, wb):                                   # the moving statistics, updated in place
        torch.testing.assert_close(p, q, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(masked_lse(Y, got, w, [T] * B), O.specweighted_lse_loss(Y, want, w), rtol=1e-12, atol=1e-14)


def test_a_single_real_value_per_channel_is_refused():
    x = torch.zeros(1, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        masked_bn(x, [1], torch.ones(2), torch.zeros(2), torch.zeros(2), torch.ones(2))


@pytest.mark.parametrize('geom', GEOMS)
def test_the_inputs_have_teeth(geom):
    """Without the rule the padded batch misses the cost and at least one gradient tensor by more than 100 x the GPU bounds."""
    loss_m, grads_m = cost_and_gradients(geom, True)
    loss_u, grads_u = cost_and_gradients(geom, False)
    lx = float((loss_u - loss_m).abs() / (LOSS_TOL[1] + LOSS_TOL[0] * loss_m.abs()))
    gmax = max(float(g.abs().max()) for g in grads_m)
    gx = [float(((u - m_).abs() / (GRAD_ATOL_REL * gmax + GRAD_ATOL + GRAD_RTOL * m_.abs())).max()) for u, m_ in zip(grads_u, grads_m)]
    print('{}: cost {:.6f} masked, {:.6f} unmasked: {:.0f} x the GPU bound; worst gradient tensor {:.0f} x, {} of {} tensors beyond 100 x'.format(
        geom, float(loss_m), float(loss_u), lx, max(gx), sum(x > 100.0 for x in gx), len(gx)))
    assert lx > 100.0
    assert max(gx) > 100.0


# ---------------------------------------------------------------------------------------------------------------------------
# the critic and the two steps' costs under the rule
# ---------------------------------------------------------------------------------------------------------------------------
def masked_critic_forward(weights, a, features, ctx, lens):
    """oracle.critic_forward with rows t >= n[b] zeroed in front of every convolution and in the scores."""
    take = O._Take(weights)
    B, T = features.shape[0], features.shape[1]
    m = lambda x: rr.zero_pad_rows(x, lens)
    spec = features[:, :, 1:1 + a.specsize]
    if a.L > 0:
        h = spec.reshape(B, T, a.specsize, 1)
        for _ in range(a.L):
            w, b = take(2)
            h = O.lrelu(O.conv2d_nhwc(m(h), w, b))
        h = h.reshape(B, T, a.specsize * a.C)
    else:
        h = spec
        for _ in range(3):
            w, b = take(2)
            h = O.lrelu(O.dense(h, w, b))
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


def masked_mean(v, lens, sign):
    """sign * sum_{b, t<n[b]} v / (N * elements per frame)"""
    return sign * (v * frame_mask(v, lens)).sum() / (sum(lens) * v[0, 0].numel())


def masked_critic_step_loss(cw, gw, a, X, Y, alpha, lens, gp_lambda=10.0, fake=None):
    """oracle.critic_step_loss(training=True) under the rule; `fake`: a given sample instead of the frozen generator's."""
    if fake is None:
        with torch.no_grad():
            fake = ragged_train_generator_forward([t.clone() for t in gw], a, X, lens)      # masked statistics, no moving update
    valid = masked_critic_forward(cw, a, Y, X, lens)
    fake_v = masked_critic_forward(cw, a, fake, X, lens)
    x_hat = O.random_weighted_average(Y, fake, alpha).detach().requires_grad_(True)
    v_hat = masked_critic_forward(cw, a, x_hat, X, lens)
    gp, g = O.gradient_penalty_loss(v_hat, x_hat)
    l_valid, l_fake = masked_mean(valid, lens, -1.0), masked_mean(fake_v, lens, +1.0)
    return l_valid + l_fake + gp_lambda * gp, {'valid': l_valid, 'fake': l_fake, 'gp': gp, 'g': g, 'fake_sample': fake}


def masked_generator_step_loss(cw, gw, a, X, Y, lens, errtype='WLSWGAN', w_ls=None, wgan_weight=1.0, update_moving=True):
    """oracle.generator_step_loss(training=True) under the rule."""
    pred = ragged_train_generator_forward(gw, a, X, lens, update_moving=update_moving)
    l_w = masked_mean(masked_critic_forward(cw, a, pred, X, lens), lens, -1.0)
    if errtype == 'WGAN':
        return l_w, {'wgan': l_w, 'pred': pred}
    l_ls = masked_lse(Y, pred, w_ls, lens)
    return wgan_weight * l_w + l_ls, {'wgan': l_w, 'ls': l_ls, 'pred': pred}


@pytest.mark.parametrize('geom', GEOMS)
def test_the_critics_cost_and_gradients_are_the_weighted_lone_ones(geom):
    a, gw, X, Y, w, lens = train_batch(geom)
    B, N = len(lens), sum(lens)
    cw = O.random_weights(O.critic_weight_shapes(a), seed=12)
    al = torch.rand(B, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        fake = ragged_train_generator_forward([t.clone() for t in gw], a, X, lens)
    ws = [t.clone().requires_grad_(True) for t in cw]
    total, parts = masked_critic_step_loss(ws, gw, a, X, Y, al, lens, fake=fake)
    grads = torch.autograd.grad(total, ws)
    for i, n in enumerate(lens):
        assert float(parts['g'][i, n:].abs().sum()) == 0.0, 'gradient with respect to x^ behind the end of row {}'.format(i)
    lone_total, lone_grads = 0.0, [torch.zeros_like(t) for t in cw]
    for i, n in enumerate(lens):
        wl = [t.clone().requires_grad_(True) for t in cw]
        _, p = masked_critic_step_loss(wl, gw, a, X[i:i + 1, :n], Y[i:i + 1, :n], al[i:i + 1], [n], fake=fake[i:i + 1, :n])
        # alone the row IS the oracle's critic step on that utterance
        v1, f1 = O.critic_forward(cw, a, Y[i:i + 1, :n], X[i:i + 1, :n]), O.critic_forward(cw, a, fake[i:i + 1, :n], X[i:i + 1, :n])
        torch.testing.assert_close(p['valid'], O.wasserstein_loss(-1.0, v1), rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(p['fake'], O.wasserstein_loss(+1.0, f1), rtol=1e-10, atol=1e-12)
        part = n / N * (p['valid'] + p['fake']) + 10.0 / B * p['gp']
        lone_total = lone_total + part.detach()
        for acc, g_ in zip(lone_grads, torch.autograd.grad(part, wl)):
            acc += g_
    torch.testing.assert_close(total.detach(), lone_total, rtol=1e-10, atol=1e-12)
    for k, (g_, want) in enumerate(zip(grads, lone_grads)):
        torch.testing.assert_close(g_, want, rtol=1e-10, atol=1e-12, msg=lambda m_: 'critic weight {}: {}'.format(k, m_))


@pytest.mark.parametrize('geom', GEOMS)
def test_full_lengths_are_the_oracles_steps(geom):
    a, gw, X, Y, w, _ = train_batch(geom)
    B, T = X.shape[0], X.shape[1]
    g = torch.Generator().manual_seed(6)
    X = torch.rand(X.shape, generator=g, dtype=torch.float64) * 2 - 1
    Y = torch.randn(Y.shape, generator=g, dtype=torch.float64)
    al = torch.rand(B, generator=g, dtype=torch.float64)
    cw = O.random_weights(O.critic_weight_shapes(a), seed=12)
    full = [T] * B
    t0, p0 = O.critic_step_loss(cw, gw, a, X, Y, al)
    t1, p1 = masked_critic_step_loss(cw, gw, a, X, Y, al, full)
    torch.testing.assert_close(t1.detach(), t0.detach(), rtol=1e-10, atol=1e-12)
    with torch.no_grad():
        g0, _ = O.generator_step_loss(cw, [t.clone() for t in gw], a, X, Y, 'WLSWGAN', w, 0.7)
        g1, _ = masked_generator_step_loss(cw, [t.clone() for t in gw], a, X, Y, full, 'WLSWGAN', w, 0.7)
    torch.testing.assert_close(g1, g0, rtol=1e-10, atol=1e-12)
