"""The kernels of masked training (a zero-padded batch [B,T,...] with a length per row), each against a float64 restatement.

  ptts_colstats_rows                  sums over the real frames only; pad frames of the input hold NaN (they are never read)
  ptts_affine_act_rows_bwd_params     dx as ptts_affine_act_rows_bwd (bit for bit) + the fp64 (dscale, dshift) sums over real frames
  ptts_axpby_cols_rows                the statistics' share of the BatchNorm backward on real frames, +0 behind them; in place
  ptts_rows_combine, ptts_rows_mean_bwd, ptts_wlse_rows_bwd   the batch costs out of the per-row ones, and their gradients
  ops.affine_act_rows(train=True)     first- and second-order gradients (the gradient penalty's sweep through a mask)
  ops.batchnorm_affine(lengths, count)  masked statistics, moving statistics, all three gradients
  ptts_lstm_bwd_ragged, ptts_gru_bwd_ragged (and ops.lstm / ops.gru with lengths)   every row over its own length: h, dgates, dx, dW,
                                      dU, db against the float64 oracle run on each row alone, at the bounds at the head of
                                      tests/test_lstm.py and tests/test_gru.py; B = 4, T = 12, NaN on the pad frames of gates, cell
                                      states and dh; every step-kernel path of the LSTM (H = 5, 48, 64, 192, 256), the GRU widths
                                      of tests/test_gru.py; one and two directions, a reversed single direction

Shapes: [4, 12, C] with C = 3 (scalar path), 4 and 256 (float4 path; one element off a 16-byte boundary: scalar path), and the
Conv2D map [3, 9, 5, 4]; lengths [T, T-1, 3, 1] ([T, 2, 1] for the map): a full row, a row one short, a short row, a single frame.

Bounds.  colstats_rows adds fp32 values and their exact squares in fp64: rtol 1e-6 / atol 1e-6 of the fp64 sums of the same fp32
input, as tests/test_lstm.py::test_column_sums_beyond_2048_columns states for column sums.  The (dscale, dshift) sums add fp32 TERMS
(dy d and dy d x: one and two roundings of 2^-24) that cancel, in fp32 runs of at most 16 rows on the float4 path: 1e-6 of the sum
plus 20 x 2^-24 x the sum of the terms' magnitudes.  dx: tests/test_elementwise.py's rtol 1e-4 / atol 1e-5 for ptts_affine_act_bwd.
axpby_cols_rows: that file's 4 x 2^-24 x (|c0| + |a| + |x c2|) for ptts_axpby_cols.  The loss gradients are a handful of fp32
products of exact inputs: 8 x 2^-24 relative, no absolute term.  The batch costs: two fp32 roundings (the per-row mean, the
result) around an fp64 sum: 4 x 2^-24 x sum_b |row_b| n_b / N.  Pad frames of every gradient: the bits of +0.0f.
"""
import numpy as np
import pytest
import torch

import test_elementwise as te
import test_gru as tg
import test_lstm as tl
from test_elementwise import ALPHA, AT, RT, U32, Guard, check, dev, gen, intact, r32, rand32, randn32

pytestmark = pytest.mark.gpu

SUM_TOL = (1e-6, 1e-6)
CASES = [((4, 12, 3), 0), ((4, 12, 4), 0), ((4, 12, 4), 1), ((4, 12, 256), 0), ((4, 12, 256), 1), ((3, 9, 5, 4), 0), ((3, 9, 5, 4), 1)]
IDS = ['x'.join(map(str, s)) + ('+1' if o else '') for s, o in CASES]


def lengths_of(shape):
    T = shape[1]
    return [T, T - 1, 3, 1] if shape[0] == 4 else [T, 2, 1]


def real_mask(shape, lens):
    """float64 [B, T, 1...]: 1 on real frames"""
    m = torch.zeros(shape[0], shape[1], dtype=torch.float64)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m.view(shape[0], shape[1], *([1] * (len(shape) - 2)))


def with_nan_pads(x, m):
    return torch.where(m.expand_as(x) > 0, x, torch.full_like(x, float('nan')))


def ilens(lens):
    return torch.tensor(lens, dtype=torch.int32, device='cuda')


def pads_are_plus_zero(t, m, what):
    bits = t.detach().contiguous().view(torch.int32).cpu()
    assert bool((bits[(m.expand(t.shape) == 0)] == 0).all()), '{}: a pad frame is not +0.0'.format(what)


def _inputs(shape, seed):
    g = gen(seed)
    C = shape[-1]
    x, dy, a = (randn32(g, *shape) for _ in range(3))
    return x, dy, a, r32(rand32(g, C) + 0.5), randn32(g, C) * 0.3


def _dims(shape):
    B, T, C = shape[0], shape[1], shape[-1]
    return B, T, int(np.prod(shape[2:])), C


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_colstats_rows(case):
    ops, call, P, S, lib = te._api()
    shape, off = case
    B, T, inner, C = _dims(shape)
    lens = lengths_of(shape)
    m = real_mask(shape, lens)
    x = _inputs(shape, 7)[0]
    xd, ld = dev(with_nan_pads(x, m), off), ilens(lens)
    nws = lib.ptts_colstats_rows_workspace_bytes(B, T, inner, C)
    assert nws == lib.ptts_colstats_workspace_bytes(B * T * inner // C, C) > 0
    got = []
    for _ in range(2):
        sums, ws = Guard(2 * C, torch.float64), Guard(nws, torch.uint8)
        call('ptts_colstats_rows', P(xd), P(ld), B, T, inner, C, P(sums.t), P(ws.t), ws.n, S())
        intact('colstats_rows {}'.format(case), sums, ws)
        got.append(sums.t.clone())
    xm = (x * m).reshape(-1, C)
    check(got[0][:C], xm.sum(0), SUM_TOL, 'colstats_rows {} sum'.format(case))
    check(got[0][C:], (xm * xm).sum(0), SUM_TOL, 'colstats_rows {} sumsq'.format(case))
    assert torch.equal(got[0], got[1]), 'colstats_rows {}: two calls differ'.format(case)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_affine_act_rows_bwd_params(case):
    ops, call, P, S, lib = te._api()
    shape, off = case
    B, T, inner, C = _dims(shape)
    lens = lengths_of(shape)
    m = real_mask(shape, lens)
    x, dy, _, sc, sh = _inputs(shape, 11)
    xd, dyd, scd, shd, ld = dev(with_nan_pads(x, m), off), dev(with_nan_pads(dy, m), off), dev(sc), dev(sh), ilens(lens)
    nws = lib.ptts_colstats_rows_workspace_bytes(B, T, inner, C)
    for act, affine in ((None, True), ('lrelu', True), ('lrelu', False), (None, False)):
        code = te.ACTS[act]
        s_, h_ = (sc, sh) if affine else (None, None)
        sd_, hd_ = (scd, shd) if affine else (None, None)
        x2, dy2, m2 = x.reshape(-1, C), dy.reshape(-1, C), m.expand(shape).reshape(-1, C)
        d = torch.ones_like(x2)
        if act == 'lrelu':            # the mask at the float32 pre-activation, where the kernel's function has its kink (act_bwd_ref)
            p32 = x2.to(torch.float32) * sc.to(torch.float32) + sh.to(torch.float32) if affine else x2.to(torch.float32)
            d = torch.where(p32 > 0, 1.0, ALPHA).to(torch.float64)
        gd = dy2 * d * m2             # the terms of dshift; gd x those of dscale
        dxr = gd * s_ if affine else gd
        tag = 'affine_act_rows_bwd_params {} {} {}'.format(act, 'affine' if affine else 'plain', case)
        got = []
        for _ in range(2):
            dx, dsums, ws = Guard(x.numel(), off=off), Guard(2 * C, torch.float64), Guard(nws, torch.uint8)
            call('ptts_affine_act_rows_bwd_params', P(dyd), P(xd), P(sd_), P(hd_), P(dx.t), P(dsums.t), P(ld), P(ws.t), ws.n,
                 B, T, inner, C, code, ALPHA, S())
            intact(tag, dx, dsums, ws)
            got.append((dx.t.clone().view(shape), dsums.t.clone()))
        dxg, ds = got[0]
        check(dxg, dxr.view(shape), (RT, AT), tag + ' dx')
        pads_are_plus_zero(dxg, m, tag + ' dx')
        check(ds[:C], (gd * x2).sum(0), 1e-6 * (gd * x2).sum(0).abs() + 20 * U32 * (gd * x2).abs().sum(0), tag + ' dscale')
        check(ds[C:], gd.sum(0), 1e-6 * gd.sum(0).abs() + 20 * U32 * gd.abs().sum(0), tag + ' dshift')
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), tag + ': two calls differ'
        # dx is ptts_affine_act_rows_bwd's, bit for bit
        dx1 = Guard(x.numel(), off=off)
        call('ptts_affine_act_rows_bwd', P(dyd), P(xd), P(sd_), P(hd_), P(dx1.t), P(ld), B, T, inner, C, code, ALPHA, S())
        assert torch.equal(dx1.t.view(shape), dxg), tag + ': dx differs from ptts_affine_act_rows_bwd'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_axpby_cols_rows(case):
    ops, call, P, S, lib = te._api()
    shape, off = case
    B, T, inner, C = _dims(shape)
    lens = lengths_of(shape)
    m = real_mask(shape, lens)
    x, _, a, c2, c0 = _inputs(shape, 13)
    xd, ad, c2d, c0d, ld = dev(with_nan_pads(x, m), off), dev(with_nan_pads(a, m), off), dev(c2), dev(c0), ilens(lens)
    want = (a + x * c2 + c0) * m
    bound = 4 * U32 * (a.abs() + (x * c2).abs() + c0.abs().expand(shape)) * m
    got = []
    for _ in range(2):
        out = Guard(x.numel(), off=off)
        call('ptts_axpby_cols_rows', P(ad), P(xd), P(c2d), P(c0d), P(out.t), P(ld), B, T, inner, C, S())
        intact('axpby_cols_rows {}'.format(case), out)
        got.append(out.t.clone().view(shape))
    check(got[0], want, bound, 'axpby_cols_rows {}'.format(case))
    pads_are_plus_zero(got[0], m, 'axpby_cols_rows {}'.format(case))
    assert torch.equal(got[0], got[1]), 'axpby_cols_rows {}: two calls differ'.format(case)
    call('ptts_axpby_cols_rows', P(ad), P(xd), P(c2d), P(c0d), P(ad), P(ld), B, T, inner, C, S())       # out == a
    assert torch.equal(ad, got[0]), 'axpby_cols_rows {}: in place differs'.format(case)


@pytest.mark.parametrize('with_w', [False, True], ids=['plain', 'weighted'])
def test_masked_costs_and_their_gradients(with_w):
    ops, call, P, S, lib = te._api()
    shape = (4, 12, 7)
    B, T, D = shape
    lens = lengths_of(shape)
    N = sum(lens)
    m = real_mask(shape, lens)
    g = gen(17)
    y, yhat, v = randn32(g, *shape), randn32(g, *shape), randn32(g, *shape)
    w = r32(rand32(g, D) + 0.5) if with_w else None
    up = 1.7
    ld, wd = ilens(lens), dev(w)
    w1 = w if with_w else torch.ones(D, dtype=torch.float64)
    # least squares
    yh = dev(with_nan_pads(yhat, m)).requires_grad_(True)
    loss = ops.masked_wlse(dev(with_nan_pads(y, m)), yh, wd, ld, N)
    (loss * up).backward()
    sq = ((y - yhat) ** 2 * w1 * m)
    rows = r32(torch.stack([sq[b, :n].sum() / (n * D) for b, n in enumerate(lens)]))
    check(loss, sq.sum() / (N * D), 4 * U32 * sum(float(rows[b].abs()) * n for b, n in enumerate(lens)) / N * torch.ones(1), 'masked_wlse')
    want = r32(torch.tensor(up)) * 2 * (yhat - y) * w1 / (N * D) * m
    check(yh.grad, want, 8 * U32 * want.abs(), 'masked_wlse dyhat')
    pads_are_plus_zero(yh.grad, m, 'masked_wlse dyhat')
    # Wasserstein terms, both signs; inner = 7 (a critic's [B,T,1] map is the case inner = 1)
    for sign in (1.0, -1.0):
        vd = dev(with_nan_pads(v, m)).requires_grad_(True)
        loss = ops.masked_mean(vd, ld, N, sign)
        (loss * up).backward()
        rows = r32(torch.stack([sign * v[b, :n].sum() / (n * D) for b, n in enumerate(lens)]))
        check(loss, sign * (v * m).sum() / (N * D), 4 * U32 * sum(float(rows[b].abs()) * n for b, n in enumerate(lens)) / N * torch.ones(1),
              'masked_mean {}'.format(sign))
        want = r32(torch.tensor(up)) * sign / (N * D) * m.expand(shape)
        check(vd.grad, want, 8 * U32 * want.abs(), 'masked_mean dv {}'.format(sign))
        pads_are_plus_zero(vd.grad, m, 'masked_mean dv')
    # the critic's shape, scalar store path, no upstream: sign / N on real frames
    dv = Guard(B * T)
    call('ptts_rows_mean_bwd', None, P(ld), B, T, 1, -1.0, N, P(dv.t), S())
    intact('rows_mean_bwd', dv)
    want = -1.0 / N * m.view(B, T)
    check(dv.t.view(B, T), want, 8 * U32 * want.abs(), 'rows_mean_bwd inner=1')
    # with every length T these are the dense costs
    full = ilens([T] * B)
    for got, ref in ((ops.masked_wlse(dev(y), dev(yhat), wd, full, B * T), ops.wlse(dev(yhat), dev(y), wd)),
                     (ops.masked_mean(dev(v), full, B * T, -1.0), ops.wasserstein(dev(v), -1.0))):
        check(got, ref, (RT, AT), 'full lengths against the dense cost')
    with pytest.raises(ValueError):
        ops.masked_mean(dev(v), ld, B * T + 1, 1.0)


@pytest.mark.parametrize('case', [CASES[0], CASES[1], CASES[5]], ids=[IDS[0], IDS[1], IDS[5]])
def test_affine_act_rows_training_gradients_first_and_second_order(case):
    """y = mask(lrelu(x scale + shift)): gradients for x, scale and shift, and the gradient of |dL/dx|^2 with respect to what came
    in from above (the gradient penalty differentiates the critic's input gradient once more), against float64 autograd."""
    ops, call, P, S, lib = te._api()
    shape, off = case
    lens = lengths_of(shape)
    m = real_mask(shape, lens)
    x, dy, _, sc, sh = _inputs(shape, 19)
    p32 = x.to(torch.float32) * sc.to(torch.float32) + sh.to(torch.float32)
    far = (p32.abs() > 1e-3).to(torch.float64)                 # keep the float32 and float64 pre-activations on one side of the kink
    x = r32(x * far + (1 - far) * (1.0 - sh) / sc)
    ld = ilens(lens)

    def run(mk, mask, where):
        xs, ss, hs, ws = (mk(t).requires_grad_(True) for t in (x, sc, sh, dy))
        if where == 'dev':
            yv = ops.affine_act_rows(ops.Lazy(xs, ss, hs, lrelu=True, alpha=ALPHA), ld, train=True)
        else:
            p = xs * ss + hs
            yv = torch.where(p > 0, p, ALPHA * p) * mask
        L = (yv * ws).sum()
        L.backward(retain_graph=True)
        first = [t.grad.clone() for t in (xs, ss, hs)]
        # the second sweep with the affine as a constant (the critic's masks carry none): d |dL/dx|^2 / d(what came in from above)
        if where == 'dev':
            L = (ops.affine_act_rows(ops.Lazy(xs, ss.detach(), hs.detach(), lrelu=True, alpha=ALPHA), ld, train=True) * ws).sum()
        else:
            p = xs * ss.detach() + hs.detach()
            L = (torch.where(p > 0, p, ALPHA * p) * mask * ws).sum()
        gx, = torch.autograd.grad(L, xs, create_graph=True)
        ws.grad = None
        (gx * gx).sum().backward()
        return yv.detach(), first, ws.grad, gx.detach()
    yr, fr, sr, gxr = run(lambda t: t.clone(), m, 'ref')
    yd, fd, sd, gxd = run(lambda t: dev(t), None, 'dev')
    check(yd, yr, (RT, AT), 'train mask {} y'.format(case))
    check(fd[0], fr[0], (RT, AT), 'train mask {} dx'.format(case))
    C = shape[-1]
    gd = (dy * torch.where(x * sc + sh > 0, 1.0, ALPHA) * m).reshape(-1, C)          # the terms of dshift; gd x those of dscale
    for k, name, terms in ((1, 'dscale', gd * x.reshape(-1, C)), (2, 'dshift', gd)):
        # the fp64 sums' bound (see the head of the file) and their one rounding to float32
        check(fd[k], fr[k], 2e-6 * fr[k].abs() + 20 * U32 * terms.abs().sum(0), 'train mask {} {}'.format(case, name))
    check(sd, sr, (RT, AT), 'train mask {} second order'.format(case))
    pads_are_plus_zero(fd[0], m, 'train mask dx')
    pads_are_plus_zero(gxd, m, 'train mask input gradient')
    pads_are_plus_zero(sd, m, 'train mask second-order gradient')
    # an affine that wants its share of the second sweep is refused, not dropped
    xs, ss, hs, ws = (dev(t).requires_grad_(True) for t in (x, sc, sh, dy))
    L = (ops.affine_act_rows(ops.Lazy(xs, ss, hs, lrelu=True, alpha=ALPHA), ld, train=True) * ws).sum()
    gx, = torch.autograd.grad(L, xs, create_graph=True)
    with pytest.raises(NotImplementedError):
        (gx * gx).sum().backward()


@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_batchnorm_affine_with_lengths(case):
    """ops.batchnorm_affine(lengths, count) + the masked LeakyReLU behind it against a float64 BatchNormalization over the real
    frames written here: output, moving statistics (Bessel factor from the masked count on the 4-D map, as fused4d asks), and the
    gradients of z, gamma and beta at the dense layer's bounds (tests/test_ops_gpu.py::test_batchnorm_train_and_infer).  The
    gradient of z is +0 on pad frames, whose z holds NaN."""
    ops, call, P, S, lib = te._api()
    shape, off = case
    C = shape[-1]
    lens = lengths_of(shape)
    m = real_mask(shape, lens)
    count = sum(lens) * int(np.prod(shape[2:])) // C
    g = gen(23)
    z = r32(torch.randn(*shape, generator=g, dtype=torch.float64) * 2 + 0.7)
    gamma, beta, dy = r32(rand32(g, C) + 0.5), randn32(g, C), randn32(g, *shape)
    fused4d = len(shape) == 4
    zr, gr, br = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    me = m.expand(shape)
    mean = (zr * me).reshape(-1, C).sum(0) / count
    var = (((zr - mean) * me) ** 2).reshape(-1, C).sum(0) / count
    p = (zr - mean) / torch.sqrt(var + te.EPS) * gr + br
    yr = torch.where(p > 0, p, ALPHA * p) * me
    yr.backward(dy)
    mm = torch.zeros(C, dtype=torch.float64) * te.MOM + mean.detach() * (1 - te.MOM)
    mv = torch.ones(C, dtype=torch.float64) * te.MOM + var.detach() * (count / (count - 1.0) if fused4d else 1.0) * (1 - te.MOM)
    zd, gd, bd = (dev(t).requires_grad_(True) for t in (with_nan_pads(z, m), gamma, beta))
    mmd, mvd, ld = dev(torch.zeros(C)), dev(torch.ones(C)), ilens(lens)
    zt, sc, sh = ops.batchnorm_affine(zd, gd, bd, mmd, mvd, True, True, fused4d, lengths=ld, count=count)
    yd = ops.affine_act_rows(ops.Lazy(zt, sc, sh, lrelu=True, alpha=ALPHA), ld, train=True)
    check(yd, yr, (RT, AT), 'masked bn {} y'.format(case))
    yd.backward(dev(with_nan_pads(dy, m)))
    check(zd.grad, zr.grad, (3e-4, 3e-5), 'masked bn {} dz'.format(case))
    check(gd.grad, gr.grad, (3e-4, 1e-4), 'masked bn {} dgamma'.format(case))
    check(bd.grad, br.grad, (3e-4, 1e-4), 'masked bn {} dbeta'.format(case))
    check(mmd, mm, (RT, AT), 'masked bn {} moving mean'.format(case))
    check(mvd, mv, (RT, AT), 'masked bn {} moving variance'.format(case))
    pads_are_plus_zero(zd.grad, m, 'masked bn dz')
    with pytest.raises(ValueError):
        ops.batchnorm_affine(zd.detach(), gd, bd, mmd, mvd, True, lengths=ld, count=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the recurrences: every row over its own length, forward and backward
# ---------------------------------------------------------------------------------------------------------------------------
RB, RT_, RIN = 4, 12, 6                       # batch, padded length, input width of the recurrence cases
RLENS = [RT_, RT_ - 1, 3, 1]


def _rows_reference(kind, x, W, U, b, dh, nd, reverse=False):
    """float64, every row ALONE over its own length: (h, dgates, dx, dW, dU, db, kinks), zero on pad frames.  The recurrence runs
    on the input projection xp = x.W + b as a leaf through identity input weights, so xp.grad is the gradient of the gate
    pre-activations; dx, dW and db follow from it as the products they are, dU comes from autograd."""
    B, T, G = x.shape[0], x.shape[1], (4 if kind == 'lstm' else 3) * U.shape[1]
    Wc = W if kind == 'lstm' else torch.cat([W[d] for d in range(nd)], dim=1)          # [In, nd*G]
    xp = (x @ Wc + b.reshape(-1)).detach().requires_grad_(True)
    Ur = U.clone().requires_grad_(True)
    eye = torch.eye(nd * G, dtype=torch.float64)
    h = x.new_zeros(B, T, nd * U.shape[1])
    pre = []
    for i, n in enumerate(RLENS):
        if kind == 'lstm':
            hi = tl.oracle(xp[i:i + 1, :n], eye, Ur, torch.zeros(nd * G, dtype=torch.float64), reverse=reverse)
        else:
            hi = tg.gru_ref(xp[i:i + 1, :n], torch.stack([eye[:, d * G:(d + 1) * G] for d in range(nd)]), Ur,
                            torch.zeros(nd, G, dtype=torch.float64), pre=pre)
        hi.backward(dh[i:i + 1, :n])
        h[i, :n] = hi.detach()[0]
    dg = xp.grad
    m = real_mask((B, T, 1), RLENS)
    assert float((dg * (1 - m)).abs().sum()) == 0.0
    dg2, x2 = dg.reshape(B * T, nd * G), x.reshape(B * T, -1)
    dW = x2.t() @ dg2
    if kind == 'gru':
        dW = torch.stack([dW[:, d * G:(d + 1) * G] for d in range(nd)])
    kinks = int(sum(int(((p.abs() - 2.5).abs() < 1e-5).sum()) for p in pre))
    return h, dg, dg @ Wc.t(), dW, Ur.grad, dg2.sum(0).reshape(b.shape), kinks


def _nan_pads_dev(t, m):
    t = t.clone()
    t[(m.expand(t.shape) == 0).cuda()] = float('nan')
    return t


@pytest.mark.parametrize('nd,reverse', [(2, False), (1, False), (1, True)])
@pytest.mark.parametrize('H', [5, 48, 64, 192, 256])          # scalar; MFMA; packed <4> (one and three chunks); packed, eight waves
def test_lstm_backward_over_each_rows_own_length(H, nd, reverse):
    ops, call, P, S, lib = te._api()
    x, W, U, b, dh = tl.rand_lstm(RB, RT_, RIN, H, nd)
    hr, dgr, dxr, dWr, dUr, dbr, _ = _rows_reference('lstm', x, W, U, b, dh, nd, reverse)
    m = real_mask((RB, RT_, 1), RLENS)
    ld = ilens(RLENS)
    tag = 'lstm H={} nd={} reverse={}'.format(H, nd, reverse)
    ds = [tl._dev(t, True) for t in (x, W, U, b)]
    dhd = _nan_pads_dev(tl._dev(dh), m)
    hd = ops.lstm(*ds, reverse=reverse, lengths=ld)
    tl.close(hd, hr, tl.H_TOL, 'h ' + tag)
    pads_are_plus_zero(hd, m, 'h ' + tag)
    hd.backward(dhd)
    for name, d, r in zip(('dx', 'dW', 'dU', 'db'), ds, (dxr, dWr, dUr, dbr)):
        tl.close(d.grad, r, tl.G_TOL[name], '{} {}'.format(name, tag))
    pads_are_plus_zero(ds[0].grad, m, 'dx ' + tag)
    # the kernel itself, with NaN on every pad frame of what it is given
    with torch.no_grad():
        h, c, gates = ops._lstm_rows_launch(ds[0].detach(), ds[1].detach(), ds[2].detach(), ds[3].detach(), ld, reverse, True)
    c, gates = _nan_pads_dev(c, m), _nan_pads_dev(gates, m)
    got = []
    for _ in range(2):
        dg, ws = Guard(gates.numel()), Guard(lib.ptts_lstm_bwd_workspace_bytes(RB, RT_, H, nd), torch.uint8)
        call('ptts_lstm_bwd_ragged', P(dhd), P(ds[2].detach()), P(gates), P(c), P(dg.t), P(ld), P(ws.t), ws.n, RB, RT_, H, nd,
             int(reverse), S())
        intact(tag, dg, ws)
        got.append(dg.t.clone().view(gates.shape))
    tl.close(got[0], dgr, tl.G_TOL['dx'], 'dgates ' + tag)              # dgates is dx through identity input weights
    pads_are_plus_zero(got[0], m, 'dgates ' + tag)
    assert torch.equal(got[0], got[1]), tag + ': two calls differ'


@pytest.mark.parametrize('nd', [1, 2])
@pytest.mark.parametrize('H', [4, 5, 64, 70, 256])            # the widths of tests/test_gru.py: padded tail tiles, whole tiles
def test_gru_backward_over_each_rows_own_length(H, nd):
    ops, call, P, S, lib = te._api()
    x, W, U, b = tg.rand_gru(RB, RT_, RIN, H, nd, seed=10)
    dh = torch.randn(RB, RT_, nd * H, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    hr, dgr, dxr, dWr, dUr, dbr, kinks = _rows_reference('gru', x, W, U, b, dh, nd)
    m = real_mask((RB, RT_, 1), RLENS)
    ld = ilens(RLENS)
    tag = 'gru H={} nd={}'.format(H, nd)
    ds = [tg._dev(t, True) for t in (x, W, U, b)]
    dhd = _nan_pads_dev(tg._dev(dh), m)
    hd = ops.gru(*ds, lengths=ld)
    tg.close(hd, hr, 2e-4, 2e-5, 'h ' + tag)
    pads_are_plus_zero(hd, m, 'h ' + tag)
    hd.backward(dhd)
    for name, d, r in zip(('dx', 'dW', 'dU', 'db'), ds, (dxr, dWr, dUr, dbr)):
        assert bool(torch.isfinite(d.grad).all()), '{} {}: not finite'.format(name, tag)
        tg.close(d.grad, r, 3e-4, 2e-4, '{} {}'.format(name, tag), kinks)
    pads_are_plus_zero(ds[0].grad, m, 'dx ' + tag)
    with torch.no_grad():
        h, gates, rh = ops._gru_rows_launch(ds[0].detach(), ds[1].detach(), ds[2].detach(), ds[3].detach(), ld, True)
    h, gates = _nan_pads_dev(h, m), _nan_pads_dev(gates, m)
    got = []
    for _ in range(2):
        dg, ws = Guard(gates.numel()), Guard(lib.ptts_gru_bwd_workspace_bytes(RB, RT_, H, nd), torch.uint8)
        call('ptts_gru_bwd_ragged', P(dhd), P(ds[2].detach()), P(h), P(gates), P(dg.t), P(ld), P(ws.t), ws.n, RB, RT_, H, nd, S())
        intact(tag, dg, ws)
        got.append(dg.t.clone().view(gates.shape))
    tg.close(got[0], dgr, 3e-4, 2e-4, 'dgates ' + tag, kinks)
    pads_are_plus_zero(got[0], m, 'dgates ' + tag)
    assert torch.equal(got[0], got[1]), tag + ': two calls differ'
