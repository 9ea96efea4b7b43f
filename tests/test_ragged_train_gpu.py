"""Masked training on the device against the float64 restatement of tests/test_ragged_train_rule.py: the generator's training
forward on a zero-padded batch with a length per row (memo['lengths'] + memo['lengths_train'] = N), the least-squares step
OptimizerTTS.train_on_batch(..., lengths=) -- cost, every weight gradient, the moving statistics -- and the critic / generator
steps of OptimizerTTSWGAN: critic_loss(..., lengths) with injected alpha (parts, total, every gradient, x^'s gradient bitwise zero
on pad frames), generator_loss(..., lengths) for WLSWGAN and WGAN (parts, every gradient, moving statistics), and
device_step(..., lengths=) over 11 batches on the critic_runs schedule without a graph.  Critic gradients at that test's
1e-3 / 2e-5 gmax + 1e-6.

Geometries 'test' and 'nocnn' at B = 4 with lengths [T, T-1, 3, 1], 'default' with [50, 49, 3].  Bounds: those of
tests/test_model_gpu.py::test_critic_and_generator_steps for the dense path, whose products the masked path uses -- outputs
5e-4 / 5e-5 (predict), cost 5e-4 / 1e-5, generator gradients 2e-3 / 5e-5 gmax + 1e-6 with kinks=True and a relative L2 error of at
most 3e-3 over all tensors, moving statistics 5e-4 / 1e-5.  Output pad frames are bitwise zero; with every length equal to T the
masked step meets the dense step within the same bounds."""
import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

import test_model_gpu as tm
import test_ragged_rule as rr
import test_ragged_train_rule as rt

pytestmark = pytest.mark.gpu

CASES = {'test': None, 'nocnn': None, 'default': [50, 49, 3]}


def _setup(geom, lens=None, seed=8):
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build(geom)
    T = tm.GEOMS[geom]['T']
    lens = lens or CASES[geom] or [T, T - 1, 3, 1]
    gen = torch.Generator().manual_seed(seed)
    X = rr.zero_pad_rows(torch.rand(len(lens), T, a.ctxsize, generator=gen, dtype=torch.float64) * 2 - 1, lens)
    Y = rr.zero_pad_rows(torch.randn(len(lens), T, a.outsize, generator=gen, dtype=torch.float64), lens)
    cfg.train_batch_size = len(lens)
    _setup.last = (crit, cw)
    return cfg, mod, a, gw, X, Y, lens


def _wgan(geom, errtype='WLSWGAN', lens=None, **options):
    """(optimiser, arch, generator weights, critic weights, X, Y, alpha, lengths) with OptimizerTTSWGAN prepared"""
    from percivaltts_amd import optimizertts_wgan
    cfg, mod, a, gw, X, Y, lens = _setup(geom, lens)
    crit, cw = _setup.last
    cfg.train_wgan_critic_LSWGANtransidx = 30.0 if geom != 'nocnn' else 4.0
    for k, v in options.items():
        setattr(cfg, k, v)
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype=errtype, critic=crit)
    opt.prepare()
    al = torch.rand(len(lens), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return opt, cfg, a, gw, cw, X, Y, al, lens


def _compare_gradients(params, grads, rtol, arel, what):
    gmax = max(float(g.abs().max()) for g in grads if g is not None)
    num = den = 0.0
    for p, g_ in zip(params, grads):
        want = g_ if g_ is not None else torch.zeros_like(p, dtype=torch.float64, device='cpu')
        tm.close(p.grad, want, rtol, arel * max(gmax, 1.0) + 1e-6, '{} gradient {}'.format(what, tuple(p.shape)), kinks=True)
        num += float((p.grad.detach().cpu().double() - want).pow(2).sum()); den += float(want.pow(2).sum())
    print('{}: relative L2 error of all gradients {:.3e}'.format(what, (num / den) ** 0.5))
    assert num <= (3e-3 ** 2) * den, '{} gradients: relative L2 error {:.3e} over all tensors'.format(what, (num / den) ** 0.5)


def _trainable(a):
    """indices of the oracle's generator weights that are trained: everything but the BatchNorm moving statistics"""
    shapes = O.generator_weight_shapes(a)
    out, i = [], 0
    while i < len(shapes):
        if len(shapes[i]) == 1 and i + 3 < len(shapes) and all(shapes[i + k] == shapes[i] for k in range(4)):
            out += [i, i + 1]; i += 4
        else:
            out.append(i); i += 1
    return out


def _plus_zero(t, lens, what):
    bits = t.detach().contiguous().view(torch.int32)
    for b, n in enumerate(lens):
        assert bool((bits[b, n:] == 0).all()), '{}: pad frames of row {} are not +0.0'.format(what, b)


@pytest.mark.parametrize('geom', list(CASES))
def test_masked_training_forward(geom):
    cfg, mod, a, gw, X, Y, lens = _setup(geom)
    N = sum(lens)
    ws = [t.clone() for t in gw]
    with torch.no_grad():
        want = rt.ragged_train_generator_forward(ws, a, X, lens, update_moving=True)
    mod.to_device()
    n = torch.tensor(lens, dtype=torch.int32, device='cuda')
    got = mod.kerasmodel(tm.f32(X), training=True, memo={'lengths': n, 'lengths_train': N})
    assert got.requires_grad
    tm.close(got, want, 5e-4, 5e-5, 'masked training forward')
    _plus_zero(got, lens, 'outputs')
    for (k, t), w in zip(mod.kerasmodel.weights(), ws):
        if 'moving' in k:
            tm.close(t, w, 5e-4, 1e-5, k)
    # frozen statistics: the same outputs, the moving statistics untouched
    before = [t.detach().clone() for _, t in mod.kerasmodel.weights()]
    with torch.no_grad():
        again = mod.kerasmodel(tm.f32(X), training=True, memo={'lengths': n, 'lengths_train': N, 'freeze_bn_stats': True})
    tm.close(again, want, 5e-4, 5e-5, 'masked training forward, frozen statistics')
    for (k, t), w in zip(mod.kerasmodel.weights(), before):
        assert torch.equal(t, w), k
    # without the training mode the lengths are still for inference only
    with pytest.raises(ValueError):
        mod.kerasmodel(tm.f32(X), training=True, memo={'lengths': n})


@pytest.mark.parametrize('geom', list(CASES))
def test_masked_lse_step(geom):
    from percivaltts_amd import optimizertts
    cfg, mod, a, gw, X, Y, lens = _setup(geom)
    trainable = _trainable(a)
    ws = [t.clone() for t in gw]
    for i in trainable: ws[i].requires_grad_(True)
    ones = torch.ones(a.outsize, dtype=torch.float64)
    loss = rt.masked_lse(Y, rt.ragged_train_generator_forward(ws, a, X, lens, update_moving=True), ones, lens)
    grads = torch.autograd.grad(loss, [ws[i] for i in trainable], allow_unused=True)
    opt = optimizertts.OptimizerTTS(cfg, mod)
    opt.prepare()
    cost = opt.train_on_batch(0, X.numpy().astype(np.float32), Y.numpy().astype(np.float32), lengths=np.array(lens, dtype=np.int32))
    print('{}: masked LSE cost {:.6f} (float64 {:.6f})'.format(geom, cost ** 2, float(loss)))
    tm.close(torch.tensor(cost ** 2), loss.detach(), 5e-4, 1e-5, 'masked LSE cost')
    gmax = max(float(g.abs().max()) for g in grads if g is not None)
    num = den = 0.0
    for p, g_ in zip(opt.opti.flat.params, grads):
        want = g_ if g_ is not None else torch.zeros_like(p, dtype=torch.float64, device='cpu')
        tm.close(p.grad, want, 2e-3, 5e-5 * max(gmax, 1.0) + 1e-6, 'gradient {}'.format(tuple(p.shape)), kinks=True)
        num += float((p.grad.detach().cpu().double() - want).pow(2).sum()); den += float(want.pow(2).sum())
    print('{}: relative L2 error of all gradients {:.3e}'.format(geom, (num / den) ** 0.5))
    assert num <= (3e-3 ** 2) * den, 'gradients: relative L2 error {:.3e} over all tensors'.format((num / den) ** 0.5)
    for (k, t), w in zip(mod.kerasmodel.weights(), ws):
        if 'moving' in k:
            tm.close(t, w, 5e-4, 1e-5, k)
    with pytest.raises(ValueError):
        opt.train_on_batch(1, X.numpy().astype(np.float32), Y.numpy().astype(np.float32), lengths=np.array([0] + lens[1:], dtype=np.int32))


@pytest.mark.parametrize('geom', ['test', 'nocnn'])
def test_full_lengths_meet_the_dense_step(geom):
    from percivaltts_amd import optimizertts
    T = tm.GEOMS[geom]['T']
    out = []
    for masked in (False, True):
        cfg, mod, a, gw, X, Y, lens = _setup(geom, lens=[T] * 4)
        opt = optimizertts.OptimizerTTS(cfg, mod)
        opt.prepare()
        Xn, Yn = X.numpy().astype(np.float32), Y.numpy().astype(np.float32)
        cost = opt.train_on_batch(0, Xn, Yn, lengths=np.array(lens, dtype=np.int32)) if masked else opt.train_on_batch(0, Xn, Yn)
        out.append((cost, [p.grad.detach().cpu().double() for p in opt.opti.flat.params]))
    (c0, g0), (c1, g1) = out
    tm.close(torch.tensor(c1 ** 2), torch.tensor(c0 ** 2), 5e-4, 1e-5, 'cost')
    gmax = max(float(g.abs().max()) for g in g0)
    for a_, b_ in zip(g1, g0):
        tm.close(a_, b_, 2e-3, 5e-5 * max(gmax, 1.0) + 1e-6, 'gradient {}'.format(tuple(b_.shape)), kinks=True)


def test_refused_with_synchronised_batchnorm():
    """(the two other refused pairs: test_refused_with_more_than_one_rank, test_refused_with_the_bf16_critic)"""
    from percivaltts_amd import optimizertts, optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build('nocnn')
    cfg.train_batch_padtype = 'randshiftpad'
    cfg.train_sync_batchnorm = True
    with pytest.raises(ValueError, match='randshiftpad.*train_sync_batchnorm'):
        optimizertts.OptimizerTTS(cfg, mod).prepare()
    with pytest.raises(ValueError, match='randshiftpad.*train_sync_batchnorm'):
        optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit).prepare()
    cfg.train_sync_batchnorm = False
    optimizertts.OptimizerTTS(cfg, mod).prepare()               # both optimisers take it on one rank
    optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit).prepare()


@pytest.mark.parametrize('geom', list(CASES))
def test_masked_critic_loss(geom):
    import contextlib
    from percivaltts_amd import ops
    opt, cfg, a, gw, cw, X, Y, al, lens = _wgan(geom)
    opt.debug_keep_x_hat = True                      # the interpolated sample of the last masked critic loss stays in opt._x_hat
    for w in cw: w.requires_grad_(True)
    total, parts = rt.masked_critic_step_loss(cw, gw, a, X, Y, al, lens, gp_lambda=10.0)
    grads = torch.autograd.grad(total, cw)
    before = [t.detach().clone() for _, t in opt._model.kerasmodel.weights()]
    # plainly, and on 'nocnn' also the way critic_step runs it: weight gradients queued and grouped (the queue keeps no gradient
    # for x^, which the step does not need)
    for mode in [contextlib.nullcontext] + ([ops.deferred_weight_grads] if geom == 'nocnn' else []):
        opt.critic_opti.zero_grad()
        with mode():
            tot_d, (lv, lf, gp) = opt.critic_loss(tm.f32(X), tm.f32(Y), tm.f32(al), training=True, lengths=np.array(lens, dtype=np.int32))
            tm.close(lv, parts['valid'], 5e-4, 1e-5, 'L valid')
            tm.close(lf, parts['fake'], 5e-4, 1e-5, 'L fake')
            tm.close(gp, parts['gp'], 5e-4, 1e-5, 'gradient penalty')
            tm.close(tot_d, total, 5e-4, 1e-5, 'critic loss')
            tot_d.backward()
        _compare_gradients(opt.critic_opti.flat.params, grads, 1e-3, 2e-5, 'critic ' + geom)
        if mode is contextlib.nullcontext and geom != 'nocnn':
            # d total / d x^ (through the penalty's second sweep); the all-Dense critic of 'nocnn' is piecewise linear in x^ with no
            # mask between x^ and its first product, so autograd finds no path at all there and leaves None
            _plus_zero(opt._x_hat.grad, lens, 'the gradient of x^')
    # the gradient the penalty takes its norm of, d sum(v^) / d x^: the float64 one on real frames, bitwise zero behind them
    n = torch.tensor(lens, dtype=torch.int32, device='cuda')
    xh = opt._x_hat.detach().clone().requires_grad_(True)
    v = opt.critic_net.forward_multi_at(opt.critic.node_spec_in, [xh], {opt.critic.input_ctx: tm.f32(X)}, training=True,
                                        memo={'lengths': n, 'lengths_train': sum(lens)})[0]
    g, = torch.autograd.grad(v.sum(), xh)
    gref = parts['g'][:, :, 1:1 + a.specsize].detach()
    tm.close(g, gref, 1e-3, 2e-5 * float(gref.abs().max()) + 1e-6, 'd sum(v^) / d x^', kinks=True)
    _plus_zero(g, lens, 'd sum(v^) / d x^')
    for (k, t), w in zip(opt._model.kerasmodel.weights(), before):
        assert torch.equal(t, w), 'the frozen generator moved ' + k


@pytest.mark.parametrize('geom,errtype', [(g, e) for g in CASES for e in ('WLSWGAN', 'WGAN')])
def test_masked_generator_loss(geom, errtype):
    opt, cfg, a, gw, cw, X, Y, al, lens = _wgan(geom, errtype)
    trainable = _trainable(a)
    gw_t = [w.detach().clone() for w in gw]
    for i in trainable: gw_t[i].requires_grad_(True)
    w_ls, ww = O.wls_weights(a.specsize, a.noisesize, 0, 0.25, cfg.train_wgan_critic_LSWGANtransidx)
    ltot, lparts = rt.masked_generator_step_loss(cw, gw_t, a, X, Y, lens, errtype, torch.tensor(w_ls), ww, update_moving=True)
    ggrads = torch.autograd.grad(ltot, [gw_t[i] for i in trainable], allow_unused=True)
    opt.gen_opti.zero_grad()
    for p in opt.critic_opti.flat.params: p.requires_grad_(False)
    ltot_d, (lw_d, lls_d) = opt.generator_loss(tm.f32(X), tm.f32(Y), training=True, lengths=np.array(lens, dtype=np.int32))
    tm.close(lw_d, lparts['wgan'], 5e-4, 1e-5, 'generator wgan term')
    if errtype == 'WLSWGAN':
        tm.close(lls_d, lparts['ls'], 5e-4, 1e-5, 'generator ls term')
    tm.close(ltot_d, ltot, 5e-4, 1e-5, 'generator loss')
    ltot_d.backward()
    for p in opt.critic_opti.flat.params: p.requires_grad_(True)
    _compare_gradients(opt.gen_opti.flat.params, ggrads, 2e-3, 5e-5, 'generator {} {}'.format(geom, errtype))
    for (k, t), w in zip(opt._model.kerasmodel.weights(), gw_t):
        if 'moving' in k:
            tm.close(t, w, 5e-4, 1e-5, k)


@pytest.mark.parametrize('geom', ['test', 'nocnn'])
def test_full_lengths_meet_the_dense_critic_and_generator_losses(geom):
    T = tm.GEOMS[geom]['T']
    out = []
    for masked in (False, True):
        opt, cfg, a, gw, cw, X, Y, al, lens = _wgan(geom, lens=[T] * 4)
        kw = dict(lengths=np.array(lens, dtype=np.int32)) if masked else {}
        opt.critic_opti.zero_grad()
        tot, parts = opt.critic_loss(tm.f32(X), tm.f32(Y), tm.f32(al), training=True, **kw)
        tot.backward()
        cg = [p.grad.detach().cpu().double() for p in opt.critic_opti.flat.params]
        opt.gen_opti.zero_grad()
        for p in opt.critic_opti.flat.params: p.requires_grad_(False)
        gtot, _ = opt.generator_loss(tm.f32(X), tm.f32(Y), training=True, **kw)
        gtot.backward()
        for p in opt.critic_opti.flat.params: p.requires_grad_(True)
        out.append(([tot.detach().cpu().double()] + [t.detach().cpu().double() for t in parts], cg, gtot.detach().cpu().double(),
                    [p.grad.detach().cpu().double() for p in opt.gen_opti.flat.params]))
    (l0, cg0, g0, gg0), (l1, cg1, g1, gg1) = out
    for x1, x0 in zip(l1 + [g1], l0 + [g0]):
        tm.close(x1, x0, 5e-4, 1e-5, 'loss')
    for (got, ref, rtol, arel) in ((cg1, cg0, 1e-3, 2e-5), (gg1, gg0, 2e-3, 5e-5)):
        gmax = max(float(g.abs().max()) for g in ref)
        for x1, x0 in zip(got, ref):
            tm.close(x1, x0, rtol, arel * max(gmax, 1.0) + 1e-6, 'gradient {}'.format(tuple(x0.shape)), kinks=True)


def test_device_step_with_lengths_follows_the_schedule_and_captures_no_graph():
    opt, cfg, a, gw, cw, X, Y, al, lens = _wgan('nocnn', train_wgan_hipgraph=True)     # (asked for graphs: lengths overrule it)
    Xd, Yd, n = tm.f32(X), tm.f32(Y), np.array(lens, dtype=np.int32)
    assert opt._use_graph(Xd, 'critic', Yd) is True and opt._use_graph(Xd, 'critic', Yd, lengths=n) is False
    fired = []
    for batchid in range(11):
        lc, lg = opt.device_step(batchid, Xd, Yd, lengths=n)
        assert bool(torch.isfinite(lc)) and (lg is None or bool(torch.isfinite(lg)))
        fired.append(lg is not None)
    runs = O.critic_runs(0)
    assert [i for i, f in enumerate(fired) if f] == [i for i in range(11) if i % runs == 0] == [0, 10]
    assert opt.generator_updates == 2 and not opt._graphs, 'a graph was captured'
    # through the driver's hook too
    assert opt.train_on_batch(20, X.numpy().astype(np.float32), Y.numpy().astype(np.float32), lengths=n) is not None


def test_device_corpus_batch_with_lengths():
    """DeviceCorpus.batch(padtype='randshiftpad', want_lengths=True) is data.batching's batch for the same seed, lengths on the host."""
    from percivaltts_amd import data
    rng = np.random.RandomState(2)
    lens = [37, 9, 52, 20, 21]
    Xs = [rng.rand(k, 7).astype(np.float32) + 1 for k in lens]
    Ys = [rng.rand(k, 5).astype(np.float32) + 1 for k in lens]
    Ws = [np.ones((k, 1), dtype=np.float32) for k in lens]
    corpus = data.DeviceCorpus.from_utterances(Xs, Ys, Ws)
    ids = [3, 0, 2, 1]
    for length, lengthmax in ((None, 20), (None, None), (30, None)):
        np.random.seed(6)
        [Xh, Yh], _ = data.batching([[Xs[i] for i in ids], [Ys[i] for i in ids]], length=length, lengthmax=lengthmax, padtype='randshiftpad')
        np.random.seed(6)
        Xd, Yd, n = corpus.batch(ids, length=length, lengthmax=lengthmax, padtype='randshiftpad', want_lengths=True)
        assert isinstance(n, np.ndarray) and n.dtype == np.int32 and n.tolist() == [min(lens[i], Xh.shape[1]) for i in ids]
        np.testing.assert_array_equal(Xd.cpu().numpy(), Xh)
        np.testing.assert_array_equal(Yd.cpu().numpy(), Yh)
    assert len(corpus.batch(ids, lengthmax=20, padtype='randshiftpad')) == 2


def test_refused_with_the_bf16_critic():
    from percivaltts_amd import optimizertts_wgan, networks_critic
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build('default')
    cfg.train_batch_padtype = 'randshiftpad'
    for form in (True, 'layers'):                  # the one-launch chain (Conv2DStack) and the layer-wise bf16 maps
        cfg.arch_critic_bf16 = form
        crit = networks_critic.Critic(voc, tm.GEOMS['default']['ctx'], cfg)
        with pytest.raises(ValueError, match='randshiftpad.*arch_critic_bf16'):
            optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit).prepare()


@pytest.mark.parametrize('which', ['LSE', 'WLSWGAN'])
def test_refused_with_more_than_one_rank(monkeypatch, which):
    """'randshiftpad' with data parallelism: prepare() learns the number of ranks from parallel.init() and refuses, naming both."""
    from percivaltts_amd import optimizertts, optimizertts_wgan, parallel
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build('nocnn')
    monkeypatch.setattr(parallel, 'init', lambda *a_, **k_: (2, 0))
    make = (lambda: optimizertts.OptimizerTTS(cfg, mod)) if which == 'LSE' else \
        (lambda: optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit))
    cfg.train_batch_padtype = 'randshiftpad'
    opt = make()
    with pytest.raises(ValueError, match='randshiftpad.*ranks'):
        opt.prepare()
    assert opt.world == 2
    assert not hasattr(opt, 'opti') and not hasattr(opt, 'critic_opti'), 'refused only after the optimisers were built'
