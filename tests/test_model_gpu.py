"""GPU parity of the networks and of the WGAN-GP critic / generator steps against the CPU oracle on identical
weights, inputs and injected alpha (the reference draws alpha and the initial weights from TF's RNG, so both are
injected: SURVEY.md section 7, 'RNG parity').  Bar: rtol 1e-3 (north star), checked here at 5e-4 or tighter."""
import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

pytestmark = pytest.mark.gpu


def close(got, want, rtol, atol, what='', kinks=False):
    """kinks=True (gradient comparisons): LeakyReLU makes the gradient discontinuous in the pre-activations, so a
    pre-activation that is ~0 can take a different side in fp32 (HIP) and fp64 (oracle); the handful of gradient entries
    fed by that one mask then differ by a few percent (one flipped mask of a hidden unit moves a whole row/column of a
    weight gradient, which at these small B*T is up to ~1 % of the tensor's norm).  When the elementwise check fails,
    the tensor still passes if its relative L2 error is <= 2e-2 and no entry is off by more than 5 % of the largest
    gradient; the callers also bound the relative L2 error over ALL gradients of a network together by 3e-3.  Wiring
    mistakes give O(1) errors, and the kernels themselves are pinned elementwise in test_ops_gpu.py."""
    got = torch.as_tensor(np.asarray(got.detach().cpu() if torch.is_tensor(got) else got), dtype=torch.float64)
    want = torch.as_tensor(np.asarray(want.detach().cpu() if torch.is_tensor(want) else want), dtype=torch.float64)
    assert got.shape == want.shape, '{}: {} vs {}'.format(what, tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    if kinks and (err > tol).any():
        if float(err.norm()) <= 2e-2 * float(want.norm()) and float(err.max()) <= 0.05 * float(want.abs().max()):
            return
    if (err > tol).any():
        i = int(torch.argmax(err - tol))
        raise AssertionError('{}: {}/{} off, worst err {:.3e} (got {:.6e} want {:.6e}) max|want| {:.3e}, rel L2 {:.3e}'.format(
            what, int((err > tol).sum()), err.numel(), float(err.flatten()[i]), float(got.flatten()[i]),
            float(want.flatten()[i]), float(want.abs().max()), float(err.norm()) / max(float(want.norm()), 1e-300)))


GEOMS = {
    # the geometry of the reference's DCNN/WGAN smoke test (tests/test_smoke_tensorflowkeras.py:184-203)
    'test': dict(ctx=425, spec=65, nm=17, H=2, nctx=2, kctx=3, L=2, C=2, kt=3, kf=3, B=2, T=16),
    # the default architecture (run.py:114-120) at reduced width/length
    'default': dict(ctx=61, spec=65, nm=20, H=32, nctx=1, kctx=21, L=8, C=4, kt=5, kf=5, B=3, T=50),
    # no conv layers: the critic's FC spectral branch (networks_critic.py:72-76)
    'nocnn': dict(ctx=20, spec=9, nm=3, H=8, nctx=1, kctx=5, L=0, C=2, kt=3, kf=3, B=2, T=12),
    # 4160 frames: large enough for the paths the small geometries never reach -- LDS-DMA GEMM tiles (interior and edge),
    # split-K weight gradients, the grouped (deferred) weight-gradient launch, multi-tile conv2d, the packed LSTM kernels
    'mid': dict(ctx=61, spec=65, nm=20, H=64, nctx=1, kctx=21, L=2, C=4, kt=5, kf=5, B=8, T=520),
    # the generator's spectral branch built from pGCNN2D (networktts.py:128-134; the alternative commented at
    # modeltts_common.py:99) exactly as the reference defines it: dilation 1, symmetric padding
    'gated': dict(ctx=31, spec=65, nm=20, H=16, nctx=1, kctx=5, L=3, C=4, kt=5, kf=5, B=2, T=40, gated=True),
    # BASELINE configs[4]: gated, time dilations 1,2,4,8 and causal padding (build extensions)
    'gated_dilated': dict(ctx=31, spec=65, nm=20, H=16, nctx=1, kctx=5, L=4, C=4, kt=5, kf=5, B=2, T=70, gated=True,
                          dils=[1, 2, 4, 8], causal=True),
}


def build(geom):
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common, networks_critic, optimizertts_wgan
    g = GEOMS[geom]
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = g['H']; cfg.arch_ctx_nbcnnlayers = g['nctx']; cfg.arch_ctx_winlen = g['kctx']
    cfg.arch_gen_nbcnnlayers = g['L']; cfg.arch_gen_nbfilters = g['C']; cfg.arch_gen_winlen = g['kt']
    cfg.arch_spec_freqlen = g['kf']; cfg.train_batch_size = g['B']
    if g.get('gated'):
        cfg.arch_gen_gated = True; cfg.arch_gen_dilations = g.get('dils'); cfg.arch_gen_causal = bool(g.get('causal', False))
    voc = vocoders.VocoderPML(16000, 0.005, g['spec'], g['nm'])
    mod = modeltts_common.DCNNF0SpecNoiseFeatures(g['ctx'], voc, cfg)
    crit = networks_critic.Critic(voc, g['ctx'], cfg)
    a = O.Arch(g['ctx'], g['spec'], g['nm'], g['H'], g['nctx'], g['kctx'], g['L'], g['C'], g['kt'], g['kf'],
               gen_gated=bool(g.get('gated')), gen_dilations=g.get('dils'), gen_causal=bool(g.get('causal', False)))
    gw = O.random_weights(O.generator_weight_shapes(a), seed=11)
    cw = O.random_weights(O.critic_weight_shapes(a), seed=12)
    assert mod.count_params() == O.count_params(O.generator_weight_shapes(a))
    assert crit.model.count_params() == O.count_params(O.critic_weight_shapes(a))
    mod.kerasmodel.set_weights([w.numpy() for w in gw])
    crit.model.set_weights([w.numpy() for w in cw])
    gen = torch.Generator().manual_seed(5)
    X = torch.rand(g['B'], g['T'], g['ctx'], generator=gen, dtype=torch.float64) * 2 - 1
    Y = torch.randn(g['B'], g['T'], a.outsize, generator=gen, dtype=torch.float64)
    Y[:, :, 1 + g['spec']:] = torch.rand(g['B'], g['T'], g['nm'], generator=gen, dtype=torch.float64)
    al = torch.rand(g['B'], generator=gen, dtype=torch.float64)
    return cfg, voc, mod, crit, a, gw, cw, X, Y, al


def f32(t):
    return t.to(torch.float32).cuda().contiguous()


@pytest.mark.parametrize('geom', ['test', 'default', 'nocnn', 'gated', 'gated_dilated'])
def test_predict_and_critic_forward(geom):
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build(geom)
    want = O.generator_forward(gw, a, X, training=False)
    got = mod.predict(X.numpy().astype(np.float32))
    close(got, want, 5e-4, 5e-5, 'predict (BN inference)')
    dev = mod.to_device()
    crit.model.to(dev)
    with torch.no_grad():
        v = crit.model(f32(Y), f32(X), training=False)
        gt = mod.kerasmodel(f32(X), training=True, memo={'freeze_bn_stats': True})
    close(v, O.critic_forward(cw, a, Y, X), 5e-4, 5e-5, 'critic forward')
    close(gt, O.generator_forward(gw, a, X, training=True), 5e-4, 5e-5, 'generator forward (BN batch statistics)')
    # a frozen forward must not touch the moving statistics
    for (k, t), w in zip(mod.kerasmodel.weights(), gw):
        close(t, w, 1e-6, 1e-7, 'weights untouched ' + k)


@pytest.mark.parametrize('geom,errtype', [(g, e) for g in ('test', 'default', 'nocnn') for e in ('WLSWGAN', 'WGAN')] + [('mid', 'WLSWGAN'), ('gated', 'WLSWGAN'), ('gated_dilated', 'WLSWGAN')])
def test_critic_and_generator_steps(geom, errtype):
    from percivaltts_amd import optimizertts_wgan, ops
    import contextlib
    # 'mid' runs the device side the way critic_step / generator_step do: Dense weight gradients queued and grouped
    deferred = ops.deferred_weight_grads if geom == 'mid' else contextlib.nullcontext
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build(geom)
    cfg.train_wgan_critic_LSWGANtransidx = 30.0 if geom != 'nocnn' else 4.0
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype=errtype, critic=crit)
    opt.prepare()
    if geom.startswith('gated'):
        from percivaltts_amd import layers as _kl
        assert sum(isinstance(l, _kl.GatedMultiply) for l in mod.kerasmodel.layers_list) == GEOMS[geom]['L']
    Xd, Yd, ald = f32(X), f32(Y), f32(al)

    # ---- critic: loss parts, every weight gradient, Keras-Adam update --------------------------------------
    for w in cw: w.requires_grad_(True)
    total, parts = O.critic_step_loss(cw, gw, a, X, Y, al, gp_lambda=10.0)
    grads = torch.autograd.grad(total, cw)
    opt.critic_opti.zero_grad()
    with deferred():
        tot_d, (lv, lf, gp) = opt.critic_loss(Xd, Yd, ald, training=True)
        close(lv, parts['valid'], 5e-4, 1e-5, 'L valid')
        close(lf, parts['fake'], 5e-4, 1e-5, 'L fake')
        close(gp, parts['gp'], 5e-4, 1e-5, 'gradient penalty')
        close(tot_d, total, 5e-4, 1e-5, 'critic loss')
        tot_d.backward()
    gmax = max(float(g.abs().max()) for g in grads)
    num = den = 0.0
    for p, g_ in zip(opt.critic_opti.flat.params, grads):
        close(p.grad, g_, 1e-3, 2e-5 * max(gmax, 1.0) + 1e-6, 'critic grad {}'.format(tuple(g_.shape)), kinks=True)
        num += float((p.grad.detach().cpu().double() - g_.detach()).pow(2).sum()); den += float(g_.detach().pow(2).sum())
    assert num <= (3e-3 ** 2) * den, 'critic gradients: relative L2 error {:.3e} over all tensors'.format((num / den) ** 0.5)
    ms = [torch.zeros_like(w) for w in cw]; vs = [torch.zeros_like(w) for w in cw]
    with torch.no_grad():
        cw2 = [w.detach().clone() for w in cw]
    O.adam_keras(cw2, grads, ms, vs, 1, 1e-4, 0.5, 0.9, 1e-7)
    opt.critic_opti.step()
    # Adam's first step moves every weight by ~lr*sign(g): compare the moves where the gradient is not tiny
    for p, w_new, w_old, g_ in zip(opt.critic_opti.flat.params, cw2, cw, grads):
        big = g_.abs() > 1e-3 * gmax
        close((p.detach().cpu().double() - w_old.detach())[big], (w_new - w_old.detach())[big], 2e-2, 1e-7, 'critic Adam move')

    # ---- generator: loss, gradients, update, BN moving statistics ----------------------------------------------
    cw_now = [p.detach().cpu().double() for _, p in crit.model.weights()]
    gw_t = [w.detach().clone() for w in gw]
    shapes = O.generator_weight_shapes(a)
    # trainable = everything except BN moving statistics (3rd/4th of each run of four equal 1-D shapes)
    trainable, i = [], 0
    while i < len(shapes):
        if len(shapes[i]) == 1 and i + 3 < len(shapes) and all(shapes[i + k] == shapes[i] for k in range(4)):
            trainable += [i, i + 1]; i += 4
        else:
            trainable.append(i); i += 1
    for i in trainable: gw_t[i].requires_grad_(True)
    w_ls, ww = O.wls_weights(a.specsize, a.noisesize, 0, 0.25, cfg.train_wgan_critic_LSWGANtransidx)
    ltot, lparts = O.generator_step_loss(cw_now, gw_t, a, X, Y, errtype, torch.tensor(w_ls), ww, update_moving=True)
    ggrads = torch.autograd.grad(ltot, [gw_t[i] for i in trainable], allow_unused=True)
    opt.gen_opti.zero_grad()
    for p in opt.critic_opti.flat.params: p.requires_grad_(False)
    with deferred():
        ltot_d, (lw_d, lls_d) = opt.generator_loss(Xd, Yd, training=True)
        close(lw_d, lparts['wgan'], 5e-4, 1e-5, 'generator wgan term')
        if errtype == 'WLSWGAN':
            close(lls_d, lparts['ls'], 5e-4, 1e-5, 'generator ls term')
        close(ltot_d, ltot, 5e-4, 1e-5, 'generator loss')
        ltot_d.backward()
    for p in opt.critic_opti.flat.params: p.requires_grad_(True)
    ggmax = max(float(g.abs().max()) for g in ggrads if g is not None)
    num = den = 0.0
    for p, g_ in zip(opt.gen_opti.flat.params, ggrads):
        want = g_ if g_ is not None else torch.zeros_like(p, dtype=torch.float64, device='cpu')
        close(p.grad, want, 2e-3, 5e-5 * max(ggmax, 1.0) + 1e-6, 'generator grad {}'.format(tuple(p.shape)), kinks=True)
        num += float((p.grad.detach().cpu().double() - want).pow(2).sum()); den += float(want.pow(2).sum())
    assert num <= (3e-3 ** 2) * den, 'generator gradients: relative L2 error {:.3e} over all tensors'.format((num / den) ** 0.5)
    # moving statistics after one training forward
    for (k, t), w in zip(mod.kerasmodel.weights(), gw_t):
        if 'moving' in k:
            close(t, w, 5e-4, 1e-5, k)


@pytest.mark.parametrize('geom', ['default', 'test'])
@pytest.mark.parametrize('T', [1, 37, 601])
def test_evaluation_mode_losses_whole_utterances(geom, T):
    """update_validation_cost (optimizertts_wgan.py:244-268): `generator_model.evaluate` and `critic_model.evaluate` run with
    learning phase 0 -- BatchNorm on its moving statistics, also inside the frozen generator of the critic loss, the
    gradient penalty still evaluated -- at batch size 1 on whole utterances (T ~ 600, no multiple of any tile; T = 1 is the
    degenerate utterance).  Both losses and their parts against the oracle."""
    from percivaltts_amd import optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build(geom)
    cfg.train_wgan_critic_LSWGANtransidx = 30.0
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    gen = torch.Generator().manual_seed(100 + T)
    g = GEOMS[geom]
    X1 = torch.rand(1, T, g['ctx'], generator=gen, dtype=torch.float64) * 2 - 1
    Y1 = torch.randn(1, T, a.outsize, generator=gen, dtype=torch.float64)
    al1 = torch.rand(1, generator=gen, dtype=torch.float64)
    total, parts = O.critic_step_loss(cw, gw, a, X1, Y1, al1, gp_lambda=10.0, training=False)
    tot_d, (lv, lf, gp) = opt.critic_loss(f32(X1), f32(Y1), f32(al1), training=False)
    close(lv, parts['valid'], 5e-4, 1e-5, 'L valid (eval)')
    close(lf, parts['fake'], 5e-4, 1e-5, 'L fake (eval)')
    close(gp, parts['gp'], 5e-4, 1e-5, 'gradient penalty (eval)')
    close(tot_d, total, 5e-4, 1e-5, 'critic loss (eval)')
    w_ls, ww = O.wls_weights(a.specsize, a.noisesize, 0, 0.25, 30.0)
    ltot, lparts = O.generator_step_loss(cw, gw, a, X1, Y1, 'WLSWGAN', torch.tensor(w_ls), ww, training=False)
    with torch.no_grad():
        ltot_d, (lw_d, lls_d) = opt.generator_loss(f32(X1), f32(Y1), training=False)
    close(lw_d, lparts['wgan'], 5e-4, 1e-5, 'generator wgan term (eval)')
    close(lls_d, lparts['ls'], 5e-4, 1e-5, 'generator ls term (eval)')
    close(ltot_d, ltot, 5e-4, 1e-5, 'generator loss (eval)')
    # evaluation must not move the moving statistics
    for (k, t), w in zip(mod.kerasmodel.weights(), gw):
        close(t, w, 1e-6, 1e-7, 'weights untouched ' + k)


def test_generic_model_count_params_and_lse_step():
    """Generic 3xFC, the reference's known answer 2195 (tests/test_smoke_tensorflowkeras.py:53), then one LSE step."""
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common, optimizertts
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 4
    cfg.train_batch_size = 2
    voc = vocoders.VocoderPML(16000, 0.005, 65, 17)
    model = modeltts_common.Generic(425, voc, layertypes=['FC', 'FC', 'FC'], cfgarch=cfg)
    assert model.count_params() == 2195
    opt = optimizertts.OptimizerTTS(cfg, model)
    opt.prepare()
    rng = np.random.RandomState(0)
    X = rng.rand(2, 30, 425).astype(np.float32) * 2 - 1
    Y = rng.randn(2, 30, 83).astype(np.float32)
    c0 = opt.train_on_batch(0, X, Y)
    for i in range(30):
        c = opt.train_on_batch(i + 1, X, Y)
    assert np.isfinite(c0) and np.isfinite(c) and c < c0
    out = model.predict(X[:1])
    assert out.shape == (1, 30, 83) and np.isfinite(out).all()


def test_schedule_and_train_on_batch_api():
    from percivaltts_amd import optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('test')
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    Xn, Yn = X.numpy().astype(np.float32), Y.numpy().astype(np.float32)
    rets = [opt.train_on_batch(b, Xn, Yn) for b in range(12)]
    # critic_runs = 10 while generator_updates < 25: generator steps at batchid 0 and 10 (optimizertts_wgan.py:225-231)
    assert [r is not None for r in rets] == [True] + [False] * 9 + [True, False]
    assert opt.generator_updates == 2 and len(opt.costs_tra_critic_batches) == 12
    assert all(np.isfinite(c) for c in opt.costs_tra_critic_batches)


def test_hipgraph_replay_matches_eager():
    from percivaltts_amd import optimizertts_wgan
    outs = []
    for use_graph in (False, True):
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
        cfg.train_wgan_hipgraph = use_graph
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        Xd, Yd, ald = f32(X), f32(Y), f32(al)
        if use_graph:
            # capture (includes 2 warm-up steps), then restore the initial state and replay 3 steps
            opt._graphed('critic', Xd, Yd)
            crit.model.set_weights([w.numpy() for w in cw])
            opt.critic_opti.m.zero_(); opt.critic_opti.v.zero_(); opt.critic_opti.step_count.zero_()
            g, sX, sY, sA, out, _ = opt._graphs[('critic', tuple(Xd.shape), tuple(Yd.shape), True, False)]
            losses = []
            for _ in range(3):
                sA.copy_(ald); g.replay(); losses.append(float(out.item()))
        else:
            losses = [float(opt.critic_step(Xd, Yd, ald).item()) for _ in range(3)]
        outs.append((losses, opt.critic_opti.flat.flat.detach().cpu().clone()))
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-6)
    close(outs[1][1], outs[0][1], 1e-3, 1e-5, 'critic weights after 3 steps, graph vs eager')


def test_hipgraph_critic_costs_are_per_batch_and_async_whole_graph():
    """costs_tra_critic_batches under cfg.train_wgan_hipgraph: every replay returns the SAME static loss tensor
    of the captured graph, so the device-side cost list must copy it -- pending views would all read the last batch's loss.
    Two different batches: the two fetched costs differ and equal the values read right after each step.  The same loop with
    cfg.train_wgan_async_update in whole-graph mode (the update left pending by the warm-up must not leak a wait into the
    capture): finite, and the weights move."""
    from percivaltts_amd import optimizertts_wgan
    for async_update in (False, True):
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
        cfg.train_wgan_hipgraph = 'auto' if async_update else True      # 'auto': graphs for batches of <= 8192 frames (this one)
        cfg.train_wgan_async_update = async_update
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        opt.generator_updates = 26
        w0 = opt.critic_opti.flat.flat.detach().clone()
        Xd, Yd = f32(X), f32(Y)
        X2, Y2 = f32(X.flip(0) * 0.5), f32(Y.flip(1) + 0.25)
        seen = []
        for b, (xb, yb) in enumerate(((Xd, Yd), (X2, Y2), (Xd, Yd))):
            lc, _ = opt.device_step(b + 1, xb, yb)            # batchid 1..3: critic steps only
            opt.costs_tra_critic_batches.append_device(lc)
            seen.append(float(lc.item()))
        assert opt._use_graph(Xd) and len(opt._graphs) == 1
        fetched = list(opt.costs_tra_critic_batches)
        assert fetched == seen, (fetched, seen)
        assert abs(seen[0] - seen[1]) > 1e-6 * max(1.0, abs(seen[0])), seen
        opt.wait_updates(); torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in seen) and not torch.equal(w0, opt.critic_opti.flat.flat)


def test_hipgraph_tune_restores_training_state_and_trains_like_eager():
    """cfg.train_wgan_hipgraph = 'tune' times eager launches against a hipGraph replay per step kind with REAL steps on the first
    batch: weights, Adam moments and step counters, BatchNorm moving averages and the device's random stream must be back
    afterwards, so that the steps that follow are the ones an untuned run makes (same losses, same weights after a critic-only
    step and after a critic + generator step)."""
    from percivaltts_amd import optimizertts_wgan
    res = []
    for mode in (False, 'tune'):
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
        cfg.train_wgan_hipgraph = mode
        cfg.train_wgan_hipgraph_maxframes = 0            # no 'auto' shortcut for this small batch: the timing runs decide
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        opt.generator_updates = 26
        Xd, Yd, ald = f32(X), f32(Y), f32(al)
        if mode == 'tune':
            state = lambda: [t.detach().clone() for o in (opt.critic_opti, opt.gen_opti) for t in (o.flat.flat, o.m, o.v, o.step_count)] + \
                            [b.detach().clone() for net in (opt.critic_net, opt._model.kerasmodel) for b in net.buffers()] + [torch.cuda.get_rng_state()]
            before = state()
            for kind in ('critic', 'generator'):
                assert opt._use_graph(Xd, kind, Yd) in (True, False)
            assert set(k[0] for k in opt._graph_tuning) == {'critic', 'generator'}
            for x, y in zip(before, state()):
                assert torch.equal(x, y), 'the tuning runs left a trace in the training state'
        out = []
        for b in (1, 5):                                  # batchid 1: critic only; 5: critic + generator (critic_runs = 5)
            lc, lg = opt.device_step(b, Xd, Yd, ald)
            out.append((float(lc.item()), None if lg is None else float(lg.item())))
        opt.wait_updates(); torch.cuda.synchronize()
        assert out[0][1] is None and out[1][1] is not None
        res.append((out, opt.critic_opti.flat.flat.detach().cpu().clone(), opt.gen_opti.flat.flat.detach().cpu().clone()))
    np.testing.assert_allclose([v for o in res[0][0] for v in o if v is not None], [v for o in res[1][0] for v in o if v is not None], rtol=2e-5, atol=1e-6)
    close(res[1][1], res[0][1], 1e-4, 1e-6, "critic weights, 'tune' vs eager", kinks=True)
    close(res[1][2], res[0][2], 1e-4, 1e-6, "generator weights, 'tune' vs eager", kinks=True)


def _look_ahead_pair(opt, X, Y, al):
    """(X, Y, alpha) of batch 4 (critic only; it launches the generator forward of batch 5 when that is named as the next batch) and
    of batch 5 (trains both, consumes it), with the optimiser set to critic_runs = 5."""
    opt.generator_updates = 26
    Xd, Yd, ald = f32(X), f32(Y), f32(al)
    X2, Y2 = f32(X.flip(0) * 0.5), f32(Y.flip(1) + 0.25)
    return (Xd, Yd, ald), (X2, Y2, ald)


def test_retired_schedule_switches_are_inert():
    """The benchmark still sets cfg.train_wgan_fake_ahead, _side_backward_first, _ctx_stream, _graph_streams and _batch_graph from its
    environment switches; the schedules behind them are gone (DESIGN.md keeps their measurements).  With all five set, a critic-only
    batch that launches the generator look-ahead and the batch that consumes it give bit for bit the losses and weights of the
    default configuration (deterministic mode)."""
    from percivaltts_amd import optimizertts_wgan, ops
    res = []
    ops.deterministic(True)
    try:
        for retired in (False, True):
            cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
            cfg.train_wgan_parallel_streams = True
            cfg.train_wgan_hipgraph = False
            if retired:
                for name in ('fake_ahead', 'side_backward_first', 'ctx_stream', 'graph_streams', 'batch_graph'):
                    setattr(cfg, 'train_wgan_' + name, True)
            opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
            opt.prepare()
            (Xd, Yd, ald), (X2, Y2, _) = _look_ahead_pair(opt, X, Y, al)
            lc4, lg4 = opt.device_step(4, Xd, Yd, ald, nxt=(X2, Y2))
            assert lg4 is None and opt._ahead is not None
            lc5, lg5 = opt.device_step(5, X2, Y2, ald)
            assert lg5 is not None and opt._ahead is None
            opt.wait_updates(); torch.cuda.synchronize()
            res.append((torch.stack([lc4.detach(), lc5.detach(), lg5.detach()]).cpu(), opt.critic_opti.flat.flat.detach().cpu().clone(),
                        opt.gen_opti.flat.flat.detach().cpu().clone(), int(opt.critic_opti.step_count), int(opt.gen_opti.step_count)))
    finally:
        ops.deterministic(False)
    assert res[0][3:] == res[1][3:] == (2, 1)
    assert bool(torch.isfinite(res[0][0]).all())
    for x, y, what in zip(res[0][:3], res[1][:3], ('losses', 'critic weights', 'generator weights')):
        assert torch.equal(x, y), what


def test_prepare_forgets_the_state_kept_across_batches():
    """prepare() is where the step's cross-batch state comes into being, and a second prepare() on the same optimiser (the next
    hyper-parameter trial after an aborted one) forgets it: a generator forward launched one batch ahead is neither consumed nor
    dropped -- dropping would write the moving averages it saved over the model the trial has just loaded -- and the frozen-plane
    buffers of the previous trial's graphs are let go."""
    from percivaltts_amd import optimizertts_wgan

    def fresh(opt):
        return opt._ahead is None and opt._next_batch is None and opt._gen_deferred is None and opt._gen_cuts is None and \
            opt._graph_frozen == {}
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
    cfg.train_wgan_parallel_streams = True
    cfg.train_wgan_hipgraph = False
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    assert fresh(opt)
    (Xd, Yd, ald), (X2, Y2, _) = _look_ahead_pair(opt, X, Y, al)
    lc, lg = opt.device_step(4, Xd, Yd, ald, nxt=(X2, Y2))
    assert lg is None and opt._ahead is not None          # the look-ahead itself: launched for the batch named as the next one
    opt._graph_frozen['stale'] = {'items': [], 'epoch': -1}
    opt.prepare()
    assert fresh(opt)
    lc, lg = opt.device_step(1, Xd, Yd, ald)
    opt.wait_updates(); torch.cuda.synchronize()
    assert lg is None and np.isfinite(float(lc))


def test_parallel_streams_match_single_stream():
    """cfg.train_wgan_parallel_streams runs the three critic evaluations on three HIP streams: same loss and gradients."""
    from percivaltts_amd import optimizertts_wgan
    res = []
    for par in (False, True):
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
        cfg.train_wgan_parallel_streams = par
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        Xd, Yd, ald = f32(X), f32(Y), f32(al)
        losses = []
        for _ in range(3):
            losses.append(float(opt.critic_step(Xd, Yd, ald).item()))
        torch.cuda.synchronize()
        res.append((losses, opt.critic_opti.flat.flat.detach().cpu().clone(), opt.critic_opti.flat.grad.detach().cpu().clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    close(res[1][2], res[0][2], 1e-4, 1e-6, 'last critic gradient, 3 streams vs 1', kinks=True)
    close(res[1][1], res[0][1], 1e-4, 1e-6, 'critic weights after 3 steps, 3 streams vs 1', kinks=True)


def test_async_update_on_a_communication_stream_matches_the_plain_step():
    """What data parallelism runs, exercised in one process: the optimiser update (all-reduce + Adam) on a communication
    stream behind an event of the backward pass, with the compute stream going on to the next forward and waiting only
    where it reads the updated weights (cfg.train_wgan_async_update).  Six train_on_batch-equivalents (critic steps and two
    generator steps) must leave bit for bit the weights of the plain eager steps (deterministic mode)."""
    from percivaltts_amd import optimizertts_wgan, ops
    res = []
    ops.deterministic(True)
    try:
        for on in (False, True):
            cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
            cfg.train_wgan_async_update = on
            opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
            opt.prepare()
            opt.generator_updates = 26          # critic_runs = 5: batch 0 and batch 5 also train the generator
            Xd, Yd = f32(X), f32(Y)
            losses = []
            ag = torch.Generator().manual_seed(17)
            for b in range(6):
                lc, lg = opt.device_step(b, Xd, Yd, alpha=torch.rand(Xd.shape[0], generator=ag).cuda())   # injected: no RNG in the comparison
                losses.append(float(lc))
            assert on == bool(opt._pending)        # the last update is still registered as in flight
            opt.wait_updates(); torch.cuda.synchronize()
            res.append((losses, opt.critic_opti.flat.flat.detach().cpu().clone(), opt.gen_opti.flat.flat.detach().cpu().clone(),
                        int(opt.critic_opti.step_count), int(opt.gen_opti.step_count)))
    finally:
        ops.deterministic(False)
    assert res[0][3:] == res[1][3:] == (6, 2)
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=0, atol=0)
    assert torch.equal(res[1][1], res[0][1]) and torch.equal(res[1][2], res[0][2])


def test_split_hipgraph_recomputes_every_weight_derived_operand():
    """cfg.train_wgan_graph_split (what a data-parallel run uses: the gradient all-reduce cannot be captured): the hipGraph
    ends with the backward pass and the update follows eagerly.  Every operand derived from the weights (Toeplitz tables of
    the Conv2D kernels, bf16 planes) must be rebuilt INSIDE the graph: the graphs are replayed at five different weight
    states (the states an eager run went through) and their gradients compared with the eager run's at the same state --
    no Adam step in between that would turn a last-bit difference into a sign flip of the first updates."""
    from percivaltts_amd import optimizertts_wgan, ops
    ops.deterministic(True)
    try:
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = build('default')
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        opt.generator_updates = 26
        Xd, Yd = f32(X), f32(Y)
        ag = torch.Generator().manual_seed(17)
        alphas = [torch.rand(Xd.shape[0], generator=ag).cuda() for _ in range(5)]
        moving = [t for k, t in mod.kerasmodel.weights() if 'moving' in k]

        def state():
            return [t.detach().clone() for t in (opt.critic_opti.flat.flat, opt.gen_opti.flat.flat)] + [t.detach().clone() for t in moving]

        def load(st):
            opt.wait_updates()
            opt.critic_opti.flat.flat.copy_(st[0]); opt.gen_opti.flat.flat.copy_(st[1])
            for dst, src in zip(moving, st[2:]): dst.copy_(src)
            opt.critic_opti.flat.epoch += 1; opt.gen_opti.flat.epoch += 1

        trace = []
        for b in range(5):
            st = state()
            lc = opt.critic_step(Xd, Yd, alphas[b]); gc = opt.critic_opti.flat.grad.detach().clone()
            st2 = state()
            lg = opt.generator_step(Xd, Yd); gg = opt.gen_opti.flat.grad.detach().clone()
            trace.append((st, float(lc), gc, st2, float(lg), gg))
        # the same states through the split graphs
        opt.cfg.train_wgan_hipgraph = True; opt.cfg.train_wgan_graph_split = True
        opt._graphed('critic', Xd, Yd, alphas[0]); opt._graphed('generator', Xd, Yd)      # capture (their warm-up steps move the weights)
        for b, (st, lc, gc, st2, lg, gg) in enumerate(trace):
            load(st)
            lc_g = opt._graphed('critic', Xd, Yd, alphas[b])
            opt.wait_updates(); torch.cuda.synchronize()
            close(lc_g, lc, 1e-6, 1e-7, 'critic loss, graph vs eager, state {}'.format(b))
            err = float((opt.critic_opti.flat.grad - gc).norm() / gc.norm())
            assert err < 1e-5, 'critic gradient, state {}: rel L2 {:.3e}'.format(b, err)
            load(st2)
            lg_g = opt._graphed('generator', Xd, Yd)
            opt.wait_updates(); torch.cuda.synchronize()
            close(lg_g, lg, 1e-6, 1e-7, 'generator loss, graph vs eager, state {}'.format(b))
            err = float((opt.gen_opti.flat.grad - gg).norm() / gg.norm())
            assert err < 1e-5, 'generator gradient, state {}: rel L2 {:.3e}'.format(b, err)
        assert len(opt._graphs) == 2
    finally:
        ops.deterministic(False)


@pytest.mark.parametrize('form', ['chain', 'layers'])
def test_bf16_storage_critic_conv_stack(form):
    """BASELINE configs[2] (build extension; the reference is fp32, README.md:166).  form 'chain' (cfg.arch_critic_bf16 = True):
    the WHOLE Conv2D stack per launch with the maps between the layers in the LDS (kl.Conv2DStack -> csrc/conv2d_chain.hip),
    every kernel and every layer's post-activation map in bf16; oracle.critic_forward(bf16_stack='chain') has those roundings.
    form 'layers' (cfg.arch_critic_bf16 = 'layers', the round-2 path): cfg.arch_critic_bf16 keeps the maps between
    the critic's 4 -> 4 channel Conv2D layers, and their gradients, as bf16 in HBM and multiplies in bf16 on the matrix cores
    with fp32 accumulation; master weights, weight gradients, the first layer and everything outside the stack stay fp32.
    Oracle: fp64 with the same roundings (oracle.bf16_st: activation after the LeakyReLU, the kernel's bf16 copy, the stored
    maps) and straight-through gradients.  Derived tolerances: a stored value is off by at most 2^-9 relative, and a
    different summation order can move a stored map by one bf16 ulp (2^-8) where the fp64 sum lies at a rounding boundary, so
    forward values are compared at 2^-7 of the map's scale; the oracle's backward does not round the stored gradient maps
    (7 layers: sqrt(14) x 2^-9 = 0.7 % expected), so gradients are bounded by 3e-2 relative L2 -- and both must stay within
    the bf16 error budget of the fp32 oracle."""
    from percivaltts_amd import optimizertts_wgan, vocoders, modeltts_common, networks_critic, ops
    import percivaltts_amd
    g = dict(ctx=61, spec=65, nm=20, H=32, nctx=1, kctx=21, L=8, C=4, kt=5, kf=5, B=3, T=50)
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = g['H']; cfg.arch_ctx_nbcnnlayers = g['nctx']; cfg.arch_ctx_winlen = g['kctx']
    cfg.arch_gen_nbcnnlayers = g['L']; cfg.arch_gen_nbfilters = g['C']; cfg.arch_gen_winlen = g['kt']
    cfg.arch_spec_freqlen = g['kf']; cfg.train_batch_size = g['B']
    cfg.arch_critic_bf16 = True if form == 'chain' else 'layers'
    omode = 'chain' if form == 'chain' else True
    voc = vocoders.VocoderPML(16000, 0.005, g['spec'], g['nm'])
    mod = modeltts_common.DCNNF0SpecNoiseFeatures(g['ctx'], voc, cfg)
    crit = networks_critic.Critic(voc, g['ctx'], cfg)
    a = O.Arch(g['ctx'], g['spec'], g['nm'], g['H'], g['nctx'], g['kctx'], g['L'], g['C'], g['kt'], g['kf'])
    gw = O.random_weights(O.generator_weight_shapes(a), seed=11)
    cw = O.random_weights(O.critic_weight_shapes(a), seed=12)
    mod.kerasmodel.set_weights([w.numpy() for w in gw]); crit.model.set_weights([w.numpy() for w in cw])
    gen = torch.Generator().manual_seed(5)
    X = torch.rand(g['B'], g['T'], g['ctx'], generator=gen, dtype=torch.float64) * 2 - 1
    Y = torch.randn(g['B'], g['T'], a.outsize, generator=gen, dtype=torch.float64)
    al = torch.rand(g['B'], generator=gen, dtype=torch.float64)
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    from percivaltts_amd import layers as kl
    if form == 'layers':
        modes = [l.bf16 for l in crit.model.layers_list if isinstance(l, kl.Conv2D)]
        assert modes == [None] + ['out16'] * 6 + ['out32'], modes
    else:
        assert sum(isinstance(l, kl.Conv2DStack) for l in crit.model.layers_list) == 1
        assert [tuple(w.shape) for w in crit.model.get_weights()] == [tuple(w.shape) for w in cw]
    Xd, Yd, ald = f32(X), f32(Y), f32(al)

    # ---- forward
    with torch.no_grad(), ops._hip.KernelTimer() as kt:
        v = crit.model(Yd, Xd, training=False)
    if form == 'layers':
        assert sum(1 for r in kt.records if r[0] == 'ptts_conv2d_mfma_fwd' and r[1][-1] == 1) == 7      # one-plane kernels
    else:
        assert [r[0] for r in kt.records if r[0].startswith('ptts_conv2d')] in (['ptts_conv2d_chain_fwd'], ['ptts_conv2d_chain_tables', 'ptts_conv2d_chain_fwd'])
    v16 = O.critic_forward(cw, a, Y, X, bf16_stack=omode)
    v32 = O.critic_forward(cw, a, Y, X)
    scale = float(v16.abs().mean())
    assert float((v.double().cpu() - v16).abs().max()) < 2.0 ** -7 * max(scale, float(v16.abs().max())), 'critic forward vs bf16 oracle'
    rel16 = float((v.double().cpu() - v16).norm() / v16.norm()); rel32 = float((v.double().cpu() - v32).norm() / v32.norm())
    assert rel16 < 3e-3 and rel32 < 3e-2 and rel16 < rel32, (rel16, rel32)

    # ---- critic step: loss parts and gradients (first and second order through the bf16 maps)
    for w in cw: w.requires_grad_(True)
    total, parts = O.critic_step_loss(cw, gw, a, X, Y, al, gp_lambda=10.0, bf16_stack=omode)
    grads = torch.autograd.grad(total, cw)
    opt.critic_opti.zero_grad()
    with ops.deferred_weight_grads(), ops._hip.KernelTimer() as kt2:
        tot_d, (lv, lf, gp) = opt.critic_loss(Xd, Yd, ald, training=True)
        tot_d.backward()
    if form == 'chain':
        names = [r[0] for r in kt2.records if r[0].startswith('ptts_conv2d_chain')]
        # forward of the stacked real+fake pass and of x_hat, backward-data + gamma maps of the gradient penalty, its second-order
        # sweep, and ONE weight-gradient chain for the stacked pass
        assert sorted(n for n in names if n != 'ptts_conv2d_chain_tables') == sorted(['ptts_conv2d_chain_fwd'] * 2 + ['ptts_conv2d_chain_bwd_data', 'ptts_conv2d_chain_second', 'ptts_conv2d_chain_bwd']), names
    close(lv, parts['valid'], 5e-3, 1e-4, 'L valid (bf16)')
    close(lf, parts['fake'], 5e-3, 1e-4, 'L fake (bf16)')
    close(gp, parts['gp'], 2e-2, 1e-4, 'gradient penalty (bf16)')
    num = den = 0.0
    for p, g_ in zip(opt.critic_opti.flat.params, grads):
        assert p.grad.dtype == torch.float32
        num += float((p.grad.detach().cpu().double() - g_.detach()).pow(2).sum()); den += float(g_.detach().pow(2).sum())
    assert num <= (3e-2 ** 2) * den, 'critic gradients (bf16 stack): relative L2 error {:.3e}'.format((num / den) ** 0.5)
    # the generator step through the frozen bf16 critic runs and is finite
    lg = opt.generator_step(Xd, Yd)
    assert torch.isfinite(lg) and torch.isfinite(opt.gen_opti.flat.grad).all()
