"""The critic with cfg.arch_critic_bf16 = 'chain' at the reference's spectrum width (spec_size = 129, run.py:89): the 'chain'
leg of test_model_gpu.py::test_bf16_storage_critic_conv_stack restated at spec=129, nm=33 -- the whole Conv2D stack in one
launch per pass, in three frequency blocks per time tile (csrc/conv2d_chain.hip) -- with that test's oracle
(oracle.critic_forward / critic_step_loss with bf16_stack='chain') and its bounds, whose derivation does not depend on the
width: forward 2^-7 of the scale; loss parts 5e-3 / 5e-3 / 2e-2; all critic gradients 3e-2 relative L2.  And what the other
values of the option select at this width: True keeps the layer-wise bf16 form, 'chain' beyond the kernels' limit is an error."""
import importlib.util
import os

import pytest
import torch

from oracle import percival_oracle as O

pytestmark = pytest.mark.gpu

# close() and f32() of the model tests, unchanged (loaded by path: that file is not edited, and tests/ is no package)
_spec = importlib.util.spec_from_file_location('_model_gpu_helpers', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_model_gpu.py'))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
close, f32 = M.close, M.f32

G = dict(ctx=61, spec=129, nm=33, H=32, nctx=1, kctx=21, L=8, C=4, kt=5, kf=5, B=3, T=50)


def _cfg(bf16):
    import percivaltts_amd
    g = G
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = g['H']; cfg.arch_ctx_nbcnnlayers = g['nctx']; cfg.arch_ctx_winlen = g['kctx']
    cfg.arch_gen_nbcnnlayers = g['L']; cfg.arch_gen_nbfilters = g['C']; cfg.arch_gen_winlen = g['kt']
    cfg.arch_spec_freqlen = g['kf']; cfg.train_batch_size = g['B']
    cfg.arch_critic_bf16 = bf16
    return cfg


def test_critic_chain_at_129_bins():
    from percivaltts_amd import optimizertts_wgan, vocoders, modeltts_common, networks_critic, ops
    from percivaltts_amd import layers as kl
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    g = G
    cfg = _cfg('chain')
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
    assert sum(isinstance(l, kl.Conv2DStack) for l in crit.model.layers_list) == 1
    assert not any(isinstance(l, kl.Conv2D) for l in crit.model.layers_list)
    assert [tuple(w.shape) for w in crit.model.get_weights()] == [tuple(w.shape) for w in cw]
    Xd, Yd, ald = f32(X), f32(Y), f32(al)

    # ---- forward: one chain launch (and the operand tables the first time)
    with torch.no_grad(), ops._hip.KernelTimer() as kt:
        v = crit.model(Yd, Xd, training=False)
    assert [r[0] for r in kt.records if r[0].startswith('ptts_conv2d')] in (['ptts_conv2d_chain_fwd'], ['ptts_conv2d_chain_tables', 'ptts_conv2d_chain_fwd'])
    v16 = O.critic_forward(cw, a, Y, X, bf16_stack='chain')
    v32 = O.critic_forward(cw, a, Y, X)
    scale = float(v16.abs().mean())
    rel16 = float((v.double().cpu() - v16).norm() / v16.norm()); rel32 = float((v.double().cpu() - v32).norm() / v32.norm())
    print('forward: max |d| {:.3e} (scale {:.3e}), rel L2 vs bf16 oracle {:.3e}, vs fp32 oracle {:.3e}'.format(
        float((v.double().cpu() - v16).abs().max()), max(scale, float(v16.abs().max())), rel16, rel32))
    assert float((v.double().cpu() - v16).abs().max()) < 2.0 ** -7 * max(scale, float(v16.abs().max())), 'critic forward vs bf16 oracle'
    assert rel16 < 3e-3 and rel32 < 3e-2 and rel16 < rel32, (rel16, rel32)

    # ---- critic step: loss parts and gradients (first and second order through the bf16 maps)
    for w in cw: w.requires_grad_(True)
    total, parts = O.critic_step_loss(cw, gw, a, X, Y, al, gp_lambda=10.0, bf16_stack='chain')
    grads = torch.autograd.grad(total, cw)
    opt.critic_opti.zero_grad()
    with ops.deferred_weight_grads(), ops._hip.KernelTimer() as kt2:
        tot_d, (lv, lf, gp) = opt.critic_loss(Xd, Yd, ald, training=True)
        tot_d.backward()
    names = [r[0] for r in kt2.records if r[0].startswith('ptts_conv2d_chain')]
    # forward of the stacked real+fake pass and of x_hat, backward-data + gamma maps of the gradient penalty, its second-order
    # sweep, and ONE weight-gradient chain for the stacked pass
    assert sorted(n for n in names if n != 'ptts_conv2d_chain_tables') == sorted(['ptts_conv2d_chain_fwd'] * 2 + ['ptts_conv2d_chain_bwd_data', 'ptts_conv2d_chain_second', 'ptts_conv2d_chain_bwd']), names
    print('loss parts: valid {:.6f} / {:.6f}, fake {:.6f} / {:.6f}, gp {:.6f} / {:.6f}'.format(
        *[float(v.detach()) for v in (lv, parts['valid'], lf, parts['fake'], gp, parts['gp'])]))
    close(lv, parts['valid'], 5e-3, 1e-4, 'L valid (bf16)')
    close(lf, parts['fake'], 5e-3, 1e-4, 'L fake (bf16)')
    close(gp, parts['gp'], 2e-2, 1e-4, 'gradient penalty (bf16)')
    num = den = 0.0
    for p, g_ in zip(opt.critic_opti.flat.params, grads):
        assert p.grad.dtype == torch.float32
        num += float((p.grad.detach().cpu().double() - g_.detach()).pow(2).sum()); den += float(g_.detach().pow(2).sum())
    print('critic gradients: relative L2 error {:.3e}'.format((num / den) ** 0.5))
    assert num <= (3e-2 ** 2) * den, 'critic gradients (bf16 stack): relative L2 error {:.3e}'.format((num / den) ** 0.5)
    # the generator step through the frozen bf16 critic runs and is finite
    lg = opt.generator_step(Xd, Yd)
    assert torch.isfinite(lg) and torch.isfinite(opt.gen_opti.flat.grad).all()


def test_what_the_option_selects_at_129_bins_and_beyond():
    from percivaltts_amd import vocoders, networks_critic, _hip
    from percivaltts_amd import layers as kl
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    g = G
    # True: the rule of the default is one frequency block -- at 129 bins the layer-wise bf16 form, as before
    crit = networks_critic.Critic(vocoders.VocoderPML(16000, 0.005, g['spec'], g['nm']), g['ctx'], _cfg(True))
    assert not any(isinstance(l, kl.Conv2DStack) for l in crit.model.layers_list)
    modes = [l.bf16 for l in crit.model.layers_list if isinstance(l, kl.Conv2D)]
    assert modes == [None] + ['out16'] * 6 + ['out32'], modes
    # ... and at 65 bins the chain, under True and under 'chain' alike
    for opt_value in (True, 'chain'):
        crit = networks_critic.Critic(vocoders.VocoderPML(16000, 0.005, 65, 20), g['ctx'], _cfg(opt_value))
        assert sum(isinstance(l, kl.Conv2DStack) for l in crit.model.layers_list) == 1
    # 'chain' where the library has no chain kernel: an error that names the limit, never another form
    fmax = networks_critic.chain_max_bins()
    assert fmax >= 132 and _hip.lib().ptts_conv2d_chain_supported(fmax, 8, 1, 4, 5, 5) == 1
    assert _hip.lib().ptts_conv2d_chain_supported(fmax + 1, 8, 1, 4, 5, 5) == 0
    with pytest.raises(ValueError) as e:
        networks_critic.Critic(vocoders.VocoderPML(16000, 0.005, fmax + 1, g['nm']), g['ctx'], _cfg('chain'))
    assert str(fmax) in str(e.value) and str(fmax + 1) in str(e.value), str(e.value)
    cfg = _cfg('chain'); cfg.arch_gen_nbfilters = 8
    with pytest.raises(ValueError):
        networks_critic.Critic(vocoders.VocoderPML(16000, 0.005, g['spec'], g['nm']), g['ctx'], cfg)
