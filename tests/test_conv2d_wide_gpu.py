"""The wide / non-square Conv2D tier (csrc/conv2d_wide.hip) against the fp64 oracle: op level in the pattern and at the
tolerances of tests/test_ops_gpu.py::test_conv2d_forward_backward, the second-order sweep and the deferred queue at those of
tests/test_deferred.py, the networks at those of tests/test_model_gpu.py.  Every case also asserts which entry points ran."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

pytestmark = pytest.mark.gpu

RT, AT = 1e-4, 1e-5                        # y, dx
W_TOL = dict(rtol=2e-4, atol=1e-4)         # dw, db
REDUCE = 'ptts_conv2d_reduce_grouped'
WIDE = ('ptts_conv2d_wide_fwd', 'ptts_conv2d_wide_bwd_partials')
GENERIC = ('ptts_conv2d_fwd', 'ptts_conv2d_bwd', 'ptts_conv2d_bwd_partials')


def dev(t, grad=False):
    return t.detach().to(torch.float32).cuda().contiguous().requires_grad_(grad)


def ref(t, grad=False):
    return t.detach().to(torch.float64).cpu().requires_grad_(grad)


def param(t):
    p = dev(t, True)
    p.grad = torch.zeros_like(p)
    return p


def gen(seed):
    return torch.Generator().manual_seed(seed)


def names(kt, start=0):
    return [r[0] for r in kt.records[start:]]


def close(got, want, rtol=RT, atol=AT, what=''):
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().to(torch.float64)
    assert got.shape == want.shape, '{}: shape {} vs {}'.format(what, tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    print('{}: worst err/tol {:.3f}'.format(what, float((err / tol).max())))
    bad = err > tol
    if bad.any():
        i = int(torch.argmax(err - tol))
        raise AssertionError('{}: {} / {} mismatches, worst |err|={:.3e} at flat {} (got {:.6e}, want {:.6e}), max|want|={:.3e}'.format(
            what, int(bad.sum()), bad.numel(), float(err.flatten()[i]), i, float(got.flatten()[i]),
            float(want.flatten()[i]), float(want.abs().max())))


@pytest.fixture
def ops():
    from percivaltts_amd import ops as _ops
    old = _ops.deterministic()
    _ops.deterministic(False)
    _ops.conv2d_wide(True)
    try:
        yield _ops
    finally:
        _ops.deterministic(old)
        _ops.conv2d_wide(None)
    assert not (_ops._Deferred.active or _ops._Deferred.items or _ops._Deferred.conv_items or _ops._Deferred.streams)


CASES = [
    # B, T, F, Cin, Cout, KT, KF, dil, causal
    (2, 12, 9, 8, 8, 5, 5, 1, False), (2, 12, 9, 1, 8, 5, 5, 1, False), (2, 12, 9, 8, 1, 5, 5, 1, False),      # the layers of a wide stack
    (2, 12, 9, 4, 16, 3, 3, 1, False), (2, 12, 9, 16, 4, 3, 3, 1, False), (2, 12, 9, 12, 8, 7, 7, 1, False),   # unequal counts, 12, 7x7
    (2, 20, 17, 4, 4, 5, 3, 1, False), (2, 20, 17, 4, 4, 3, 7, 1, False), (2, 12, 9, 1, 4, 7, 5, 1, False),    # non-square windows
    (2, 12, 9, 4, 1, 3, 5, 1, False),
    (3, 100, 65, 16, 16, 3, 3, 1, False), (1, 37, 129, 8, 8, 5, 5, 1, False),      # time tiles, ragged last tile, frequency blocks
    (2, 50, 33, 8, 8, 5, 5, 2, True), (1, 9, 6, 8, 8, 5, 5, 8, True),              # dilated causal; a span longer than T
    (1, 3, 2, 8, 8, 5, 5, 1, False), (1, 1, 5, 8, 8, 5, 5, 1, False),              # an image smaller than the window
]
INELIGIBLE = (2, 10, 7, 3, 5, 3, 3, 1, False)


@functools.lru_cache(maxsize=None)
def op_case(case, mode):
    """fp64: the inputs and (y, dx, dw, db, dscale, dshift) of one layer."""
    B, T, F, Cin, Cout, KT, KF, dil, causal = case
    g = gen(1)
    x = torch.randn(B, T, F, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(KT, KF, Cin, Cout, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    sc = torch.rand(Cin, generator=g, dtype=torch.float64) + 0.5
    sh = torch.randn(Cin, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(B, T, F, Cout, generator=g, dtype=torch.float64)
    xr, wr, br, scr, shr = ref(x, True), ref(w, True), ref(b, True), ref(sc, True), ref(sh, True)
    a = xr if mode == 'none' else O.lrelu(xr) if mode == 'lrelu' else O.lrelu(xr * scr + shr)
    yr = O.conv2d_nhwc(a, wr, br, dil_t=dil, causal=causal)
    yr.backward(dy)
    return (x, w, b, sc, sh, dy), (yr.detach(), xr.grad, wr.grad, br.grad, scr.grad, shr.grad)


def run_layer(ops, case, mode, leaves=None):
    """Forward and backward of the layer on the device; returns (y, leaves = (x, w, b, scale, shift))."""
    B, T, F, Cin, Cout, KT, KF, dil, causal = case
    (x, w, b, sc, sh, dy), _ = op_case(case, mode)
    xd, wd, bd, scd, shd = leaves or (dev(x, True), dev(w, True), dev(b, True), dev(sc, True), dev(sh, True))
    v = xd if mode == 'none' else ops.Lazy(xd, lrelu=True) if mode == 'lrelu' else ops.Lazy(xd, scd, shd, lrelu=True)
    yd = ops.conv2d(v, wd, bd, dil_t=dil, pad_mode=ops.PAD_CAUSAL if causal else ops.PAD_SAME)
    yd.backward(dev(dy))
    return yd, (xd, wd, bd, scd, shd)


def check_layer(case, mode, yd, leaves, times=1):
    B, T, F = case[:3]
    _, (y, dx, dw, db, dsc, dsh) = op_case(case, mode)
    xd, wd, bd, scd, shd = leaves
    if yd is not None:
        close(yd, y, what='y')
    close(xd.grad, times * dx, what='dx')
    close(wd.grad, times * dw, what='dw', **W_TOL)
    close(bd.grad, times * db, what='db', **W_TOL)
    if mode == 'affine':
        at = max(1e-4, 5e-8 * B * T * F)
        close(scd.grad, times * dsc, rtol=2e-4, atol=at, what='dscale')
        close(shd.grad, times * dsh, rtol=2e-4, atol=at, what='dshift')


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('mode', ['none', 'lrelu', 'affine'])
def test_conv2d_wide_forward_backward(ops, case, mode):
    with ops._hip.KernelTimer() as kt:
        yd, leaves = run_layer(ops, case, mode)
    ran = names(kt)
    assert ran.count(WIDE[0]) == 1 and ran.count(WIDE[1]) == 1, ran
    assert not any(k in ran for k in GENERIC), ran
    check_layer(case, mode, yd, leaves)


@pytest.mark.parametrize('mode', ['none', 'lrelu', 'affine'])
def test_ineligible_shape_keeps_the_generic_kernels(ops, mode):
    with ops._hip.KernelTimer() as kt:
        yd, leaves = run_layer(ops, INELIGIBLE, mode)
    ran = names(kt)
    assert ran.count('ptts_conv2d_fwd') == 1 and ran.count('ptts_conv2d_bwd') == 1 and not any(k in ran for k in WIDE), ran
    check_layer(INELIGIBLE, mode, yd, leaves)


@pytest.mark.parametrize('mode', ['none', 'lrelu', 'affine'])
def test_switch_off_sends_an_eligible_shape_to_the_generic_kernels(ops, mode):
    ops.conv2d_wide(False)
    with ops._hip.KernelTimer() as kt:
        yd, leaves = run_layer(ops, CASES[0], mode)
    ran = names(kt)
    assert ran.count('ptts_conv2d_fwd') == 1 and ran.count('ptts_conv2d_bwd') == 1 and not any(k in ran for k in WIDE), ran
    check_layer(CASES[0], mode, yd, leaves)


@pytest.mark.parametrize('call_name', ['fwd', 'bwd'])
def test_entry_points_refuse_an_unsupported_shape(ops, call_name):
    """An unsupported shape is an error code and no launch (the outputs keep their fill)."""
    from percivaltts_amd.ops import ptr, stream
    import ctypes
    B, T, F, Cin, Cout, K = 1, 4, 5, 3, 5, 3
    x = torch.zeros(B, T, F, Cin, device='cuda'); w = torch.zeros(K, K, Cin, Cout, device='cuda')
    y = torch.full((B, T, F, Cout), 7.0, device='cuda'); dx = torch.full((B, T, F, Cin), 7.0, device='cuda')
    lib = ops._hip.lib()
    if call_name == 'fwd':
        rc = lib.ptts_conv2d_wide_fwd(ptr(x), ptr(w), None, None, None, None, ptr(y), B, T, F, Cin, Cout, K, K, 1, 0, 0, 0.3, stream())
    else:
        nb, npart = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.ptts_conv2d_wide_bwd_partials(ptr(y), ptr(x), ptr(w), None, None, None, ptr(dx), None, 0, ctypes.byref(nb),
                                               ctypes.byref(npart), 0, 0, B, T, F, Cin, Cout, K, K, 1, 0, 0, 0.3, stream())
    assert rc != 0 and 'unsupported shape' in ops._hip.last_error()
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(dx.min()) == 7.0


SECOND = [(2, 12, 9, 8, 8, 5, 5, 1, False), (2, 20, 17, 4, 4, 5, 3, 1, False)]


@functools.lru_cache(maxsize=None)
def second_order_case(case):
    """fp64: R, and the gradients of sum((d sum(R . y) / dx)^2) with respect to the kernel and to R."""
    B, T, F, Cin, Cout, KT, KF, dil, causal = case
    (x, w, b, _, _, dy), _ = op_case(case, 'lrelu')
    R = torch.randn(*dy.shape, generator=gen(32), dtype=torch.float64)
    xr, wr, Rr = (t.clone().requires_grad_(True) for t in (x, w, R))
    y = O.conv2d_nhwc(O.lrelu(xr), wr, b, dil_t=dil, causal=causal)
    gx = torch.autograd.grad(y, xr, Rr, create_graph=True)[0]
    (gx * gx).sum().backward()
    return R, wr.grad, Rr.grad


@pytest.mark.parametrize('deferred', [True, False], ids=['deferred', 'immediate'])
@pytest.mark.parametrize('case', SECOND)
def test_second_order_sweep(ops, case, deferred):
    """The gradient penalty's pattern through one layer: backward data, then its masked forward and weight gradient."""
    (x, w, b, _, _, _), _ = op_case(case, 'lrelu')
    R, dw64, dR64 = second_order_case(case)
    xd, wd, bd, Rd = dev(x, True), param(w), param(b), dev(R, True)
    with ops._hip.KernelTimer() as kt:
        with (ops.deferred_weight_grads() if deferred else contextlib.nullcontext()):
            y = ops.conv2d(ops.Lazy(xd, lrelu=True), wd, bd)
            with ops.input_grad_only():
                gx = torch.autograd.grad(y, xd, grad_outputs=Rd, create_graph=True)[0]
            n1 = len(kt.records)
            (gx * gx).sum().backward()
            inside, items = names(kt, n1), list(ops._Deferred.conv_items)
    ran = names(kt)
    assert not any(k in ran for k in GENERIC), ran
    assert inside.count(WIDE[0]) == 1 and inside.count(WIDE[1]) == 1, inside       # the masked forward, the sweep's dW
    if deferred:
        assert REDUCE not in inside and len(items) == 1 and items[0][6] is wd.grad and items[0][7] is None, inside
    else:
        assert inside.count(REDUCE) == 1 and not items, inside
    assert float(bd.grad.abs().max()) == 0.0
    close(wd.grad, dw64, what='second-order dw', **W_TOL)
    close(Rd.grad, dR64, what='second-order dR', **W_TOL)


def test_deferred_queue(ops):
    """Queued rows leave the gradient buffer alone until the context exits, then ONE grouped reduction; two passes add up; the
    immediate path gives the same values."""
    case = CASES[0]
    (x, w, b, _, _, _), _ = op_case(case, 'lrelu')
    leaves = (dev(x, True), param(w), param(b), None, None)
    with ops._hip.KernelTimer() as kt:
        with ops.deferred_weight_grads():
            run_layer(ops, case, 'lrelu', leaves)
            inside, queued, early = names(kt), len(ops._Deferred.conv_items), float(leaves[1].grad.abs().max())
            run_layer(ops, case, 'lrelu', leaves)
            assert len(ops._Deferred.conv_items) == 2 and float(leaves[1].grad.abs().max()) == 0.0
        total = names(kt)
    assert queued == 1 and early == 0.0 and REDUCE not in inside and inside.count(WIDE[1]) == 1, (queued, early, inside)
    assert total.count(REDUCE) == 1 and not any(k in total for k in GENERIC), total
    check_layer(case, 'lrelu', None, leaves, times=2)
    _, now = run_layer(ops, case, 'lrelu')                   # immediate: gradients through autograd
    close(leaves[1].grad, 2 * now[1].grad.double().cpu(), what='deferred vs immediate dw', **W_TOL)
    close(leaves[2].grad, 2 * now[2].grad.double().cpu(), what='deferred vs immediate db', **W_TOL)


def test_deterministic_mode_is_bit_identical(ops):
    case = CASES[10]
    assert case[:5] == (3, 100, 65, 16, 16)
    ops.deterministic(True)
    runs = []
    for _ in range(2):
        yd, leaves = run_layer(ops, case, 'affine')
        runs.append([yd.detach().clone()] + [t.grad.clone() for t in leaves])
    for p, q in zip(*runs):
        assert torch.equal(p, q)
    check_layer(case, 'affine', runs[1][0], leaves)


# ---------------------------------------------------------------------------------------------------------------------------
# model level: the DCNN and the critic with wide / non-square stacks (the checks of tests/test_model_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
_WIDE = dict(ctx=31, spec=33, nm=5, H=16, nctx=1, kctx=5, L=3, C=8, kt=5, kf=5, B=2, T=40)
GEOMS = {
    'wide': dict(_WIDE),
    'wide16': dict(_WIDE, spec=17, L=2, C=16, kt=3, kf=3, T=24),
    'nonsquare': dict(_WIDE, L=2, C=4, kt=5, kf=3),
    'wide_gated_dilated': dict(_WIDE, C=8, L=3, gated=True, dils=[1, 2, 4], causal=True, T=70),
}


def mclose(got, want, rtol, atol, what='', kinks=False):
    """tests/test_model_gpu.py::close."""
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


def build(geom):
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common, networks_critic
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
    gn = torch.Generator().manual_seed(5)
    X = torch.rand(g['B'], g['T'], g['ctx'], generator=gn, dtype=torch.float64) * 2 - 1
    Y = torch.randn(g['B'], g['T'], a.outsize, generator=gn, dtype=torch.float64)
    Y[:, :, 1 + g['spec']:] = torch.rand(g['B'], g['T'], g['nm'], generator=gn, dtype=torch.float64)
    al = torch.rand(g['B'], generator=gn, dtype=torch.float64)
    return cfg, voc, mod, crit, a, gw, cw, X, Y, al


def f32(t):
    return t.to(torch.float32).cuda().contiguous()


@pytest.mark.parametrize('geom', list(GEOMS))
def test_predict_and_critic_forward(ops, geom):
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build(geom)
    want = O.generator_forward(gw, a, X, training=False)
    with ops._hip.KernelTimer() as kt:
        got = mod.predict(X.numpy().astype(np.float32))
        dv = mod.to_device()
        crit.model.to(dv)
        with torch.no_grad():
            v = crit.model(f32(Y), f32(X), training=False)
            gt = mod.kerasmodel(f32(X), training=True, memo={'freeze_bn_stats': True})
    ran = names(kt)
    assert WIDE[0] in ran and not any(k in ran for k in GENERIC), ran
    mclose(got, want, 5e-4, 5e-5, 'predict (BN inference)')
    mclose(v, O.critic_forward(cw, a, Y, X), 5e-4, 5e-5, 'critic forward')
    mclose(gt, O.generator_forward(gw, a, X, training=True), 5e-4, 5e-5, 'generator forward (BN batch statistics)')


@pytest.mark.parametrize('geom', list(GEOMS))
def test_critic_and_generator_steps(ops, geom):
    """tests/test_model_gpu.py::test_critic_and_generator_steps with errtype WLSWGAN; the critic's gradients must meet the
    elementwise bound (kinks=False): the fp32 oracle does at these geometries and seeds."""
    from percivaltts_amd import optimizertts_wgan
    errtype = 'WLSWGAN'
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = build(geom)
    cfg.train_wgan_critic_LSWGANtransidx = 30.0
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype=errtype, critic=crit)
    opt.prepare()
    Xd, Yd, ald = f32(X), f32(Y), f32(al)
    kt = ops._hip.KernelTimer()

    for w in cw: w.requires_grad_(True)
    total, parts = O.critic_step_loss(cw, gw, a, X, Y, al, gp_lambda=10.0)
    grads = torch.autograd.grad(total, cw)
    opt.critic_opti.zero_grad()
    with kt:
        tot_d, (lv, lf, gp) = opt.critic_loss(Xd, Yd, ald, training=True)
        tot_d.backward()
    mclose(lv, parts['valid'], 5e-4, 1e-5, 'L valid')
    mclose(lf, parts['fake'], 5e-4, 1e-5, 'L fake')
    mclose(gp, parts['gp'], 5e-4, 1e-5, 'gradient penalty')
    mclose(tot_d, total, 5e-4, 1e-5, 'critic loss')
    gmax = max(float(g.abs().max()) for g in grads)
    num = den = 0.0
    for p, g_ in zip(opt.critic_opti.flat.params, grads):
        mclose(p.grad, g_, 1e-3, 2e-5 * max(gmax, 1.0) + 1e-6, 'critic grad {}'.format(tuple(g_.shape)), kinks=False)
        num += float((p.grad.detach().cpu().double() - g_.detach()).pow(2).sum()); den += float(g_.detach().pow(2).sum())
    print('critic gradients: relative L2 error {:.3e}'.format((num / den) ** 0.5))
    assert num <= (3e-3 ** 2) * den, 'critic gradients: relative L2 error {:.3e} over all tensors'.format((num / den) ** 0.5)
    ms = [torch.zeros_like(w) for w in cw]; vs = [torch.zeros_like(w) for w in cw]
    with torch.no_grad():
        cw2 = [w.detach().clone() for w in cw]
    O.adam_keras(cw2, grads, ms, vs, 1, 1e-4, 0.5, 0.9, 1e-7)
    opt.critic_opti.step()
    for p, w_new, w_old, g_ in zip(opt.critic_opti.flat.params, cw2, cw, grads):
        big = g_.abs() > 1e-3 * gmax
        mclose((p.detach().cpu().double() - w_old.detach())[big], (w_new - w_old.detach())[big], 2e-2, 1e-7, 'critic Adam move')

    cw_now = [p.detach().cpu().double() for _, p in crit.model.weights()]
    gw_t = [w.detach().clone() for w in gw]
    shapes = O.generator_weight_shapes(a)
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
    with kt:
        ltot_d, (lw_d, lls_d) = opt.generator_loss(Xd, Yd, training=True)
        ltot_d.backward()
    for p in opt.critic_opti.flat.params: p.requires_grad_(True)
    mclose(lw_d, lparts['wgan'], 5e-4, 1e-5, 'generator wgan term')
    mclose(lls_d, lparts['ls'], 5e-4, 1e-5, 'generator ls term')
    mclose(ltot_d, ltot, 5e-4, 1e-5, 'generator loss')
    ggmax = max(float(g.abs().max()) for g in ggrads if g is not None)
    num = den = 0.0
    for p, g_ in zip(opt.gen_opti.flat.params, ggrads):
        want = g_ if g_ is not None else torch.zeros_like(p, dtype=torch.float64, device='cpu')
        mclose(p.grad, want, 2e-3, 5e-5 * max(ggmax, 1.0) + 1e-6, 'generator grad {}'.format(tuple(p.shape)), kinks=True)
        num += float((p.grad.detach().cpu().double() - want).pow(2).sum()); den += float(want.pow(2).sum())
    assert num <= (3e-3 ** 2) * den, 'generator gradients: relative L2 error {:.3e} over all tensors'.format((num / den) ** 0.5)
    for (k, t), w in zip(mod.kerasmodel.weights(), gw_t):
        if 'moving' in k:
            mclose(t, w, 5e-4, 1e-5, k)
    ran = names(kt)
    assert WIDE[0] in ran and WIDE[1] in ran and not any(k in ran for k in GENERIC), sorted(set(ran))
