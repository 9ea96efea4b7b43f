"""GPU tests of the batched transposed-reduction product ptts_dense_tn_bf16x6_batched (csrc/dense.hip) and of the weight gradient of
the frequency-domain context Conv1D built on it (ops._C1FFT.wgrad with ops._C1FFT.tn_enabled): the per-frequency correlations read
their fp32 operands as they lie, without the split of the input's transform and the transpose of the gradient's.  The gradient's own
DFT keeps its 'dy' ptts_split3_frame_windows call and its ptts_dense_bf16x6_batched product."""
import ctypes
import gc
import math

import pytest
import torch

from oracle import percival_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.625          # exactly representable: an untouched cell compares equal bit for bit


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tn_call(ops, A, sA, B, sB, C, sC, nbatch, M, Kin, N, lda, ldb, ldc, planes=3, a_off=0):
    h = ops._hip
    pa = ctypes.c_void_p(A.data_ptr() + a_off)
    h.call('ptts_dense_tn_bf16x6_batched', pa, sA, h.ptr(B), sB, h.ptr(C), sC, nbatch, M, Kin, N, lda, ldb, ldc, planes, h.stream())
    torch.cuda.synchronize()


def tn_case(M, Kin, N, nbatch, shared_a=False, lda=None, ldc=None, interleaved_c=False, seed=3):
    """Operands of one case on the host (fp32) and the geometry of C: (A, B, strides, leading dims, C's float count, index of cell
    (z, k, n) in C).  interleaved_c: row k of member z lies at (k nbatch + z) N -- the layout the gradient's DFT writes."""
    g = gen(seed + M + N)
    lda = lda or Kin
    A = torch.zeros(1 if shared_a else nbatch, M, lda)
    A[:, :, :Kin] = torch.randn(A.shape[0], M, Kin, generator=g)
    B = torch.randn(nbatch, M, N, generator=g)
    if interleaved_c:
        ldc, sC, rows = nbatch * N, N, (Kin + 3) // 4 * 4          # (the rows behind the guard exist and must stay untouched)
        numel = rows * ldc
    else:
        ldc = ldc or N
        rows = Kin + 8
        sC, numel = rows * ldc, nbatch * rows * ldc
    return A, B, (0 if shared_a else M * lda), M * N, sC, lda, ldc, numel


def run_tn(ops, M, Kin, N, nbatch, planes=3, **kw):
    A, B, sA, sB, sC, lda, ldc, numel = tn_case(M, Kin, N, nbatch, **kw)
    C = torch.full((numel,), SENTINEL, device='cuda')
    tn_call(ops, A.cuda(), sA, B.cuda(), sB, C, sC, nbatch, M, Kin, N, lda, N, ldc, planes)
    C = C.cpu()
    idx = (torch.arange(nbatch).view(-1, 1, 1) * sC + torch.arange(Kin).view(1, -1, 1) * ldc + torch.arange(N).view(1, 1, -1)).reshape(-1)
    got = C[idx].view(nbatch, Kin, N).double()
    untouched = torch.ones(numel, dtype=torch.bool)
    untouched[idx] = False
    assert bool((C[untouched] == SENTINEL).all()), 'cells outside the guards were written: {} of {}'.format(
        int((C[untouched] != SENTINEL).sum()), int(untouched.sum()))
    assert int(untouched.sum()) > 0
    return A[:, :, :Kin], B, got


TN_SHAPES = {
    # less than one slab of 32 rows; one partial tile in each direction; a gap between N and ldc
    'sub_slab': dict(M=24, Kin=32, N=144, nbatch=3, ldc=160),
    # the gradient transform's addressing: a shared left operand with two zero pad columns, the store guarded at 122, the members' rows interleaved
    'dft_addressing': dict(M=100, Kin=122, N=256, nbatch=5, shared_a=True, lda=124, interleaved_c=True),
    # the correlation's tiles: two row tiles, nine column tiles and a half-filled tenth
    'correlation': dict(M=512, Kin=256, N=1216, nbatch=2, ldc=1216 + 4),
    # many members
    'many_members': dict(M=96, Kin=256, N=128, nbatch=61),
}


@pytest.mark.parametrize('name', sorted(TN_SHAPES))
def test_tn_product_against_fp64(ops, name):
    """C_z = A_z^T B_z per batch member against the fp64 product of the same fp32 operands: relative L2 <= 3e-6, the bound the Dense
    weight-gradient product (the same construction) is held to in test_ops_gpu.py; every cell of C outside [Kin] x [N] of every
    member keeps the sentinel it was filled with."""
    A, B, got = run_tn(ops, **TN_SHAPES[name])
    want = torch.matmul(A.double().transpose(1, 2), B.double())           # (a shared A broadcasts)
    for z in range(B.shape[0]):
        e = float((got[z] - want[z]).norm() / want[z].norm())
        print('{} member {}: rel L2 {:.3e}'.format(name, z, e))
        assert e <= 3e-6, (name, z, e)


def test_tn_product_one_plane(ops):
    """planes_count = 1: one product of the operands' bf16 roundings with fp32 accumulation, against the fp64 product of the rounded
    operands; what is left is the fp32 summation order: 3e-5 of the mean magnitude, the bound of the one-product Conv1D kernels."""
    A, B, got = run_tn(ops, planes=1, **TN_SHAPES['correlation'])
    bf = lambda t: t.to(torch.bfloat16).double()
    want = torch.matmul(bf(A).transpose(1, 2), bf(B))
    e = float((got - want).abs().max() / want.abs().mean())
    print('one plane: max error {:.3e} of the mean magnitude'.format(e))
    assert e < 3e-5, e


def test_tn_product_refuses_bad_arguments(ops):
    M, Kin, N, nb = 32, 64, 64, 2
    A = torch.zeros(nb * M * Kin + 8, device='cuda'); B = torch.zeros(nb * M * N + 8, device='cuda'); C = torch.zeros(nb * Kin * N + 8, device='cuda')
    good = dict(sA=M * Kin, sB=M * N, sC=Kin * N, nbatch=nb, M=M, Kin=Kin, N=N, lda=Kin, ldb=N, ldc=N)
    tn_call(ops, A, good['sA'], B, good['sB'], C, good['sC'], nb, M, Kin, N, Kin, N, N)          # the good call passes
    bad = [dict(lda=Kin + 2), dict(ldb=N + 1), dict(ldc=N + 2), dict(sA=M * Kin + 2), dict(sB=M * N + 1), dict(sC=Kin * N + 2),
           dict(lda=Kin - 4), dict(ldc=N - 4), dict(planes=2), dict(nbatch=0), dict(M=0), dict(a_off=4)]
    for change in bad:
        a = dict(good, planes=3, a_off=0); a.update(change)
        with pytest.raises(ops._hip.HipLibraryError):
            tn_call(ops, A, a['sA'], B, a['sB'], C, a['sC'], a['nbatch'], a['M'], a['Kin'], a['N'], a['lda'], a['ldb'], a['ldc'], a['planes'], a['a_off'])


# ---- the weight gradient of the layer, both stage lists ------------------------------------------------------------------------------

_REF = {}


def conv_case(case):
    """Operands (fp64 values of fp32 numbers) and the fp64 weight gradient of a case, computed once."""
    if case not in _REF:
        B, T, Cin, N, KW = case
        g = gen(91 + B)
        x = torch.randn(B, T, Cin, generator=g).double()
        w = (torch.randn(KW, Cin, N, generator=g) / math.sqrt(KW * Cin)).double()
        b = torch.randn(N, generator=g).double()
        dy = torch.randn(B, T, N, generator=g).double()
        wr = w.clone().requires_grad_(True)
        O.conv1d_ntc(x, wr, b).backward(dy)
        _REF[case] = (x, w, b, dy, wr.grad.detach())
    return _REF[case]


def layer_wgrad(ops, case, tn, bf16=False):
    """dW and the (name, tag) list of the backward's launches with the switch at `tn`."""
    x, w, b, dy, _ = conv_case(case)
    f = lambda t: t.float().cuda().contiguous()
    saved = ops._C1FFT.tn_enabled
    ops._C1FFT.tn_enabled = tn
    ops.clear_caches()
    if bf16:
        ops.bf16_products(True)
    try:
        wd = f(w).requires_grad_(True)
        y = ops.conv1d(f(x), wd, f(b))
        with ops._hip.KernelTimer() as kt:
            y.backward(f(dy))
        torch.cuda.synchronize()
    finally:
        ops._C1FFT.tn_enabled = saved
        if bf16:
            ops.bf16_products(False)
        ops.clear_caches()
    return wd.grad.double().cpu(), [(r[0], r[1]) for r in kt.records]


def is_new_list(tags):
    """True: the stage list on the new entry point; False: the older one; None: no frequency-domain weight gradient at all."""
    has = lambda name, tag0=None: any(n == name and (tag0 is None or (t and t[0] == tag0)) for n, t in tags)
    count_new = sum(1 for n, _ in tags if n == 'ptts_dense_tn_bf16x6_batched')
    common = [has('ptts_split3_frame_windows', 'dy'), has('ptts_dense_bf16x6_batched', 'dft_dy')]       # the gradient's DFT, in both
    old_parts = [has('ptts_transpose_batched'), has('ptts_split3_dense_weight_strided', 'xw'), has('ptts_dense_bf16x6_batched', 'corr')]
    if count_new == 1 and all(common) and not any(old_parts):
        return True
    if count_new == 0 and all(common) and all(old_parts):
        return False
    if count_new == 0 and not any(common + old_parts) and not has('ptts_conv1d_freq_wgrad_inverse') and not has('ptts_conv1d_freq_wgrad_combine'):
        return None                       # the time-domain weight gradient
    raise AssertionError('neither stage list: {}'.format(tags))


@pytest.mark.parametrize('seg', [100, 0], ids=['segments', 'whole'])
@pytest.mark.parametrize('case', [(16, 256, 70, 32, 5), (5, 1000, 64, 16, 3), (12, 400, 601, 256, 21)])
def test_wgrad_new_against_old_and_fp64(ops, case, seg):
    """Both stage lists within 2e-5 relative L2 of the fp64 gradient (the bound of test_conv1d_frequency_domain_forward) and within
    4e-5 of each other (twice that bound: each may be off by it in another direction).  An odd number of segments in the batch (five
    whole utterances) takes the time-domain kernel whatever the switch says, as before; the bounds hold there too."""
    B, T, Cin, N, KW = case
    want = conv_case(case)[4]
    seg0 = ops._C1FFT.seg_target
    ops._C1FFT.seg_target = seg
    try:
        g_new, tags_new = layer_wgrad(ops, case, True)
        g_old, tags_old = layer_wgrad(ops, case, False)
        nseg = B * (T // ops._C1FFT.segment(T, KW))
    finally:
        ops._C1FFT.seg_target = seg0
    if nseg % 2 == 0:
        assert is_new_list(tags_new) is True and is_new_list(tags_old) is False
    else:
        assert is_new_list(tags_new) is None and is_new_list(tags_old) is None
    e_new = float((g_new - want).norm() / want.norm())
    e_old = float((g_old - want).norm() / want.norm())
    e_pair = float((g_new - g_old).norm() / want.norm())
    print('{} seg {}: new {:.3e}, old {:.3e}, new against old {:.3e}'.format(case, seg, e_new, e_old, e_pair))
    assert e_new <= 2e-5 and e_old <= 2e-5, (e_new, e_old)
    assert e_pair <= 4e-5, e_pair


def test_wgrad_launch_lists(ops):
    """Switch on, fp32 arithmetic: the new entry once (the correlation) and neither the transpose nor the 'xw' split.  Switch off, or
    one-product bf16 arithmetic: the older list, with its 'corr'-tagged ptts_dense_bf16x6_batched."""
    case = (16, 256, 70, 32, 5)
    assert ops._C1FFT.tn_enabled, 'the switch is on by default'
    assert is_new_list(layer_wgrad(ops, case, True)[1]) is True
    assert is_new_list(layer_wgrad(ops, case, False)[1]) is False
    assert is_new_list(layer_wgrad(ops, case, True, bf16=True)[1]) is False
    assert is_new_list(layer_wgrad(ops, case, False, bf16=True)[1]) is False


def _small_critic_step_setup():
    """A critic / generator pair at 4096 frames with a 64-channel context (the smallest the frequency-domain path takes), seeded weights
    and one batch: (optimiser, the context Conv1D's kernel parameter, X, Y, alpha)."""
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common, networks_critic, optimizertts_wgan
    ctx, spec, nm, H, B, T, KW = 64, 65, 20, 32, 8, 512, 21
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = H; cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = KW
    cfg.arch_gen_nbcnnlayers = 2; cfg.arch_gen_nbfilters = 4; cfg.arch_gen_winlen = 5; cfg.arch_spec_freqlen = 5
    cfg.train_batch_size = B
    voc = vocoders.VocoderPML(16000, 0.005, spec, nm)
    mod = modeltts_common.DCNNF0SpecNoiseFeatures(ctx, voc, cfg)
    crit = networks_critic.Critic(voc, ctx, cfg)
    a = O.Arch(ctx, spec, nm, H, 1, KW, 2, 4, 5, 5)
    mod.kerasmodel.set_weights([w.numpy() for w in O.random_weights(O.generator_weight_shapes(a), seed=11)])
    crit.model.set_weights([w.numpy() for w in O.random_weights(O.critic_weight_shapes(a), seed=12)])
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    kernels = [p for p in opt.critic_opti.flat.params if tuple(p.shape) == (KW, ctx, H)]
    assert len(kernels) == 1
    g = gen(5)
    X = (torch.rand(B, T, ctx, generator=g) * 2 - 1).cuda()
    Y = torch.randn(B, T, a.outsize, generator=g).cuda()
    al = torch.rand(B, generator=g).cuda()
    return opt, kernels[0], X, Y, al


def test_graph_replay_equals_eager():
    """One small critic step as a hipGraph captured on a side stream and replayed twice from the same weights, and the same step
    launched eagerly, in deterministic mode: the gradient of the context Conv1D's kernel is the same bit for bit.

    The two forms run on two separately built, identically seeded pairs of networks, the replayed one first and with nothing launched
    eagerly in front of its capture: a parameter's AccumulateGrad node keeps the stream it was created on for as long as an autograd
    graph that holds it is alive, and a node born in an eager step on the default stream would draw that stream into a capture made on
    a side stream (torch warns of exactly this).  In deterministic mode every weight gradient of the step goes through such a node."""
    from percivaltts_amd import ops
    ops.deterministic(True)
    try:
        opt, kernel, X, Y, al = _small_critic_step_setup()
        opt.cfg.train_wgan_hipgraph = True
        snap = opt._state_snapshot()
        gc.collect()
        replays = []
        for i in range(2):
            if i:
                opt._state_restore(snap)                     # (the replayed step ends with the update)
            opt._graphed('critic', X, Y, al)                 # the first call captures (side stream) and replays, the second replays
            opt.wait_updates(); torch.cuda.synchronize()
            replays.append(kernel.grad.detach().clone())
        assert len(opt._graphs) == 1
        opt, kernel, X, Y, al = _small_critic_step_setup()
        opt.cfg.train_wgan_hipgraph = False
        with ops._hip.KernelTimer() as kt:
            opt.critic_step(X, Y, al)
        opt.wait_updates(); torch.cuda.synchronize()
        assert [r[0] for r in kt.records].count('ptts_dense_tn_bf16x6_batched') >= 1, 'the step does not reach the new stage list'
        eager = kernel.grad.detach().clone()
        assert float(eager.abs().max()) > 0
        assert torch.equal(replays[0], eager) and torch.equal(replays[1], eager)
    finally:
        ops.deterministic(False)
        ops.clear_caches()
