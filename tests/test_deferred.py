"""The deferred weight-gradient queue of percivaltts_amd/ops.py (_Deferred, deferred_weight_grads, flush_weight_grads).

CPU: the queue's bookkeeping with faked streams -- objects with `cuda_stream` and a recording `wait_stream`;
torch.cuda.current_stream and _hip.stream_id are patched to match.

GPU: every producer of the queue, each case twice -- its backward inside deferred_weight_grads() and without it -- against the fp64
torch result on the CPU, at the tolerances the op-level tests of these reductions use: rtol 2e-4 / atol 1e-4 for dW and db and RT / AT
for dx (tests/test_ops_gpu.py), 2e-3 relative L2 against the same-roundings restatement for the chain (tests/test_chain_gpu.py),
DSUM_TOL for the BatchNorm sums (tests/test_elementwise.py), G_TOL for the LSTM (tests/test_lstm.py), the bf16 budget of
test_conv2d_bf16_storage_layer (tests/test_ops_gpu.py) for the bf16-storage Conv2D layer.  Parameters are leaves whose
.grad is preallocated to zeros, so that grad_target finds them."""
import contextlib
import functools

import pytest
import torch

from oracle import percival_oracle as O
from test_chain_gpu import _device_maps, _manual_chain, _rel, _weights
from test_elementwise import DSUM_TOL
from test_lstm import G_TOL, reference as lstm_reference
from test_ops_gpu import AT, RT, close

W_TOL = dict(rtol=2e-4, atol=1e-4)       # dW, db: tests/test_ops_gpu.py, test_conv2d_forward_backward
CHAIN_TOL = 2e-3                         # same roundings: tests/test_chain_gpu.py, test_chain_first_and_second_order_gradients
REDUCE = 'ptts_conv2d_reduce_grouped'


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------
class FakeStream(object):
    def __init__(self, handle):
        self.cuda_stream = handle
        self.joined = []

    def wait_stream(self, s):
        self.joined.append(s.cuda_stream)


@pytest.fixture
def fake(monkeypatch):
    """(ops, main, side, use): `use(s)` makes the fake stream s the current one."""
    from percivaltts_amd import ops
    main, side = FakeStream(11), FakeStream(22)
    state = {'cur': main}
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: state['cur'])
    monkeypatch.setattr(ops._hip, 'stream_id', lambda: state['cur'].cuda_stream)
    assert not (ops._Deferred.active or ops._Deferred.items or ops._Deferred.conv_items or ops._Deferred.streams)
    return ops, main, side, lambda s: state.update(cur=s)


def test_exit_joins_a_noted_stream_when_both_queues_are_empty(fake):
    """BatchNorm and LSTM add their gradients on the stream of the backward pass and only note it: the context's exit must make the
    current stream wait for it although nothing is queued."""
    ops, main, side, _ = fake
    with ops.deferred_weight_grads():
        ops._Deferred.streams.append(side)
    assert main.joined == [side.cuda_stream]
    assert ops._Deferred.streams == [] and ops._Deferred.items == [] and ops._Deferred.conv_items == []


def test_noting_the_same_stream_twice_keeps_one_entry(fake):
    ops, main, side, use = fake
    with ops.deferred_weight_grads():
        use(side)
        assert ops._Deferred.note_stream() == side.cuda_stream
        ops._Deferred.note_stream()
        assert ops._Deferred.streams == [side]
        use(main)
        ops._Deferred.note_stream()
        ops._Deferred.note_stream(FakeStream(side.cuda_stream))      # another object for the same handle
        assert ops._Deferred.streams == [side, main]
    assert main.joined == [side.cuda_stream]                         # the current stream does not wait for itself


def test_detach_then_attach_keeps_the_order_and_merges_the_streams(fake):
    ops, main, side, use = fake
    third = FakeStream(33)
    try:
        with ops.deferred_weight_grads():
            ops._Deferred.items += ['a1', 'a2']
            ops._Deferred.conv_items += ['ca']
            use(side)
            ops._Deferred.note_stream()
            use(main)
            ops._Deferred.note_stream()
            st = ops.deferred_detach()
            assert ops._Deferred.streams == [] and ops._Deferred.items == [] and ops._Deferred.conv_items == []
        assert main.joined == []                                     # the detached streams are not joined by this context
        with ops.deferred_weight_grads():
            ops._Deferred.items += ['o1']
            ops._Deferred.conv_items += ['co1', 'co2']
            ops._Deferred.note_stream()                              # main
            ops._Deferred.note_stream(third)
            ops.deferred_attach(st)
            assert ops._Deferred.items == ['a1', 'a2', 'o1']
            assert ops._Deferred.conv_items == ['ca', 'co1', 'co2']
            assert ops._Deferred.streams == [main, third, side]
            ops._Deferred.items, ops._Deferred.conv_items = [], []   # (placeholders: nothing a flush could launch)
        assert main.joined == [third.cuda_stream, side.cuda_stream]
    finally:
        ops._Deferred.reset()


def test_attach_none_is_a_no_op(fake):
    ops, main, side, _ = fake
    with ops.deferred_weight_grads():
        ops._Deferred.note_stream()
        ops.deferred_attach(None)
        assert ops._Deferred.streams == [main] and ops._Deferred.items == [] and ops._Deferred.conv_items == []


def test_not_live_outside_a_context_and_in_deterministic_mode(fake):
    ops = fake[0]
    p = torch.zeros(3, requires_grad=True)
    p.grad = torch.zeros(3)
    assert not ops._Deferred.live() and ops._Deferred.targets(p, None, p) == (None, None, None)
    old = ops.deterministic()
    try:
        ops.deterministic(False)
        with ops.deferred_weight_grads():
            assert ops._Deferred.live()
            t = ops._Deferred.targets(p, None)
            assert t[0] is p.grad and t[1] is None
            ops.deterministic(True)
            assert not ops._Deferred.live() and ops._Deferred.targets(p, None, p) == (None, None, None)
    finally:
        ops.deterministic(old)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: every producer, deferred and immediate, against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ops():
    from percivaltts_amd import ops as _ops
    old = _ops.deterministic()
    _ops.deterministic(False)
    try:
        yield _ops
    finally:
        _ops.deterministic(old)
    assert not (_ops._Deferred.active or _ops._Deferred.items or _ops._Deferred.conv_items or _ops._Deferred.streams)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def dev(t, grad=False):
    return t.detach().to(torch.float32).cuda().contiguous().requires_grad_(grad)


def param(t):
    """A float32 device leaf with its gradient buffer in place."""
    p = dev(t, True)
    p.grad = torch.zeros_like(p)
    return p


def scope(ops, deferred):
    return ops.deferred_weight_grads() if deferred else contextlib.nullcontext()


def names(kt, start=0):
    return [r[0] for r in kt.records[start:]]


MODES = pytest.mark.parametrize('deferred', [True, False], ids=['deferred', 'immediate'])

CONV = {
    # B, T, F, Cin, Cout, K, dilation, causal, LeakyReLU on the input
    'fused': (2, 16, 65, 4, 4, 5, 1, False, True),        # matrix cores, dx + dW + dbias in one launch
    'unfused': (2, 40, 7, 4, 4, 5, 2, True, True),        # matrix cores, dx through the transposed table + the partial rows
    'stencil': (2, 12, 9, 1, 4, 5, 1, False, False),      # packed-FMA stencil with partial rows
    'generic': (2, 10, 7, 3, 5, 3, 1, False, True),       # no tiled kernel: the queue declines
    'wide': (2, 12, 9, 8, 8, 5, 1, False, True),          # fp32 matrix-core kernels, partial rows from the buffer's first byte
    'bn-fused': (2, 16, 65, 4, 4, 5, 1, False, True),     # BatchNorm-fused input: the affine's sums behind dW | dbias, never queued
    'bn-fused-no-stats': (2, 16, 65, 4, 4, 5, 1, False, True),       # conv_bn_stats(False): the generic kernel
    'bn-wide': (2, 12, 9, 8, 8, 5, 1, False, True),       # BatchNorm-fused input of a wide layer: never queued
    'fused-switched-off': (2, 16, 65, 4, 4, 5, 1, False, True),  # conv2d_fused(False): the pair of launches
    'fused-no-mfma': (2, 16, 65, 4, 4, 5, 1, False, True),   # conv2d_mfma(False): the stencil's kernels
    'bf16': (2, 16, 65, 4, 4, 5, 1, False, True),         # bf16 = 'out32': one-plane kernels, no fused launch
}
# the backward's launches: (deferred, immediate)
CONV_BWD = {
    'fused': (['ptts_conv2d_mfma_bwd_fused'],) * 2,
    'unfused': (['ptts_conv2d_mfma_fwd', 'ptts_conv2d_mfma_wgrad_partials'],) * 2,
    'stencil': (['ptts_conv2d_bwd_partials'], ['ptts_conv2d_bwd']),
    'generic': (['ptts_conv2d_bwd'],) * 2,
    'wide': (['ptts_conv2d_wide_bwd_partials'],) * 2,
    'bn-fused': (['ptts_conv2d_mfma_bwd_fused_affine'],) * 2,
    'bn-fused-no-stats': (['ptts_conv2d_bwd'],) * 2,
    'bn-wide': (['ptts_conv2d_wide_bwd_partials'],) * 2,
    'fused-switched-off': (['ptts_conv2d_mfma_fwd', 'ptts_conv2d_mfma_wgrad_partials'],) * 2,
    'fused-no-mfma': (['ptts_conv2d_bwd_partials'], ['ptts_conv2d_bwd']),
    'bf16': (['ptts_conv2d_mfma_fwd', 'ptts_conv2d_mfma_wgrad_partials'],) * 2,
}
CONV_QUEUED = {'fused', 'unfused', 'stencil', 'wide', 'fused-switched-off', 'fused-no-mfma', 'bf16'}   # inside the context
CONV_REDUCED = {'fused', 'unfused', 'wide', 'bn-fused', 'bn-wide', 'fused-switched-off', 'bf16'}   # where not queued: ONE reduce at once
CONV_AFFINE = {'bn-fused', 'bn-fused-no-stats', 'bn-wide'}                                             # input lrelu(scale x + shift)
CONV_SWITCH = {'bn-fused-no-stats': 'conv_bn_stats', 'fused-switched-off': 'conv2d_fused', 'fused-no-mfma': 'conv2d_mfma'}
CONV_BF16 = {'bf16': 'out32'}
BF16_TOL = 2.0 ** -8       # relative L2 of dx and dW at the bf16 budget: tests/test_ops_gpu.py, test_conv2d_bf16_storage_layer
BF16_DB = dict(rtol=2e-4, atol=1e-3)                    # db sums the raw dy values (the same test)


@functools.lru_cache(maxsize=None)
def conv_case_full(name):
    """fp64: the inputs (x, w, b, dy, scale, shift) and the gradients (dx, dw, db, dscale, dshift); scale / shift are None
    without a BatchNorm-fused input.  The bf16 case: the oracle with the kernels' roundings (the activation and the kernel to
    bf16, exact products), as in tests/test_ops_gpu.py, test_conv2d_bf16_storage_layer."""
    B, T, F, Cin, Cout, K, dil, causal, act = CONV[name]
    g = gen(31)
    x, w, b, dy = randn(g, B, T, F, Cin), randn(g, K, K, Cin, Cout) * 0.3, randn(g, Cout), randn(g, B, T, F, Cout)
    sc = sh = None
    if name in CONV_AFFINE:
        sc, sh = torch.rand(Cin, generator=g, dtype=torch.float64) + 0.5, randn(g, Cin)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, sc, sh) if t is not None]
    xr, wr, br = leaves[:3]
    a = xr if sc is None else xr * leaves[3] + leaves[4]
    a = O.lrelu(a) if act else a
    if name in CONV_BF16:
        a, wr = O.bf16_st(a), O.bf16_st(wr)
    O.conv2d_nhwc(a, wr, br, dil_t=dil, causal=causal).backward(dy)
    return (x, w, b, dy, sc, sh), tuple(t.grad for t in leaves) + (None,) * (5 - len(leaves))


def conv_case(name):
    """fp64: the inputs (x, w, b, dy) and the gradients (dx, dw, db)."""
    ins, grads = conv_case_full(name)
    return ins[:4], grads[:3]


@contextlib.contextmanager
def conv_switches(ops, name):
    """The case's tier switch off, and back at its default afterwards."""
    sw = CONV_SWITCH.get(name)
    if sw is not None:
        getattr(ops, sw)(False)
    try:
        yield
    finally:
        if sw is not None:
            getattr(ops, sw)(None)


def conv_layer(ops, name, x, w, b, affine=()):
    dil, causal, act = CONV[name][6:]
    return ops.conv2d(ops.Lazy(x, *affine, lrelu=True) if act else x, w, b, dil_t=dil, pad_mode=ops.PAD_CAUSAL if causal else ops.PAD_SAME,
                      bf16=CONV_BF16.get(name))


def conv_step(ops, name, leaves=None):
    """Forward and backward of the layer; returns its leaves (x, w, b)."""
    (x, w, b, dy), _ = conv_case(name)
    xd, wd, bd = leaves or (dev(x, True), param(w), param(b))
    conv_layer(ops, name, xd, wd, bd).backward(dev(dy))
    return xd, wd, bd


def l2(got, want):
    return float((got.detach().double().cpu() - want).norm() / want.norm())


def conv_check(name, leaves, times=1, affine=()):
    _, (dx, dw, db, dsc, dsh) = conv_case_full(name)
    if name in CONV_BF16:
        errs = l2(leaves[0].grad, times * dx), l2(leaves[1].grad, times * dw)
        print(name, 'relative L2 of dx, dw', errs)
        assert max(errs) < BF16_TOL, errs
        close(leaves[2].grad, times * db, what=name + ' db', **BF16_DB)
        return
    close(leaves[0].grad, times * dx, RT, AT, what=name + ' dx')
    close(leaves[1].grad, times * dw, what=name + ' dw', **W_TOL)
    close(leaves[2].grad, times * db, what=name + ' db', **W_TOL)
    for nm, p, want in zip(('dscale', 'dshift'), affine, (dsc, dsh)):
        close(p.grad, times * want, what=name + ' ' + nm, **W_TOL)


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize('name', list(CONV))
def test_conv2d_every_backward_path(ops, name, deferred):
    """Queued passes leave the gradient buffer alone until the context exits, then ONE grouped reduction; a shape without a tiled
    kernel is declined and its gradient arrives through autograd, and so does every gradient of a layer with a BatchNorm-fused
    input (reduced at once, with the affine's sums, in ONE launch)."""
    (x, w, b, dy, sc, sh), _ = conv_case_full(name)
    xd, wd, bd = dev(x, True), param(w), param(b)
    affine = (dev(sc, True), dev(sh, True)) if name in CONV_AFFINE else ()
    with conv_switches(ops, name), ops._hip.KernelTimer() as kt:
        with scope(ops, deferred):
            y = conv_layer(ops, name, xd, wd, bd, affine)
            nfwd = len(kt.records)
            y.backward(dev(dy))
            inside, queued = names(kt, nfwd), len(ops._Deferred.conv_items)
            early = float(wd.grad.abs().max())
        total = names(kt, nfwd)
    for k in CONV_BWD[name][0 if deferred else 1]:
        assert inside.count(k) == 1, (k, inside)
    if deferred and name in CONV_QUEUED:
        assert queued == 1 and REDUCE not in inside and early == 0.0, (queued, inside, early)
        assert total.count(REDUCE) == 1, total
    else:
        assert queued == 0 and early > 0.0
        assert total.count(REDUCE) == inside.count(REDUCE) == int(name in CONV_REDUCED), total
    conv_check(name, (xd, wd, bd), affine=affine)


@pytest.mark.gpu
@MODES
def test_two_backward_passes_in_one_context_add_up(ops, deferred):
    with scope(ops, deferred):
        leaves = conv_step(ops, 'fused')
        conv_step(ops, 'fused', leaves)
    conv_check('fused', leaves, times=2)


@functools.lru_cache(maxsize=None)
def second_order_case(name):
    """fp64: R and the gradient of sum((d sum(R . y) / dx)^2) with respect to the kernel."""
    (x, w, b, dy), _ = conv_case(name)
    dil, causal, _ = CONV[name][6:]
    R = randn(gen(32), *dy.shape)
    xr, wr, Rr = (t.clone().requires_grad_(True) for t in (x, w, R))
    y = O.conv2d_nhwc(O.lrelu(xr), wr, b, dil_t=dil, causal=causal)
    gx = torch.autograd.grad(y, xr, Rr, create_graph=True)[0]
    (gx * gx).sum().backward()
    return R, wr.grad


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize('name', ['fused', 'unfused'])
def test_conv2d_second_order_sweep(ops, name, deferred):
    """The gradient penalty's pattern through one 4 -> 4 layer.  Dilation 1: the masked forward and the weight gradient of the
    sweep are ONE launch (kind 2), queued with no bias target."""
    (x, w, b, _), _ = conv_case(name)
    R, dw64 = second_order_case(name)
    xd, wd, bd, Rd = dev(x, True), param(w), param(b), dev(R, True)
    with ops._hip.KernelTimer() as kt:
        with scope(ops, deferred):
            y = conv_layer(ops, name, xd, wd, bd)
            with ops.input_grad_only():
                gx = torch.autograd.grad(y, xd, grad_outputs=Rd, create_graph=True)[0]
            n1 = len(kt.records)
            (gx * gx).sum().backward()
            inside, items = names(kt, n1), list(ops._Deferred.conv_items)
    want = ['ptts_conv2d_mfma_bwd_fused'] if name == 'fused' else ['ptts_conv2d_mfma_fwd', 'ptts_conv2d_mfma_wgrad_partials']
    for k in want:
        assert inside.count(k) == 1, (k, inside)
    if deferred:
        assert REDUCE not in inside and len(items) == 1 and items[0][6] is wd.grad and items[0][7] is None, inside
    else:
        assert inside.count(REDUCE) == 1 and not items, inside
    assert Rd.grad is not None and float(bd.grad.abs().max()) == 0.0
    close(wd.grad, dw64, what=name + ' second-order dw', **W_TOL)


@functools.lru_cache(maxsize=None)
def pair_case():
    g = gen(33)
    buf, w, b, dy = randn(g, 3, 16, 65, 4), randn(g, 5, 5, 4, 4) * 0.3, randn(g, 4), randn(g, 3, 16, 65, 4)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (buf, w, b))
    O.conv2d_nhwc(O.lrelu(xr), wr, br).backward(dy)
    return (buf, w, b, dy), (xr.grad, wr.grad, br.grad)


@pytest.mark.gpu
@MODES
def test_conv2d_pair_on_two_back_to_back_inputs(ops, deferred):
    """Two evaluations (2 and 1 utterances) sliced from one buffer: one forward launch, and both halves' gradients in the one buffer."""
    (buf, w, b, dy), (dx, dw, db) = pair_case()
    bufd, wd, bd, dyd = dev(buf, True), param(w), param(b), dev(dy)
    with ops._hip.KernelTimer() as kt:
        with scope(ops, deferred):
            y0, y1 = ops.conv2d_pair(ops.Lazy(bufd[:2], lrelu=True), ops.Lazy(bufd[2:], lrelu=True), wd, bd)
            assert names(kt).count('ptts_conv2d_mfma_fwd') == 1 and y1.data_ptr() == y0.data_ptr() + 4 * y0.numel()
            torch.autograd.backward([y0, y1], [dyd[:2], dyd[2:]])
            assert len(ops._Deferred.conv_items) == (2 if deferred else 0)
    assert names(kt).count('ptts_conv2d_mfma_bwd_fused') == 2
    close(bufd.grad, dx, RT, AT, what='pair dx')
    close(wd.grad, dw, what='pair dw', **W_TOL)
    close(bd.grad, db, what='pair db', **W_TOL)


CHAIN = dict(B=2, T=16, F=33, L=2)


@functools.lru_cache(maxsize=None)
def chain_case():
    """The chain's inputs and its arithmetic restated in fp64 with all its roundings, on the forward kernel's own maps."""
    from percivaltts_amd import ops
    B, T, F, L = CHAIN['B'], CHAIN['T'], CHAIN['F'], CHAIN['L']
    ws, bs = _weights(L, 1, 5)
    g = gen(11)
    x0, R, S = randn(g, B, T, F), randn(g, B, T, F, 4), randn(g, B, T, F)
    with torch.no_grad():
        maps = _device_maps(ops, dev(x0), [dev(w) for w in ws], [dev(b) for b in bs])
    m_dw, m_db, _, m_dw2, _ = _manual_chain(x0, ws, bs, R, S, maps)
    return (x0, ws, bs, R, S), (m_dw, m_db, m_dw2)


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize('order', ['first', 'second'])
def test_conv2d_chain_first_order_pass_and_second_order_sweep(ops, order, deferred):
    (x0, ws, bs, R, S), (m_dw, m_db, m_dw2) = chain_case()
    L = CHAIN['L']
    xd, wd, bd, Rd = dev(x0, True), [param(w) for w in ws], [param(b) for b in bs], dev(R, True)
    with scope(ops, deferred):
        a = ops.conv2d_chain(xd, wd, bd, 0.3)
        l1 = (a.float() * Rd).sum()
        if order == 'first':
            l1.backward()
        else:
            with ops.input_grad_only():
                g0 = torch.autograd.grad(l1, xd, create_graph=True)[0]
            (g0 * dev(S)).sum().backward()
        assert len(ops._Deferred.conv_items) == (L if deferred else 0)
    cpu = lambda t: t.detach().double().cpu()
    errs = {}
    for l in range(L):
        if order == 'first':
            errs['dW{}'.format(l + 1)] = _rel(cpu(wd[l].grad), m_dw[l])
            errs['db{}'.format(l + 1)] = _rel(cpu(bd[l].grad), m_db[l])
        else:
            errs['second-order dW{}'.format(l + 1)] = _rel(cpu(wd[l].grad), m_dw2[l])
            assert float(bd[l].grad.abs().max()) == 0.0
    print('deferred-chain', order, deferred, errs)
    assert all(e < CHAIN_TOL for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def bn_case():
    g = gen(34)
    z, gamma, beta, dy = randn(g, 2048, 8) * 2 + 0.7, torch.rand(8, generator=g, dtype=torch.float64) + 0.5, randn(g, 8), randn(g, 2048, 8)
    zr, gr, br = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    bn = O.BN(gr, br, torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64))
    O.lrelu(bn(zr, True, update=True, unbiased_moving=False)).backward(dy)
    return (z, gamma, beta, dy), (gr.grad, br.grad)


def bn_step(ops):
    z, gamma, beta, dy = bn_case()[0]
    zd, gd, bd = dev(z, True), param(gamma), param(beta)
    zt, sc, sh = ops.batchnorm_affine(zd, gd, bd, torch.zeros(8, device='cuda'), torch.ones(8, device='cuda'), True, True, False)
    ops.Lazy(zt, sc, sh, lrelu=True).tensor().backward(dev(dy))
    return gd, bd


def bn_check(leaves):
    for nm, p, want in zip(('dgamma', 'dbeta'), leaves, bn_case()[1]):
        close(p.grad, want, DSUM_TOL[0], DSUM_TOL[1], what='batchnorm ' + nm)


LSTM = (2, 8, 16, 64, 1)      # B, T, In, H, directions


def lstm_step(ops):
    x, W, U, b, dh = lstm_reference(*LSTM)[0]
    leaves = dev(x, True), param(W), param(U), param(b)
    ops.lstm(*leaves).backward(dev(dh))
    return leaves


def lstm_check(leaves):
    for nm, p, want in zip(('dx', 'dW', 'dU', 'db'), leaves, lstm_reference(*LSTM)[1][1:]):
        close(p.grad, want, G_TOL[nm][0], G_TOL[nm][1], what='lstm ' + nm)


DIRECT = {'batchnorm': (bn_step, bn_check), 'lstm': (lstm_step, lstm_check)}


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize('name', list(DIRECT))
def test_direct_add_producers(ops, name, deferred):
    """BatchNorm and LSTM write the gradient buffers at once on the stream of their backward pass and only note that stream."""
    step, check = DIRECT[name]
    with scope(ops, deferred):
        leaves = step(ops)
        assert not ops._Deferred.items and not ops._Deferred.conv_items
        assert len(ops._Deferred.streams) == int(deferred)
    check(leaves)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(DIRECT) + ['conv2d'])
def test_a_producer_on_a_side_stream_is_noted_and_joined(ops, name):
    """Forward and backward under torch.cuda.stream(side): the side stream is in the noted list while the context is open and gone
    after it closes; the exit has made the current stream wait for it, so the gradients are complete."""
    step, check = DIRECT.get(name, (lambda o: conv_step(o, 'fused'), lambda lv: conv_check('fused', lv)))
    side = torch.cuda.Stream()
    with ops.deferred_weight_grads():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            leaves = step(ops)
        assert [s.cuda_stream for s in ops._Deferred.streams] == [side.cuda_stream]
        assert len(ops._Deferred.conv_items) == int(name == 'conv2d')
    assert ops._Deferred.streams == []
    check(leaves)
