"""The kernels behind the batched validation costs (csrc/evalcosts.hip) against numpy: the backward of the row mask
(ptts_affine_act_rows_bwd), the per-row reductions (ptts_rows_mean, ptts_wlse_rows, ptts_gp_penalty_rows) and the autograd
Function that ops.affine_act_rows becomes in the input-gradient mode.

Bounds.  The mask's backward is one or two fp32 multiplies per element (the build has no contraction): it must equal the same
expression in numpy float32 bit for bit, and the fp64 value to 2 ulp of the result; pad frames are +0.0f by their bytes.  The
reductions sum fp64 partials and round once to fp32: 1e-6 relative against numpy fp64 (out_sq stays fp64: 1e-12), and a row's
result is byte-identical whether it is computed in a batch of 17 or alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lens_dev(lens):
    return torch.tensor(list(lens), dtype=torch.int32, device='cuda')


def frame_mask(lens, shape):
    """[B, T, 1, ...] boolean: t < lens[b]."""
    B, T = shape[0], shape[1]
    m = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    return m.reshape((B, T) + (1,) * (len(shape) - 2))


# ---- ptts_affine_act_rows_bwd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 12, 8), (3, 12, 1), (17, 12, 9, 2), (2, 5, 260)])
@pytest.mark.parametrize('act', [None, 'lrelu'])
@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('full', [False, True])
@pytest.mark.parametrize('inplace', [False, True])
def test_affine_act_rows_bwd(shape, act, affine, full, inplace):
    from percivaltts_amd import ops
    from percivaltts_amd._hip import call, ptr, stream
    B, T, C = shape[0], shape[1], shape[-1]
    rng = np.random.RandomState(3 + B + C)
    lens = [T] * B if full else ([11, 1, 12] * 6)[:B] if T == 12 else [T - 1, 1][:B]
    x = rng.randn(*shape).astype(np.float32)
    dy = rng.randn(*shape).astype(np.float32)
    scale = (rng.rand(C) + 0.5).astype(np.float32) * np.where(rng.rand(C) < 0.3, -1, 1).astype(np.float32)
    shift = rng.randn(C).astype(np.float32)
    x_d, dy_d, l_d = dev(x), dev(dy), lens_dev(lens)
    sc_d, sh_d = (dev(scale), dev(shift)) if affine else (None, None)
    dx_d = dy_d if inplace else torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    call('ptts_affine_act_rows_bwd', ptr(dy_d), ptr(x_d), ptr(sc_d), ptr(sh_d), ptr(dx_d), ptr(l_d), B, T,
         int(np.prod(shape[2:])), C, ops.ACT_CODES[act], ALPHA, stream())
    got = dx_d.cpu().numpy()

    # the kernel's expression in float32: g = dy; g *= act'(x*scale + shift); g *= scale
    one, al = np.float32(1), np.float32(ALPHA)
    want32 = dy.copy()
    want64 = dy.astype(np.float64)
    if act == 'lrelu':
        p = (x * scale + shift) if affine else x
        d = np.where(p > 0, one, al)
        want32 = want32 * d
        want64 = want64 * d.astype(np.float64)
    if affine:
        want32 = want32 * scale
        want64 = want64 * scale.astype(np.float64)
    real = np.broadcast_to(frame_mask(lens, shape), shape)
    assert got.dtype == np.float32
    assert np.array_equal(got[real].view(np.uint32), want32[real].view(np.uint32)), 'real frames differ from the float32 expression'
    ulp = np.spacing(np.abs(want64[real]).astype(np.float32)).astype(np.float64)
    assert (np.abs(got[real].astype(np.float64) - want64[real]) <= 2 * ulp).all()
    assert (got[~real].view(np.uint32) == 0).all(), 'pad frames are not +0.0f'


def test_affine_act_rows_bwd_refuses_what_it_cannot_do():
    from percivaltts_amd import ops
    from percivaltts_amd._hip import call, ptr, stream, HipLibraryError
    x = torch.zeros(2, 3, 4, device='cuda')
    l_d = lens_dev([3, 1])
    with pytest.raises(HipLibraryError, match='none and lrelu'):
        call('ptts_affine_act_rows_bwd', ptr(x), ptr(x), None, None, ptr(x.clone()), ptr(l_d), 2, 3, 4, 4, ops.ACT_SIGMOID, ALPHA, stream())
    with pytest.raises(HipLibraryError, match='together'):
        call('ptts_affine_act_rows_bwd', ptr(x), ptr(x), ptr(x), None, ptr(x.clone()), ptr(l_d), 2, 3, 4, 4, ops.ACT_NONE, ALPHA, stream())
    with pytest.raises(HipLibraryError, match='multiple'):
        call('ptts_affine_act_rows_bwd', ptr(x), ptr(x), None, None, ptr(x.clone()), ptr(l_d), 2, 3, 4, 3, ops.ACT_NONE, ALPHA, stream())


# ---- per-row reductions -------------------------------------------------------------------------------------------------
def row_lengths(B, T):
    return ([T, 1, max(1, T - 1), max(1, T // 2), 2 if T > 1 else 1] * 4)[:B]


GEOMETRIES = [(12, 86), (700, 86), (12, 1), (700, 1)]       # T * inner below and above one workgroup's stride of 1024


@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('T,D', GEOMETRIES)
def test_rows_mean(B, T, D):
    from percivaltts_amd import ops
    rng = np.random.RandomState(B + T + D)
    lens = row_lengths(B, T)
    v = (rng.randn(B, T, D) + 0.25).astype(np.float32)
    v_d, l_d = dev(v), lens_dev(lens)
    for sign in (1.0, -1.0):
        got = ops.rows_mean(v_d, l_d, sign).cpu().numpy()
        want = np.array([sign * v[b, :n].astype(np.float64).mean() for b, n in enumerate(lens)])
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
        for b in (0, B - 1):                                 # a row alone: the same bytes
            alone = ops.rows_mean(v_d[b:b + 1].contiguous(), l_d[b:b + 1].contiguous(), sign).cpu().numpy()
            assert alone.view(np.uint32)[0] == got.view(np.uint32)[b]


@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('T,D', GEOMETRIES)
@pytest.mark.parametrize('weighted', [False, True])
def test_wlse_rows(B, T, D, weighted):
    from percivaltts_amd import ops
    rng = np.random.RandomState(7 + B + T + D)
    lens = row_lengths(B, T)
    y = rng.randn(B, T, D).astype(np.float32)
    yhat = (y + 0.5 * rng.randn(B, T, D)).astype(np.float32)
    w = (rng.rand(D) + 0.01).astype(np.float32) if weighted else None
    y_d, yh_d, l_d, w_d = dev(y), dev(yhat), lens_dev(lens), (dev(w) if weighted else None)
    d2 = (y.astype(np.float64) - yhat.astype(np.float64)) ** 2
    want_sq = np.array([d2[b, :n].sum() for b, n in enumerate(lens)])
    want_ls = np.array([(d2[b, :n] * (w.astype(np.float64) if weighted else 1.0)).mean() for b, n in enumerate(lens)])
    ls, sq = ops.wlse_rows(y_d, yh_d, w_d, l_d)
    assert ls.dtype == torch.float32 and sq.dtype == torch.float64
    np.testing.assert_allclose(ls.cpu().numpy(), want_ls, rtol=1e-6, atol=0)
    np.testing.assert_allclose(sq.cpu().numpy(), want_sq, rtol=1e-12, atol=0)
    # each output NULL in turn: the other one is the same bytes
    ls_only, none = ops.wlse_rows(y_d, yh_d, w_d, l_d, want_sq=False)
    none2, sq_only = ops.wlse_rows(y_d, yh_d, w_d, l_d, want_ls=False)
    assert none is None and none2 is None
    assert torch.equal(ls_only, ls) and torch.equal(sq_only, sq)
    for b in (0, B - 1):                                     # a row alone: the same bytes
        ls1, sq1 = ops.wlse_rows(y_d[b:b + 1].contiguous(), yh_d[b:b + 1].contiguous(), w_d, l_d[b:b + 1].contiguous())
        assert torch.equal(ls1[0], ls[b]) and torch.equal(sq1[0], sq[b])


def test_wlse_rows_needs_an_output():
    from percivaltts_amd import ops
    from percivaltts_amd._hip import HipLibraryError
    y = torch.zeros(1, 2, 3, device='cuda')
    with pytest.raises(HipLibraryError, match='both outputs'):
        ops.wlse_rows(y, y, None, lens_dev([2]), want_ls=False, want_sq=False)


@pytest.mark.parametrize('B', [1, 3, 17])
def test_gp_penalty_rows(B):
    from percivaltts_amd import ops
    from percivaltts_amd._hip import call, ptr, stream
    rng = np.random.RandomState(B)
    sq = (rng.rand(B) * 4.0).astype(np.float32)                # norms on both sides of 1
    sq[0] = 0.0                                                # the degenerate sample: penalty 1
    if B > 2:
        sq[1], sq[2] = 1.0, np.nextafter(np.float32(1), np.float32(2))      # penalty 0, and the smallest one above it
    out = torch.full((B,), float('nan'), dtype=torch.float32, device='cuda')
    call('ptts_gp_penalty_rows', ptr(dev(sq)), ptr(out), B, stream())
    got = out.cpu().numpy()
    want = (1.0 - np.sqrt(sq.astype(np.float64))) ** 2
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert got[0] == np.float32(1.0)
    # behind ptts_gp_sqnorm (an existing kernel: fp64 partials, rounded once): the composite of the optimiser, a sample alone the same bytes
    g = (rng.randn(B, 40, 65) * rng.rand(B, 1, 1) * 0.05).astype(np.float32)
    got = ops.gp_penalty_rows(dev(g)).cpu().numpy()
    sq32 = np.array([(g[b].astype(np.float64) ** 2).sum() for b in range(B)]).astype(np.float32)
    call('ptts_gp_penalty_rows', ptr(dev(sq32)), ptr(out), B, stream())
    n = np.sqrt(sq32.astype(np.float64))
    slack = 1e-6 * sq32 * np.abs(n - 1.0) / n                  # 1e-6 relative on sq through d/dsq (1 - sqrt(sq))^2 = (sqrt(sq) - 1) / sqrt(sq)
    assert (np.abs(got.astype(np.float64) - (1.0 - n) ** 2) <= 1e-6 * (1.0 - n) ** 2 + slack).all()
    alone = ops.gp_penalty_rows(dev(g[B - 1:B])).cpu().numpy()
    assert alone.view(np.uint32)[0] == got.view(np.uint32)[B - 1]


# ---- autograd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,lazy', [((3, 12, 8), False), ((3, 12, 9, 2), True), ((3, 12, 1), False)])
def test_affine_act_rows_input_gradient(shape, lazy):
    from percivaltts_amd import ops
    from percivaltts_amd._hip import call, ptr, stream
    B, T, C = shape[0], shape[1], shape[-1]
    rng = np.random.RandomState(11)
    lens = [11, 1, 12]
    l_d = lens_dev(lens)
    x = dev(rng.randn(*shape).astype(np.float32)).requires_grad_(True)
    cot = dev(rng.randn(*shape).astype(np.float32))
    scale, shift = (dev((rng.rand(C) + 0.5).astype(np.float32)), dev(rng.randn(C).astype(np.float32))) if lazy else (None, None)
    v = ops.Lazy(x, scale, shift, lrelu=True, alpha=ALPHA) if lazy else x
    with torch.no_grad():
        want_y = ops.affine_act_rows(ops.Lazy(x.detach(), scale, shift, lrelu=lazy, alpha=ALPHA), l_d)
    y = ops.affine_act_rows(v, l_d, input_grad=True)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    got, = torch.autograd.grad(y, x, grad_outputs=cot)
    want = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    call('ptts_affine_act_rows_bwd', ptr(cot), ptr(x.detach()), ptr(scale), ptr(shift), ptr(want), ptr(l_d), B, T,
         int(np.prod(shape[2:])), C, ops.ACT_CODES['lrelu' if lazy else None], ALPHA, stream())
    assert torch.equal(got, want), 'the gradient is not the kernel\'s'
    pad = ~torch.from_numpy(np.broadcast_to(frame_mask(lens, shape), shape).copy()).cuda()
    assert (got[pad].view(torch.int32) == 0).all()
    # once differentiable; plain `lengths` keeps refusing gradients
    y2 = ops.affine_act_rows(v, l_d, input_grad=True)
    g2, = torch.autograd.grad(y2, x, grad_outputs=cot, create_graph=True)
    with pytest.raises(RuntimeError):
        g2.sum().backward()
    with pytest.raises(ValueError, match='no_grad'):
        ops.affine_act_rows(v, l_d)
    with pytest.raises(ValueError, match='no_grad'):
        ops.check_lengths(l_d, B, T)
    assert ops.check_lengths(l_d, B, T, allow_grad=True) is l_d
    with torch.no_grad():                                   # without gradients the mode is the plain forward
        assert torch.equal(ops.affine_act_rows(v, l_d, input_grad=True), want_y)
