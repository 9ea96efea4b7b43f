"""The per-row form of the Conv2D chain kernels (ptts_conv2d_chain_{fwd,bwd,bwd_data,second}_rows, ops.conv2d_chain(lengths=)):
zero-padded batches with a length per row ("The per-row chain").

The reference is the PLAIN entry point run on each utterance alone at T = n: tests/test_chain_gpu.py shows that a tile does not
depend on its batch, and the tile origins and the chunking do not depend on T, so the real rows must agree bit for bit
(torch.equal); the pad rows must be +0.0 bit for bit.  Every input and gradient tensor handed to a per-row launch -- the maps
and gamma maps that an earlier launch produced included -- holds NaN in its pad rows, and every output buffer of a raw entry
point is pre-filled with NaN: a pad row that is read shows as NaN, a row that is not written stays NaN.

Weight and bias gradients are sums over the batch: against the sum of the lone utterances' gradients accumulated in float64,
relative L2 per tensor <= 2e-3 -- test_chain_gpu.py's "same roundings" bound, what the order of fp32 summation leaves (the
addends are the same numbers: only their grouping into workgroups and tiles differs).

Cases (the places the row limit can go wrong):
    a  F 65, L 8, T 70   one block, 17 bin groups; lengths 70 (full, a ragged last tile), 1 (one frame), 32 (the end on a tile
                         border: the next tile is all pad), 33 (one real row in a tile), 47 (the end inside the 16-row halo of an
                         all-pad tile)
    b  F 13, L 3, T 37   a small stack
    c  F 66, L 1, T 33   even F (no pad bin) and a single layer (no internal map, the first layer's dW from the input)
    d  F 129, L 8, T 40  frequency blocks
    e  F 150, L 2, T 33  blocks, a short last block and shallow halos"""
import ctypes

import pytest
import torch

from test_chain_gpu import _weights

pytestmark = pytest.mark.gpu

ALPHA = 0.3
CASES = {
    'a': dict(F=65, L=8, T=70, lengths=[70, 1, 32, 33, 47]),
    'b': dict(F=13, L=3, T=37, lengths=[37, 2]),
    'c': dict(F=66, L=1, T=33, lengths=[33, 32, 1]),
    'd': dict(F=129, L=8, T=40, lengths=[40, 7, 33]),
    'e': dict(F=150, L=2, T=33, lengths=[33, 32, 1]),
}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from percivaltts_amd import ops as _ops
    return _ops


def _plus_zero(t):
    """Every value is +0.0, bit for bit."""
    t = t.contiguous()
    return bool((t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) == 0).all())


def _pad_mask(lengths, T):
    n = torch.as_tensor(lengths).clamp(0, T)
    return (torch.arange(T)[None, :] >= n[:, None]).cuda()          # [B, T], True on pad rows


def _poison(t, pad, lead=0):
    """A copy of t ([*lead dims, B, T, ...]) with NaN in its pad rows."""
    t = t.clone()
    if lead:
        t[:, pad] = float('nan')
    else:
        t[pad] = float('nan')
    return t


def _inputs(case, seed, lengths=None):
    """x0, R = dL/da_L, S = d/d(g0) on the device, NaN in their pad rows, and the stack's weights."""
    F, L, T = case['F'], case['L'], case['T']
    lengths = case['lengths'] if lengths is None else lengths
    B = len(lengths)
    ws, bs = _weights(L, 1, seed)
    g = torch.Generator().manual_seed(seed + 100)
    pad = _pad_mask(lengths, T)
    x = _poison(torch.randn(B, T, F, generator=g).cuda(), pad)
    R = _poison(torch.randn(B, T, F, 4, generator=g).cuda(), pad)
    S = _poison(torch.randn(B, T, F, generator=g).cuda(), pad)
    wd = [w.float().cuda().contiguous() for w in ws]
    bd = [b.float().cuda().contiguous() for b in bs]
    return x, R, S, wd, bd, pad


def _raw(ops, x, R, S, wd, bd, lengths=None, pad=None):
    """All four passes through the C ABI: the plain entry points (lengths None), or the per-row ones with `lengths` (a list).
    Output buffers start as NaN; under lengths the maps / gamma maps go into the next pass with NaN in their pad rows."""
    from percivaltts_amd import _hip
    ptr, call = _hip.ptr, _hip.call
    B, T, F = x.shape
    L = len(wd)
    FP = (F + 1) & ~1
    rows = lengths is not None
    sfx = '_rows' if rows else ''
    ld = torch.tensor(lengths, dtype=torch.int32, device='cuda') if rows else None
    la = (ptr(ld),) if rows else ()
    nan = float('nan')
    tab = ops._C2C.table(wd, bd)
    full = lambda shape, dt: torch.full(shape, nan, dtype=dt, device='cuda')
    out = {}

    maps, a_last = full((max(L - 1, 1), B, T, FP, 4), torch.bfloat16), full((B, T, F, 4), torch.bfloat16)
    call('ptts_conv2d_chain_fwd' + sfx, ptr(x), x.stride(1), ptr(tab), ptr(maps), ptr(a_last), *la, B, T, F, L, ALPHA, _hip.stream())
    out['maps'], out['a_last'] = maps[:L - 1], a_last
    maps_in = _poison(maps, pad, lead=1) if rows else maps
    a_in = _poison(a_last, pad) if rows else a_last

    gmaps, g0 = full((L, B, T, FP, 4), torch.bfloat16), full((B, T, F), torch.float32)
    call('ptts_conv2d_chain_bwd_data' + sfx, ptr(R), 0, ptr(maps_in), ptr(a_in), ptr(tab), ptr(gmaps), ptr(g0), *la, B, T, F, L, ALPHA, _hip.stream())
    out['gmaps'], out['g0'] = gmaps, g0
    g0_alone = full((B, T, F), torch.float32)
    call('ptts_conv2d_chain_bwd_data' + sfx, ptr(R), 0, ptr(maps_in), ptr(a_in), ptr(tab), None, ptr(g0_alone), *la, B, T, F, L, ALPHA, _hip.stream())
    out['g0 without gmaps'] = g0_alone
    gm_in = _poison(gmaps, pad, lead=1) if rows else gmaps

    nbytes = int(_hip.lib().ptts_conv2d_chain_partials_bytes(L))

    def partial_rows(name, head):
        buf = torch.zeros(nbytes // 4, dtype=torch.float32, device='cuda')         # (a row's unused tail is not written)
        nb, npart = ctypes.c_int(0), ctypes.c_int(0)
        call(name + sfx, *head, ptr(buf), nbytes, ctypes.byref(nb), ctypes.byref(npart), *la, B, T, F, L, 1, ALPHA, _hip.stream())
        assert nb.value > 0 and npart.value > 0
        return buf[:L * nb.value * npart.value].view(L, nb.value, npart.value)

    d_out = full((B, T, F, 4), torch.float32)
    out['second rows'] = partial_rows('ptts_conv2d_chain_second', (ptr(S), ptr(gm_in), ptr(maps_in), ptr(a_in), ptr(tab), ptr(d_out), 0))
    out['d/d(d_last)'] = d_out
    out['bwd rows'] = partial_rows('ptts_conv2d_chain_bwd', (ptr(R), 0, ptr(x), x.stride(1), ptr(maps_in), ptr(a_in), ptr(tab)))
    torch.cuda.synchronize()
    return out


# what lies where in an output of _raw: name -> index of the batch axis (T follows it)
BATCH_AXIS = {'maps': 1, 'a_last': 0, 'gmaps': 1, 'g0': 0, 'g0 without gmaps': 0, 'd/d(d_last)': 0}


def _grads(ops, x, R, S, wd, bd, lengths=None):
    """Through ops.conv2d_chain and autograd, as the critic does: (a_L, g0, [dW_l], [db_l], [second-order dW_l], d/dR)."""
    L = len(wd)
    ws = [w.clone().requires_grad_(True) for w in wd]
    bs = [b.clone().requires_grad_(True) for b in bd]
    xr = x.clone().requires_grad_(True)
    Rr = R.clone().requires_grad_(True)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device='cuda')
    a = ops.conv2d_chain(xr, ws, bs, ALPHA, lengths=ld)
    # the incoming gradients R and S keep their NaN pad rows: they enter as grad_outputs, not through a sum
    af = a.float()              # (as layers.Conv2DStack hands the map on: dL/da_L arrives rounded to bf16)
    g1 = torch.autograd.grad(af, ws + bs, grad_outputs=Rr.detach(), retain_graph=True)
    g0 = torch.autograd.grad(af, xr, grad_outputs=Rr, create_graph=True)[0]
    g2 = torch.autograd.grad(g0, ws + [Rr], grad_outputs=S)
    torch.cuda.synchronize()
    return a.detach(), g0.detach(), list(g1[:L]), list(g1[L:]), list(g2[:L]), g2[L]


_RUNS = {}


def _runs(ops, name):
    """Per case, computed once and left unchanged: the per-row launches on the padded batch and the plain ones on every lone utterance."""
    if name not in _RUNS:
        case = CASES[name]
        x, R, S, wd, bd, pad = _inputs(case, seed=3)
        batch = _raw(ops, x, R, S, wd, bd, case['lengths'], pad)
        lone = []
        for b, n in enumerate(case['lengths']):
            lone.append(_raw(ops, x[b:b + 1, :n].contiguous(), R[b:b + 1, :n].contiguous(), S[b:b + 1, :n].contiguous(), wd, bd))
        _RUNS[name] = (case, batch, lone, pad)
    return _RUNS[name]


def _check_rows(name, key, batch, lone, case, pad):
    ax = BATCH_AXIS[key]
    got = batch[key]
    assert got.shape[ax + 1] == case['T']
    for b, n in enumerate(case['lengths']):
        mine = got.select(ax, b).narrow(ax, 0, n)                   # utterance b, real rows
        ref = lone[b][key].select(ax, 0)
        assert torch.equal(mine, ref), 'case {} {}: real rows of utterance {} (n = {}) differ from the lone utterance: {} of {} values'.format(
            name, key, b, n, int((mine != ref).sum()), mine.numel())
        tail = got.select(ax, b).narrow(ax, n, case['T'] - n)
        assert _plus_zero(tail), 'case {} {}: pad rows of utterance {} (n = {}) are not +0.0 (NaN: {})'.format(
            name, key, b, n, int(torch.isnan(tail.float()).sum()))


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_rows(ops, name):
    """a_L and every internal map: real rows bit-equal to the lone utterance's, pad rows +0.0, the pad bin of the internal maps too."""
    case, batch, lone, pad = _runs(ops, name)
    _check_rows(name, 'a_last', batch, lone, case, pad)
    if case['L'] > 1:
        _check_rows(name, 'maps', batch, lone, case, pad)
        if case['F'] & 1:
            assert _plus_zero(batch['maps'][:, :, :, case['F']:]), 'the pad bin of the internal maps'


@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_data_rows(ops, name):
    """g0 (with and without the gamma maps) and the gamma maps."""
    case, batch, lone, pad = _runs(ops, name)
    for key in ('g0', 'g0 without gmaps', 'gmaps'):
        _check_rows(name, key, batch, lone, case, pad)
    assert torch.equal(batch['g0'], batch['g0 without gmaps'])
    if case['F'] & 1:
        assert _plus_zero(batch['gmaps'][:, :, :, case['F']:]), 'the pad bin of the gamma maps'


@pytest.mark.parametrize('name', sorted(CASES))
def test_second_order_rows(ops, name):
    """The second-order sweep's output d/d(d_last)."""
    case, batch, lone, pad = _runs(ops, name)
    _check_rows(name, 'd/d(d_last)', batch, lone, case, pad)


@pytest.mark.parametrize('name', sorted(CASES))
def test_weight_and_bias_gradients_sum_over_real_rows(ops, name):
    """dW_l, db_l (first order) and the second-order sweep's dW_l of the padded batch against the float64 sum of the lone
    utterances' gradients: relative L2 per tensor <= 2e-3 (fp32 summation order), all values finite.  The activations, the input
    gradient and d/dR that autograd returns obey the row rule as well."""
    case = CASES[name]
    L, T = case['L'], case['T']
    x, R, S, wd, bd, pad = _inputs(case, seed=5)
    a, g0, dw, db, dw2, dR = _grads(ops, x, R, S, wd, bd, case['lengths'])
    sums = None
    for b, n in enumerate(case['lengths']):
        la, lg0, ldw, ldb, ldw2, ldR = _grads(ops, x[b:b + 1, :n].contiguous(), R[b:b + 1, :n].contiguous(), S[b:b + 1, :n].contiguous(), wd, bd)
        assert torch.equal(a[b, :n], la[0]) and torch.equal(g0[b, :n], lg0[0]) and torch.equal(dR[b, :n], ldR[0])
        assert _plus_zero(a[b, n:]) and _plus_zero(g0[b, n:]) and _plus_zero(dR[b, n:])
        parts = [t.double() for t in ldw + ldb + ldw2]
        sums = parts if sums is None else [s + p for s, p in zip(sums, parts)]
    names = ['dW{}'.format(l + 1) for l in range(L)] + ['db{}'.format(l + 1) for l in range(L)] + ['second-order dW{}'.format(l + 1) for l in range(L)]
    errs = {}
    for k, got, ref in zip(names, dw + db + dw2, sums):
        assert torch.isfinite(got).all(), '{}: non-finite'.format(k)
        errs[k] = float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    print('case {}: '.format(name) + ', '.join('{} {:.1e}'.format(k, e) for k, e in errs.items()))
    bad = ['{}: {:.3e}'.format(k, e) for k, e in errs.items() if not e <= 2e-3]
    assert not bad, 'case {}: relative L2 > 2e-3: '.format(name) + '; '.join(bad)


@pytest.mark.parametrize('name', ['a', 'd'])
def test_full_lengths_equal_the_plain_entry_points(ops, name):
    """n[b] = T for all b: every output of every _rows entry point -- the partial-sum rows included -- and every landed gradient
    equals the plain entry point's, bit for bit."""
    case = CASES[name]
    full = [case['T']] * len(case['lengths'])
    x, R, S, wd, bd, pad = _inputs(case, seed=7, lengths=full)
    assert not bool(pad.any())
    plain = _raw(ops, x, R, S, wd, bd)
    rows = _raw(ops, x, R, S, wd, bd, full, pad)
    for key in plain:
        assert torch.equal(plain[key], rows[key]), 'case {} {}: {} values differ'.format(name, key, int((plain[key] != rows[key]).sum()))
        assert not bool(torch.isnan(rows[key].float()).any()), key
    gp = _grads(ops, x, R, S, wd, bd)
    gr = _grads(ops, x, R, S, wd, bd, full)
    flat = lambda g: [g[0], g[1]] + g[2] + g[3] + g[4] + [g[5]]
    for i, (p, r) in enumerate(zip(flat(gp), flat(gr))):
        assert torch.equal(p, r), 'case {}: result {} through ops.conv2d_chain differs'.format(name, i)


def test_lengths_are_clamped(ops):
    """A length of T + 5 behaves as T, 0 (and a negative one) gives an all-zero row: by result, against the clamped lengths."""
    case = dict(CASES['b'], lengths=[37 + 5, 0, -3, 7])
    T = case['T']
    clamped = [T, 0, 0, 7]
    x, R, S, wd, bd, pad = _inputs(case, seed=9, lengths=clamped)
    want = _raw(ops, x, R, S, wd, bd, clamped, pad)
    got = _raw(ops, x, R, S, wd, bd, case['lengths'], pad)
    for key in want:
        assert torch.equal(want[key], got[key]), key
        assert not bool(torch.isnan(got[key].float()).any()), key
    for key, ax in BATCH_AXIS.items():
        for b in (1, 2):
            assert _plus_zero(got[key].select(ax, b)), '{}: the row of length 0 is not all +0.0'.format(key)


def test_null_lengths_are_refused(ops):
    from percivaltts_amd import _hip
    case = CASES['b']
    x, R, S, wd, bd, pad = _inputs(case, seed=9)
    B, T, F = x.shape
    L = len(wd)
    tab = ops._C2C.table(wd, bd)
    maps = torch.zeros((L - 1, B, T, (F + 1) & ~1, 4), dtype=torch.bfloat16, device='cuda')
    a_last = torch.zeros((B, T, F, 4), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(_hip.HipLibraryError, match='lengths'):
        _hip.call('ptts_conv2d_chain_fwd_rows', _hip.ptr(x), x.stride(1), _hip.ptr(tab), _hip.ptr(maps), _hip.ptr(a_last), None,
                  B, T, F, L, ALPHA, _hip.stream())
    with pytest.raises(_hip.HipLibraryError, match='lengths'):
        ops.conv2d_chain(x, wd, bd, ALPHA, lengths=torch.tensor(case['lengths'], dtype=torch.int64, device='cuda'))
