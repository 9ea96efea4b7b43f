"""GPU tests of the resident-left form of ptts_dense_bf16x6_batched (csrc/dense.hip, dense_bf16x6_resident_kernel): members that share
a left operand of at most 128 x 128 -- the transforms of the frequency-domain context Conv1D (ops._C1FFT: 'dft', 'idft', 'dft_dy') --
split it once per workgroup into the LDS and walk (member, 32-column slice) items.  Every case runs with the switch
(ptts_set_dense_batched_resident) on and off: the whole C buffer, sentinel cells included, must be equal bit for bit, and the result lies
within 2e-5 of mean |C| of the fp64 product (the bound of test_ops_gpu.py::test_frequency_domain_building_blocks; for planes_count 1
the fp64 product of the operands' bf16 roundings, which is what one bf16 product with fp32 accumulation computes)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.625          # exactly representable: an untouched cell compares equal bit for bit


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


@pytest.fixture()
def switch(ops):
    """Sets the switch; the setting found is put back afterwards."""
    lib = ops._hip.lib()
    first = lib.ptts_set_dense_batched_resident(1)
    yield lambda on: lib.ptts_set_dense_batched_resident(1 if on else 0)
    lib.ptts_set_dense_batched_resident(first)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# name -> (nbatch, M, N, K, strideC, ldc, floats of the C buffer, bias); nbatch may be a function of the CU count
def layouts():
    many = 3 * cus() * 4
    return {
        # the x-transform's interleaved rows: partial last slice, N % 4 != 0 (the last quad of a row is stored element-wise), a partial last
        # k-step, pad rows
        'dft': (3, 122, 601, 120, 2 * 608, 3 * 2 * 608, 122 * 3 * 2 * 608, False),
        # the inverse transform
        'idft': (7, 100, 256, 124, 100 * 256, 256, 7 * 100 * 256 + 64, True),
        # the gradient's transform: fewer items than waves
        'dft_dy': (2, 122, 32, 120, 32, 2 * 32, 122 * 2 * 32 + 64, False),
        # one row, one k-quad, N < 32
        'one_row': (1, 1, 20, 4, 20, 20, 20 + 64, False),
        # full tile, no padding anywhere
        'full_tile': (2, 128, 288, 128, 128 * 288, 288, 2 * 128 * 288 + 64, False),
        # every wave walks several items
        'many_members': (many, 16, 64, 32, 16 * 64, 64, many * 16 * 64 + 64, False),
    }


_CASES = {}


def operands(name, ops):
    """Seeded fp64 values of fp32 numbers: A [M][K] (shared), B [nbatch][K][N], bias [N]; the planes of B; the fp64 products for three
    planes and for one (computed once per case)."""
    if name not in _CASES:
        nbatch, M, N, K, sC, ldc, numel, has_bias = layouts()[name]
        g = torch.Generator().manual_seed(1000 + M + N + K)
        A = torch.randn(M, K, generator=g, dtype=torch.float64).float()
        B = (torch.randn(nbatch, K, N, generator=g, dtype=torch.float64) / math.sqrt(K)).float()
        bias = torch.randn(N, generator=g, dtype=torch.float64).float()
        lib = ops._hip.lib()
        npb = lib.ptts_dense_planes_bytes(N, K)
        Bd = B.cuda()
        planes = torch.empty(nbatch * npb, dtype=torch.uint8, device='cuda')
        ops.call('ptts_split3_dense_weight_strided', ops.ptr(Bd), K * N, ops.ptr(planes), npb, nbatch, N, K, N, 0, ops.stream())
        torch.cuda.synchronize()
        add = bias.double() if has_bias else 0.0
        want3 = torch.matmul(A.double(), B.double()) + add
        want1 = torch.matmul(A.bfloat16().double(), B.bfloat16().double()) + add
        _CASES[name] = (A.cuda(), planes, npb, bias.cuda() if has_bias else None, want3, want1)
    return _CASES[name]


def product(ops, name, planes_count):
    """The whole C buffer (on the host) after one call at the current switch setting."""
    nbatch, M, N, K, sC, ldc, numel, _ = layouts()[name]
    A, planes, npb, bias, _, _ = operands(name, ops)
    C = torch.full((numel,), SENTINEL, device='cuda')
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ops.ptr(planes), npb, ops.ptr(bias), ops.ptr(C), sC, nbatch, M, N, K, K, ldc,
             planes_count, ops.stream())
    torch.cuda.synchronize()
    return C.cpu()


def check_case(ops, switch, name, planes_count):
    nbatch, M, N, K, sC, ldc, numel, _ = layouts()[name]
    lib = ops._hip.lib()
    assert lib.ptts_dense_batched_resident_eligible(0, M, N, K, planes_count) == 1
    switch(True)
    c_on = product(ops, name, planes_count)
    switch(False)
    c_off = product(ops, name, planes_count)
    assert torch.equal(c_on, c_off), '{}: {} cells differ between the two kernels'.format(name, int((c_on != c_off).sum()))
    written = torch.zeros(numel, dtype=torch.bool)
    written.as_strided((nbatch, M, N), (sC, ldc, 1)).fill_(True)
    assert int((~written).sum()) > 0
    assert bool((c_on[~written] == SENTINEL).all()), '{}: cells outside the M x N guards were written'.format(name)
    got = c_on.as_strided((nbatch, M, N), (sC, ldc, 1)).double()
    want = operands(name, ops)[4 if planes_count == 3 else 5]
    e = float((got - want).abs().max() / want.abs().mean())
    print('{} planes {}: max error {:.3e} of mean |C|'.format(name, planes_count, e))
    assert e < 2e-5, (name, planes_count, e)


@pytest.mark.parametrize('name', ['dft', 'idft', 'dft_dy', 'one_row', 'full_tile', 'many_members'])
def test_resident_kernel_bit_for_bit_and_against_fp64(ops, switch, name):
    check_case(ops, switch, name, 3)


@pytest.mark.parametrize('name', ['idft', 'dft_dy'])
def test_resident_kernel_one_product(ops, switch, name):
    check_case(ops, switch, name, 1)


@pytest.mark.parametrize('what', ['M129', 'K132', 'strideA'])
def test_not_eligible_shapes_take_the_general_kernel(ops, switch, what):
    """M = 129, K = 132, or a left operand per member: not eligible, the same result whatever the switch says, and right against fp64."""
    nbatch, N = 3, 70
    M, K, shared = {'M129': (129, 120, True), 'K132': (100, 132, True), 'strideA': (100, 120, False)}[what]
    lib = ops._hip.lib()
    sA = 0 if shared else M * K
    assert lib.ptts_dense_batched_resident_eligible(sA, M, N, K, 3) == 0
    g = torch.Generator().manual_seed(77 + M + K)
    A = torch.randn(1 if shared else nbatch, M, K, generator=g, dtype=torch.float64).float()
    B = (torch.randn(nbatch, K, N, generator=g, dtype=torch.float64) / math.sqrt(K)).float()
    Ad, Bd = A.cuda(), B.cuda()
    npb = lib.ptts_dense_planes_bytes(N, K)
    planes = torch.empty(nbatch * npb, dtype=torch.uint8, device='cuda')
    ops.call('ptts_split3_dense_weight_strided', ops.ptr(Bd), K * N, ops.ptr(planes), npb, nbatch, N, K, N, 0, ops.stream())
    out = []
    for on in (True, False):
        switch(on)
        C = torch.full((nbatch * M * N + 64,), SENTINEL, device='cuda')
        ops.call('ptts_dense_bf16x6_batched', ops.ptr(Ad), sA, ops.ptr(planes), npb, None, ops.ptr(C), M * N, nbatch, M, N, K, K, N, 3, ops.stream())
        torch.cuda.synchronize()
        out.append(C.cpu())
    assert torch.equal(out[0], out[1])
    assert bool((out[0][nbatch * M * N:] == SENTINEL).all())
    want = torch.matmul(A.double(), B.double())
    e = float((out[0][:nbatch * M * N].view(nbatch, M, N).double() - want).abs().max() / want.abs().mean())
    assert e < 2e-5, (what, e)


@pytest.mark.parametrize('case', [(4, 200, 72, 32, 5), (16, 256, 72, 32, 5)], ids=['small', 'frequency_domain'])
def test_conv1d_layer_is_the_same_with_either_kernel(ops, switch, case):
    """ops.conv1d, forward and backward, seg_target = 100: y, dW and db equal bit for bit and the same launches (names and tags) with the
    switch on and off.  ops._C1FFT takes layers of B T >= 4096 frames only, so the first case (800 frames) runs the time-domain kernels
    and holds whatever the switch does -- in deterministic mode, since the time-domain weight gradient adds its partial sums with fp32
    atomics and two runs of it differ by themselves; the second is the smallest of its kind that does go through the three transforms
    (whose weight gradient has no atomics), and says so."""
    B, T, Cin, N, KW = case
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(KW, Cin, N, generator=g) / math.sqrt(KW * Cin)
    b = torch.randn(N, generator=g)
    dy = torch.randn(B, T, N, generator=g)
    ops.conv1d_fft(True); ops.conv1d_split(True)
    seg0 = ops._C1FFT.seg_target
    ops._C1FFT.seg_target = 100
    det0 = ops.deterministic()
    res = []
    try:
        ops.deterministic(B * T < 4096)
        for on in (True, False):
            switch(on)
            ops.clear_caches()
            xd, wd, bd = x.cuda(), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
            with ops._hip.KernelTimer() as kt:
                y = ops.conv1d(xd, wd, bd)
                y.backward(dy.cuda())
            torch.cuda.synchronize()
            res.append((y.detach().cpu(), wd.grad.cpu(), bd.grad.cpu(), [(r[0], r[1]) for r in kt.records]))
    finally:
        ops.deterministic(det0)
        ops._C1FFT.seg_target = seg0
        ops.conv1d_fft(None); ops.conv1d_split(None)
        ops.clear_caches()
    (y1, dw1, db1, l1), (y0, dw0, db0, l0) = res
    if B * T >= 4096:
        tags = [t[0] for n, t in l1 if n == 'ptts_dense_bf16x6_batched' and t]
        assert all(t in tags for t in ('dft', 'idft', 'dft_dy')), l1           # the three transforms ran
    assert [n for n, _ in l1] == [n for n, _ in l0] and l1 == l0
    assert torch.equal(y1, y0) and torch.equal(dw1, dw0) and torch.equal(db1, db0)
