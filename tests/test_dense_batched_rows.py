"""GPU tests of the fp32-rows form of ptts_dense_bf16x6_batched's right operand (csrc/dense.hip, dense_bf16x6_resident_kernel<.., ROWS>;
planes_count | PTTS_PLANES_ROWS, a ptts_dense_rows_desc in place of the planes) and of its mirrored store: the product reads the rows
of the frequency-domain context Conv1D's single-use operands -- the windows of the input ('dft'), the per-frequency products ('idft') --
as fp32 and splits them itself.  Every case compares the WHOLE C buffer, pre-filled with a sentinel, bit for bit (torch.equal) with the
older two or three launches: split pass (ptts_split3_frame_windows / ptts_split3_dense_weight_strided), product on the planes, and
ptts_dft_mirror where the store is mirrored.  The source is a view inside a larger allocation whose margins are NaN: a row that counts
as zero and is read all the same shows as a NaN in C, not as a read out of bounds.

The windows case with kvalid < P runs at P = 112, kvalid = 104: the product's reduction length must be a multiple of 4, which the
110 rows of the split pass's own test of that geometry (test_ops_gpu.py::test_frame_window_and_strided_planes_bit_for_bit) are not.

The layer-level tests: ops.conv1d forward and backward with the switch (ops.conv1d_fft_rows) on and off, bit for bit, and the launch
lists.  The second layer (16, 256, 70, 32, 5) has segments of 128 frames -- the divisor of 256 closest to 100 -- so its windows are
132 rows, more than the resident-left kernel's 128: it keeps the older stage list whatever the switch says, and the test says so."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.625          # exactly representable: an untouched cell compares equal bit for bit
MARGIN = 64 * 1024             # NaN floats in front of and behind every source (a multiple of 4: the views keep 16-byte alignment)


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


@pytest.fixture()
def switch(ops):
    """Sets the resident-left switch; the setting found is put back afterwards."""
    lib = ops._hip.lib()
    first = lib.ptts_set_dense_batched_resident(1)
    yield lambda on: lib.ptts_set_dense_batched_resident(1 if on else 0)
    lib.ptts_set_dense_batched_resident(first)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def inside_nan(values):
    """A device copy of `values` (flat, fp32) as a view with MARGIN NaNs on either side."""
    buf = torch.full((MARGIN + values.numel() + MARGIN,), float('nan'), device='cuda')
    view = buf[MARGIN:MARGIN + values.numel()]
    view.copy_(values.reshape(-1))
    return buf, view


# windows: (B, T, C, NS, S, row_off, P, kvalid); the product is [M = 2 NB][P] . window [P][C] into Ap [NB][2][Z][2 Kh], mirrored
WINDOWS = {
    'x601': (3, 200, 601, 2, 100, -10, 120, 120),       # N % 4 != 0, a partial last slice, four k-steps (the compile-time count)
    'x70': (3, 200, 70, 2, 100, -10, 120, 120),
    'small': (5, 37, 13, 1, 37, -1, 40, 40),            # N < 32, two k-steps (the run-time count)
    'kvalid': (2, 300, 260, 3, 100, -5, 112, 104),      # kvalid < P
}
# strided rows: (nbatch, M, N, K, kvalid, bias); member z's row k at z N + k nbatch N, as the inverse transform reads Yh.  'many': one
# matrix after the other, so many members that every wave walks several items
ROWS = {
    'idft256': (7, 100, 256, 124, 122, True),
    'idft20': (7, 100, 20, 124, 122, True),
    'many': (None, 16, 64, 32, 32, False),
}

_CACHE = {}


def windows_case(ops, name, planes_count):
    """(C of the rows form, C of split + product + mirror), both on the host."""
    B, T, C, NS, S, row_off, P, kvalid = WINDOWS[name]
    lib = ops._hip.lib()
    Z, NB, Kh = B * NS, P // 2 + 1, (C + 7) // 8 * 8
    M = 2 * NB
    if name not in _CACHE:
        g = torch.Generator().manual_seed(500 + C + P)
        A = torch.randn(M, P, generator=g, dtype=torch.float64).float().cuda()
        x = torch.randn(B, T, C, generator=g, dtype=torch.float64).float()
        _CACHE[name] = (A,) + inside_nan(x)
    A, keep, xd = _CACHE[name]
    numel = NB * 2 * Z * 2 * Kh
    # the older three launches
    npb = lib.ptts_dense_planes_bytes(C, P)
    planes = torch.empty(Z * npb, dtype=torch.uint8, device='cuda')
    ops.call('ptts_split3_frame_windows', ops.ptr(xd), B, T, C, NS, S, row_off, P, kvalid, ops.ptr(planes), npb, ops.stream())
    want = torch.full((numel,), SENTINEL, device='cuda')
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ops.ptr(planes), npb, None, ops.ptr(want), 2 * Kh, Z, M, C, P, P, Z * 2 * Kh,
             planes_count, ops.stream())
    ops.call('ptts_dft_mirror', ops.ptr(want), NB, Z, C, Kh, ops.stream())
    # one launch on the rows
    got = torch.full((numel,), SENTINEL, device='cuda')
    d = ops._hip.DenseRowsDesc(B=xd.data_ptr(), strideB=0, ldb=C, windows=1, nB=B, T=T, NS=NS, S=S, row_off=row_off, kvalid=kvalid, mirror_cols=Kh)
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ctypes.byref(d), 0, None, ops.ptr(got), 2 * Kh, Z, M, C, P, P, Z * 2 * Kh,
             planes_count | ops._hip.PLANES_ROWS, ops.stream())
    torch.cuda.synchronize()
    return got.cpu(), want.cpu()


def rows_case(ops, name, planes_count):
    nbatch, M, N, K, kvalid, has_bias = ROWS[name]
    lib = ops._hip.lib()
    if nbatch is None:
        nbatch = 3 * cus() * 4
        strideB, ldb = kvalid * N, N
    else:
        strideB, ldb = N, nbatch * N
    key = (name, nbatch)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(900 + N + K)
        A = torch.randn(M, K, generator=g, dtype=torch.float64).float().cuda()
        Bm = (torch.randn(kvalid * nbatch * N, generator=g, dtype=torch.float64) / math.sqrt(K)).float()
        bias = torch.randn(N, generator=g, dtype=torch.float64).float().cuda()
        _CACHE[key] = (A, bias) + inside_nan(Bm)
    A, bias, keep, Bd = _CACHE[key]
    bias = bias if has_bias else None
    numel = nbatch * M * N + 64
    npb = lib.ptts_dense_planes_bytes(N, kvalid)
    planes = torch.empty(nbatch * npb, dtype=torch.uint8, device='cuda')
    ops.call('ptts_split3_dense_weight_strided', ops.ptr(Bd), strideB, ops.ptr(planes), npb, nbatch, ldb, kvalid, N, 0, ops.stream())
    want = torch.full((numel,), SENTINEL, device='cuda')
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ops.ptr(planes), npb, ops.ptr(bias), ops.ptr(want), M * N, nbatch, M, N, K, K, N,
             planes_count, ops.stream())
    got = torch.full((numel,), SENTINEL, device='cuda')
    d = ops._hip.DenseRowsDesc(B=Bd.data_ptr(), strideB=strideB, ldb=ldb, windows=0, nB=0, T=0, NS=0, S=0, row_off=0, kvalid=kvalid, mirror_cols=0)
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ctypes.byref(d), 0, ops.ptr(bias), ops.ptr(got), M * N, nbatch, M, N, K, K, N,
             planes_count | ops._hip.PLANES_ROWS, ops.stream())
    torch.cuda.synchronize()
    return got.cpu(), want.cpu()


def check(got, want, what):
    assert not bool(torch.isnan(want).any()), '{}: the reference read a NaN margin'.format(what)
    assert not bool(torch.isnan(got).any()), '{}: {} NaN cells: a row that counts as zero was read'.format(what, int(torch.isnan(got).sum()))
    assert int((want != SENTINEL).sum()) > 0 and int((want == SENTINEL).sum()) > 0
    assert torch.equal(got, want), '{}: {} cells differ from split + product (+ mirror)'.format(what, int((got != want).sum()))


@pytest.mark.parametrize('planes_count', [3, 1])
@pytest.mark.parametrize('name', sorted(WINDOWS))
def test_windows_with_mirror_bit_for_bit(ops, switch, name, planes_count):
    switch(True)
    got, want = windows_case(ops, name, planes_count)
    check(got, want, (name, planes_count))


@pytest.mark.parametrize('planes_count', [3, 1])
@pytest.mark.parametrize('name', sorted(ROWS))
def test_strided_rows_bit_for_bit(ops, switch, name, planes_count):
    switch(True)
    got, want = rows_case(ops, name, planes_count)
    check(got, want, (name, planes_count))


@pytest.mark.parametrize('what', ['M129', 'switch_off'])
def test_rows_form_needs_the_resident_kernel(ops, switch, what):
    """M = 129 (not eligible), or the resident-left switch off: the rows form returns an error and launches nothing."""
    M, N, K, nbatch = (129 if what == 'M129' else 100), 70, 120, 3
    switch(what != 'switch_off')
    A = torch.randn(M, K).cuda()
    keep, Bd = inside_nan(torch.randn(nbatch, K, N))
    C = torch.full((nbatch * M * N + 64,), SENTINEL, device='cuda')
    d = ops._hip.DenseRowsDesc(B=Bd.data_ptr(), strideB=K * N, ldb=N, windows=0, nB=0, T=0, NS=0, S=0, row_off=0, kvalid=K, mirror_cols=0)
    with pytest.raises(ops._hip.HipLibraryError, match='resident-left'):
        ops.call('ptts_dense_bf16x6_batched', ops.ptr(A), 0, ctypes.byref(d), 0, None, ops.ptr(C), M * N, nbatch, M, N, K, K, N,
                 3 | ops._hip.PLANES_ROWS, ops.stream())
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())


def _layer(ops, case, rows, seg):
    """y, dW, db of ops.conv1d forward + backward and the launches (name, tag) of the forward."""
    B, T, Cin, N, KW = case
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(KW, Cin, N, generator=g) / math.sqrt(KW * Cin)
    b = torch.randn(N, generator=g)
    dy = torch.randn(B, T, N, generator=g)
    ops.conv1d_fft(True); ops.conv1d_split(True)
    seg0 = ops._C1FFT.seg_target
    ops._C1FFT.seg_target = seg
    try:
        ops.conv1d_fft_rows(rows)
        ops.clear_caches()
        xd, wd, bd = x.cuda(), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        assert ops._C1FFT.eligible(xd, wd)
        with ops._hip.KernelTimer() as kt:
            y = ops.conv1d(xd, wd, bd)
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        return y.detach().cpu(), wd.grad.cpu(), bd.grad.cpu(), [(r[0], r[1]) for r in kt.records]
    finally:
        ops._C1FFT.seg_target = seg0
        ops.conv1d_fft_rows(None)
        ops.conv1d_fft(None); ops.conv1d_split(None)
        ops.clear_caches()


def _tags(launches, name):
    return [t[0] for n, t in launches if n == name and t]


def _old_list(launches):
    """The forward as split, 'dft', mirror, 'freq', split, 'idft'."""
    names = [n for n, _ in launches]
    assert names.count('ptts_dense_bf16x6_batched') == 3 and _tags(launches, 'ptts_dense_bf16x6_batched') == ['dft', 'freq', 'idft'], launches
    assert _tags(launches, 'ptts_split3_frame_windows') == ['x'] and names.count('ptts_dft_mirror') == 1, launches
    assert _tags(launches, 'ptts_split3_dense_weight_strided') == ['y'], launches


@pytest.mark.parametrize('case', [(12, 400, 601, 256, 21), (16, 256, 70, 32, 5)], ids=['flagship', 'small'])
def test_conv1d_layer_rows_on_and_off(ops, switch, case):
    """seg = 100: y, dW and db bit for bit with the switch on and off; with it on, and where the transforms run on the resident-left
    kernel, three products and none of the three passes in the forward -- elsewhere the older stage list."""
    B, T, Cin, N, KW = case
    switch(True)
    y1, dw1, db1, l1 = _layer(ops, case, True, 100)
    y0, dw0, db0, l0 = _layer(ops, case, False, 100)
    assert torch.equal(y1, y0) and torch.equal(dw1, dw0) and torch.equal(db1, db0)
    _old_list(l0)
    S = ops._C1FFT.segment(T, KW)
    P = (S + KW - 1 + 3) // 4 * 4
    names1 = [n for n, _ in l1]
    assert names1.count('ptts_dense_bf16x6_batched') == 3, l1
    if P <= 128:
        assert 'x' not in _tags(l1, 'ptts_split3_frame_windows') and 'ptts_dft_mirror' not in names1, l1
        assert 'y' not in _tags(l1, 'ptts_split3_dense_weight_strided'), l1
        assert _tags(l1, 'ptts_dense_bf16x6_batched') == ['dft', 'freq', 'idft'], l1
    else:
        assert case == (16, 256, 70, 32, 5) and P == 132         # windows beyond the resident-left kernel: the older list
        assert l1 == l0


def test_conv1d_layer_whole_utterances_keep_the_old_list(ops, switch):
    """seg = 0 (one window of 420 rows per utterance): the older stage list with the switch on, within 2e-5 of mean |y| of the fp64
    convolution (the bound of test_ops_gpu.py::test_conv1d_frequency_domain_forward)."""
    case = (12, 400, 601, 256, 21)
    B, T, Cin, N, KW = case
    switch(True)
    y1, _, _, l1 = _layer(ops, case, True, 0)
    _old_list(l1)
    g = torch.Generator().manual_seed(5)                          # _layer's operands
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(KW, Cin, N, generator=g) / math.sqrt(KW * Cin)
    b = torch.randn(N, generator=g)
    want = torch.nn.functional.conv1d(x.double().transpose(1, 2), w.double().permute(2, 1, 0), b.double(), padding=(KW - 1) // 2).transpose(1, 2)
    e = float((y1.double() - want).abs().max() / want.abs().mean())
    print('seg 0: max error {:.3e} of mean |y|'.format(e))
    assert e < 2e-5, e
