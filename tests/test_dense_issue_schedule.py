"""The k-loops of csrc/dense.hip at the smallest shapes that reach every loop form, each case against a float64 numpy product of the
same inputs.  What a re-scheduled k-step can break is the hand-over between its stages -- a staging slice written to the wrong buffer or
skipped on the tail step, a load consumed one step early -- so the shapes walk the step counts (one, two, three, many; odd and even per
workgroup), the ragged last slab or quad, dead waves and the extra tiles, not the sizes of the workload (tests/test_ops_gpu.py has those).

Tolerances are test_ops_gpu.test_dense_forward_backward's, restated: Dense forward / backward-data rtol 2e-4, atol 1e-4; Dense weight
gradient and the column sums rtol 2e-4, atol 2e-4.

Row tiles per workgroup (MT) of dense_bf16x6_kernel: ptts_dense_bf16x6 and its siblings take pick_mt's choice, which is 4 for every M of a
single round of workgroups and 7 from 24 577 to 28 672 rows (the smallest M that reach it); it never returns 8 on its own (at equal
efficiency the smaller tile wins), and PTTS_DENSE_MT is read once per process, so MT = 8 (and 6) come from ptts_dense_bf16x6_batched with a left operand per member, whose
choice is the tile with the least row padding.

Every case function returns (got, want) lists of arrays, so that a script can also dump `got` for a bit-for-bit comparison of two
builds of the library."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.3
KS = (32, 64, 96, 256, 260)                 # one, two, three k-steps (the two-stage loop and each tail), many, a last step with quads beyond K
NS = (64, 256, 260)                         # dead waves, the full block, the extra column tile
MODES = ('plain', 'lrelu', 'maskmul', 'affine')
FWD_TOL = dict(rtol=2e-4, atol=1e-4)        # test_dense_forward_backward: y, dx
WG_TOL = dict(rtol=2e-4, atol=2e-4)         # test_dense_forward_backward: dw, db, dscale, dshift


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


def close(got, want, rtol, atol, what):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '{}: shape {} vs {}'.format(what, got.shape, want.shape)
    err = np.abs(got - want); tol = atol + rtol * np.abs(want)
    if (err > tol).any():
        i = int(np.argmax(err - tol))
        raise AssertionError('{}: {} / {} mismatches, worst |err|={:.3e} at flat {} (got {:.6e}, want {:.6e})'.format(
            what, int((err > tol).sum()), err.size, err.flat[i], i, got.flat[i], want.flat[i]))


def rng(*key):
    return np.random.RandomState(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def lrelu(x):
    return np.where(x > 0, x, ALPHA * x)


def planes_of(ops, w):
    """planes of B[K][N] = w (row-major)"""
    K, N = w.shape
    wd = dev(w)
    planes = torch.zeros(ops._hip.lib().ptts_dense_planes_bytes(N, K), dtype=torch.uint8, device='cuda')
    ops.call('ptts_split3_dense_weight', ops.ptr(wd), N, K, N, 0, ops.ptr(planes), ops.stream())
    return planes


def dense_inputs(M, N, K, mode, seed):
    r = rng(M, N, K, MODES.index(mode), seed)
    a = r.randn(M, K).astype(np.float32)
    w = (r.randn(K, N) / np.sqrt(K)).astype(np.float32)
    b = r.randn(N).astype(np.float32)
    msk = r.randn(M, K).astype(np.float32)
    sc = (r.rand(K) + 0.5).astype(np.float32); sh = (0.3 * r.randn(K)).astype(np.float32)
    a64 = a.astype(np.float64)
    ta = {'plain': a64, 'lrelu': lrelu(a64), 'maskmul': a64 * np.where(msk > 0, 1.0, ALPHA),
          'affine': lrelu(a64 * sc.astype(np.float64) + sh.astype(np.float64))}[mode]
    return a, w, b, msk, sc, sh, ta


def mode_args(ops, mode, msk, sc, sh):
    """(in_mode, in_scale, in_shift, mask_src) and the tensors that must stay alive"""
    if mode == 'plain': return (ops.IN_NONE, None, None, None), ()
    if mode == 'lrelu': return (ops.IN_LRELU, None, None, None), ()
    if mode == 'maskmul':
        m = dev(msk)
        return (ops.IN_MASKMUL, None, None, ops.ptr(m)), (m,)
    s, h = dev(sc), dev(sh)
    return (ops.IN_LRELU, ops.ptr(s), ops.ptr(h), None), (s, h)


def dense_case(ops, M, N, K, mode):
    """ptts_dense_bf16x6: T(A) . W + bias"""
    a, w, b, msk, sc, sh, ta = dense_inputs(M, N, K, mode, 1)
    planes = planes_of(ops, w)
    (im, ps, ph, pm), keep = mode_args(ops, mode, msk, sc, sh)
    ad, bd = dev(a), dev(b)
    c = torch.full((M, N), 7.0, dtype=torch.float32, device='cuda')
    ops.call('ptts_dense_bf16x6', ops.ptr(ad), ops.ptr(planes), ops.ptr(bd), ops.ptr(c), M, N, K, K, N, im, ps, ph, pm, ALPHA, 0, None, ops.stream())
    return [c.cpu().numpy()], [ta @ w.astype(np.float64) + b.astype(np.float64)]


def dense_res_case(ops, M, N, K, mode):
    """ptts_dense_bf16x6_res: + res[m % res_rows][:] in the store, and an output mask instead of a bias (backward-data's form)"""
    a, w, b, msk, sc, sh, ta = dense_inputs(M, N, K, mode, 2)
    r = rng(M, N, K, 22)
    res_rows = (M + 1) // 2
    res = r.randn(res_rows, N).astype(np.float32); om = r.randn(M, N).astype(np.float32)
    planes = planes_of(ops, w)
    (im, ps, ph, pm), keep = mode_args(ops, mode, msk, sc, sh)
    ad, rd, od = dev(a), dev(res), dev(om)
    c = torch.full((M, N), 7.0, dtype=torch.float32, device='cuda')
    ops.call('ptts_dense_bf16x6_res', ops.ptr(ad), ops.ptr(planes), None, ops.ptr(c), M, N, K, K, N, im, ps, ph, pm, ALPHA,
             ops.ptr(rd), res_rows, N, ops.ptr(od), ops.stream())
    want = (ta @ w.astype(np.float64)) * np.where(om > 0, 1.0, ALPHA) + res.astype(np.float64)[np.arange(M) % res_rows]
    return [c.cpu().numpy()], [want]


def dense_stats_case(ops, M, N, K, mode):
    """ptts_dense_bf16x6_stats: the product and, per row tile, the column sums and sums of squares of what it stores (no mask mode)"""
    a, w, b, msk, sc, sh, ta = dense_inputs(M, N, K, mode, 3)
    planes = planes_of(ops, w)
    (im, ps, ph, pm), keep = mode_args(ops, mode, msk, sc, sh)
    ad, bd = dev(a), dev(b)
    c = torch.full((M, N), 7.0, dtype=torch.float32, device='cuda')
    need = ops._hip.lib().ptts_dense_bf16x6_stats_rows(M, N)
    rows = torch.zeros(need, 2 * N, dtype=torch.float64, device='cuda'); n = ctypes.c_int(-1)
    ops.call('ptts_dense_bf16x6_stats', ops.ptr(ad), ops.ptr(planes), ops.ptr(bd), ops.ptr(c), M, N, K, K, N, im, ps, ph, ALPHA,
             ops.ptr(rows), need, ctypes.byref(n), ops.stream())
    assert n.value == need
    y = ta @ w.astype(np.float64) + b.astype(np.float64)
    return [c.cpu().numpy(), rows.cpu().numpy().sum(0)], [y, np.concatenate([y.sum(0), (y * y).sum(0)])]


def dense_bwd_affine_case(ops, M, N, K):
    """ptts_dense_bf16x6_bwd_affine: dz = (A . B) lrelu'(sc z + sh) sc and the two column sums"""
    a, w, b, msk, sc, sh, ta = dense_inputs(M, N, K, 'plain', 4)
    r = rng(M, N, K, 44)
    z = r.randn(M, N).astype(np.float32); osc = (r.rand(N) + 0.5).astype(np.float32); osh = (0.3 * r.randn(N)).astype(np.float32)
    planes = planes_of(ops, w)
    ad, zd, sd, hd = dev(a), dev(z), dev(osc), dev(osh)
    c = torch.full((M, N), 7.0, dtype=torch.float32, device='cuda')
    need = ops._hip.lib().ptts_dense_bf16x6_stats_rows(M, N)
    rows = torch.zeros(need, 2 * N, dtype=torch.float64, device='cuda'); n = ctypes.c_int(-1)
    ops.call('ptts_dense_bf16x6_bwd_affine', ops.ptr(ad), ops.ptr(planes), ops.ptr(c), M, N, K, K, N, ops.ptr(zd), ops.ptr(sd), ops.ptr(hd), ALPHA,
             ops.ptr(rows), need, ctypes.byref(n), ops.stream())
    assert n.value == need
    z64 = z.astype(np.float64)
    # the sign of sc z + sh as fp32 takes it (a product and a sum, each rounded): among millions of cells one lies within a rounding of zero,
    # and there the float64 sign would pick the other slope
    gd = (ta @ w.astype(np.float64)) * np.where(z * osc + osh > 0, 1.0, ALPHA)
    return [c.cpu().numpy(), rows.cpu().numpy().sum(0)], [gd * osc.astype(np.float64), np.concatenate([(gd * z64).sum(0), gd.sum(0)])]


def dense_batched_case(ops, nb, M, N, K):
    """ptts_dense_bf16x6_batched with a left operand per member (dense_bf16x6_kernel, plain mode, MT by least row padding)"""
    r = rng(nb, M, N, K, 5)
    a = r.randn(nb, M, K).astype(np.float32); w = (r.randn(nb, K, N) / np.sqrt(K)).astype(np.float32); b = r.randn(N).astype(np.float32)
    pb = ops._hip.lib().ptts_dense_planes_bytes(N, K)
    planes = torch.zeros(nb * pb, dtype=torch.uint8, device='cuda')
    wd = dev(w)
    ops.call('ptts_split3_dense_weight_strided', ops.ptr(wd), K * N, ops.ptr(planes), pb, nb, N, K, N, 0, ops.stream())
    ad, bd = dev(a), dev(b)
    c = torch.full((nb, M, N), 7.0, dtype=torch.float32, device='cuda')
    ops.call('ptts_dense_bf16x6_batched', ops.ptr(ad), M * K, ops.ptr(planes), pb, ops.ptr(bd), ops.ptr(c), M * N, nb, M, N, K, K, N, 3, ops.stream())
    return [c.cpu().numpy()], [np.matmul(a.astype(np.float64), w.astype(np.float64)) + b.astype(np.float64)]


def wgrad_case(ops, M, Kin, N, mode, bias):
    """ptts_dense_wgrad_bf16x6 into zeroed buffers; the partial rows of two launches of the first stage, bit for bit"""
    r = rng(M, Kin, N, mode, 6)
    a = r.randn(M, Kin).astype(np.float32); dy = r.randn(M, N).astype(np.float32); msk = r.randn(M, Kin).astype(np.float32)
    ad, dd, md = dev(a), dev(dy), dev(msk)
    lib = ops._hip.lib()
    nbytes = lib.ptts_dense_wgrad_workspace_bytes(Kin, N, M)
    ws = [torch.full((nbytes // 4,), 7.0, dtype=torch.float32, device='cuda') for _ in range(2)]
    split = ctypes.c_int(0)
    pm = ops.ptr(md) if mode == ops.IN_MASKMUL else None
    for w in ws:
        ops.call('ptts_dense_wgrad_bf16x6_partials', ops.ptr(ad), ops.ptr(dd), pm, None, None, ops.ptr(w), nbytes, ctypes.byref(split),
                 Kin, N, M, Kin, N, mode, ALPHA, ops.stream())
    torch.cuda.synchronize()
    # (the remainder tile's 16 rows of a partial row belong to the last tile row's workgroups alone: the others never write theirs)
    assert torch.equal(ws[0], ws[1]), 'partial rows differ between two launches'
    c = torch.zeros(Kin, N, dtype=torch.float32, device='cuda')
    db = torch.zeros(N, dtype=torch.float32, device='cuda') if bias else None
    ops.call('ptts_dense_wgrad_bf16x6', ops.ptr(ad), ops.ptr(dd), pm, None, None, ops.ptr(c), ops.ptr(db), ops.ptr(ws[0]), nbytes,
             Kin, N, M, Kin, N, N, mode, ALPHA, ops.stream())
    a64 = a.astype(np.float64)
    ta = a64 if mode == ops.IN_NONE else (lrelu(a64) if mode == ops.IN_LRELU else a64 * np.where(msk > 0, 1.0, ALPHA))
    got, want = [c.cpu().numpy()], [ta.T @ dy.astype(np.float64)]
    if bias:
        got.append(db.cpu().numpy()); want.append(dy.astype(np.float64).sum(0))
    return got, want


def tn_case(ops, nb, M, Kin, N, shared_a=False):
    """ptts_dense_tn_bf16x6_batched: C_z = A_z^T . B_z; rows of C padded by four floats that must stay untouched"""
    r = rng(nb, M, Kin, N, 7)
    lda, ldb, ldc = (Kin + 3) // 4 * 4, (N + 3) // 4 * 4, N + 4
    na = 1 if shared_a else nb
    a = r.randn(na, M, lda).astype(np.float32); b = r.randn(nb, M, ldb).astype(np.float32)
    ad, bd = dev(a), dev(b)
    c = torch.full((nb, Kin, ldc), 7.0, dtype=torch.float32, device='cuda')
    ops.call('ptts_dense_tn_bf16x6_batched', ops.ptr(ad), 0 if shared_a else M * lda, ops.ptr(bd), M * ldb, ops.ptr(c), Kin * ldc,
             nb, M, Kin, N, lda, ldb, ldc, 3, ops.stream())
    got = c.cpu().numpy()
    assert (got[:, :, N:] == 7.0).all(), 'cells beyond N were written'
    a64 = np.broadcast_to(a.astype(np.float64), (nb, M, lda))
    want = np.matmul(a64[:, :, :Kin].transpose(0, 2, 1), b.astype(np.float64)[:, :, :N])
    return [got[:, :, :N]], [want]


def check(got, want, tols, what):
    for i, (g, w) in enumerate(zip(got, want)):
        close(g, w, what='{} [{}]'.format(what, i), **(tols[i] if isinstance(tols, (list, tuple)) else tols))


MT4_MS = (64, 69, 144)                      # MT = 4: 16 MT, 16 MT + 5, 2 x 16 MT + 16
MT7_MS = (24640, 24640 + 5, 24640 + 112 + 16)   # MT = 7 (pick_mt's choice from 24 577 to 28 672 rows): whole tiles, a ragged last tile, 16 rows into one
# MT = 7: every K at the ragged M and the 260-wide output, the other two M at three k-steps with dead waves
MT7_CASES = tuple((MT7_MS[1], 260, K) for K in KS) + ((MT7_MS[0], 64, 96), (MT7_MS[2], 64, 96), (MT7_MS[0], 256, 256))


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('mode', MODES)
def test_dense_forward_every_k_loop_form(ops, mode, N):
    for K in KS:
        for M in MT4_MS:
            got, want = dense_case(ops, M, N, K, mode)
            check(got, want, FWD_TOL, 'dense {} M={} N={} K={}'.format(mode, M, N, K))


@pytest.mark.parametrize('mode', MODES)
def test_dense_forward_seven_row_tiles(ops, mode):
    for M, N, K in MT7_CASES:
        got, want = dense_case(ops, M, N, K, mode)
        check(got, want, FWD_TOL, 'dense {} M={} N={} K={}'.format(mode, M, N, K))


def test_dense_siblings_seven_row_tiles(ops):
    M = MT7_MS[1]
    for K in KS:
        mode = MODES[KS.index(K) % len(MODES)]
        got, want = dense_res_case(ops, M, 256, K, mode)
        check(got, want, FWD_TOL, 'dense_res {} M={} K={}'.format(mode, M, K))
        got, want = dense_stats_case(ops, M, 256, K, 'affine' if mode == 'maskmul' else mode)
        check(got, want, [FWD_TOL, WG_TOL], 'dense_stats M={} K={}'.format(M, K))
        got, want = dense_bwd_affine_case(ops, M, 256, K)
        check(got, want, [FWD_TOL, WG_TOL], 'dense_bwd_affine M={} K={}'.format(M, K))


@pytest.mark.parametrize('M', [128, 123, 272])                 # MT = 8, 8 (ragged), 6
def test_dense_batched_general_kernel_taller_tiles(ops, M):
    for K in KS:
        for N in NS:
            got, want = dense_batched_case(ops, 2, M, N, K)
            check(got, want, FWD_TOL, 'batched M={} N={} K={}'.format(M, N, K))


@pytest.mark.parametrize('mode', MODES)
def test_dense_residual_and_output_mask(ops, mode):
    for K in KS:
        for M, N in ((69, 64), (144, 256), (64, 260)):
            got, want = dense_res_case(ops, M, N, K, mode)
            check(got, want, FWD_TOL, 'dense_res {} M={} N={} K={}'.format(mode, M, N, K))


@pytest.mark.parametrize('mode', ['plain', 'lrelu', 'affine'])
def test_dense_with_column_statistics(ops, mode):
    for K in KS:
        for M, N in ((69, 64), (144, 256), (64, 260)):
            got, want = dense_stats_case(ops, M, N, K, mode)
            check(got, want, [FWD_TOL, WG_TOL], 'dense_stats {} M={} N={} K={}'.format(mode, M, N, K))


def test_dense_backward_data_through_an_affine(ops):
    for K in KS:
        for M, N in ((69, 64), (144, 256), (64, 260)):
            got, want = dense_bwd_affine_case(ops, M, N, K)
            check(got, want, [FWD_TOL, WG_TOL], 'dense_bwd_affine M={} N={} K={}'.format(M, N, K))


# 32-row steps per workgroup (64 workgroups per tile): 1, 1-2 and 2-3 with a ragged last slab, and 4 = two trips of the two-step loop
WG_MS = (2048, 2048 + 33, 4096 + 31, 8192)


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('Kin', [256, 260])
def test_dense_weight_gradient_step_counts(ops, Kin, mode, bias):
    for M in WG_MS:
        got, want = wgrad_case(ops, M, Kin, 256, mode, bias)
        check(got, want, WG_TOL, 'wgrad M={} Kin={} mode={} bias={}'.format(M, Kin, mode, bias))


@pytest.mark.parametrize('nb', [2, 3])
def test_dense_tn_batched_step_counts(ops, nb):
    for M in (32, 33, 64, 95):                  # one step, one and a ragged second, two, three with a ragged last
        for Kin in (128, 130):
            for N in (128, 256):
                got, want = tn_case(ops, nb, M, Kin, N)
                check(got, want, WG_TOL, 'tn nb={} M={} Kin={} N={}'.format(nb, M, Kin, N))


def test_dense_tn_batched_shared_left_operand(ops):
    got, want = tn_case(ops, 3, 95, 130, 256, shared_a=True)
    check(got, want, WG_TOL, 'tn shared A')


def all_cases(ops):
    """(name, got arrays) of every case above, for a bit-for-bit comparison of two builds"""
    for mode in MODES:
        for N in NS:
            for K in KS:
                for M in MT4_MS:
                    yield 'dense_{}_{}_{}_{}'.format(mode, M, N, K), dense_case(ops, M, N, K, mode)[0]
        for M, N, K in MT7_CASES:
            yield 'dense7_{}_{}_{}_{}'.format(mode, M, N, K), dense_case(ops, M, N, K, mode)[0]
        for K in KS:
            for M, N in ((69, 64), (144, 256), (64, 260)):
                yield 'res_{}_{}_{}_{}'.format(mode, M, N, K), dense_res_case(ops, M, N, K, mode)[0]
                if mode != 'maskmul':
                    yield 'stats_{}_{}_{}_{}'.format(mode, M, N, K), dense_stats_case(ops, M, N, K, mode)[0]
    for K in KS:
        for M, N in ((69, 64), (144, 256), (64, 260)):
            yield 'bwdaff_{}_{}_{}'.format(M, N, K), dense_bwd_affine_case(ops, M, N, K)[0]
        for M in (128, 123, 272):
            for N in NS:
                yield 'batched_{}_{}_{}'.format(M, N, K), dense_batched_case(ops, 2, M, N, K)[0]
    for K in KS:
        mode = MODES[KS.index(K) % len(MODES)]
        yield 'res7_{}'.format(K), dense_res_case(ops, MT7_MS[1], 256, K, mode)[0]
        yield 'stats7_{}'.format(K), dense_stats_case(ops, MT7_MS[1], 256, K, 'affine' if mode == 'maskmul' else mode)[0]
        yield 'bwdaff7_{}'.format(K), dense_bwd_affine_case(ops, MT7_MS[1], 256, K)[0]
    for Kin in (256, 260):
        for mode in (0, 1, 2):
            for M in WG_MS:
                yield 'wgrad_{}_{}_{}'.format(M, Kin, mode), wgrad_case(ops, M, Kin, 256, mode, True)[0]
    for nb in (2, 3):
        for M in (32, 33, 64, 95):
            for Kin in (128, 130):
                for N in (128, 256):
                    yield 'tn_{}_{}_{}_{}'.format(nb, M, Kin, N), tn_case(ops, nb, M, Kin, N)[0]
    yield 'tn_shared', tn_case(ops, 3, 95, 130, 256, shared_a=True)[0]
