"""csrc/dense.hip, the few columns / rows beyond a whole tile (the critic's 260 = 256 + 4 wide layer) without a pass or a tile row
of their own: the extra column tile of dense_bf16x6_kernel, the remainder tile of dense_wgrad_bf16x6_kernel, and the waves of a
narrow product that only stage.  Everything through ops.gemm_raw, the routing the layers use; bounds as in
test_ops_gpu.test_dense_bf16x6_planes_and_products / test_dense_weight_gradient_bf16x6."""
import pytest
import torch

from oracle import percival_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _weight(src):
    """src as a weight of a flat parameter buffer (what ops._DenseSplit builds planes for)."""
    from percivaltts_amd import layers

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(src.clone())
    h = Holder()
    flat = layers.FlatParams(h, 'cuda')
    return h, flat, h.w


def _product(ops, split, A, w, M, N, K, transposed, ldb, ldc, init=None, **kw):
    """C [M, ldc] after gemm_raw of an [M, N] product (columns >= N keep the canary), and the C-ABI calls made."""
    ops.dense_split(split)
    try:
        C = torch.full((M, ldc), 7.0, dtype=torch.float32, device='cuda') if init is None else init.clone()
        with ops._hip.KernelTimer() as kt:
            ops.gemm_raw(A, w, C, M, N, K, transB=transposed, ldb=ldb, ldc=ldc, **kw)
        return C.cpu(), [r[0] for r in kt.records]
    finally:
        ops.dense_split(None)


@pytest.mark.parametrize('case', [(1500, 260, 256, 1), (2048, 272, 64, 0), (1100, 516, 256, 0), (1024, 276, 64, 0)])
def test_extra_column_tile(ops, case):
    """N mod 256 in 1..16: one ptts_dense_bf16x6 launch whose last column block multiplies the remainder as a 17th tile, no thin
    product.  Cases: the critic's backward-data shape (ragged last row tile, 4 live columns, W^T planes), a full extra tile over two
    k-steps, two column blocks with the remainder on the second, and a remainder of 20 that keeps the old cut (256 columns, then
    the remainder as a second product).  Bias, LeakyReLU, affine + LeakyReLU, gradient-penalty mask, output mask, accumulate; ldc = N.
    Every column against fp64 at the bound of test_dense_bf16x6_planes_and_products; columns below the last multiple of 256
    BIT-identical to the product of just those columns on the same operands: the main tiles' arithmetic does not move."""
    M, N, K, transposed = case
    N0 = N - N % 256
    g = gen(91)
    A = torch.randn(M, K, generator=g, dtype=torch.float64).float()
    W = (torch.randn(K, N, generator=g, dtype=torch.float64) / K ** 0.5).float()
    b = torch.randn(N, generator=g, dtype=torch.float64).float()
    scale = (torch.rand(K, generator=g, dtype=torch.float64) + 0.5).float(); shift = torch.randn(K, generator=g, dtype=torch.float64).float()
    msk = torch.randn(M, K, generator=g, dtype=torch.float64).float()
    omask = torch.randn(M, N, generator=g, dtype=torch.float64).float()
    c0 = torch.randn(M, N, generator=g, dtype=torch.float64).float()
    src = (W.t().contiguous() if transposed else W).cuda()
    holder, flat, w = _weight(src)
    ldb = src.shape[1]
    Ad, bd = A.cuda(), b.cuda()
    A64, W64 = A.double(), W.double()
    variants = [
        ('plain+bias', dict(bias=bd), A64 @ W64 + b.double()),
        ('lrelu', dict(mode=ops.IN_LRELU, alpha=0.3), O.lrelu(A64) @ W64),
        ('affine+lrelu', dict(mode=ops.IN_LRELU, scale=scale.cuda(), shift=shift.cuda(), alpha=0.3, bias=bd),
         O.lrelu(A64 * scale.double() + shift.double()) @ W64 + b.double()),
        ('maskmul', dict(mode=ops.IN_MASKMUL, mask_src=msk.cuda(), alpha=0.3), (A64 * torch.where(msk.double() > 0, 1.0, 0.3)) @ W64),
        ('out_mask', dict(out_mask=omask.cuda(), alpha=0.3), (A64 @ W64) * torch.where(omask.double() > 0, 1.0, 0.3)),
        ('accumulate', dict(accumulate=1, init=c0.cuda()), A64 @ W64 + c0.double()),
    ]
    for name, kw, ref64 in variants:
        y, names = _product(ops, True, Ad, w, M, N, K, transposed, ldb, N, **kw)
        y32, _ = _product(ops, False, Ad, w, M, N, K, transposed, ldb, N, **kw)
        head, names_head = _product(ops, True, Ad, w, M, N0, K, transposed, ldb, N, **kw)
        products = [n for n in names if n in ('ptts_dense_bf16x6', 'ptts_gemm')]
        if N % 256 <= 16:
            assert products == ['ptts_dense_bf16x6'], (name, names)
        else:                                           # the old cut: the first 256 columns, then the remainder as a product of its own
            assert len(products) == 2 and products[0] == 'ptts_dense_bf16x6', (name, names)
        assert names_head.count('ptts_dense_bf16x6') == 1 and 'ptts_gemm' not in names_head, (name, names_head)
        sc = ref64.abs().mean()
        e = ((y.double() - ref64).abs().max() / sc).item(); e32 = ((y32.double() - ref64).abs().max() / sc).item()
        e_tail = ((y.double() - ref64)[:, N0:].abs().max() / sc).item()
        print('{} {}: e = {:.3e} (columns beyond {}: {:.3e}), fp32 kernel {:.3e}'.format(case, name, e, N0, e_tail, e32))
        assert e < 3e-5 and e < max(4 * max(e32, 2e-6), 8 * 2.0 ** -24 * K ** 0.5), (name, e, e32)
        # The fp32 kernel is under test as well, not only a yardstick: its own error under the accumulation bound.  With the output mask
        # the bound is taken of mean |A.W|, the sum it describes: the mask scales half of the outputs by 0.3 AFTER the accumulation, so
        # mean |ref| falls to 0.65 of it while the error of the other half stays.  Measured at (2048, 272, 64): 3.854e-6 of mean |ref|
        # against the bound 3.815e-6 -- from the kernel and from a float32 torch.matmul on the CPU alike -- and 2.503e-6 of mean |A.W|.
        sc32 = (A64 @ W64).abs().mean() if name == 'out_mask' else sc
        e32_own = ((y32.double() - ref64).abs().max() / sc32).item()
        assert e32_own < 8 * 2.0 ** -24 * K ** 0.5, '{}: the fp32 kernel itself is {:.3e} off'.format(name, e32_own)
        assert torch.equal(y[:, :N0], head[:, :N0]), '{}: columns below {} differ from the {}-column product in {} entries'.format(
            name, N0, N0, int((y[:, :N0] != head[:, :N0]).sum()))
        want_tail = c0[:, N0:] if name == 'accumulate' else torch.full((M, N - N0), 7.0)
        assert torch.equal(head[:, N0:], want_tail), name + ': the head product wrote beyond its columns'


@pytest.mark.parametrize('case', [(260, 256, 3001), (272, 128, 2048), (388, 64, 2100), (276, 256, 2048)])
def test_weight_gradient_remainder_tile(ops, case):
    """Kin mod 128 in 1..16: the workgroups of the last full tile row also accumulate the 16-row remainder tile; no tile row for it.
    Cases: the critic's 260-wide input over a ragged frame count, a full 16-row remainder at one tile column, three
    full tile rows plus 4 at a narrow N, and a remainder of 20 on the old path (a tile row of its own).  Plain, LeakyReLU,
    affine + LeakyReLU and gradient-penalty mask on A.  dW against fp64 at the bound of test_dense_weight_gradient_bf16x6, db against
    the fp64 column sums, nothing written beyond row Kin, and -- where the remainder tile runs -- rows below 128 (Kin // 128)
    BIT-identical to the product of just those columns of A (lda = Kin): the same split, the same steps, one add into zeros."""
    Kin, N, M = case
    Kf = Kin - Kin % 128
    g = gen(92)
    A = torch.randn(M, Kin, generator=g, dtype=torch.float64).float()
    dY = torch.randn(M, N, generator=g, dtype=torch.float64).float()
    scale = (torch.rand(Kin, generator=g, dtype=torch.float64) + 0.5).float(); shift = torch.randn(Kin, generator=g, dtype=torch.float64).float()
    msk = torch.randn(M, Kin, generator=g, dtype=torch.float64).float()
    Ad, dYd = A.cuda(), dY.cuda()
    A64, dY64 = A.double(), dY.double()

    def run(split, kin, **kw):
        ops.dense_split(split)
        min_n, ops._DenseSplit.wgrad_min_n = ops._DenseSplit.wgrad_min_n, 16
        try:
            big = torch.full((Kin + 3, N), 7.0, dtype=torch.float32, device='cuda')      # rows >= kin: the canary
            db = torch.full((N,), 7.0, dtype=torch.float32, device='cuda')
            with ops._hip.KernelTimer() as kt:
                ops.gemm_raw(Ad, dYd, big[:kin], kin, N, M, transA=1, lda=Kin, rows_per_seg=M, colsum_b=db, **kw)
            return big.cpu(), db.cpu().double(), [r[0] for r in kt.records]
        finally:
            ops.dense_split(None)
            ops._DenseSplit.wgrad_min_n = min_n

    variants = [
        ('plain', dict(), A64),
        ('lrelu', dict(mode=ops.IN_LRELU, alpha=0.3), O.lrelu(A64)),
        ('affine+lrelu', dict(mode=ops.IN_LRELU, scale=scale.cuda(), shift=shift.cuda(), alpha=0.3), O.lrelu(A64 * scale.double() + shift.double())),
        ('maskmul', dict(mode=ops.IN_MASKMUL, mask_src=msk.cuda(), alpha=0.3), A64 * torch.where(msk.double() > 0, 1.0, 0.3)),
    ]
    for name, kw, TA in variants:
        ref = TA.t() @ dY64
        big, db, names = run(True, Kin, **kw)
        big32, _, names32 = run(False, Kin, **kw)
        assert 'ptts_dense_wgrad_bf16x6' in names and 'ptts_dense_wgrad_bf16x6' not in names32, (name, names, names32)
        sc = ref.abs().mean()
        e = ((big[:Kin].double() - ref).abs().max() / sc).item(); e32 = ((big32[:Kin].double() - ref).abs().max() / sc).item()
        e_rem = ((big[Kf:Kin].double() - ref[Kf:]).abs().max() / sc).item()
        print('{} {}: e = {:.3e} (rows beyond {}: {:.3e}), fp32 kernel {:.3e}'.format(case, name, e, Kf, e_rem, e32))
        assert e < 3e-5 and e < max(4 * max(e32, 2e-6), 8 * 2.0 ** -24 * M ** 0.5), (name, e, e32)
        assert e32 < 8 * 2.0 ** -24 * M ** 0.5, '{}: the fp32 kernel itself is {:.3e} off'.format(name, e32)      # (not only a yardstick)
        assert (big[Kin:] == 7.0).all(), name + ': rows beyond Kin were written'
        want_db = dY64.sum(0)
        assert ((db - want_db).abs() <= 2e-3 + 2e-4 * want_db.abs()).all(), name + ': db'
        if Kin % 128 <= 16:
            head, db_head, names_head = run(True, Kf, **kw)
            assert 'ptts_dense_wgrad_bf16x6' in names_head
            assert (head[Kf:] == 7.0).all()
            assert torch.equal(big[:Kf], head[:Kf]), '{}: rows below {} differ from the {}-row product in {} entries'.format(
                name, Kf, Kf, int((big[:Kf] != head[:Kf]).sum()))
            assert torch.equal(db, db_head), name + ': db differs from the product without the remainder'


@pytest.mark.parametrize('N', [65, 20])
def test_narrow_output_waves_that_only_stage(ops, N):
    """N < 256: the waves whose columns lie beyond N stage their share of A and meet the barriers, without weight loads and MFMAs.
    The library has no switch that turns this off, so the check is two-fold: every column against fp64 at the bound of
    test_dense_bf16x6_planes_and_products, and BIT-identity with the columns [0, N) of a 256-wide product whose first N weight columns
    are the same -- there every wave is live, and a column's arithmetic does not depend on its neighbours."""
    M, K = 1111, 256
    g = gen(93)
    A = torch.randn(M, K, generator=g, dtype=torch.float64).float()
    W = (torch.randn(K, 256, generator=g, dtype=torch.float64) / K ** 0.5).float()
    Ad = A.cuda()
    hw, fw, wide = _weight(W.cuda())
    hn, fn, narrow = _weight(W[:, :N].contiguous().cuda())
    y, names = _product(ops, True, Ad, narrow, M, N, K, 0, N, N, mode=ops.IN_LRELU, alpha=0.3)
    y32, _ = _product(ops, False, Ad, narrow, M, N, K, 0, N, N, mode=ops.IN_LRELU, alpha=0.3)
    full, names_full = _product(ops, True, Ad, wide, M, 256, K, 0, 256, 256, mode=ops.IN_LRELU, alpha=0.3)
    assert names.count('ptts_dense_bf16x6') == 1 and names_full.count('ptts_dense_bf16x6') == 1 and 'ptts_gemm' not in names + names_full, (names, names_full)
    ref64 = O.lrelu(A.double()) @ W[:, :N].double()
    sc = ref64.abs().mean()
    e_col = (y.double() - ref64).abs().max(0).values / sc
    e32 = ((y32.double() - ref64).abs().max() / sc).item()
    print('N = {}: worst column e = {:.3e}, fp32 kernel {:.3e}'.format(N, e_col.max().item(), e32))
    assert (e_col < 3e-5).all() and (e_col < max(4 * max(e32, 2e-6), 8 * 2.0 ** -24 * K ** 0.5)).all()
    assert torch.equal(y, full[:, :N]), 'columns differ from the 256-wide product in {} entries'.format(int((y != full[:, :N]).sum()))
