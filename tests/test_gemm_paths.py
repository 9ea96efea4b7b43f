"""csrc/gemm.hip and csrc/thin.hip -- the fp32 products the bf16x6 split kernels decline -- on every kernel ptts_gemm,
ptts_gemm_wgrad_grouped and thin_gemm_dispatch can launch without an environment switch, against float64.

Every case states the path it is meant to reach (a PTTS_GEMM_PATH_* value) and asserts it with ptts_gemm_path, the host function
ptts_gemm itself chooses with: a moved threshold is a failed assert here, not coverage silently lost.  Every output lies inside a
larger buffer whose margins -- in front, behind, and the columns N..ldc of every row -- hold a sentinel that is compared after
every call; outputs start as NaN (or the values an accumulating call adds to).  Every output element is compared with the fp64
product of the fp32-rounded operands, the transform restated in fp64 with the LeakyReLU mask taken at the fp32 pre-activation.
The module runs with ops.dense_split(False) (the train_wgan_split_bf16 = False configuration) and plain tensors, so that
ops.gemm_raw reaches ptts_gemm whatever the shape; no PTTS_* switch is set.  Each check prints its worst error / bound ratio
(`pytest -s`, lines `gemm-ratio <path> <case> <ratio>`).

Path -> case that reaches it (ids of the parametrised tests; TA/TB = transA/transB; modes NONE, LRELU, affine + LRELU = "AFF",
MASKMUL = "MM")

  gemm_tall_kc_kernel<TB, MODE, MT, 16>  (transA = 0, 128 < N <= 256, M >= 2048, K <= 2048)
      <0,NONE,4>   tall-n256-k16-vec (one k-step, float4 epilogue, ragged last row block), tall-n256-k100-cmis (C at 4 mod 16 bytes:
                   element-wise epilogue at N = 256, output mask at a ragged row block, accumulate), tall-conv (implicit-convolution rows)
      <0,LRELU,4>  tall-n256-k18-lrelu-maskmis (K % 4 != 0; output mask at 4 mod 16), tall-n200-k17-aff (AFF, bias, N < 256)
      <0,MM,4>     tall-n129-k16-mm
      <1,NONE,4>   tall-tb-n256-k40-omask (float4 output mask), tall-tb-n256-k16-acc-ldc (ldc > N, accumulate)
      <1,LRELU,4>  tall-tb-n256-k17-lrelu-ldc, tall-tb-n200-k40-aff-acc
      <1,MM,4>     tall-tb-n129-k100-mm-omask
      <TB,MODE,5>, <TB,MODE,6>, <TB,MODE,7>: test_tall_rows_per_workgroup[16400], [16401], [20500], [24600] x TB 0, 1 x NONE, AFF, MM, K = 16
      MT = 8       not reachable without PTTS_TALL_MT: pick_tall_mt tries MT = 4 first and MT = 8 fills 256 CUs no better for any M
                   (rounds(8) >= rounds(4) / 2); test_tall_mt8_needs_the_switch enumerates M = 2048 .. 400 000.  Not tested.
  N split (256 < N <= 512, M >= 2048, K <= 2048, transA = 0): 256 columns on the tall kernel, then the rest
      rest <= 4 -> gemv         split-260-gemv-vec (TB 0, LRELU, bias), split-258-gemv-tb (TB 1, output mask, accumulate)
      rest in (4, 128] -> tile  split-300-tile-tb (TB 1, AFF, bias), split-356-dma (TB 0, K = 100: the LDS-DMA kernel)
      rest > 128 -> tall again  split-400-tall (TB 0, MM, output mask, accumulate), split-400-tall-tb (TB 1, bias)
  gemm_f32_mfma_kernel<TA, TB, 0, MODE>   tile-taX-tbY-MODE for all 4 x 4 (K = 33 < 64 keeps NONE off the DMA kernel; 2 x 2 tiles,
                   ragged in M, N and K; for TA = 1 the affine channel is the stored column m)
  gemm_f32_mfma_kernel<0, 0, 1, NONE> / <1, 0, 1, NONE> (implicit convolution, K < 64)   tile-conv-fwd, tile-conv-wgrad
  gemm_dma_kernel<0, 0>   dma-k64 (K = 4 BK exactly: the path switches on; dma-k63-tile is its neighbour on the register-staged
                   kernel), dma-k70-unaligned (K tail through stage_tail, lda and ldb odd: sources at 4-byte alignment, accumulate);
                   both have interior tiles (DMA body) and edge tiles (register-staged body on the same LDS) in one launch
  gemm_dma_kernel<1, 0>   dma-ta-colsum (colsum_b, lda odd)
  gemm_dma_kernel<0, 1>   dma-conv-fwd
  gemm_dma_kernel<1, 1>   dma-conv-wgrad (rows_per_seg = 50: a segment border inside a k-step; colsum_b)
  stream-K (K >= 2048, 9 or 4 tiles on 512 slots)
      gemm_dma_kernel       sk-dma-wgrad (TA 1, colsum_b, accumulate onto a non-zero C, ragged tiles and K), sk-dma-fwd (bias, NaN C
                            zero-filled by the call, ldc > N)
      gemm_f32_mfma_kernel  sk-tile-wgrad-aff (TA 1, AFF, bias, colsum_b), sk-tile-mm-omask (TB 1, MM, output mask)
      the same four under ops.deterministic(True): one workgroup per tile (PTTS_GEMM_PATH_DMA / _TILE), two runs bit-identical
  gemm_wgrad_grouped_kernel  test_grouped_weight_gradients[1], [3], [13] (13 > WG_MAX = 12: two launches): NONE / LRELU / AFF / MM
                   mixed, a product smaller than one tile beside a deep one (a workgroup's range crosses products), colsum_b
                   present and absent, non-zero initial C and colsum_b (both accumulate), lda / ldb / ldc beyond the widths
  thin.hip
      gemv_rows_kernel<1|2|4, VEC>     gemv-n1-vec-k16 (K = 16 threshold), gemv-n2-vec-k256-tb, gemv-n4-vec-mm, gemv-n3-vec-omask
      gemv_rows_kernel<1|2|4, scalar>  gemv-n1-k260 (K > 256), gemv-n2-k18 (K % 4), gemv-n4-lda (lda % 4), gemv-n1-amis (A at 4 mod 16),
                                       gemv-n3-k1023-tb-acc
      thresholds                       gemv-m255-tile, gemv-k15-tile (the register-staged tile kernel takes both)
      thin_k_kernel<1|2|4, VEC>        think-k1-vec (M N = 65536), think-k2-vec-omask-acc, think-k3-vec-tb, think-k4-vec-mm
      thin_k_kernel<1|2|4, scalar>     think-k1-n219 (N % 4), think-k2-ldc (ldc % 4), think-k4-cmis-aff (C at 4 mod 16)
      threshold                        think-65535-tile
      wcol_part4_kernel<1|2> + wcol_reduce_kernel<1|2>   wcol4-n1-k1024 (K = 1024 threshold), wcol4-n2-aff-acc
      wcol_part_kernel<1|2> + wcol_reduce_kernel<1|2>    wcol-n1-m255 (M % 4), wcol-n2-lda-mm (lda % 4), wcol-n1-amis
      threshold                        wcol-k1023-dma
      the wcol forms under deterministic mode: test_deterministic_mode_is_bitwise_repeatable (same kernels: they have no atomics)
      wcol_kernel (atomics)            needs a stream capture or M > 524 288 to be chosen: out of scope, not tested
  degenerate sizes               tiny-1x1x1, tiny-1x1x17, tiny-1x5x17-tb, tiny-3x1x1-ta, tiny-7x2x17-ta (all on the tile kernel)

Bounds.  MFMA kernels: tests/test_ops_gpu.py::test_gemm's, rtol 2e-4 and atol 2e-4 sqrt(K) for unit-variance operands, 4e-4 sqrt(K)
after an accumulate.  Thin kernels: test_gemm_thin_shapes', rtol 2e-4 with atol 2e-3 for the row products at its K = 256 (scaled by
sqrt(K / 256) here, the same sqrt(K) law), 1e-4 (2e-4 after an accumulate) for K <= 4, 5e-3 (1e-2 accumulating) for the weighted
column sums over its 3000 rows (scaled by sqrt(rows / 3000)).
"""
import collections
import ctypes
import math
import os

import pytest
import torch

ALPHA = 0.3
PAD = 64
SENTINEL = 12345.0
NONE, LRELU, MM = 0, 1, 2


def _lib():
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    return _hip.lib()


class _Paths(object):
    """PTTS_GEMM_PATH_* of include/percival_hip.h by name: P.TALL_MT4 ..."""
    def __getattr__(self, name):
        from percivaltts_amd import _hip
        v = _hip._define('PTTS_GEMM_PATH_' + name)
        setattr(self, name, v)
        return v

    def name(self, value):
        from percivaltts_amd import _hip
        for n in ('GEMV', 'GEMV_VEC', 'THIN_K', 'THIN_K_VEC', 'WCOL_PART', 'WCOL_PART4', 'WCOL_ATOMIC', 'NSPLIT', 'TALL_MT4', 'TALL_MT5',
                  'TALL_MT6', 'TALL_MT7', 'TALL_MT8', 'DMA', 'DMA_STREAMK', 'TILE', 'TILE_STREAMK'):
            if _hip._define('PTTS_GEMM_PATH_' + n) == value:
                return n
        return str(value)


P = _Paths()


# ---------------------------------------------------------------------------------------------------------------------------
# case description
# ---------------------------------------------------------------------------------------------------------------------------
_FIELDS = dict(M=None, N=None, K=None, ta=0, tb=0, mode=NONE, affine=False, bias=False, omask=False, acc=False, colsum=False,
               lda=None, ldb=None, ldc=None, conv=None, a_off=0, c_off=0, om_off=0, path=None, rest=None, seed=0)
Case = collections.namedtuple('Case', ['id'] + list(_FIELDS))


def case(id_, M, N, K, path, **kw):
    """conv = (T, seg_stride): implicit-convolution addressing, rows_per_seg = T (lda is then the channel count).
    rest: for an N split, the path of the columns beyond 256."""
    d = dict(_FIELDS, M=M, N=N, K=K, path=path)
    assert set(kw) <= set(_FIELDS), kw
    d.update(kw)
    return Case(id_, **d)


def dims(c):
    """(lda, rows_per_seg, seg_stride, ldb, ldc) as ops.gemm_raw defaults them."""
    lda = c.lda if c.lda is not None else (c.K if c.ta == 0 else c.M)
    rps, seg = (c.conv[0], c.conv[1]) if c.conv else ((c.M if c.ta == 0 else c.K), 0)
    ldb = c.ldb if c.ldb is not None else (c.N if c.tb == 0 else c.K)
    ldc = c.ldc if c.ldc is not None else c.N
    return lda, rps, seg, ldb, ldc


def a_index(c):
    """Element offset of A(m, k) in its storage, [M, K]: the addressing rule of include/percival_hip.h."""
    lda, rps, seg, _, _ = dims(c)
    m = torch.arange(c.M, dtype=torch.int64).view(-1, 1)
    k = torch.arange(c.K, dtype=torch.int64).view(1, -1)
    if c.ta == 0:
        return (m // rps) * seg + (m % rps) * lda + k
    return (k // rps) * seg + (k % rps) * lda + m


def r32(t):
    return t.to(torch.float32).to(torch.float64)


def randn32(g, *shape):
    return r32(torch.randn(*shape, generator=g, dtype=torch.float64))


Operands = collections.namedtuple('Operands', 'sa sm sb bias sc sh om c0 TA Bm')


def operands(c):
    """Host operands (fp64 values exactly representable in fp32) and the fp64 logical T(A) [M, K] and B [K, N]."""
    g = torch.Generator().manual_seed(4000 + c.seed + 7 * c.M + 13 * c.N + 17 * c.K)
    lda, rps, seg, ldb, ldc = dims(c)
    idx = a_index(c)
    sa = randn32(g, int(idx.max()) + 1)
    sm = randn32(g, sa.numel()) if c.mode == MM else None
    nchan = c.K if c.ta == 0 else c.M                       # the transform's channel is the stored column of A
    sc = r32(torch.rand(nchan, generator=g, dtype=torch.float64) + 0.5) if c.affine else None
    sh = randn32(g, nchan) * 0.3 if c.affine else None
    sh = r32(sh) if sh is not None else None
    sb = randn32(g, c.K, ldb) if c.tb == 0 else randn32(g, c.N, ldb)
    Bm = sb[:, :c.N] if c.tb == 0 else sb[:, :c.K].t()
    bias = randn32(g, c.N) if c.bias else None
    om = randn32(g, c.M, c.N) if c.omask else None
    c0 = randn32(g, c.M, c.N) if c.acc else None
    a = sa[idx]
    chan = (torch.arange(c.K).view(1, -1) if c.ta == 0 else torch.arange(c.M).view(-1, 1)).expand(c.M, c.K)
    if c.mode == LRELU:
        if c.affine:
            p = a * sc[chan] + sh[chan]
            p32 = a.to(torch.float32) * sc.to(torch.float32)[chan] + sh.to(torch.float32)[chan]     # one rounded product, one rounded sum
        else:
            p, p32 = a, a
        TA = torch.where(p32 > 0, p, ALPHA * p)
    elif c.mode == MM:
        TA = a * torch.where(sm[idx] > 0, 1.0, ALPHA)
    else:
        TA = a
    return Operands(sa, sm, sb, bias, sc, sh, om, c0, TA, Bm)


def reference(c, o, rows=None):
    """fp64 result [rows or M, N] and the elementwise bound."""
    TA = o.TA if rows is None else o.TA[rows]
    ref = TA @ o.Bm
    if o.bias is not None:
        ref = ref + o.bias
    if o.om is not None:
        ref = ref * torch.where((o.om if rows is None else o.om[rows]) > 0, 1.0, ALPHA)
    if o.c0 is not None:
        ref = ref + (o.c0 if rows is None else o.c0[rows])
    return ref


def bound_for(c, path, ref):
    gemv = path in (P.GEMV, P.GEMV_VEC)
    think = path in (P.THIN_K, P.THIN_K_VEC)
    wcol = path in (P.WCOL_PART, P.WCOL_PART4)
    if gemv:
        atol = 2e-3 * math.sqrt(c.K / 256.0) * (2 if c.acc else 1)
    elif think:
        atol = 2e-4 if c.acc else 1e-4
    elif wcol:
        atol = (1e-2 if c.acc else 5e-3) * math.sqrt(c.K / 3000.0)
    else:
        atol = (4e-4 if c.acc else 2e-4) * math.sqrt(c.K)
    return atol + 2e-4 * ref.abs()


def dev(t, off=0):
    """A contiguous float32 device copy whose first element lies `off` elements past a 512-byte boundary."""
    if t is None:
        return None
    t = t.detach().to(torch.float32)
    flat = torch.empty(t.numel() + off, dtype=torch.float32, device='cuda')
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


class OutBuf(object):
    """[M, N] with row stride ldc at `off` elements past a 256-byte boundary, inside a sentinel-filled buffer: the margins in
    front and behind AND the columns N..ldc of every row are compared by intact().  Starts as NaN, or as `init`."""
    def __init__(self, M, N, ldc, off=0, init=None):
        self.buf = torch.full((2 * PAD + off + M * ldc,), SENTINEL, dtype=torch.float32, device='cuda')
        self.t = self.buf.as_strided((M, N), (ldc, 1), PAD + off)
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        self.inside.as_strided((M, N), (ldc, 1), PAD + off).fill_(True)
        if init is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(init.to(torch.float32))
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    def intact(self, what):
        torch.cuda.synchronize()
        bad = (self.buf != SENTINEL) & ~self.inside
        assert not bool(bad.any()), '{}: {} elements written outside the output (first at buffer offset {}, the output starts at {})'.format(
            what, int(bad.sum()), int(torch.nonzero(bad)[0]), self.t.storage_offset())


def check(got, want, bound, what, key=''):
    got = got.detach().cpu().to(torch.float64).reshape(-1)
    want = want.reshape(-1)
    bound = bound.reshape(-1)
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), '{}: {} elements not finite (left unwritten?)'.format(what, int((~torch.isfinite(got)).sum()))
    err = (got - want).abs()
    ratio = err / bound
    i = int(torch.argmax(ratio))
    print('gemm-ratio {} {} {:.5f}'.format(key, what, float(ratio[i])))
    assert float(ratio[i]) <= 1.0, '{}: {} / {} off, worst err {:.3e} = {:.2f} x bound at {} (got {:.9e} want {:.9e})'.format(
        what, int((ratio > 1.0).sum()), err.numel(), float(err[i]), float(ratio[i]), i, float(got[i]), float(want[i]))


def query(lib, c, al16, N=None):
    lda, rps, seg, ldb, ldc = dims(c)
    return lib.ptts_gemm_path(c.M, c.N if N is None else N, c.K, c.ta, lda, rps, seg, c.tb, ldb, ldc, c.mode, int(c.acc), int(c.bias),
                              int(c.omask), int(c.colsum), int(al16))


def launch(ops, c, o, rows=None):
    """One ops.gemm_raw call of case c on fresh device buffers; asserts the path, the margins, and the values.  Returns (C, colsum)."""
    lib = ops._hip.lib()
    lda, rps, seg, ldb, ldc = dims(c)
    A, msk = dev(o.sa, c.a_off), dev(o.sm, c.a_off)
    Bd, bias, sc, sh = dev(o.sb), dev(o.bias), dev(o.sc), dev(o.sh)
    C = OutBuf(c.M, c.N, ldc, c.c_off, o.c0)
    om = OutBuf(c.M, c.N, ldc, c.om_off, o.om) if c.omask else None
    cs = OutBuf(1, c.N, c.N, 0, torch.full((1, c.N), 5.0)) if c.colsum else None
    al16 = all(t is None or t.data_ptr() % 16 == 0 for t in (A, msk, C.t, om.t if om else None))
    got_path = query(lib, c, al16)
    assert got_path == c.path, '{}: meant for {} but ptts_gemm takes {}'.format(c.id, P.name(c.path), P.name(got_path))
    if c.path == P.NSPLIT:
        assert query(lib, c, al16, N=256) == P.TALL_MT4
        got_rest = query(lib, c, al16, N=c.N - 256)
        assert got_rest == c.rest, '{}: columns beyond 256 meant for {} but take {}'.format(c.id, P.name(c.rest), P.name(got_rest))
    with ops._hip.KernelTimer() as kt:
        ops.gemm_raw(A, Bd, C.t, c.M, c.N, c.K, transA=c.ta, lda=lda, rows_per_seg=rps, seg_stride=seg, transB=c.tb, ldb=ldb, ldc=ldc,
                     bias=bias, mode=c.mode, scale=sc, shift=sh, mask_src=msk, alpha=ALPHA, accumulate=int(c.acc),
                     out_mask=om.t if om else None, colsum_b=cs.t.view(-1) if cs else None)
    assert [r[0] for r in kt.records] == ['ptts_gemm'], kt.records
    C.intact(c.id + ' C')
    if cs:
        cs.intact(c.id + ' colsum_b')
    ref = reference(c, o, rows)
    key = P.name(c.path) + ('+' + P.name(c.rest) if c.path == P.NSPLIT else '')
    got = C.t if rows is None else C.t[rows.cuda()]
    check(got, ref, _split_bound(c, ref) if c.path == P.NSPLIT else bound_for(c, c.path, ref), c.id, key)
    if cs:
        want = o.Bm.sum(0)                      # overwritten, not added to
        check(cs.t, want, 2e-4 * math.sqrt(c.K) + 2e-4 * want.abs(), c.id + ' colsum_b', key)
    return C, cs


def _split_bound(c, ref):
    """N split: the first 256 columns at the MFMA bound, the rest at the bound of the kernel that takes them."""
    b = bound_for(c, P.TALL_MT4, ref)
    b[:, 256:] = bound_for(c, c.rest, ref)[:, 256:]
    return b


@pytest.fixture(scope='module')
def ops():
    from percivaltts_amd import ops as _ops
    _ops.dense_split(False)          # every product on the fp32 kernels of gemm.hip / thin.hip
    try:
        yield _ops
    finally:
        _ops.dense_split(None)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _tall_cases():
    T4 = P.TALL_MT4
    return [
        case('tall-n256-k16-vec', 2049, 256, 16, T4, bias=True),
        case('tall-n256-k100-cmis', 2049, 256, 100, T4, omask=True, acc=True, c_off=1),
        case('tall-conv', 2100, 200, 18, T4, bias=True, lda=6, conv=(420, (420 + 2) * 6)),
        case('tall-n256-k18-lrelu-maskmis', 2100, 256, 18, T4, mode=LRELU, omask=True, om_off=1),
        case('tall-n200-k17-aff', 2100, 200, 17, T4, mode=LRELU, affine=True, bias=True),
        case('tall-n129-k16-mm', 2049, 129, 16, T4, mode=MM),
        case('tall-tb-n256-k40-omask', 2100, 256, 40, T4, tb=1, omask=True),
        case('tall-tb-n256-k16-acc-ldc', 2049, 256, 16, T4, tb=1, acc=True, ldc=260),
        case('tall-tb-n256-k17-lrelu-ldc', 2100, 256, 17, T4, tb=1, mode=LRELU, bias=True, ldc=260),
        case('tall-tb-n200-k40-aff-acc', 2049, 200, 40, T4, tb=1, mode=LRELU, affine=True, acc=True, ldb=41),
        case('tall-tb-n129-k100-mm-omask', 2100, 129, 100, T4, tb=1, mode=MM, omask=True, ldc=131),
    ]


def _split_cases():
    S = P.NSPLIT
    return [
        case('split-260-gemv-vec', 2049, 260, 40, S, rest=P.GEMV_VEC, mode=LRELU, bias=True),
        case('split-258-gemv-tb', 2100, 258, 17, S, rest=P.GEMV, tb=1, omask=True, acc=True),
        case('split-300-tile-tb', 2049, 300, 40, S, rest=P.TILE, tb=1, mode=LRELU, affine=True, bias=True),
        case('split-356-dma', 2100, 356, 100, S, rest=P.DMA),
        case('split-400-tall', 2049, 400, 17, S, rest=P.TALL_MT4, mode=MM, omask=True, acc=True),
        case('split-400-tall-tb', 2100, 400, 40, S, rest=P.TALL_MT4, tb=1, bias=True, ldc=404),
    ]


def _tile_cases():
    out = []
    for ta in (0, 1):
        for tb in (0, 1):
            for name, kw in (('none', dict(bias=True)), ('lrelu', dict(mode=LRELU, acc=True)),
                             ('aff', dict(mode=LRELU, affine=True, bias=True)), ('mm', dict(mode=MM, omask=True))):
                out.append(case('tile-ta{}-tb{}-{}'.format(ta, tb, name), 150, 140, 33, P.TILE, ta=ta, tb=tb, ldc=143, **kw))
    out.append(case('tile-conv-fwd', 200, 70, 18, P.TILE, lda=6, conv=(100, 102 * 6), bias=True))
    out.append(case('tile-conv-wgrad', 18, 70, 40, P.TILE, ta=1, lda=6, conv=(20, 22 * 6), colsum=True))
    return out


def _dma_cases():
    return [
        case('dma-k64', 260, 260, 64, P.DMA, bias=True),
        case('dma-k63-tile', 260, 260, 63, P.TILE, bias=True),
        case('dma-k70-unaligned', 260, 260, 70, P.DMA, lda=71, ldb=261, acc=True, ldc=263),
        case('dma-ta-colsum', 200, 130, 100, P.DMA, ta=1, lda=201, colsum=True),
        case('dma-conv-fwd', 150, 130, 80, P.DMA, lda=16, conv=(50, 54 * 16), bias=True),
        case('dma-conv-wgrad', 200, 130, 150, P.DMA, ta=1, lda=40, conv=(50, 54 * 40), colsum=True),
    ]


def _streamk_cases(det=False):
    D, T = (P.DMA, P.TILE) if det else (P.DMA_STREAMK, P.TILE_STREAMK)
    return [
        case('sk-dma-wgrad', 260, 260, 2100, D, ta=1, colsum=True, acc=True),
        case('sk-dma-fwd', 200, 130, 2049, D, bias=True, ldc=133),
        case('sk-tile-wgrad-aff', 260, 130, 2100, T, ta=1, mode=LRELU, affine=True, bias=True, colsum=True),
        case('sk-tile-mm-omask', 200, 130, 2049, T, tb=1, mode=MM, omask=True),
    ]


def _thin_cases():
    return [
        case('gemv-n1-vec-k16', 256, 1, 16, P.GEMV_VEC, bias=True),
        case('gemv-n2-vec-k256-tb', 300, 2, 256, P.GEMV_VEC, tb=1, mode=LRELU, affine=True, bias=True),
        case('gemv-n4-vec-mm', 1031, 4, 64, P.GEMV_VEC, mode=MM, ldc=5),
        case('gemv-n3-vec-omask', 257, 3, 100, P.GEMV_VEC, omask=True, acc=True, ldc=7),
        case('gemv-n1-k260', 300, 1, 260, P.GEMV, mode=LRELU),
        case('gemv-n2-k18', 300, 2, 18, P.GEMV, bias=True),
        case('gemv-n4-lda', 300, 4, 64, P.GEMV, lda=65, mode=MM),
        case('gemv-n1-amis', 300, 1, 64, P.GEMV, a_off=1, mode=LRELU, affine=True),
        case('gemv-n3-k1023-tb-acc', 9000, 3, 1023, P.GEMV, tb=1, acc=True),
        case('gemv-m255-tile', 255, 1, 16, P.TILE, bias=True),
        case('gemv-k15-tile', 256, 1, 15, P.TILE, bias=True),
        case('think-k1-vec', 256, 256, 1, P.THIN_K_VEC, bias=True),
        case('think-k2-vec-omask-acc', 300, 220, 2, P.THIN_K_VEC, omask=True, acc=True, ldc=224),
        case('think-k3-vec-tb', 300, 220, 3, P.THIN_K_VEC, tb=1, mode=LRELU),
        case('think-k4-vec-mm', 300, 220, 4, P.THIN_K_VEC, mode=MM),
        case('think-k1-n219', 300, 219, 1, P.THIN_K, tb=1, bias=True),
        case('think-k2-ldc', 256, 256, 2, P.THIN_K, ldc=257, omask=True),
        case('think-k4-cmis-aff', 300, 220, 4, P.THIN_K, c_off=1, mode=LRELU, affine=True, acc=True),
        case('think-65535-tile', 257, 255, 2, P.TILE, bias=True),
        case('wcol4-n1-k1024', 256, 1, 1024, P.WCOL_PART4, ta=1, mode=LRELU),
        case('wcol4-n2-aff-acc', 260, 2, 1500, P.WCOL_PART4, ta=1, mode=LRELU, affine=True, acc=True, ldc=3),
        case('wcol-n1-m255', 255, 1, 1100, P.WCOL_PART, ta=1),
        case('wcol-n2-lda-mm', 256, 2, 1100, P.WCOL_PART, ta=1, lda=257, mode=MM),
        case('wcol-n1-amis', 64, 1, 1024, P.WCOL_PART, ta=1, a_off=1, acc=True),
        case('wcol-k1023-dma', 256, 1, 1023, P.DMA, ta=1),
        case('tiny-1x1x1', 1, 1, 1, P.TILE, bias=True),
        case('tiny-1x1x17', 1, 1, 17, P.TILE, mode=LRELU, affine=True),
        case('tiny-1x5x17-tb', 1, 5, 17, P.TILE, tb=1, acc=True),
        case('tiny-3x1x1-ta', 3, 1, 1, P.TILE, ta=1),
        case('tiny-7x2x17-ta', 7, 2, 17, P.TILE, ta=1, tb=1, mode=MM),
    ]


def _lazy(maker):
    """The cases name PTTS_GEMM_PATH_* values read from the header: built at collection time, ids included."""
    cases = maker()
    return dict(argnames='c', argvalues=cases, ids=[c.id for c in cases])


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the path function itself
# ---------------------------------------------------------------------------------------------------------------------------
def _path(lib, M, N, K, ta=0, tb=0, lda=None, ldb=None, ldc=None, rps=None, seg=0, mode=0, bias=0, om=0, cs=0, al=1):
    lda = lda or (K if ta == 0 else M)
    ldb = ldb or (N if tb == 0 else K)
    return lib.ptts_gemm_path(M, N, K, ta, lda, rps or (M if ta == 0 else K), seg, tb, ldb, ldc or N, mode, 0, bias, om, cs, al)


def test_tall_mt8_needs_the_switch():
    """pick_tall_mt by hand -- 16 384 rows fill 256 workgroups of 64 rows, one more row needs 80 rows each, and so on -- and by
    enumeration: no M chooses MT = 8 (MT = 4 is tried first and MT = 8 never fills the CUs better)."""
    lib = _lib()
    for M, want in ((2048, P.TALL_MT4), (16384, P.TALL_MT4), (16385, P.TALL_MT5), (16400, P.TALL_MT5), (16401, P.TALL_MT5), (20480, P.TALL_MT5),
                    (20500, P.TALL_MT6), (24576, P.TALL_MT6), (24600, P.TALL_MT7), (25600, P.TALL_MT7), (28672, P.TALL_MT7)):
        assert _path(lib, M, 256, 16) == want, M
    seen = set(_path(lib, M, 256, 16) for M in list(range(2048, 70000)) + list(range(70000, 400000, 7)))
    assert seen == {P.TALL_MT4, P.TALL_MT5, P.TALL_MT6, P.TALL_MT7}


def test_path_thresholds():
    """Every threshold of ptts_gemm's choice, from both sides, without a device."""
    lib = _lib()
    p = lambda *a, **k: _path(lib, *a, **k)
    # tall: M >= 2048, 128 < N <= 256, K <= 2048, transA = 0 (before the DMA test: an implicit convolution goes there too)
    assert p(2047, 256, 64) == P.DMA and p(2048, 256, 64) == P.TALL_MT4
    assert p(2048, 128, 64) == P.DMA and p(2048, 129, 64) == P.TALL_MT4
    assert p(2048, 256, 2048) == P.TALL_MT4 and p(2048, 256, 2049) == P.DMA_STREAMK
    assert p(2048, 256, 64, ta=1) == P.DMA and p(2048, 256, 64, tb=1) == P.TALL_MT4
    assert p(2100, 200, 18, lda=6, rps=420, seg=422 * 6) == P.TALL_MT4
    # N split
    assert p(2048, 257, 64) == P.NSPLIT and p(2048, 512, 64) == P.NSPLIT and p(2048, 513, 64) == P.DMA
    assert p(2047, 257, 64) == P.DMA and p(2048, 257, 2049) == P.DMA_STREAMK and p(2048, 257, 64, ta=1) == P.DMA
    # DMA: no transform, B stored [k][n], no output mask, K >= 64
    assert p(300, 300, 63) == P.TILE and p(300, 300, 64) == P.DMA
    assert p(300, 300, 64, mode=LRELU) == P.TILE and p(300, 300, 64, tb=1) == P.TILE and p(300, 300, 64, om=1) == P.TILE
    # stream-K: 128 k-steps, uneven slots
    assert p(260, 260, 2032) == P.DMA and p(260, 260, 2033) == P.DMA_STREAMK
    assert p(260, 260, 2100, tb=1) == P.TILE_STREAMK
    assert p(128 * 23, 128 * 20, 2100) == P.DMA_STREAMK and p(128 * 23, 128 * 21, 2100) == P.DMA       # 460 / 483 of 512 slots
    # thin kernels
    assert p(256, 4, 16) == P.GEMV_VEC and p(255, 4, 16) == P.TILE and p(256, 5, 16) == P.TILE and p(256, 4, 15) == P.TILE
    assert p(256, 4, 256) == P.GEMV_VEC and p(256, 4, 260) == P.GEMV and p(256, 4, 18) == P.GEMV
    assert p(256, 4, 64, lda=65) == P.GEMV and p(256, 4, 64, al=0) == P.GEMV and p(256, 4, 64, ta=1) == P.DMA
    assert p(256, 256, 4) == P.THIN_K_VEC and p(256, 256, 5) == P.TILE and p(257, 255, 4) == P.TILE
    assert p(300, 219, 4) == P.THIN_K and p(256, 256, 4, ldc=257) == P.THIN_K and p(256, 256, 4, al=0) == P.THIN_K
    assert p(256, 2, 1024, ta=1) == P.WCOL_PART4 and p(256, 3, 1024, ta=1) == P.DMA and p(256, 2, 1023, ta=1) == P.DMA
    assert p(255, 2, 1024, ta=1) == P.WCOL_PART and p(256, 2, 1024, ta=1, lda=257) == P.WCOL_PART and p(256, 2, 1024, ta=1, al=0) == P.WCOL_PART
    assert p(256, 2, 1024, ta=1, tb=1) == P.TILE and p(256, 2, 1024, ta=1, bias=1) == P.DMA
    assert p(256, 2, 1024, ta=1, cs=1) == P.DMA            # a fused bias gradient: never thin
    assert p(1 << 20, 2, 1024, ta=1) == P.WCOL_ATOMIC      # partial rows beyond the 4 MB buffer
    # deterministic mode: no stream-K, no atomics
    was = lib.ptts_set_deterministic(1)
    try:
        assert p(260, 260, 2100) == P.DMA and p(260, 260, 2100, tb=1) == P.TILE
        assert p(256, 2, 1024, ta=1) == P.WCOL_PART4 and p(1 << 20, 2, 1024, ta=1) == P.DMA
    finally:
        lib.ptts_set_deterministic(was)
    # arguments ptts_gemm refuses
    for bad in (dict(M=0), dict(K=0), dict(ldc=3, N=4), dict(mode=3), dict(bias=1, om=1), dict(cs=1)):
        kw = dict(M=8, N=4, K=8)
        kw.update(bad)
        M, N, K = kw.pop('M'), kw.pop('N'), kw.pop('K')
        assert p(M, N, K, **kw) == -1, bad


def test_header_table_names_every_case():
    """The docstring's table and the case lists do not drift apart."""
    ids = [c.id for maker in (_tall_cases, _split_cases, _tile_cases, _dma_cases, _streamk_cases, _thin_cases) for c in maker()]
    assert len(ids) == len(set(ids))
    for i in ids:
        if i.startswith('tile-ta'):
            continue                    # named by their pattern
        assert i in __doc__, i


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_tall_cases))
def test_tall_kernel(ops, c):
    launch(ops, c, operands(c))


@pytest.mark.gpu
@pytest.mark.parametrize('M', [16400, 16401, 20500, 24600])
def test_tall_rows_per_workgroup(ops, M):
    """MT = 5, 6, 7 (80, 96, 112 rows per workgroup) x transB x transform at K = 16: a strided sample of rows plus both ends of every
    row block and the last rows; the margins of the whole output.  16 400 = 205 x 80 has no ragged row block (every load unchecked),
    16 401 adds one of a single row."""
    mt = {16400: 5, 16401: 5, 20500: 6, 24600: 7}[M]
    path = P.TALL_MT4 + mt - 4
    step = 16 * mt
    rows = sorted(set(list(range(0, M, 37)) + list(range(0, M, step)) + list(range(step - 1, M, step)) + list(range(M - 20, M))))
    rows = torch.tensor(rows, dtype=torch.int64)
    for tb in (0, 1):
        for name, kw in (('none', dict(bias=True)), ('aff', dict(mode=LRELU, affine=True, acc=True)), ('mm', dict(mode=MM, omask=True))):
            c = case('tall-mt{}-tb{}-{}'.format(mt, tb, name), M, 256, 16, path, tb=tb, **kw)
            launch(ops, c, operands(c), rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_split_cases))
def test_column_split(ops, c):
    launch(ops, c, operands(c))


@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_tile_cases))
def test_register_staged_kernel(ops, c):
    launch(ops, c, operands(c))


@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_dma_cases))
def test_dma_kernel(ops, c):
    launch(ops, c, operands(c))


@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_streamk_cases))
def test_stream_k(ops, c):
    assert not ops.deterministic()
    launch(ops, c, operands(c))


@pytest.mark.gpu
@pytest.mark.parametrize(**_lazy(_thin_cases))
def test_thin_kernels_and_degenerate_sizes(ops, c):
    launch(ops, c, operands(c))


@pytest.mark.gpu
def test_deterministic_mode_is_bitwise_repeatable(ops):
    """ops.deterministic(True): the stream-K shapes run one workgroup per tile with plain stores, the weighted column sums keep their
    two-stage form; values at the same bounds, and two runs on fresh buffers agree bit for bit (C and colsum_b)."""
    was = ops.deterministic()
    ops.deterministic(True)
    try:
        wcol = [c for c in _thin_cases() if c.path in (P.WCOL_PART, P.WCOL_PART4)]
        for c in _streamk_cases(det=True) + wcol:
            c = c._replace(id=c.id + '-det')
            o = operands(c)
            first, again = launch(ops, c, o), launch(ops, c, o)
            assert torch.equal(first[0].buf, again[0].buf), c.id + ': C differs between two runs'
            if c.colsum:
                assert torch.equal(first[1].buf, again[1].buf), c.id + ': colsum_b differs between two runs'
    finally:
        ops.deterministic(was)


# the products of the grouped launches: (Kin, N, rows, mode, affine, with bias gradient, lda - Kin, ldb - N, ldc - N)
_GROUPED = [
    (256, 256, 700, NONE, False, True, 0, 0, 0),          # deep: 4 tiles x 44 k-steps
    (20, 10, 8, LRELU, False, False, 1, 2, 3),            # smaller than one tile, one k-step: a workgroup's range crosses it
    (130, 70, 33, LRELU, True, True, 3, 0, 1),            # ragged tiles, ragged K, affine on the stored column
    (260, 129, 100, MM, False, True, 0, 3, 0),            # 3 x 2 tiles
    (5, 300, 17, NONE, False, False, 0, 0, 0),
    (64, 1, 50, LRELU, True, True, 0, 0, 0),              # (the grouped launch has no thin path: a 1-wide product is a tile)
]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3, 13])
def test_grouped_weight_gradients(ops, n):
    """ptts_gemm_wgrad_grouped called as ops._launch_wgrads calls it: n products C_i += T(A_i)^T . dY_i and colsum_b_i += column sums
    of dY_i in one call (13 products: two launches), each onto a non-zero C and bias gradient inside sentinel margins."""
    _hip = ops._hip
    g = torch.Generator().manual_seed(900 + n)
    descs = (_hip.WGradDesc * n)()
    keep, checks = [], []
    for i in range(n):
        Kin, N, rows, mode, affine, with_db, dla, dlb, dlc = _GROUPED[i % len(_GROUPED)]
        lda, ldb, ldc = Kin + dla, N + dlb, N + dlc
        c = case('grouped{}-{}'.format(n, i), Kin, N, rows, P.TILE, ta=1, mode=mode, affine=affine, acc=True, lda=lda, ldb=ldb, ldc=ldc, seed=i)
        o = operands(c)
        A, msk, Bd, sc, sh = dev(o.sa), dev(o.sm), dev(o.sb), dev(o.sc), dev(o.sh)
        C = OutBuf(Kin, N, ldc, 0, o.c0)
        db0 = randn32(g, 1, N)
        db = OutBuf(1, N, N, 0, db0) if with_db else None
        d = descs[i]
        d.A, d.B, d.C, d.colsum_b = A.data_ptr(), Bd.data_ptr(), C.t.data_ptr(), (db.t.data_ptr() if db else None)
        d.in_scale, d.in_shift = (sc.data_ptr() if affine else None), (sh.data_ptr() if affine else None)
        d.mask_src = msk.data_ptr() if msk is not None else None
        d.M, d.N, d.K = Kin, N, rows
        d.lda, d.ldb, d.ldc = lda, ldb, ldc
        d.in_mode, d.alpha = mode, ALPHA
        keep.append((A, msk, Bd, sc, sh))
        checks.append((c, o, C, db, db0))
    _hip.call('ptts_gemm_wgrad_grouped', ctypes.cast(descs, ctypes.c_void_p), n, _hip.stream())
    for c, o, C, db, db0 in checks:
        C.intact(c.id + ' C')
        ref = reference(c, o)
        check(C.t, ref, bound_for(c, P.TILE, ref), c.id, 'GROUPED')
        if db:
            db.intact(c.id + ' colsum_b')
            want = o.Bm.sum(0) + db0.view(-1)
            check(db.t, want, 4e-4 * math.sqrt(c.K) + 2e-4 * want.abs(), c.id + ' colsum_b', 'GROUPED')
