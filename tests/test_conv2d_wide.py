"""csrc/conv2d_wide.hip, host side: which shapes the fp32 matrix-core Conv2D tier takes, and the size of its partial rows.
The library loads without a device."""
import pytest

F_REF = 65


@pytest.fixture(scope='module')
def lib():
    from percivaltts_amd import _hip
    return _hip.lib()


# Cin, Cout, KT, KF
TAKEN = [(8, 8, 5, 5), (1, 16, 3, 3), (16, 1, 7, 7), (4, 4, 5, 3), (12, 8, 7, 7)]
DECLINED = [
    (3, 5, 3, 3), (2, 2, 5, 3),                     # channel counts that are neither 1 nor a multiple of 4
    (4, 4, 5, 5), (1, 4, 5, 5), (2, 2, 3, 3),       # the 4 -> 4 5x5 matrix-core kernels and the packed-FMA stencil take these
    (20, 8, 5, 5),                                  # more than 16 channels
    (8, 8, 4, 4), (8, 8, 9, 9),                     # an even window, a window larger than 7
]


@pytest.mark.parametrize('shape', TAKEN)
def test_supported_shapes(lib, shape):
    Cin, Cout, KT, KF = shape
    for F in (F_REF, 129, 9, 2):
        assert lib.ptts_conv2d_wide_supported(F, Cin, Cout, KT, KF, 1) == 1, (F, shape)


@pytest.mark.parametrize('shape', DECLINED)
def test_declined_shapes(lib, shape):
    Cin, Cout, KT, KF = shape
    for dil in (1, 2):
        assert lib.ptts_conv2d_wide_supported(F_REF, Cin, Cout, KT, KF, dil) == 0, shape


def test_dilation_and_degenerate_arguments(lib):
    assert lib.ptts_conv2d_wide_supported(33, 8, 8, 5, 5, 2) == 1
    assert lib.ptts_conv2d_wide_supported(6, 8, 8, 5, 5, 8) == 1
    assert lib.ptts_conv2d_wide_supported(65, 8, 8, 5, 5, 0) == 0
    assert lib.ptts_conv2d_wide_supported(0, 8, 8, 5, 5, 1) == 0
    assert lib.ptts_conv2d_wide_supported(65, 16, 16, 7, 7, 100000) == 0        # no tile holds that halo


def test_switch_and_path_description():
    from percivaltts_amd import ops
    try:
        ops.conv2d_wide(True)
        assert 'conv2d_wide' in ops.conv2d_path_description((65, 8, 8, 5, 5))
        assert 'conv2d_wide' in ops.conv2d_path_description((65, 4, 4, 5, 3))
        assert 'generic' in ops.conv2d_path_description((65, 3, 5, 3, 3))
        assert 'stencil' in ops.conv2d_path_description((65, 1, 4, 5, 5))
        assert 'matrix-core implicit GEMM' in ops.conv2d_path_description()
        ops.conv2d_wide(False)
        assert 'generic' in ops.conv2d_path_description((65, 8, 8, 5, 5))
        assert 'wide / non-square layers: generic' in ops.conv2d_path_description()
    finally:
        ops.conv2d_wide(None)


# (Cin, Cout, KT, KF, dil_t) -> the word in its description with every switch on; a tier switched off hands its shapes down
TIERS = dict([(s + (1,), 'conv2d_wide') for s in TAKEN] + [(s + (1,), 'generic') for s in DECLINED] +
             [((4, 4, 5, 5, d), 'conv2d_mfma') for d in (1, 2, 8)] + [((4, 4, 5, 5, 3), 'stencil'), ((1, 4, 5, 5, 1), 'stencil'),
                                                                      ((2, 2, 3, 3, 1), 'stencil')])
DOWN = {'conv2d_mfma': 'stencil', 'conv2d_wide': 'generic'}


@pytest.mark.parametrize('mfma', [True, False])
@pytest.mark.parametrize('wide', [True, False])
def test_path_description_names_the_tier_of_the_shape_rule(mfma, wide):
    """One rule: what conv2d_path_description says of a shape is the tier _conv2d_shape_tier returns, for every switch setting;
    (4, 4, 5, 5) at dilation 3 is no matrix-core shape."""
    from percivaltts_amd import ops
    off = [t for t, on in (('conv2d_mfma', mfma), ('conv2d_wide', wide)) if not on]
    try:
        ops.conv2d_mfma(mfma)
        ops.conv2d_wide(wide)
        for (Cin, Cout, KT, KF, dil), word in TIERS.items():
            said = ops.conv2d_path_description((F_REF, Cin, Cout, KT, KF, dil))
            assert (DOWN[word] if word in off else word) in said, (Cin, Cout, KT, KF, dil, said)
            assert said == ops._conv2d_shape_tier(F_REF, Cin, Cout, KT, KF, dil), (Cin, Cout, KT, KF, dil)
            if dil == 1:
                assert said == ops.conv2d_path_description((F_REF, Cin, Cout, KT, KF))
    finally:
        ops.conv2d_mfma(None)
        ops.conv2d_wide(None)


@pytest.mark.parametrize('case', [(2, 12, 9, 8, 8, 5, 5, 1), (64, 400, 65, 16, 16, 5, 5, 1), (1, 37, 129, 8, 8, 5, 5, 1),
                                  (3, 100, 65, 1, 16, 3, 3, 1), (2, 50, 33, 12, 8, 7, 7, 2), (1, 1, 5, 8, 1, 5, 3, 1)])
def test_workspace_covers_the_partial_rows(lib, case):
    """The rows are [nblocks][npart] floats, npart = dw | dbias | dscale | dshift, at most 512 rows (256 in deterministic mode,
    one per persistent workgroup) and never more than there are tiles."""
    B, T, F, Cin, Cout, KT, KF, dil = case
    npart = KT * KF * Cin * Cout + Cout + 2 * Cin
    nbytes = lib.ptts_conv2d_wide_bwd_workspace_bytes(B, T, F, Cin, Cout, KT, KF, dil)
    assert nbytes > 0 and nbytes % (4 * npart) == 0
    nblocks = nbytes // (4 * npart)
    assert 1 <= nblocks <= 512
    assert nblocks <= B * T * F            # a tile holds at least one pixel
    if B * T >= 512 * 64:                  # (a tile is at most 64 rows tall)
        assert nblocks == 512


def test_workspace_of_an_unsupported_shape_is_empty(lib):
    assert lib.ptts_conv2d_wide_bwd_workspace_bytes(2, 10, 7, 3, 5, 3, 3, 1) == 0
    assert lib.ptts_conv2d_wide_bwd_workspace_bytes(2, 16, 65, 4, 4, 5, 5, 1) == 0
