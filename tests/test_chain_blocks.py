"""csrc/conv2d_chain.hip, host side: the frequency blocks that carry a spectrum wider than one tile's 68 bins through the
chain kernels (ptts_conv2d_chain_blocks answers from the plan the launches use).  The library loads without a device.

A block computes min(68, F - origin) bins from its origin; at a cut (a block edge that is no image edge) the values within
2 L bins are wrong (a missing neighbour's error advances two bins per layer), so the bins a block OWNS -- the only ones stored
or summed -- must lie at least 2 L bins inside; origins and cuts are multiples of 8 bins (aligned 16-byte units in the maps; a
weight-gradient K step of two adjacent bin groups never straddles a cut)."""
import ctypes

import pytest

BLOCK = 68          # bins one tile holds
CAP = 64


@pytest.fixture(scope='module')
def lib():
    from percivaltts_amd import _hip
    return _hip.lib()


def _blocks(lib, F, L, cap=CAP):
    o, lo, hi = (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    n = lib.ptts_conv2d_chain_blocks(F, L, o, lo, hi, cap)
    return n, [(o[k], lo[k], hi[k]) for k in range(min(n, cap))]


@pytest.mark.parametrize('L', range(1, 9))
def test_plan_invariants(lib, L):
    for F in range(2, 133):
        n, blocks = _blocks(lib, F, L)
        assert n >= 1 and len(blocks) == n, (F, L)
        assert lib.ptts_conv2d_chain_supported(F, L, 1, 4, 5, 5) == 1, (F, L)
        assert (n == 1) == (F <= BLOCK), (F, L, n)
        # the owned ranges partition [0, F) in order
        assert blocks[0][1] == 0 and blocks[-1][2] == F, (F, L, blocks)
        for (o, lo, hi), nxt in zip(blocks, blocks[1:] + [None]):
            assert lo < hi, (F, L, blocks)
            if nxt is not None:
                assert hi == nxt[1], (F, L, blocks)
        for k, (o, lo, hi) in enumerate(blocks):
            width = min(BLOCK, F - o)
            assert o % 8 == 0 and 0 <= o < F, (F, L, blocks)
            assert o <= lo and hi <= o + width, (F, L, blocks)
            left_cut, right_cut = o > 0, o + width < F
            assert left_cut == (k > 0) and right_cut == (k < n - 1), (F, L, blocks)
            if left_cut:
                assert lo % 8 == 0 and lo - 2 * L >= o, (F, L, blocks)
            if right_cut:
                assert hi % 8 == 0 and hi + 2 * L <= o + width, (F, L, blocks)


def test_the_plans_the_design_names(lib):
    assert _blocks(lib, 65, 8) == (1, [(0, 0, 65)])
    assert _blocks(lib, 68, 8) == (1, [(0, 0, 68)])
    assert _blocks(lib, 69, 8) == (2, [(0, 0, 48), (32, 48, 69)])
    assert _blocks(lib, 100, 8) == (2, [(0, 0, 48), (32, 48, 100)])
    assert _blocks(lib, 129, 8) == (3, [(0, 0, 48), (32, 48, 80), (64, 80, 129)])
    assert _blocks(lib, 132, 8) == (3, [(0, 0, 48), (32, 48, 80), (64, 80, 132)])
    # a smaller stack owns more per block
    assert _blocks(lib, 132, 1)[0] == 3 and _blocks(lib, 124, 1)[0] == 2
    assert _blocks(lib, 129, 2) == (3, [(0, 0, 64), (56, 64, 120), (112, 120, 129)])


def test_supported_agrees_with_the_plan_and_unsupported_is_zero(lib):
    fmax = max(F for F in range(2, 5000) if lib.ptts_conv2d_chain_supported(F, 8, 1, 4, 5, 5))
    assert fmax >= 132
    for F in (0, 1, 2, 68, 69, 132, fmax, fmax + 1, fmax + 1000, 1 << 30, -5):
        for L in (0, 1, 8, 9):
            n, _ = _blocks(lib, F, L)
            assert (n > 0) == bool(lib.ptts_conv2d_chain_supported(F, L, 1, 4, 5, 5)), (F, L)
    assert _blocks(lib, fmax + 1, 8)[0] == 0 and _blocks(lib, fmax, 8)[0] >= 3
    assert _blocks(lib, 129, 9)[0] == 0 and _blocks(lib, 129, 0)[0] == 0
    # a short or absent result buffer: the count is returned all the same, nothing past `cap` is written
    o = (ctypes.c_int * 2)(-7, -7)
    assert lib.ptts_conv2d_chain_blocks(129, 8, o, None, None, 1) == 3 and (o[0], o[1]) == (0, -7)
    assert lib.ptts_conv2d_chain_blocks(129, 8, None, None, None, 0) == 3
    # other stacks than 4 filters of 5 x 5 have no chain kernel at any width
    assert lib.ptts_conv2d_chain_supported(129, 8, 1, 8, 5, 5) == 0 and lib.ptts_conv2d_chain_supported(129, 8, 1, 4, 3, 3) == 0
