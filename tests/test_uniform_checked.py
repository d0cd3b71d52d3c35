"""The two pair loops of the P1 uniform-order tile kernel (k_tile_uniform, pnl_tile2.h).  A pair of cells exists if both cells are real
and one of them has a DoF.  The kernel used to test that for every pair; now the two staging waves decide per tile whether all 128 cells
pass, and such a tile takes the pair loop without the test (counter uniformTilesUnchecked).  Every other tile -- padding behind the last
cell of the mesh, cells without a DoF -- keeps the loop with the test (uniformTilesChecked), and the option PNL_UNI_CHECKED sends every
tile through it.  The checked loop is the code tests/test_gpu_parity.py holds to the oracle, so the default run is compared with the run
under the option.

Both runs add the same terms; the cross blocks go through LDS atomics and the diagonal blocks through global float atomics whose order
differs from run to run, so the bound is the 1e-13 max|A| that tests/test_settled_lists.py uses for two summation orders of the same
terms, not bit equality.
"""
import numpy as np
import pytest

TOL_ORDER = 1e-13           # the same terms summed in another order (tests/test_settled_lists.py)
NOREF = 5
# target order of the disc cases.  With 0.5, the value of the other tests on disc(5), the plan has 2,418 uniform tiles of order 2 and none of
# order 3 (the band of order-3 pairs is narrower than a block); with 0.75 it has about 1,180 of order 2 and 240-250 of order 3 for each of
# the three exponents, so both the 3-point and the 6-point kernel run.
TARGET_ORDER = 0.75
# uniformSquare(n) has 2 (n-1)^2 cells; its two corner cells (bottom right, top left) have no DoF with PHYSICAL boundary conditions.
# n - 1 no multiple of 8 leaves padding behind the last cell of the last 64-cell block.  N_SQUARE is the smallest such n whose default
# run takes tiles through both loops (found by running n = 10, 11, ... on the GPU; smaller squares have no uniform tile without one of
# the corner blocks or the padded block, or no uniform tile at all).
N_SQUARE = 15

COUNTER_KEYS = ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'orders', 'singular', 'uniformTilePairs',
                'uniformTilePairsByOrder', 'workListLength')


class _options:
    """options through _lib.set_option, removed again on the way out"""

    def __init__(self, **kw):
        self.kw = {k: v for k, v in kw.items() if v is not None}

    def __enter__(self):
        from pynucleus_amd import _lib
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from pynucleus_amd import _lib
        for k in self.kw:
            _lib.set_option(k, None)


def _assemble(builder, **options):
    with _options(**options):
        A = builder.getDense()
        return A.toarray(), A.info['counters']


def _compare(builder, what):
    """default run against PNL_UNI_CHECKED: matrix, diagonal, statistics; returns the counters of both"""
    A1, cnt1 = _assemble(builder)
    A0, cnt0 = _assemble(builder, PNL_UNI_CHECKED=1)
    scale = np.abs(A0).max()
    err, derr = np.abs(A1-A0).max()/scale, np.abs(np.diag(A1)-np.diag(A0)).max()/scale
    print('%s: tiles unchecked %d checked %d (option: %d / %d), pairs by order %s, max|dA|/max|A| = %.3e, diagonal %.3e'
          % (what, cnt1['uniformTilesUnchecked'], cnt1['uniformTilesChecked'], cnt0['uniformTilesUnchecked'], cnt0['uniformTilesChecked'],
             cnt1['uniformTilePairsByOrder'], err, derr))
    for key in COUNTER_KEYS:
        assert cnt1[key] == cnt0[key], (key, cnt1[key], cnt0[key])
    assert cnt0['uniformTilesUnchecked'] == 0 and cnt0['uniformTilesChecked'] > 0
    assert cnt1['uniformTilesUnchecked']+cnt1['uniformTilesChecked'] == cnt0['uniformTilesChecked']
    assert err <= TOL_ORDER and derr <= TOL_ORDER, (what, err, derr)
    return cnt1, cnt0


@pytest.mark.gpu
@pytest.mark.parametrize('s', [0.5, 0.75, 0.4])
def test_gpu_checked_and_unchecked_loops_agree_on_the_disc(s):
    """disc(5), 6144 cells in 96 full blocks, every cell real and with a DoF: s = 1/2 (KT 2), 3/4 (KT 1, the exponent -7/4 known at
    compile time) and 0.4 (KT 0).  The default run takes no tile through the checked loop, the option every tile; orders 2 and 3 both
    have uniform tiles (the 3-point and the 6-point kernel)."""
    from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    b = nonlocalBuilder(P1_DoFMap(disc(NOREF), PHYSICAL), getFractionalKernel(2, s), {'target_order': TARGET_ORDER}, zeroExterior=True)
    cnt1, cnt0 = _compare(b, 'disc(%d), s = %g' % (NOREF, s))
    assert cnt1['uniformTilesChecked'] == 0 and cnt1['uniformTilesUnchecked'] > 0
    assert cnt1['uniformTilePairsByOrder'][2] > 0 and cnt1['uniformTilePairsByOrder'][3] > 0


@pytest.mark.gpu
def test_gpu_one_launch_takes_both_loops():
    """uniformSquare(N_SQUARE): the blocks of the two corner cells and the padded last block make checked tiles, the blocks between them
    unchecked ones, in the same launch of the kernel."""
    from pynucleus_amd import uniformSquare, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    assert (2*(N_SQUARE-1)**2) % 64 != 0
    b = nonlocalBuilder(P1_DoFMap(uniformSquare(N_SQUARE), PHYSICAL), getFractionalKernel(2, 0.5), {'target_order': 0.5}, zeroExterior=True)
    cnt1, cnt0 = _compare(b, 'uniformSquare(%d)' % N_SQUARE)
    assert cnt1['uniformTilesChecked'] > 0 and cnt1['uniformTilesUnchecked'] > 0
