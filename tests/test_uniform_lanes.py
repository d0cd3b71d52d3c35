"""Lane layout of the 64-cell blocks for the P1 uniform-order tile kernels (k_tile_uniform, pnl_tile2.h; the host search is
uni_lane_layout in pnl_setup.hip, reached through pnl_uniform_lane_layout without a device).

A pair-wave issues nine ds_add_f64 into the LDS sub-block of its tile.  The LDS serves the instruction in four groups of 16 contiguous
lanes over 16 double-banks (tools/probes/lds_atomic_probe.hip: distinct banks inside every group cost 8.1 cycles whatever the other
groups hold, n lanes of a group on one bank n times that, and the groups add up).  With the lanes on the cells of the column block and a
row stride that is a multiple of 16 doubles the bank of an add is the LDS column of the lane's DoF mod 16, so the host places cells in
lanes and DoFs in columns such that the 16 lanes of a group hold different residues.  The option PNL_UNI_LANES selects the layout:
1 searched (default), 0 identity with the former stride (1 mod 32: bank = row + column), 2 random.

CPU: properties of the tables and the modelled cost, computed here from the tables (not the library's own figure).  GPU: the three
settings give the same operator -- the adds are atomics, the layout only decides speed -- to the 1e-13 max|A| that
tests/test_settled_lists.py uses for two summation orders of the same terms, with equal counters.
"""
import numpy as np
import pytest

TOL_ORDER = 1e-13           # the same terms summed in another order (tests/test_settled_lists.py)
TARGET_ORDER = 0.75         # disc(5): uniform tiles of order 2 and of order 3 (tests/test_uniform_checked.py)
N_SQUARE = 15               # cells without a DoF, padding behind the last cell (tests/test_uniform_checked.py)
MEAN_BOUND = 2.0            # mean modelled multiplier over the blocks of disc(5)

COUNTER_KEYS = ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'orders', 'singular', 'uniformTilePairs',
                'uniformTilePairsByOrder', 'workListLength', 'uniformTilesUnchecked', 'uniformTilesChecked')

LAYERS = (np.array([-1., -0.3, 0.3, 1.]), np.array([[0.3, 0.4, 0.5], [0.4, 0.5, 0.6], [0.5, 0.6, 0.7]]))


def _mesh_case(name):
    from pynucleus_amd import disc, uniformSquare, P1_DoFMap, PHYSICAL
    if name == 'disc4':
        return P1_DoFMap(disc(4), PHYSICAL)
    if name == 'disc5':
        return P1_DoFMap(disc(5), PHYSICAL)
    if name == 'square':
        return P1_DoFMap(uniformSquare(N_SQUARE), PHYSICAL)
    from pynucleus_amd.builder import label_blocks
    from pynucleus_amd.fractionalOrders import layersFractionalOrder
    dm = P1_DoFMap(disc(4), PHYSICAL)
    dmb = label_blocks(dm, layersFractionalOrder(2, *LAYERS).labels(dm.mesh.getCellCenters()))
    assert dmb is not dm and dmb.cell_is_padding.any()
    return dmb


def _block_slots(dofs, nblocks):
    """slot of every (cell, local vertex) in the sorted unique DoFs of its block, -1 where there is none; padded to 64 cells"""
    nc = dofs.shape[0]
    slots = -np.ones((nblocks*64, 3), dtype=np.int64)
    ndof = np.zeros(nblocks, dtype=np.int64)
    for b in range(nblocks):
        d = dofs[b*64:min(nc, (b+1)*64)]
        u = np.unique(d[d >= 0])
        ndof[b] = u.shape[0]
        s = np.searchsorted(u, np.where(d >= 0, d, 0))
        slots[b*64:b*64+d.shape[0]] = np.where(d >= 0, s, -1)
    return slots, ndof


def _multiplier(rows, cols, stride):
    """modelled LDS cycles of the sub-block adds of the tile (block, block) over the conflict-free ones.  rows [64, 3]: sub-block row of
    (lane position, local vertex) of the travelling cells, cols [64, 3]: column of the lanes' cells.  Lane l meets the travelling cell
    at position (l + step) mod 64; per (step, row vertex, column vertex) and 16-lane group the cost is the largest number of lanes on
    one double-bank, bank = (row stride + column) mod 16.  Lanes on the same address count like lanes on different ones (measured: more)."""
    lanes = np.arange(64)
    steps = np.arange(64 if stride % 16 else 1)              # stride = 0 mod 16: the bank does not depend on the travelling cell
    trav = (lanes[None, :]+steps[:, None]) % 64              # [step, lane]
    bank = (rows[trav][:, :, :, None]*stride+cols[None, :, None, :]) % 16          # [step, lane, row vertex, column vertex]
    onehot = bank.reshape(steps.shape[0], 4, 16, 9)[..., None] == np.arange(16)    # [step, group, lane of the group, add, bank]
    return float(onehot.sum(axis=2).max(axis=-1).mean())


@pytest.mark.parametrize('case', ['disc4', 'disc5', 'square', 'label_blocks'])
def test_lane_tables(case):
    """every block: lane_cell a permutation, lds_col injective below the stride, vertex orders permutations, cell_col consistent with
    lds_col (trash columns in the last 16 of the stride), the modelled multiplier no larger than that of the identity layout of the
    same block; disc(5): the mean over the blocks is at most MEAN_BOUND.  Two calls, and 1 host thread against 8, give the same tables."""
    from pynucleus_amd import _lib
    dm = _mesh_case(case)
    cells, dofs = np.asarray(dm.mesh.cells), np.asarray(dm.dofs)
    nc = cells.shape[0]
    T1 = _lib.uniform_lane_layout(cells, dofs, 1, 1)
    T8 = _lib.uniform_lane_layout(cells, dofs, 1, 8)
    T1b = _lib.uniform_lane_layout(cells, dofs, 1, 1)
    T0 = _lib.uniform_lane_layout(cells, dofs, 0, 0)
    T2 = _lib.uniform_lane_layout(cells, dofs, 2, 0)
    for key in ('lane_cell', 'lds_col', 'vorder', 'cell_col'):
        assert np.array_equal(T1[key], T8[key]) and np.array_equal(T1[key], T1b[key]), key
    nblocks, nU = T1['lane_cell'].shape[0], T1['nU']
    assert nblocks == (nc+63)//64 and T1['stride'] % 16 == 0 and T1['stride'] >= nU+16 and T0['stride'] == 0
    nUe = (nU+1) & ~1
    stride0 = nUe+1
    while stride0 % 32 != 1:
        stride0 += 1
    assert all(sorted(v) == [0, 1, 2] for v in T1['vorder'].tolist())
    assert np.array_equal(T1['vorder'], T0['vorder']) and np.array_equal(T1['vorder'], T2['vorder'])
    # slots in the vertex order of the tables
    dofs_t = np.take_along_axis(dofs, T1['vorder'].astype(np.int64), axis=1)
    slots, ndof = _block_slots(dofs_t, nblocks)
    assert ndof.max() == nU
    mult = {0: [], 1: [], 2: []}
    for b in range(nblocks):
        sl = slots[b*64:(b+1)*64]
        for mode, T in ((0, T0), (1, T1), (2, T2)):
            stride = T['stride'] or stride0
            lc, col = T['lane_cell'][b].astype(np.int64), T['lds_col'][b].astype(np.int64)
            assert sorted(lc.tolist()) == list(range(64)), (mode, b)
            assert len(set(col.tolist())) == nU and col.min() >= 0 and col.max() < stride, (mode, b)
            cc = T['cell_col'][:, b*64:(b+1)*64].T.astype(np.int64)              # [cell, k]
            assert (cc[sl >= 0] == col[sl[sl >= 0]]).all(), (mode, b)
            if mode:
                assert (cc[sl < 0] >= stride-16).all() and (cc[sl < 0] < stride).all() and col.max() < stride-16, (mode, b)
            else:
                assert np.array_equal(lc, np.arange(64)) and np.array_equal(col, np.arange(nU)) and (cc[sl < 0] == nUe).all()
            rows = np.where(sl >= 0, sl, nUe)[lc]
            m = _multiplier(rows, cc[lc], stride)
            mult[mode].append(m)
            if mode:
                assert abs(m-T['mult'][b]) <= 1e-12, (mode, b, m, T['mult'][b])      # the library reports the same model
        assert mult[1][-1] <= mult[0][-1], (b, mult[1][-1], mult[0][-1])
    means = {m: float(np.mean(v)) for m, v in mult.items()}
    print('%s: %d blocks, nU = %d, stride %d (identity %d); modelled multiplier identity %.3f, searched %.3f (max %.3f), random %.3f; '
          'layout of all blocks %.3f s on one thread, %.3f s on eight' % (case, nblocks, nU, T1['stride'], stride0, means[0], means[1],
                                                                         max(mult[1]), means[2], T1['seconds'], T8['seconds']))
    if case == 'disc5':
        assert means[1] <= MEAN_BOUND, means


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


def _compare(builder, what, checked=False):
    """default layout (optionally under PNL_UNI_CHECKED) and the random layout against the identity layout"""
    A0, cnt0 = _assemble(builder, PNL_UNI_LANES=0)
    A1, cnt1 = _assemble(builder, PNL_UNI_CHECKED=1 if checked else None)
    A2, cnt2 = _assemble(builder, PNL_UNI_LANES=2)
    scale = np.abs(A0).max()
    for name, A, cnt in (('default', A1, cnt1), ('random', A2, cnt2)):
        err, derr = np.abs(A-A0).max()/scale, np.abs(np.diag(A)-np.diag(A0)).max()/scale
        print('%s, %s layout against identity: pairs by order %s, max|dA|/max|A| = %.3e, diagonal %.3e'
              % (what, name, cnt['uniformTilePairsByOrder'], err, derr))
        for key in COUNTER_KEYS:
            if checked and name == 'default' and key in ('uniformTilesUnchecked', 'uniformTilesChecked'):
                continue
            assert cnt[key] == cnt0[key], (key, cnt[key], cnt0[key])
        assert err <= TOL_ORDER and derr <= TOL_ORDER, (what, name, err, derr)
    assert cnt0['uniformTilePairsByOrder'][2] > 0
    if checked:
        assert cnt1['uniformTilesUnchecked'] == 0 and cnt1['uniformTilesChecked'] == cnt0['uniformTilesUnchecked']+cnt0['uniformTilesChecked']
    return cnt0


@pytest.mark.gpu
@pytest.mark.parametrize('s,checked', [(0.5, False), (0.75, False), (0.4, False), (0.5, True)])
def test_gpu_layouts_agree_on_the_disc(s, checked):
    """disc(5), target order 0.75: the 3-point and the 6-point kernel, s = 1/2 (KT 2), 3/4 (KT 1) and 0.4 (KT 0); one case with the
    default layout under PNL_UNI_CHECKED"""
    from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    b = nonlocalBuilder(P1_DoFMap(disc(5), PHYSICAL), getFractionalKernel(2, s), {'target_order': TARGET_ORDER}, zeroExterior=True)
    cnt0 = _compare(b, 'disc(5), s = %g%s' % (s, ', checked' if checked else ''), checked)
    assert cnt0['uniformTilePairsByOrder'][3] > 0


@pytest.mark.gpu
def test_gpu_layouts_agree_on_the_square():
    """uniformSquare(15): cells without a DoF and padding behind the last cell (trash columns, tiles through the checked loop)"""
    from pynucleus_amd import uniformSquare, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    b = nonlocalBuilder(P1_DoFMap(uniformSquare(N_SQUARE), PHYSICAL), getFractionalKernel(2, 0.5), {'target_order': 0.5}, zeroExterior=True)
    cnt0 = _compare(b, 'uniformSquare(%d)' % N_SQUARE)
    assert cnt0['uniformTilesChecked'] > 0 and cnt0['uniformTilesUnchecked'] > 0


@pytest.mark.gpu
def test_gpu_layouts_agree_with_label_blocks():
    """three layers on disc(4): blocks split per label and filled with zero-volume padding cells, one launch per kernel class"""
    from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.fractionalOrders import layersFractionalOrder
    b = nonlocalBuilder(P1_DoFMap(disc(4), PHYSICAL), getFractionalKernel(2, layersFractionalOrder(2, *LAYERS)), {'target_order': 0.5},
                        zeroExterior=True)
    assert b._blocked_dense() is not None
    _compare(b, 'three layers on disc(4)')
