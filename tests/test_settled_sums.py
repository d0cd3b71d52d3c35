"""Per-point diagonal sums and staged quadrature points of the settled mixed tiles with pair lists (dense 2D P1, one order class).  The
LISTS instantiation of k_tile_distant no longer forms the diagonal blocks S1 / S2 of every pair: its evaluators hand back the cross block
and the sums vv r_i, vv c_j, the tile adds them per (cell, point) in LDS (s_R[2][64][15]: 3 + 6 + 6 points of the orders 2, 3, 4) and forms
the six entries per cell at its flush from w phi_a phi_b in the point order of each side (orbit order, except the rows of the 6-point
rules, which run in the packed order).  The six points of order 3 of both sides are staged once per tile.  PNL_SETTLED_CODES keeps the
plan without lists and with it the per-pair diagonal blocks (unchanged code); PNL_MIXED_UNSETTLED settles nothing.

The paths add the same terms in different orders: the bound is the 1e-13 max|A| of tests/test_settled_lists.py.  disc(5), 6144 cells, is
the smallest disc whose plan settles tiles; target_order 0.5 was kept, it leaves no order empty there (test_gpu_every_order_is_exercised
asserts 11,364 / 3,311,211 / 3,472,689 pairs of order 4 / 3 / 2 > 0 from the record headers).

The host guard (the plan keeps lists only where the orders 2, 3, 4 have 3, 6, 6 points: lists_wanted, pnl_setup.hip) reads the rule offsets
of a device context, so it has no CPU test: it is covered by reading.  The LDS overlay is checked where it is declared (static_assert on
TileSmem::overlay_ok, pnl_kernels.h).
"""
import numpy as np
import pytest

TOL_ORDER = 1e-13           # the same terms summed in another order (tests/test_settled_lists.py)
NOREF = 5

COUNTER_KEYS = ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'orders', 'singular', 'uniformTilePairs', 'workListLength')


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


_cache = {}


def _builder(s):
    if ('builder', s) not in _cache:
        from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
        from pynucleus_amd.builder import nonlocalBuilder
        _cache[('builder', s)] = nonlocalBuilder(P1_DoFMap(disc(NOREF), PHYSICAL), getFractionalKernel(2, s), {'target_order': 0.5},
                                                 zeroExterior=True)
    return _cache[('builder', s)]


def _assemble(s, **options):
    """(A, counters, diagonal blocks of the cells) of one assembly; computed once per (s, options) and left unchanged"""
    key = (s,)+tuple(sorted((k, v) for k, v in options.items() if v is not None))
    if key not in _cache:
        import torch
        b = _builder(s)
        with _options(**options):
            op = b.getDense()
            A, cnt = op.toarray(), op.info['counters']
            ctx = b.dense_context()
            D = torch.zeros(ctx.diag_blocks_size(), dtype=torch.float64, device=torch.device('cuda', ctx.device))
            ctx.get_diag_blocks(D.data_ptr())
            torch.cuda.synchronize()
            D = D.cpu().numpy()
        A.setflags(write=False)
        D.setflags(write=False)
        _cache[key] = (A, cnt, D)
    return _cache[key]


def _close(A, B, scale, what):
    err, derr = np.abs(A-B).max()/scale, np.abs(np.diag(A)-np.diag(B)).max()/scale
    print('%s: max|dA|/max|A| = %.3e, diagonal %.3e' % (what, err, derr))
    assert err <= TOL_ORDER and derr <= TOL_ORDER, (what, err, derr)


@pytest.mark.gpu
@pytest.mark.parametrize('s,wgs', [(0.5, None), (0.75, None), (0.4, None), (0.5, 2)])
def test_gpu_sums_codes_and_classification_agree(s, wgs):
    """s = 1/2 (KT 2), 3/4 (KT 1) and 0.4 (KT 0).  With PNL_TILE_WGS=2 one workgroup walks hundreds of settled tiles: the points of the
    next tile are staged before the flush of this one, which zeroes the sums it reads."""
    A0, cnt0, _ = _assemble(s, PNL_MIXED_UNSETTLED=1)
    AL, cntL, _ = _assemble(s, PNL_TILE_WGS=wgs)
    AC, cntC, _ = _assemble(s, PNL_TILE_WGS=wgs, PNL_SETTLED_CODES=1)
    print('settled tiles', cntL['settledTiles'], 'with lists', cntL['settledListTiles'])
    assert cnt0['settledTiles'] == 0 and cnt0['settledListTiles'] == 0
    assert cntL['settledListTiles'] == cntL['settledTiles'] > 0
    assert cntC['settledTiles'] == cntL['settledTiles'] and cntC['settledListTiles'] == 0
    for cnt in (cntL, cntC):
        for key in COUNTER_KEYS:
            assert cnt[key] == cnt0[key], (key, cnt[key], cnt0[key])
    scale = np.abs(A0).max()
    _close(AL, AC, scale, 'sums - codes')
    _close(AL, A0, scale, 'sums - unsettled')
    sym = np.abs(AL-AL.T).max()/scale
    print('symmetry %.3e' % sym)
    assert sym <= TOL_ORDER


@pytest.mark.gpu
def test_gpu_every_order_is_exercised():
    """the record headers of the settled tiles of the case: pairs of order 2, 3 and 4 (target_order 0.5 leaves none of them empty)"""
    b = _builder(0.5)
    b.getDense()
    codes, lists = b.dense_context().settled_lists()
    assert lists is not None
    n4, n3, n2 = (int(x) for x in lists[:, :3].astype(np.int64).sum(0))
    print('settled tiles %d: pairs of order 4 / 3 / 2: %d / %d / %d' % (lists.shape[0], n4, n3, n2))
    assert n2 > 0 and n3 > 0 and n4 > 0, (n2, n3, n4)


@pytest.mark.gpu
@pytest.mark.parametrize('s', [0.5, 0.75, 0.4])
def test_gpu_diagonal_blocks_alone(s):
    """the per-cell diagonal blocks (six entries per cell, before they are scattered into A) of the default path against the per-pair
    blocks of PNL_SETTLED_CODES, to 1e-13 max|D|: a wrong point order on one side cannot hide under the larger cross entries"""
    _, _, DL = _assemble(s)
    _, _, DC = _assemble(s, PNL_SETTLED_CODES=1)
    assert DL.shape == DC.shape and np.abs(DC).max() > 0.
    err = np.abs(DL-DC).max()/np.abs(DC).max()
    print('diagonal blocks: %d entries, max|dD|/max|D| = %.3e' % (DL.shape[0], err))
    assert err <= TOL_ORDER, err


@pytest.mark.gpu
def test_gpu_generic_evaluators_keep_sums():
    """PNL_MIXED_GENERIC (evaluators for arbitrary rules, both sides in the packed point order): lists path against the unsettled path
    under the same option, matrix, diagonal and diagonal blocks"""
    A0, cnt0, D0 = _assemble(0.5, PNL_MIXED_UNSETTLED=1, PNL_MIXED_GENERIC=1)
    A1, cnt1, D1 = _assemble(0.5, PNL_MIXED_GENERIC=1)
    assert cnt0['settledTiles'] == 0
    assert cnt1['settledListTiles'] == cnt1['settledTiles'] > 0
    for key in COUNTER_KEYS:
        assert cnt1[key] == cnt0[key], (key, cnt1[key], cnt0[key])
    scale = np.abs(A0).max()
    _close(A1, A0, scale, 'generic evaluators, sums - unsettled')
    assert np.abs(A1-A1.T).max() <= TOL_ORDER*scale
    err = np.abs(D1-D0).max()/np.abs(D0).max()
    print('generic evaluators, diagonal blocks: max|dD|/max|D| = %.3e' % err)
    assert err <= TOL_ORDER, err

