"""Mixed tiles (k_tile_distant, 2D P1): pairs whose rule has the orbit structure of the symmetric 3- and 6-point rules take the
structured evaluators (cross block and diagonal factors from row / column / orbit sums of the kernel values); the option
PNL_MIXED_GENERIC sends them through the evaluators for arbitrary rules."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize('s', [0.5, 0.75, 0.4])
def test_gpu_mixed_tiles_structured_and_generic_evaluators_agree(s):
    """Same matrix to rounding, same pair counts and order histogram with both evaluators of the mixed tiles; the matrices differ,
    so both evaluators ran."""
    from pynucleus_amd import _lib
    from test_nearfield import _gpu_builder
    b = _gpu_builder(6, s, params={'target_order': 0.5})           # 24,576 cells: mixed tiles with orders 2, 3, 4 and higher
    A = b.getDense()
    D1, cnt1 = A.toarray().copy(), A.info['counters']
    del A
    try:
        _lib.set_option('PNL_MIXED_GENERIC', 1)
        b2 = _gpu_builder(6, s, params={'target_order': 0.5})
        A2 = b2.getDense()
        D2, cnt2 = A2.toarray(), A2.info['counters']
    finally:
        _lib.set_option('PNL_MIXED_GENERIC', None)
    for key in ('numAssembledCellPairs', 'orders', 'singular'):
        assert cnt1[key] == cnt2[key], key
    err = np.abs(D1-D2).max()
    assert err <= 1e-13*np.abs(D1).max()
    assert err > 0.                                       # two evaluators, not one


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['dense_P1', 'near_P1'])
def test_gpu_mixed_tile_loops_with_two_workgroups_against_the_oracle(case):
    """Two workgroups walk all mixed tiles (PNL_TILE_WGS): the structured lists inside the tile loop, dense and near field, entry by
    entry against the oracle."""
    from oracle.oracle import OracleProblem
    from pynucleus_amd import _lib, clusters
    from test_nearfield import _gpu_builder, _gpu_vs_oracle
    try:
        _lib.set_option('PNL_TILE_WGS', 2)
        if case == 'dense_P1':
            b = _gpu_builder(4, 0.5, params={'target_order': 0.5})
            A = b.getDense()
            Aref, cnt, _ = OracleProblem(b.tables).get_dense()
            for key in ('numAssembledCellPairs', 'numIntegrations', 'orders', 'singular'):
                assert A.info['counters'][key] == cnt[key], key
            assert np.abs(A.toarray()-Aref).max() <= 1e-11*np.abs(Aref).max()
        else:
            b = _gpu_builder(4, 0.75, mode='tiles')
            root, Pnear, Pfar = clusters.getNearFieldClusters(b.dm, eta=3., minClusterSize=8)
            Anear, Aref = _gpu_vs_oracle(b, Pnear, symmetric=True)
            assert np.abs(Anear.toarray()-Aref).max() <= 1e-11*np.abs(Aref).max()
    finally:
        _lib.set_option('PNL_TILE_WGS', None)
