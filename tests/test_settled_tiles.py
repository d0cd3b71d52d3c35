"""Settled mixed tiles (dense 2D P1, one order class): the tile plan records for the mixed tiles that hold nothing but absent pairs and
distant pairs of the orders 2 .. 4 the order of every pair (2 bits per pair, k_tile_pair_codes), and the SETTLED instantiation of
k_tile_distant loads these codes instead of classifying the pairs in every assembly.  Both paths build the same lists in the same
order; the matrices differ by the order of the LDS additions across waves only, which
test_gpu_uniform_tiles_structured_and_generic_evaluators_agree bounds by 1e-13 max|A| for two summation orders of the same terms.
The option PNL_MIXED_UNSETTLED makes the plan settle nothing.

Settled tiles against the oracle: the plans of the disc at noRef 4 (1536 cells, the largest size of the whole-matrix oracle tests) and
of the 12-sector fan at noRef 4 (3072 cells) settle no tile, noRef 5 (6144 cells) settles 1659, and the whole oracle takes too long
there.  tests/test_graded_tiles.py holds single entries of the production run at 6144 cells (graded discs, 2691 and 1629 settled
tiles) to sums of the oracle's cell-pair contributions, more than 1000 sampled entries per case fed by a settled tile, each within
its own relative bound (1e-12 for most), and the order histogram of that run to the oracle's formula over all cell pairs.  Here the
settled path is held to the classifying path, matrix against matrix.
"""
import os

import numpy as np
import pytest

TOL_ORACLE = 1e-11          # tests/test_gpu_parity.py
TOL_ORDER = 1e-13           # the same terms summed in another order

# the smallest refinement of the disc whose plan settles at least 32 tiles (noRef 4 settles none; the tests assert the count)
NOREF = 5

COUNTER_KEYS = ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'numBoundaryPairs', 'numBoundaryIntegrations', 'orders',
                'singular', 'uniformTilePairs', 'uniformTilePairsByOrder', 'workListLength')


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


def _build(noRef, s=0.5, element='P1', mesh=None):
    from pynucleus_amd import disc, PHYSICAL, dofmapFactory, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    mesh = disc(noRef) if mesh is None else mesh
    dm = dofmapFactory(element, mesh, PHYSICAL)
    return nonlocalBuilder(dm, getFractionalKernel(2, s), {'target_order': 0.5}, zeroExterior=True)


def _assemble(builder, **options):
    """(matrix on the host, counters) of one getDense() under the options"""
    with _options(**options):
        A = builder.getDense()
        return A.toarray(), A.info['counters']


def _same_counters(got, want):
    for key in COUNTER_KEYS:
        assert got[key] == want[key], (key, got[key], want[key])


_cache = {}


def _unsettled(noRef, s):
    """builder and its assembly with PNL_MIXED_UNSETTLED, made once per case"""
    key = (noRef, s)
    if key not in _cache:
        b = _build(noRef, s)
        A0, cnt0 = _assemble(b, PNL_MIXED_UNSETTLED=1)
        assert cnt0['settledTiles'] == 0
        A0.setflags(write=False)
        _cache[key] = (b, A0, cnt0)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize('s', [0.5, 0.4, 0.75])
@pytest.mark.parametrize('wgs', [None, 2])
def test_gpu_settled_and_classified_mixed_tiles_agree(s, wgs):
    """s = 1/2 (KT = 2), s = 0.4 (KT = 0, general exponent) and s = 3/4 (KT = 1, the other quarter-integer exponents), with the full grids and with two workgroups per tile kernel (one
    workgroup then walks many settled tiles: the staging of the code word of the next tile inside the pipeline): every counter equal,
    the matrices equal to the rounding of two summation orders.  The plan must settle at least 32 tiles, so the path is in use.
    The counters include the length of the work list."""
    b, A0, cnt0 = _unsettled(NOREF, s)
    A1, cnt1 = _assemble(b, PNL_TILE_WGS=wgs)
    scale = np.abs(A0).max()
    print('settled tiles', cnt1['settledTiles'], 'max|A1 - A0|/max|A| = %.3e' % (np.abs(A1-A0).max()/scale))
    assert cnt1['settledTiles'] >= 32, cnt1['settledTiles']
    _same_counters(cnt1, cnt0)
    assert np.abs(A1-A0).max() <= TOL_ORDER*scale
    assert np.abs(A1-A1.T).max() <= TOL_ORDER*scale


@pytest.mark.gpu
def test_gpu_cell_range_that_cuts_a_block_settles_nothing():
    import torch
    b, A0, cnt0 = _unsettled(NOREF, 0.5)
    N, nc = b.dm.num_dofs, b.mesh.num_cells
    c0, c1 = 17, nc-29
    ctx = b.context()
    mats = []
    for opt in (None, 1):
        with _options(PNL_MIXED_UNSETTLED=opt):
            A = torch.zeros((N, N), dtype=torch.float64, device='cuda')
            ctx.assemble_dense(A.data_ptr(), N, True, c0, c1)
            ctx.synchronize()
            cnt = ctx.counters()
            assert cnt['settledTiles'] == 0
            mats.append((A.cpu().numpy(), cnt))
    _same_counters(mats[0][1], mats[1][1])
    assert np.abs(mats[0][0]-mats[1][0]).max() <= TOL_ORDER*np.abs(A0).max()


@pytest.mark.gpu
def test_gpu_symmetric_flush_settles_nothing():
    """PNL_FLAG_SYMMETRIC_FLUSH (the flush of the multi-rank assemblies) over the whole cell range: the plan may hold settled tiles,
    the assembly takes none through the settled instantiation, and the matrix is that of the unsettled path"""
    import torch
    from pynucleus_amd import _lib
    b, A0, cnt0 = _unsettled(NOREF, 0.5)
    N, nc = b.dm.num_dofs, b.mesh.num_cells
    ctx = b.context()
    A = torch.zeros((N, N), dtype=torch.float64, device='cuda')
    ctx.assemble_dense(A.data_ptr(), N, True, 0, nc, _lib.PNL_FLAG_SYMMETRIC_FLUSH)
    ctx.synchronize()
    cnt = ctx.counters()
    assert cnt['settledTiles'] == 0
    _same_counters(cnt, cnt0)
    assert np.abs(A.cpu().numpy()-A0).max() <= 1e-12*np.abs(A0).max()      # atomics into A instead of the fold: tests/test_gpu_parity.py


@pytest.mark.gpu
def test_gpu_blocks_that_are_not_full_are_not_settled():
    """a structured square with 6728 cells: 105 full blocks and a last one of 8 cells.  The plan settles tiles (about 2000), none of them
    with the last block, none on the diagonal, each once; both paths give the same operator"""
    from pynucleus_amd.mesh import uniformSquare
    mesh = uniformSquare(59, 59, -1., -1., 1., 1.)
    nfull = mesh.num_cells//64
    assert mesh.num_cells % 64 != 0
    b = _build(None, mesh=mesh)
    A0, cnt0 = _assemble(b, PNL_MIXED_UNSETTLED=1)
    assert cnt0['settledTiles'] == 0 and b.dense_context().settled_tiles().shape[0] == 0
    A1, cnt1 = _assemble(b)
    tiles = b.dense_context().settled_tiles()
    print('settled tiles', cnt1['settledTiles'])
    assert cnt1['settledTiles'] >= 32 and tiles.shape[0] == cnt1['settledTiles']
    assert (tiles[:, 0] < tiles[:, 1]).all() and tiles.min() >= 0
    assert tiles.max() < nfull                                   # block nfull is the one that is not full
    assert np.unique(tiles[:, 0].astype(np.int64)*(nfull+1)+tiles[:, 1]).shape[0] == tiles.shape[0]
    _same_counters(cnt1, cnt0)
    assert np.abs(A1-A0).max() <= TOL_ORDER*np.abs(A0).max()


@pytest.mark.gpu
def test_gpu_variable_order_settles_nothing():
    """three layers of orders on the disc at noRef 5, where the constant order settles 1659 tiles: several order classes with labels, so
    the plan settles nothing, with and without the option, and both assemblies agree"""
    from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.fractionalOrders import layersFractionalOrder
    order = layersFractionalOrder(2, np.array([-1., -0.3, 0.3, 1.]), np.array([[0.3, 0.4, 0.5], [0.4, 0.5, 0.6], [0.5, 0.6, 0.7]]))
    b = nonlocalBuilder(P1_DoFMap(disc(NOREF), PHYSICAL), getFractionalKernel(2, order), {'target_order': 0.5}, zeroExterior=True)
    A0, cnt0 = _assemble(b, PNL_MIXED_UNSETTLED=1)
    A1, cnt1 = _assemble(b)
    assert cnt0['settledTiles'] == 0 and cnt1['settledTiles'] == 0
    assert b.dense_context().settled_tiles().shape[0] == 0
    _same_counters(cnt1, cnt0)
    assert np.abs(A1-A0).max() <= TOL_ORDER*np.abs(A0).max()


@pytest.mark.gpu
def test_gpu_p2_settles_nothing():
    """P2 has blocks of 32 cells and a tile kernel of its own: nothing to settle at any size; against the oracle"""
    from oracle.oracle import OracleProblem
    b = _build(3, element='P2')
    A1, cnt1 = _assemble(b)
    assert cnt1['settledTiles'] == 0
    Aref, cnt, _ = OracleProblem(b.tables).get_dense()
    for key in ('numAssembledCellPairs', 'numIntegrations', 'orders', 'singular'):
        assert cnt1[key] == cnt[key], (key, cnt1[key], cnt[key])
    assert np.abs(A1-Aref).max() <= TOL_ORACLE*np.abs(Aref).max()


def _slab_worker(rank, world, port, out):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel, _lib
        from pynucleus_amd.builder import nonlocalBuilder
        dm = P1_DoFMap(disc(NOREF), PHYSICAL)
        b = nonlocalBuilder(dm, getFractionalKernel(2, 0.5), {'target_order': 0.5}, zeroExterior=True, comm=True)
        res = []
        for opt in (None, 1):
            _lib.set_option('PNL_MIXED_UNSETTLED', opt)
            op = b.getDense(distributed=True)
            res.append((op.slab.cpu().numpy(), op.dblocks.cpu().numpy(), op.info['counters'], int(b.context().settled_tiles().shape[0])))
        _lib.set_option('PNL_MIXED_UNSETTLED', None)
        (S1, D1, c1, n1), (S0, D0, c0, n0) = res
        scale = max(float(np.abs(S0).max()), float(np.abs(D0).max()))
        out.put(dict(rank=rank, settled=[c1['settledTiles'], c0['settledTiles'], n1, n0], pairs=c1['numAssembledCellPairs'],
                     same={k: c1[k] == c0[k] for k in COUNTER_KEYS}, scale=scale,
                     err=max(float(np.abs(S1-S0).max()), float(np.abs(D1-D0).max()))))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:                                # a rank that dies must not leave the others in a collective
        import traceback
        out.put(dict(error='rank {}: {}\n{}'.format(rank, repr(e), traceback.format_exc())))
        out.close()
        out.join_thread()
        os._exit(1)


@pytest.mark.gpu
def test_gpu_two_rank_slabs_settle_nothing():
    """row slabs of two gloo ranks on one card at noRef 5, where one rank alone settles 1659 tiles: no rank assembles the whole cell
    range, so neither plan settles a tile; slab, diagonal blocks and counters of every rank equal those of its assembly with
    PNL_MIXED_UNSETTLED, and the ranks together assemble the pairs of the single-rank operator"""
    import torch.multiprocessing as mp
    b, A0, cnt0 = _unsettled(NOREF, 0.5)
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = 31700+os.getpid() % 2000
    procs = [ctx.Process(target=_slab_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = []
    for _ in procs:
        r = out.get(timeout=300)
        if 'error' in r:
            for p in procs:
                p.kill()
            raise AssertionError(r['error'])
        got.append(r)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r['rank'] for r in got) == [0, 1]
    for r in got:
        assert r['settled'] == [0, 0, 0, 0], r
        assert all(r['same'].values()), r['same']
        assert r['err'] <= TOL_ORDER*r['scale'], r
    assert sum(r['pairs'] for r in got) == cnt0['numAssembledCellPairs']


@pytest.mark.gpu
def test_gpu_plan_cache_keeps_the_codes():
    """a second assembly on the same builder keeps the plan and its codes; the option PNL_MIXED_UNSETTLED makes a new plan each time it
    changes"""
    b = _build(NOREF)
    A1, cnt1 = _assemble(b)
    A2, cnt2 = _assemble(b)
    assert cnt1['settledTiles'] >= 32 and cnt2['settledTiles'] == cnt1['settledTiles']
    assert cnt1['codeBuilds'] == 1 and cnt2['codeBuilds'] == 1
    A3, cnt3 = _assemble(b, PNL_MIXED_UNSETTLED=1)
    assert cnt3['settledTiles'] == 0 and cnt3['codeBuilds'] == 1
    A4, cnt4 = _assemble(b)
    assert cnt4['settledTiles'] == cnt1['settledTiles'] and cnt4['codeBuilds'] == 2
    assert np.abs(A4-A1).max() <= TOL_ORDER*np.abs(A1).max()


def test_code_layout_round_trips():
    """The word codes[tile][tid] holds the 2-bit codes of the eight pairs of thread tid, sweep k in bits 2 k, 2 k + 1.  Restated in numpy:
    thread tid keeps cell j = tid % 64 of block b and visits row r = 8 k + tid // 64 of the wrapped diagonals, pair p = 64 r + j, cell
    i = (r + 21 j) % 64 of block a.  The library's layout function (no GPU) agrees, every pair of the tile has exactly one slot, and a
    table of codes packed by (i, j) and unpacked by (tid, k) comes back unchanged."""
    from pynucleus_amd import _lib
    tid, k = np.meshgrid(np.arange(512), np.arange(8), indexing='ij')
    got = _lib.selftest(_lib.SELFTEST_SETTLED_LAYOUT, (8*tid+k).ravel().astype(np.float64)).astype(np.int64)
    j = tid % 64
    r = 8*k+tid//64
    i = (r+21*j) % 64
    assert np.array_equal(got[:, 0], (64*r+j).ravel())
    assert np.array_equal(got[:, 1], i.ravel()) and np.array_equal(got[:, 2], j.ravel())
    # every pair index and every cell pair exactly once
    assert np.array_equal(np.sort(got[:, 0]), np.arange(4096))
    assert np.unique(got[:, 1]*64+got[:, 2]).shape[0] == 4096
    # the kernel's inverse: pair p of the lists -> j = p % 64, i = (p // 64 + 21 j) % 64
    p = got[:, 0]
    assert np.array_equal((p//64+21*(p % 64)) % 64, got[:, 1])
    # pack a table of codes by (i, j) into the words, unpack it again
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 4, size=(64, 64))
    words = np.zeros(512, dtype=np.uint16)
    for t, kk, ii, jj in zip(tid.ravel(), k.ravel(), got[:, 1], got[:, 2]):
        words[t] |= np.uint16(codes[ii, jj] << (2*kk))
    back = np.full((64, 64), -1)
    for t in range(512):
        for kk in range(8):
            rr = 8*kk+t//64
            back[(rr+21*(t % 64)) % 64, t % 64] = (int(words[t]) >> (2*kk)) & 3
    assert np.array_equal(back, codes)
