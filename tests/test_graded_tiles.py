"""The dense tile paths on graded meshes, against the oracle.

Every other GPU assembly test builds its mesh with disc, interval or uniformSquare, where the longest edge h varies by less than a
factor of 2: the per-block ranges [hmin, hmax], [Lmin, Lmax] behind the tile plan (pnl_tile_uniform_order, k_tile_order_range) are then
degenerate, the quadrature orders stay below about 10, and the settled tiles exist only at sizes the whole oracle cannot reach.  Two
meshes made by moving the vertices of disc(5) (tests/graded_meshes.py): G1, graded towards the centre (r -> r^2, h from 9.8e-4 to
6.9e-2, orders 2 .. 27), and G2, graded towards the rim (r -> 1 - (1 - r)^1.5, flat cells, shortest edge hmax / 11).

T1  strips of two full blocks +- 17 cells against the oracle's strip (range-filtered plan, classifying kernels, work lists, boundary
    tiles, touching pairs): counters exact, 1e-11 max|A|, per-entry bound on the separated entries (P1).
T2  the production launch sequence (getDense, no option: settled tiles, unchecked uniform tiles) against single entries summed from
    the oracle's cell-pair contributions, >= 2000 separated DoF pairs per case, >= 200 of them fed by a settled tile.
    The integer counters of the same run against the oracle's classification and order formula over all 1.9e7 cell pairs.
T3  the alternative paths and a partition of the cells into three ranges agree with the default run, which ties the orders of the
    production plan to the range-filtered plan of T1.

Per-entry bound (T1, T2): |A_gpu - A_ref| <= tol_ij |A_ref|, tol_ij = max(1e-12, 2e-14 + 2 P_ij 2^-53), P_ij the kernel evaluations
behind the entry.  1e-12 is REL of tests/test_small_entries.py; the second term is the rounding of two fp64 sums of P_ij terms of
one sign in any order, each term carrying the 1e-14 kernel-value bound of tests/test_device_math.py.

Condition on the inputs: every distant pair of every strip and every cell pair behind a sampled entry keeps both ceil() arguments of
the oracle's order formula at least 1e-9 from an integer (quad_order_exact may differ from the oracle within 1e-12 of a tie only);
asserted, no pair is excluded from a comparison.  Smallest margins: 2.9e-8 (G1, s = 0.75), 5.7e-7 (G2).

Measured on an MI355X.  Production plans: G1 s = 0.5 2691 settled and 1224 unchecked uniform tiles, G1 s = 0.4 2646 and 1353, G2
s = 0.5 1629 and 2448.  Worst error / tol_ij: T1 1.1e-3 (G1, s = 0.5), 2.6e-3 (G1, s = 0.75), 1.7e-3 (G1, s = 0.4), 2.4e-3 (G2,
s = 0.5), 2.1e-3 (G2, s = 0.75), max error 1.6e-13 max|A| (P2: 3.1e-15); T2 8.1e-4 (G1, s = 0.5), 1.3e-3 (G1, s = 0.4), 1.1e-3 (G2),
1100 .. 1230 of the 2470 .. 2640 sampled entries fed by a settled tile; T3 5.4e-16 max|A|.  DESIGN.md section 2 has the outcomes of
three value-only mutations of the kernels and the plan."""
import numpy as np
import pytest

from graded_meshes import (graded_disc, signed_areas, edge_lengths, cell_quality, separated, oracle_entries, pair_tie_margin,
                           strip_tie_margin, strip_distant_pairs, formula_orders, formula_counters, strip_evaluations, strips, as_oracle)
from test_settled_tiles import COUNTER_KEYS, TOL_ORDER, _options

gpu = pytest.mark.gpu

TOL = 1e-11                 # tests/test_gpu_parity.py
REL = 1e-12                 # tests/test_small_entries.py
MARGIN = 1e-9               # a thousand times the 1e-12 within which quad_order_exact may differ from the oracle
U = 2.**-53

MESHES = {'G1': (5, 'centre', 2.), 'G2': (5, 'boundary', 1.5), 'G1n4': (4, 'centre', 2.)}
STRIP_CASES = [('G1', 0.5, 'P1'), ('G1', 0.75, 'P1'), ('G1', 0.4, 'P1'), ('G2', 0.5, 'P1'), ('G2', 0.75, 'P1'), ('G1n4', 0.5, 'P2')]

_meshes, _builders, _default = {}, {}, {}


def _mesh(name):
    if name not in _meshes:
        _meshes[name] = graded_disc(*MESHES[name])
    return _meshes[name]


def _builder(name, s, element='P1'):
    """(builder, oracle problem) of the case, made once"""
    from pynucleus_amd import PHYSICAL, dofmapFactory, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    key = (name, s, element)
    if key not in _builders:
        dm = dofmapFactory(element, _mesh(name), PHYSICAL)
        b = nonlocalBuilder(dm, getFractionalKernel(2, s), {'target_order': 0.5}, zeroExterior=True)
        _builders[key] = (b, as_oracle(b.tables))
    return _builders[key]


def _case_strips(name, element):
    block, pad = (64, 17) if element == 'P1' else (32, 9)
    return strips(_mesh(name), block, pad)


def entry_tolerance(P):
    return np.maximum(REL, 2e-14+2.*P*U)


# ---- helpers, without a GPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['G1', 'G2'])
def test_graded_disc(name):
    """orientation of every cell unchanged, cells not degenerate, and the grading the tests rely on: h ratio >= 50 on G1, shortest
    edge <= hmax / 5 with a quasi-uniform h on G2"""
    from pynucleus_amd import disc
    noRef, kind, mu = MESHES[name]
    base, mesh = disc(noRef), _mesh(name)
    assert np.array_equal(mesh.cells, base.cells) and np.array_equal(mesh.boundaryEdges, base.boundaryEdges)
    assert mesh.num_cells == 6144
    assert np.array_equal(np.sign(signed_areas(mesh)), np.sign(signed_areas(base))) and np.all(signed_areas(mesh) != 0.)
    r = np.linalg.norm(mesh.vertices, axis=1)
    assert r.max() <= 1.+1e-15 and np.abs(r[mesh.boundaryVertices]-1.).max() <= 1e-15
    h, e = mesh.hVector, edge_lengths(mesh)
    assert np.array_equal(h, e.max(axis=1))
    if name == 'G1':
        assert cell_quality(mesh).min() >= 0.5
        assert h.max()/h.min() >= 50.
    else:
        assert cell_quality(mesh).min() >= 0.25
        assert e.min() <= h.max()/5. and h.max()/h.min() < 2.


def test_oracle_entries_reproduce_get_dense():
    """oracle_entries has the bits of get_dense(c0, c1) on every entry (i, j), i a DoF of the strip's cells, j sharing no cell with i
    (distant and vertex-touching cell pairs, pairs cut off by the strip's range), its P_ij equals strip_evaluations on the separated
    pairs, and the separated entries are <= 0.  G1 at noRef 4, s = 0.4, a strip of five cells."""
    b, op = _builder('G1n4', 0.4)
    dm = b.dm
    c0, c1 = 700, 705
    Aref, cnt, _ = op.get_dense(c0, c1)
    dofs = np.asarray(dm.dofs)
    rows = np.unique(dofs[c0:c1][dofs[c0:c1] >= 0])
    assert rows.size >= 3
    cell_dof = np.zeros((dm.mesh.num_cells, dm.num_dofs), dtype=bool)
    for k in range(dofs.shape[1]):
        m = dofs[:, k] >= 0
        cell_dof[np.nonzero(m)[0], dofs[m, k]] = True
    share = (cell_dof.T.astype(np.int32)@cell_dof.astype(np.int32)) > 0
    ij = [(int(i), int(j)) for i in rows for j in np.nonzero(~share[i])[0]]
    assert len(ij) > 2000
    vals, P, pairs = oracle_entries(op, ij, (c0, c1), with_pairs=True)
    I, J = np.array(ij).T
    assert np.array_equal(vals, Aref[I, J]) and np.array_equal(vals, Aref[J, I])
    assert np.count_nonzero(vals) > 2000
    assert any(p[2] < 0 for pl in pairs for p in pl) and any(p[2] >= 10 for pl in pairs for p in pl)
    sep = separated(dm)[I, J]
    assert sep.sum() > 2000 and np.all(vals[sep] <= 0.)
    assert np.array_equal(P[sep], strip_evaluations(op, c0, c1)[I, J][sep])
    # the whole operator: a few entries against the sum of strips that cover every first cell of their pairs
    sub = ij[::97]
    whole, Pw = oracle_entries(op, sub)
    parts = [oracle_entries(op, sub, (lo, hi)) for lo, hi in ((0, c0), (c0, c1), (c1, dm.mesh.num_cells))]
    assert np.array_equal(Pw, sum(p[1] for p in parts))
    assert np.abs(whole-sum(p[0] for p in parts)).max() <= 4*U*np.abs(whole).max()


@pytest.mark.parametrize('name,s,element', STRIP_CASES)
def test_strips_keep_the_tie_margin(name, s, element):
    """the condition on the inputs of T1: every distant pair (cell x cell and cell x boundary facet) of both strips keeps the ceil()
    arguments 1e-9 from an integer; by the formula the strips reach order >= 15 and stay below the cap of the rule tables"""
    b, op = _builder(name, s, element)
    for c0, c1 in _case_strips(name, element):
        margin, count = strip_tie_margin(op, c0, c1)
        q = formula_orders(op, *strip_distant_pairs(op, c0, c1))
        print(name, s, element, (c0, c1), 'pairs', count, 'margin %.3e' % margin, 'orders', q.min(), q.max())
        assert margin >= MARGIN, (c0, c1, margin)
        assert q.min() == 2 and 15 <= q.max() <= op.tables.qcap


@pytest.mark.parametrize('s', [0.5, 0.4])
def test_formula_counters_are_the_oracles(s):
    """formula_counters against the whole oracle on G1 at noRef 3 (384 cells): pairs, kernel evaluations, order histogram, touching pairs"""
    from pynucleus_amd import PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    b = nonlocalBuilder(P1_DoFMap(graded_disc(3, 'centre', 2.), PHYSICAL), getFractionalKernel(2, s), {'target_order': 0.5}, zeroExterior=True)
    op = as_oracle(b.tables)
    got, margin = formula_counters(op, rows=100)
    _, want, _ = op.get_dense(store=False)
    assert margin >= MARGIN
    assert max(want['orders']) >= 10
    for key in ('numAssembledCellPairs', 'numIntegrations', 'orders', 'singular'):
        assert got[key] == want[key], (key, got[key], want[key])


def test_entry_tolerance():
    """1e-12 up to about 4400 evaluations per entry, the rounding term above"""
    assert entry_tolerance(np.array([36, 4400]))[1] == REL and entry_tolerance(np.array([4500]))[0] > REL
    assert entry_tolerance(np.array([36*120**2]))[0] == 2e-14+2*36*120**2*U


# ---- T1: strips against the oracle --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('which', [0, 1], ids=['hmin', 'mid'])
@pytest.mark.parametrize('name,s,element', STRIP_CASES)
def test_gpu_strip_against_oracle(name, s, element, which):
    import torch
    b, op = _builder(name, s, element)
    N = b.dm.num_dofs
    c0, c1 = _case_strips(name, element)[which]
    margin, _ = strip_tie_margin(op, c0, c1)
    assert margin >= MARGIN, margin
    ctx = b.context()
    A = torch.zeros((N, N), dtype=torch.float64, device='cuda')
    ctx.assemble_dense(A.data_ptr(), N, True, c0, c1)
    ctx.synchronize()
    cnt = ctx.counters()
    Ag = A.cpu().numpy()
    Aref, cref, _ = op.get_dense(c0, c1)
    for key in ('numAssembledCellPairs', 'numIntegrations', 'numBoundaryPairs', 'orders', 'singular'):
        assert cnt[key] == cref[key], (key, cnt[key], cref[key])
    assert max(cref['orders']) >= 15 and cnt['workListLength'] > 0, (max(cref['orders']), cnt['workListLength'])
    scale = np.abs(Aref).max()
    err = np.abs(Ag-Aref).max()/scale
    line = '{} s={} {} strip {}: orders 2..{}, uniform pairs {}, work list {}, max err {:.2e} max|A|'.format(
        name, s, element, (c0, c1), max(cref['orders']), cnt['uniformTilePairs'], cnt['workListLength'], err)
    if element == 'P1':
        sep = separated(b.dm)
        assert np.all(Aref[sep] <= 0.)
        m = sep & (Aref != 0.)
        assert m.sum() > 10000
        tol = entry_tolerance(strip_evaluations(op, c0, c1)[m])
        ratio = np.abs(Ag[m]-Aref[m])/np.abs(Aref[m])/tol
        k = ratio.argmax()
        line += ', {} separated entries, worst err/tol {:.3e}'.format(m.sum(), ratio[k])
    print(line)
    assert err <= TOL, err
    if element == 'P1':
        assert ratio[k] <= 1., (ratio[k], np.argwhere(m)[k], Aref[m][k], Ag[m][k])


# ---- T2: the production launch sequence against sampled oracle entries ----------------------------------------------------------

def _whole(name, s):
    """getDense() with no option set: (matrix on the host, counters, settled tiles), made once per case"""
    key = (name, s)
    if key not in _default:
        b, _ = _builder(name, s)
        A = b.getDense()
        Ah = A.toarray()
        Ah.setflags(write=False)
        _default[key] = (Ah, A.info['counters'], b.dense_context().settled_tiles().astype(np.int64))
    return _default[key]


def _assert_paths_in_use(cnt):
    assert cnt['settledTiles'] >= 32 and cnt['settledListTiles'] == cnt['settledTiles'], (cnt['settledTiles'], cnt['settledListTiles'])
    assert cnt['uniformTilePairsByOrder'][2] > 0 and cnt['uniformTilePairsByOrder'][3] > 0, cnt['uniformTilePairsByOrder']
    assert cnt['uniformTilesUnchecked'] > 0


def sample_pairs(dm, settled, seed, per_bin=40, nsettled=300, nsize=100):
    """Seeded sample of separated DoF pairs i < j, stratified on a 8 x 8 grid, log-uniform in d / max(h_i, h_j) and in h_i / h_j
    (d the distance of the two vertices, h_i the largest h of the support of i), up to per_bin per cell of the grid, plus nsettled
    pairs with a contributing cell pair inside a settled tile (block a, block b), plus nsize tiny-tiny, tiny-large and large-large
    pairs each (tiny / large: the 15 % of the DoFs of smallest / largest h_i).  Returns (ij [n, 2], fed by a settled tile [n], (tiny-tiny, tiny-large, large-large) [n, 3])."""
    rng = np.random.default_rng(seed)
    N, nc = dm.num_dofs, dm.mesh.num_cells
    dofs, h = np.asarray(dm.dofs), dm.mesh.hVector
    hd = np.zeros(N)
    for k in range(dofs.shape[1]):
        m = dofs[:, k] >= 0
        np.maximum.at(hd, dofs[m, k], h[m])
    x = dm.getDoFCoordinates()
    I, J = np.nonzero(np.triu(separated(dm), 1))
    d = np.linalg.norm(x[I]-x[J], axis=1)
    u, v = np.log(d/np.maximum(hd[I], hd[J])), np.log(hd[I]/hd[J])

    def bins(t):
        return np.minimum(((t-t.min())/(t.max()-t.min())*8.).astype(np.int64), 7)
    cell = 8*bins(u)+bins(v)
    order = rng.permutation(I.size)
    order = order[np.argsort(cell[order], kind='stable')]
    start = np.searchsorted(cell[order], np.arange(65))
    pick = np.concatenate([order[start[k]:min(start[k+1], start[k]+per_bin)] for k in range(64)])
    # DoF x block incidence and the pairs a settled tile feeds
    nb = (nc+63)//64
    D = np.zeros((N, nb), dtype=np.int32)
    for k in range(dofs.shape[1]):
        m = dofs[:, k] >= 0
        D[dofs[m, k], np.nonzero(m)[0]//64] = 1
    S = np.zeros((nb, nb), dtype=np.int32)
    S[settled[:, 0], settled[:, 1]] = 1
    S[settled[:, 1], settled[:, 0]] = 1
    fed = (D@S@D.T) > 0
    extra = [rng.permutation(np.nonzero(fed[I, J])[0])[:nsettled]]
    # the grid is in ratios only: the absolute sizes get strata of their own (the 15 % of the DoFs of smallest / largest h)
    tiny, large = hd <= np.quantile(hd, 0.15), hd >= np.quantile(hd, 0.85)
    for m in (tiny[I] & tiny[J], (tiny[I] & large[J]) | (large[I] & tiny[J]), large[I] & large[J]):
        extra.append(rng.permutation(np.nonzero(m)[0])[:nsize])
    pick = np.unique(np.concatenate([pick]+extra))
    classes = np.stack([tiny[I[pick]] & tiny[J[pick]], (tiny[I[pick]] & large[J[pick]]) | (large[I[pick]] & tiny[J[pick]]),
                        large[I[pick]] & large[J[pick]]], axis=1)
    return np.stack([I[pick], J[pick]], axis=1), fed[I[pick], J[pick]], classes


@pytest.mark.parametrize('name', ['G1', 'G2'])
def test_sample_is_seeded_and_stratified(name):
    """without a GPU, on a made-up list of settled tiles: the same seed gives the same sample; only separated pairs i < j, each once;
    at least 2000, at least 100 of each size class, the pairs marked as fed by a settled tile have a cell pair in one"""
    b, _ = _builder(name, 0.5)
    settled = np.array([[3, 40], [10, 70], [20, 90], [33, 34]])
    ij, fed, classes = sample_pairs(b.dm, settled, seed=5)
    ij2, fed2, _ = sample_pairs(b.dm, settled, seed=5)
    assert np.array_equal(ij, ij2) and np.array_equal(fed, fed2)
    assert ij.shape[0] >= 2000 and np.unique(ij[:, 0]*b.dm.num_dofs+ij[:, 1]).size == ij.shape[0]
    assert np.all(ij[:, 0] < ij[:, 1]) and separated(b.dm)[ij[:, 0], ij[:, 1]].all()
    assert classes.sum(axis=0).min() >= 100 and 200 <= fed.sum()
    dofs = np.asarray(b.dm.dofs)
    tiles = {tuple(t) for t in settled.tolist()}
    for (i, j), f in list(zip(ij.tolist(), fed.tolist()))[::23]:
        bi, bj = np.unique(np.nonzero((dofs == i).any(axis=1))[0]//64), np.unique(np.nonzero((dofs == j).any(axis=1))[0]//64)
        assert f == any((min(x, y), max(x, y)) in tiles for x in bi for y in bj)


@gpu
@pytest.mark.parametrize('name,s', [('G1', 0.5), ('G1', 0.4), ('G2', 0.5)])
def test_gpu_production_plan_against_sampled_oracle_entries(name, s):
    b, op = _builder(name, s)
    Ag, cnt, settled = _whole(name, s)
    print(name, s, 'settled tiles', cnt['settledTiles'], 'unchecked uniform tiles', cnt['uniformTilesUnchecked'], 'checked',
          cnt['uniformTilesChecked'], 'uniform pairs by order', cnt['uniformTilePairsByOrder'], 'work list', cnt['workListLength'],
          'orders 2..{}'.format(max(cnt['orders'])))
    _assert_paths_in_use(cnt)
    assert settled.shape[0] == cnt['settledTiles']
    ij, fed, classes = sample_pairs(b.dm, settled, seed=20261020)
    assert ij.shape[0] >= 2000 and fed.sum() >= 200, (ij.shape[0], fed.sum())
    assert classes.sum(axis=0).min() >= 100, classes.sum(axis=0)         # tiny-tiny, tiny-large, large-large
    ref, P, pairs = oracle_entries(op, ij, with_pairs=True)
    cp = np.array(sorted({(c1, c2) for pl in pairs for c1, c2, _ in pl}))
    assert min(p[2] for pl in pairs for p in pl) >= 2                    # separated: distant pairs only
    margin = pair_tie_margin(op, cp[:, 0], cp[:, 1]).min()
    assert margin >= MARGIN, margin
    assert np.all(ref < 0.)
    got = Ag[ij[:, 0], ij[:, 1]]
    ratio = np.abs(got-ref)/np.abs(ref)/entry_tolerance(P)
    k = ratio.argmax()
    qs = np.array([p[2] for pl in pairs for p in pl])
    print('{} s={}: {} entries ({} fed by a settled tile), {} cell pairs of orders {}..{}, margin {:.2e}, P up to {}, worst err/tol {:.3e}, '
          'worst among the settled-fed {:.3e}'.format(name, s, ij.shape[0], fed.sum(), cp.shape[0], qs.min(), qs.max(), margin, P.max(),
                                                      ratio[k], ratio[fed].max()))
    assert ratio[k] <= 1., (ratio[k], ij[k], ref[k], got[k], P[k])
    assert np.abs(got-Ag[ij[:, 1], ij[:, 0]]).max() <= TOL_ORDER*np.abs(Ag).max()


@gpu
@pytest.mark.parametrize('name,s', [('G1', 0.5), ('G1', 0.4), ('G2', 0.5)])
def test_gpu_production_plan_counts_every_pair_at_its_order(name, s):
    """the integer counters of the production run over all 1.9e7 cell pairs against formula_counters (the oracle's classification and
    order formula without its kernel evaluations; every distant pair of the mesh keeps the tie margin): a tile that the plan wrongly
    takes for uniform, or settles at a wrong order, changes the histogram"""
    b, op = _builder(name, s)
    _, cnt, _ = _whole(name, s)
    want, margin = formula_counters(op)
    print(name, s, 'margin over all distant pairs %.3e' % margin, 'orders', want['orders'])
    assert margin >= MARGIN, margin
    for key in ('numAssembledCellPairs', 'numIntegrations', 'orders', 'singular'):
        assert cnt[key] == want[key], (key, cnt[key], want[key])


# ---- T3: the alternative paths agree on graded meshes -------------------------------------------------------------------------

OPTIONS = [('PNL_MIXED_UNSETTLED', 1), ('PNL_SETTLED_CODES', 1), ('PNL_UNI_CHECKED', 1), ('PNL_UNI_GENERIC', 1), ('PNL_MIXED_GENERIC', 1),
           ('PNL_UNI_LANES', 0), ('PNL_TILE_WGS', 2)]


@gpu
@pytest.mark.parametrize('option,value', OPTIONS)
@pytest.mark.parametrize('name', ['G1', 'G2'])
def test_gpu_alternative_paths_agree(name, option, value):
    b, _ = _builder(name, 0.5)
    A0, cnt0, _ = _whole(name, 0.5)
    _assert_paths_in_use(cnt0)
    with _options(**{option: value}):
        A = b.getDense()
        A1, cnt1 = A.toarray(), A.info['counters']
    for key in COUNTER_KEYS:
        assert cnt1[key] == cnt0[key], (key, cnt1[key], cnt0[key])
    scale = np.abs(A0).max()
    print(name, option, value, 'max|A1 - A0|/max|A| = %.3e' % (np.abs(A1-A0).max()/scale), 'settled', cnt1['settledTiles'],
          'unchecked', cnt1['uniformTilesUnchecked'], 'checked', cnt1['uniformTilesChecked'])
    if option == 'PNL_MIXED_UNSETTLED':
        assert cnt1['settledTiles'] == 0
    if option == 'PNL_UNI_CHECKED':
        assert cnt1['uniformTilesUnchecked'] == 0 and cnt1['uniformTilesChecked'] > 0
    assert np.abs(A1-A0).max() <= TOL_ORDER*scale
    assert np.abs(A1-A1.T).max() <= TOL_ORDER*scale
    assert np.abs(A0-A0.T).max() <= TOL_ORDER*scale


@gpu
@pytest.mark.parametrize('name', ['G1', 'G2'])
def test_gpu_cell_ranges_add_up_to_the_production_plan(name):
    """three cell ranges whose cuts are not block boundaries (range-filtered plans, nothing settled): pairs, kernel evaluations and
    the order histogram add up to those of the whole run"""
    import torch
    b, _ = _builder(name, 0.5)
    A0, cnt0, _ = _whole(name, 0.5)
    N, nc = b.dm.num_dofs, b.mesh.num_cells
    cuts = [0, nc//3+29, 2*(nc//3)+7, nc]
    assert all(c % 64 for c in cuts[1:3])
    ctx = b.context()
    A = torch.zeros((N, N), dtype=torch.float64, device='cuda')
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        A.zero_()
        ctx.assemble_dense(A.data_ptr(), N, True, lo, hi)
        ctx.synchronize()
        parts.append(ctx.counters())
        assert parts[-1]['settledTiles'] == 0
    for key in ('numAssembledCellPairs', 'numIntegrations', 'numBoundaryPairs'):
        assert sum(p[key] for p in parts) == cnt0[key], (key, [p[key] for p in parts], cnt0[key])
    orders = {}
    for p in parts:
        for q, n in p['orders'].items():
            orders[q] = orders.get(q, 0)+n
    assert orders == cnt0['orders'], (orders, cnt0['orders'])
    assert {k: sum(p['singular'][k] for p in parts) for k in cnt0['singular']} == cnt0['singular']
