"""The H2 near field, the cluster tree and the H2 product on graded meshes, against the oracle entry by entry.

Every other GPU test of assembleClusters and getH2 builds disc(n), interval(n) or a uniform square: no cluster tile holds cell pairs
whose h differ by more than a factor of 2, no flat rim cell meets k_cluster_boundary, the cluster trees are balanced, and the near
field is held to 1e-11 max|data| only, which checks the entries between DoFs with disjoint supports (90 % of the stored ones, 1e-6 to
1e-2 of max|data| on a graded mesh) to three to nine digits.  The meshes here (tests/graded_meshes.py) move the vertices of disc(n) and
interval(n); eta = 3, minClusterSize = 8 (discs) or 4 (intervals), target_order 0.5 (discs) or p + 1 - s (intervals).

  case         mesh                                element, s                 near / far pairs   stored (separated)   orders
  G1n4-s0.5    graded_disc(4, 'centre', 2.)        P1, 0.5                    541 / 1212          85,446 (79,419)     2 .. 19
  G1n4-s0.4    the same, h ratio 34.8              P1, 0.4                    541 / 1212          85,446 (79,419)     2 .. 18
  G2n4-s0.75   graded_disc(4, 'boundary', 1.5)     P1, 0.75                   454 / 744           61,769 (55,742)     2 .. 19
  G2n4-s0.25r  the same, flat rim cells            P1, 0.25, regional         454 / 744           61,769 (55,742)     2 .. 15
  G1n3-P2      graded_disc(3, 'centre', 2.)        P2, 0.4                    678 / 1084         126,347 (111,608)    3 .. 16
  I6           graded_interval(6, 2.), h ratio 63  P1, 0.75                    22 / 62               341 (218)        4 .. 14
  I6c          graded_interval(6, 3.), ratio 2977  P1, 0.25                    23 / 64               401 (278)        3 .. 11
  I5           graded_interval(5, 2.)              P2, 0.5                     41 / 38               545 (333)        6 .. 16
(stored entries of the symmetric storage; 'regional': zeroExterior=False; orders of the masked distant cell pairs.)

N1  near field, 'tiles' and 'masks', symmetric and unsymmetric storage, every case: pattern equal to the oracle's, counters ('masks':
    equal, 'tiles': >=), 1e-11 max|data| on all entries and the diagonal, and on every separated stored entry (both stored copies of
    the unsymmetric matrix) |gpu - ref| <= tol_ij |ref|, tol_ij = max(1e-12, 2e-14 + 2 P_ij 2^-53), the bound of test_graded_tiles.py.
N2  G1n4 with maxMasksNNZ = 100,000: 15 chunks, the bounds of N1 (counters >=: a cell pair is visited once per chunk that asks for it).
N3  graded_disc(3, 'boundary', 1.5) with target_order 3.5 in 'tiles' mode (on the noRef 4 mesh the oracle's near field takes 63 s on the
    CPU, orders up to 44; here 7 s, orders 4 .. 34): of the 14,463 cluster-local boundary items of the tile plan 12,005 are integrated in
    the lane of k_cluster_boundary (<= 200 point pairs), 1,900 handed over to k_boundary_items, 558 touch; numBoundaryPairs and
    numBoundaryIntegrations equal the item count and the 16,723,362 point pairs of the facet formula, which neither route alone
    accounts for; the bounds of N1.
N4  getDense on I6, I6c, I5 against the whole oracle: 1e-11 max|A| and the per-entry bound on every separated entry.
N5  getH2 on G2n4 (s = 0.75), G1n4 (s = 0.5) and I6: far part of the product against h2_oracle.far_field_dense within
    1e-11 max|F| N (atomic and ordered far field); |H x - A x| / |A x| <= 2 e_oracle + 1e-9, e_oracle the same quantity from the oracle
    alone on the same x; matvec_multi for 1 and 16 vectors with the bits of matvec (ordered far field, the statement of
    tests/test_h2_block.py).
N6  the tree: native host planner == numpy planner on every mesh; with numpy written here (boxes recomputed from the DoF supports):
    near and far blocks tile DoF x DoF once, every far pair satisfies eta dist >= max diam, its parent pair does not, no near pair
    does, nor its parent pairs, nor any pair of leaves below a merged near pair; device planner == host planner on G1n4, G2n4, I6c.

Condition on the inputs, asserted in the CPU tests below, no pair excluded from any comparison: every masked cell pair without a
common vertex and every (cell, facet) item without a common vertex (cluster-local and, for the regional case, global; for N4 all
cell pairs and all cell x boundary vertex items) keeps both ceil() arguments of the oracle's order formula at least 1e-9 (MARGIN of
test_graded_tiles.py) from an integer.  The oracle classifies a cluster facet by nlo_panel_boundary (nlo_assemble_boundary_masked
hands it the item's facet as the only boundary facet): the facet formula of strip_tie_margin.  Smallest margins, cell pairs / items:
G1n4-s0.5 1.5e-6 / 8.8e-6, G1n4-s0.4 3.8e-6 / 3.1e-6, G2n4-s0.75 7.5e-7 / 1.4e-5, G2n4-s0.25r 3.0e-6 / 1.2e-5 (global items 6.9e-6),
G1n3-P2 4.3e-6 / 1.0e-4, I6 1.2e-3 / 3.4e-4, I6c 8.3e-4 / 6.5e-5, I5 2.5e-4 / 1.6e-3; N3 1.2e-5 / 3.0e-4 (over the items of the tile plan); N4 I6 2.4e-4 / 1.9e-3, I6c 2.3e-4 / 1.0e-3, I5 2.5e-4 / 2.2e-2.

The per-entry bound rests on sums of one sign.  All separated entries of the P1 cases and of the intervals are < 0 (asserted).  On
G1n3-P2 they are not: 27,551 of its 111,608 separated entries are positive and the smallest is 2.6e-10 of max|data| (the P2 vertex
functions change sign inside a cell, the contributions cancel), so for these entries tol_ij |ref| is no rounding bound: measured
against it the device is at 19 .. 28 on an entry of 6.9e-10 max|data|, an absolute error of 2e-20 max|data|.  There |ref| gives way to
M_ij >= the sum of the absolute values of the terms (near_magnitudes: |phi| <= 1 and the shape functions of a cell sum to 1, so M_ij
is summed from the oracle's own cell-pair contributions; M_ij / |ref| is 7.7 at least, 9.7 in the median); the ratio against |ref|
itself is printed beside it.

Helpers tied to the oracle without a GPU: near_evaluations is built from pair_evaluations, whose sum over the distant pairs of G1n3 is
the oracle's numIntegrations less the touching pairs' rules; P_ij equals the count of oracle_entries and the oracle's near-field
value has the bits of oracle_entries on >= 2000 seeded separated entries per 2-D case (P_ij 324 .. 86,557).

Measured on an MI355X.  Worst error / tol_ij over the separated stored entries, largest of tiles / masks and sss / csr (the bound is
1), and the largest error over max|data|: G1n4-s0.5 1.2e-3, 2.9e-15; G1n4-s0.4 1.6e-3, 2.9e-15; G2n4-s0.75 1.8e-3, 4.3e-14;
G2n4-s0.25r 1.1e-3, 3.3e-15; G1n3-P2 3.3e-4 (against M_ij), 1.3e-15; I6 4.8e-3, 1.3e-13; I6c 2.7e-2, 1.8e-14; I5 7.0e-3, 2.2e-14;
N2 1.1e-3; N3 9.1e-4 on 8,276 separated entries, 4.2e-15; N4 I6 4.8e-3 (3,660 separated entries from 6.1e-9 max|A|), I6c 2.7e-2
(3,660, from 4.9e-9), I5 7.0e-3 (3,482).  The unsymmetric storage compares twice the separated entries of the table.
N5: far part / bound, atomic and ordered: G2n4 (m = 6, 744 far pairs) 4.5e-5, 2.1e-4; G1n4 (m = 7, 1212) 2.7e-5, 8.1e-5; (e_gpu,
e_oracle) on the three vectors: G2n4 (4.1002e-6, 4.1002e-6), (3.4390e-6, 3.4390e-6), (3.9132e-6, 3.9132e-6); G1n4 (1.1967e-5,
1.1967e-5), (1.2542e-5, 1.2542e-5), (1.0548e-5, 1.0548e-5); I6 (m = 10, 62 far pairs; far part / bound 1.2e-4 atomic and ordered) (3.9014e-7, 3.9014e-7), (3.9807e-7,
3.9807e-7), (4.0104e-7, 4.0104e-7): the largest ratio e_gpu / e_oracle is 1.0000, so the factor 2
of the bound is slack for the truncation of the near field only.
DESIGN.md section 2 has the outcomes of two value-only mutations of the cluster kernels."""
import numpy as np
import pytest

from graded_meshes import (graded_disc, graded_interval, separated, oracle_entries, formula_orders, as_oracle, distant_pair_mask,
                           pair_evaluations, near_evaluations, near_magnitudes, near_tie_margin, facet_item_evaluations, evaluations)
from test_graded_tiles import TOL, MARGIN, entry_tolerance
from test_nearfield import _oracle_near, _to_dense

gpu = pytest.mark.gpu

ETA = 3.
CASES = {
    'G1n4-s0.5': dict(mesh=('disc', 4, 'centre', 2.), element='P1', s=0.5),
    'G1n4-s0.4': dict(mesh=('disc', 4, 'centre', 2.), element='P1', s=0.4),
    'G2n4-s0.75': dict(mesh=('disc', 4, 'boundary', 1.5), element='P1', s=0.75),
    'G2n4-s0.25r': dict(mesh=('disc', 4, 'boundary', 1.5), element='P1', s=0.25, zeroExterior=False),
    'G1n3-P2': dict(mesh=('disc', 3, 'centre', 2.), element='P2', s=0.4),
    'I6': dict(mesh=('interval', 6, 2.), element='P1', s=0.75),
    'I6c': dict(mesh=('interval', 6, 3.), element='P1', s=0.25),
    'I5': dict(mesh=('interval', 5, 2.), element='P2', s=0.5),
    # N3: the cluster-local Gauss-theorem term made expensive, as test_gpu_near_field_heavy_boundary_pairs does
    'G2n3-heavy': dict(mesh=('disc', 3, 'boundary', 1.5), element='P1', s=0.75, target_order=3.5),
}
NEAR_CASES = [c for c in CASES if c != 'G2n3-heavy']
DISC_CASES = [c for c in NEAR_CASES if CASES[c]['mesh'][0] == 'disc']
INTERVAL_CASES = [c for c in NEAR_CASES if CASES[c]['mesh'][0] == 'interval']
ONE_SIGN_CASES = [c for c in CASES if c != 'G1n3-P2']
H2_CASES = ['G2n4-s0.75', 'G1n4-s0.5', 'I6']
CHUNK_NNZ = 100000

_meshes, _dms, _setups, _lists, _evals, _mags, _refs, _dense_refs, _far = {}, {}, {}, {}, {}, {}, {}, {}, {}


def _dm(name):
    """one DoF map per (mesh, element): the cases of one mesh share their cluster tree"""
    from pynucleus_amd import PHYSICAL, dofmapFactory
    c = CASES[name]
    if c['mesh'] not in _meshes:
        _meshes[c['mesh']] = graded_disc(*c['mesh'][1:]) if c['mesh'][0] == 'disc' else graded_interval(*c['mesh'][1:])
    key = (c['mesh'], c['element'])
    if key not in _dms:
        _dms[key] = dofmapFactory(c['element'], _meshes[c['mesh']], PHYSICAL)
    return _dms[key]


def _params(name, **extra):
    c = CASES[name]
    dm = _dm(name)
    target = c.get('target_order', 0.5 if dm.mesh.dim == 2 else dm.polynomialOrder+1.-c['s'])
    return dict({'target_order': target, 'eta': ETA, 'minClusterSize': 8 if dm.mesh.dim == 2 else 4}, **extra)


def _builder(name, **extra):
    from pynucleus_amd import getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    dm = _dm(name)
    return nonlocalBuilder(dm, getFractionalKernel(dm.mesh.dim, CASES[name]['s']), _params(name, **extra),
                           zeroExterior=CASES[name].get('zeroExterior', True))


def _setup(name):
    """(builder, oracle problem, root, Pnear, Pfar) of the case, made once; the tree of the native host planner"""
    from pynucleus_amd import clusters
    if name not in _setups:
        b = _builder(name)
        root, Pnear, Pfar = clusters.getNearFieldClusters(b.dm, ETA, _params(name)['minClusterSize'])
        _setups[name] = (b, as_oracle(b.tables), root, Pnear, Pfar)
    return _setups[name]


def _work_lists(name):
    """what the oracle's near field walks: masked cell pairs, cluster-local boundary items, global boundary items (regional case)"""
    from pynucleus_amd import clusters
    if name not in _lists:
        b, op, root, Pnear, Pfar = _setup(name)
        pairs, masks = clusters.buildMasksForClusters(b.dm, Pnear)
        bc, bf, bm = clusters.clusterBoundaryItems(b.dm, Pnear)
        gb = None if b.tables.zeroExterior else clusters.globalBoundaryItems(b.dm, b.tables.bcells)
        _lists[name] = (pairs, masks, bc, bf, gb)
    return _lists[name]


def _reference(name, symmetric):
    """the oracle's near field of the case in SSS or CSR storage, with the per-entry tolerance of its separated stored entries; made
    once and left unchanged"""
    key = (name, symmetric)
    if key not in _refs:
        b, op, root, Pnear, Pfar = _setup(name)
        pairs, masks = _work_lists(name)[:2]
        indptr, indices, data, diag, cnt = _oracle_near(b.tables, Pnear, symmetric)
        rows = np.repeat(np.arange(b.dm.num_dofs), np.diff(indptr))
        sep = separated(b.dm)[rows, indices]
        if name not in _evals:
            _evals[name] = near_evaluations(op, pairs, masks)
        tol = entry_tolerance(_evals[name][rows, indices][sep])
        if name in ONE_SIGN_CASES:
            mag = np.abs(data[sep])
        else:
            # terms of both signs: the bound of the sum of their absolute values takes the place of |ref|
            if name not in _mags:
                _mags[name] = near_magnitudes(op, pairs)
            mag = _mags[name][rows, indices][sep]
        for a in (indptr, indices, data, diag, tol, mag):
            if a is not None:
                a.setflags(write=False)
        _refs[key] = dict(indptr=indptr, indices=indices, data=data, diag=diag, cnt=cnt, rows=rows, sep=sep, tol=tol, mag=mag,
                          P=_evals[name][rows, indices][sep])
    return _refs[key]


def _all_pairs_and_items(op):
    """N4: what the oracle's whole get_dense classifies: all cell pairs a < b, all cells x boundary facets"""
    T = op.tables
    nc = T.dm.mesh.num_cells
    a, b = np.triu_indices(nc, 1)
    bc = np.asarray(T.bcells).reshape(-1, T.dm.mesh.dim)
    return np.stack([a, b], axis=1), np.repeat(np.arange(nc), bc.shape[0]), np.tile(bc, (nc, 1))


def _dense_reference(name):
    """the oracle's whole operator (N4, N5), made once"""
    if name not in _dense_refs:
        A = _setup(name)[1].get_dense()[0]
        A.setflags(write=False)
        _dense_refs[name] = A
    return _dense_refs[name]


# ---- helpers and the condition on the inputs, without a GPU -----------------------------------------------------------------------

@pytest.mark.parametrize('noRef,mu,ratio', [(6, 2., 63.), (6, 3., 2977.), (5, 2., 31.)])
def test_graded_interval(noRef, mu, ratio):
    """cells, their order and the boundary vertices of interval(noRef); vertices strictly increasing along every cell, the end points
    stay, the mesh is symmetric and the ratio of the longest to the shortest cell is the one the cases are named for"""
    from pynucleus_amd import interval
    base, mesh = interval(noRef), graded_interval(noRef, mu)
    assert np.array_equal(mesh.cells, base.cells) and np.array_equal(mesh.boundaryVertices, base.boundaryVertices)
    x, x0 = mesh.vertices[:, 0], base.vertices[:, 0]
    assert np.array_equal(np.sign(x[mesh.cells[:, 1]]-x[mesh.cells[:, 0]]), np.sign(x0[base.cells[:, 1]]-x0[base.cells[:, 0]]))
    assert x.min() == -1. and x.max() == 1. and np.array_equal(np.sort(x), -np.sort(-x)[::-1])
    h = mesh.hVector
    assert h.min() > 0. and abs(h.max()/h.min()-ratio) <= 1e-9*ratio and abs(h.sum()-2.) <= 1e-14
    assert np.array_equal(graded_interval(noRef, 1.).vertices, base.vertices)


@pytest.mark.parametrize('name', list(CASES))
def test_near_field_inputs_keep_the_tie_margin(name):
    """the condition on the inputs of N1, N2, N3 and N5: masked distant cell pairs, cluster-local and global boundary items"""
    b, op, root, Pnear, Pfar = _setup(name)
    pairs, masks, bc, bf, gb = _work_lists(name)
    mp, npairs, mi, ni = near_tie_margin(op, pairs, bc, bf)
    mg = near_tie_margin(op, pairs[:0], gb[0], gb[1])[2] if gb is not None else np.inf
    d = distant_pair_mask(b.dm.mesh, pairs)
    q = formula_orders(op, pairs[d, 0], pairs[d, 1])
    print('{}: {} near and {} far cluster pairs, {} masked cell pairs ({} distant, orders {}..{}, margin {:.2e}), {} boundary items ({} '
          'distant, margin {:.2e}), global items margin {:.2e}'.format(name, len(Pnear), sum(len(v) for v in Pfar.values()), pairs.shape[0],
                                                                       npairs, q.min(), q.max(), mp, bc.shape[0], ni, mi, mg))
    assert npairs > 100 and ni > 50 and sum(len(v) for v in Pfar.values()) > 30
    assert min(mp, mi, mg) >= MARGIN, (mp, mi, mg)
    assert q.max() <= op.tables.qcap
    if b.dm.mesh.dim == 2:
        assert q.max() >= 15


@pytest.mark.parametrize('name', INTERVAL_CASES)
def test_dense_interval_inputs_keep_the_tie_margin(name):
    """the condition on the inputs of N4: all cell pairs and all cell x boundary vertex items of the oracle's get_dense"""
    b, op = _setup(name)[:2]
    pairs, bc, bf = _all_pairs_and_items(op)
    mp, npairs, mi, ni = near_tie_margin(op, pairs, bc, bf)
    d = distant_pair_mask(b.dm.mesh, pairs)
    q = formula_orders(op, pairs[d, 0], pairs[d, 1])
    nc = b.dm.mesh.num_cells
    print('{}: {} distant cell pairs of orders {}..{}, margin {:.2e}; {} distant items, margin {:.2e}'.format(name, npairs, q.min(), q.max(), mp, ni, mi))
    assert npairs == (nc-1)*(nc-2)//2 and ni == 2*nc-2
    assert min(mp, mi) >= MARGIN, (mp, mi)
    assert q.min() == 2 and 10 <= q.max() <= op.tables.qcap


def test_near_evaluations_count_what_the_oracle_counts():
    """G1n3: pair_evaluations (behind near_evaluations) sums to the oracle's numIntegrations, the distant pairs to its share of them;
    with all the entries of a distant pair requested, P takes its n_q^2 evaluations once per entry"""
    name = 'G1n3-P2'
    b, op, root, Pnear, Pfar = _setup(name)
    pairs, masks = _work_lists(name)[:2]
    cnt = _reference(name, True)['cnt']
    ev, distant = pair_evaluations(op, pairs)
    mesh = b.dm.mesh
    common = (mesh.cells[pairs[:, 0]][:, :, None] == mesh.cells[pairs[:, 1]][:, None, :]).any(axis=2).sum(axis=1)
    touching = sum(int((common == k).sum())*evaluations(op, -k) for k in (1, 2, 3))
    assert distant.sum() == 42230 and (~distant).sum() > 2000
    assert ev.sum() == cnt['numIntegrations'] and ev[distant].sum() == cnt['numIntegrations']-touching
    assert cnt['numAssembledCellPairs'] == cnt['numCellPairs'] == pairs.shape[0]
    # one distant pair with every bit of its mask set
    k = int(np.nonzero(distant)[0][0])
    full = np.zeros((1, 4), dtype=np.uint64)
    nbits = 12*13//2
    full[0, 0], full[0, 1] = np.uint64(2**64-1), np.uint64(2**(nbits-64)-1)
    P = near_evaluations(op, pairs[k:k+1], full)
    ld = np.concatenate([b.dm.dofs[pairs[k, 0]], b.dm.dofs[pairs[k, 1]]])
    ld = ld[ld >= 0]
    want = np.zeros_like(P)
    want[np.ix_(ld, ld)] = ev[k]
    assert np.array_equal(P, want)


@pytest.mark.parametrize('name', DISC_CASES)
def test_oracle_near_field_has_the_bits_of_oracle_entries(name):
    """a seeded sample of >= 2000 separated stored entries: the oracle's near-field value is oracle_entries' sum of the cell-pair
    contributions bit for bit (the masked pairs come in the order of its loops and a cluster pair requests every cell pair of its
    DoF pairs), and P_ij of near_evaluations is its count of kernel evaluations"""
    b, op = _setup(name)[:2]
    ref = _reference(name, True)
    sep = np.nonzero(ref['sep'])[0]
    pick = np.sort(np.random.default_rng(20261021).permutation(sep.size)[:2000])
    ij = np.stack([ref['rows'][sep[pick]], ref['indices'][sep[pick]]], axis=1)
    vals, P = oracle_entries(op, ij)
    got = ref['data'][sep[pick]]
    rel = np.abs(got-vals).max()/np.abs(vals).max()
    print('{}: {} entries, largest difference {:.1e}, P_ij {} .. {}'.format(name, pick.size, rel, P.min(), P.max()))
    assert pick.size == 2000 and np.array_equal(got, vals)
    assert np.array_equal(P, ref['P'][pick])
    # the unsymmetric storage holds the same values at (i, j) and (j, i), with the same P_ij
    full = _reference(name, False)
    A = _to_dense(b.dm.num_dofs, full['indptr'], full['indices'], full['data'], None)
    assert np.array_equal(A[ij[:, 0], ij[:, 1]], vals) and np.array_equal(A[ij[:, 1], ij[:, 0]], vals)
    Pf = np.zeros(A.shape, dtype=np.int64)
    Pf[full['rows'][full['sep']], full['indices'][full['sep']]] = full['P']
    assert np.array_equal(Pf[ij[:, 0], ij[:, 1]], P) and np.array_equal(Pf[ij[:, 1], ij[:, 0]], P)
    assert full['sep'].sum() == 2*ref['sep'].sum()


@pytest.mark.parametrize('name', list(CASES))
def test_separated_entries_are_of_one_sign(name):
    """the premise of the per-entry bound: every separated stored entry is < 0.  It does not hold on G1n3-P2 (module docstring)."""
    ref = _reference(name, True)
    v = ref['data'][ref['sep']]
    scale = max(np.abs(ref['data']).max(), np.abs(ref['diag']).max())
    print('{}: {} stored entries, {} separated, {} positive, |entry| / max|data| from {:.1e} to {:.1e}'.format(
        name, ref['data'].size, v.size, (v > 0.).sum(), np.abs(v).min()/scale, np.abs(v).max()/scale))
    assert v.size >= 0.6*ref['data'].size and np.all(v != 0.)
    if name in ONE_SIGN_CASES:
        assert np.all(v < 0.)
    else:
        assert (v > 0.).sum() == 27551 and v.size == 111608
        # ... where near_magnitudes bounds the absolute terms: at least |entry|, and for most entries not much more
        mag = ref['mag']
        print('{}: M_ij / |entry| from {:.3f} to {:.1e}, median {:.2f}; M_ij / max|data| from {:.1e}'.format(
            name, (mag/np.abs(v)).min(), (mag/np.abs(v)).max(), np.median(mag/np.abs(v)), mag.min()/scale))
        assert np.all(mag >= np.abs(v)) and np.median(mag/np.abs(v)) < 20.
    if name in INTERVAL_CASES:
        # N4: the separated entries of the whole operator
        A = _dense_reference(name)
        assert np.all(A[separated(_dm(name))] < 0.)


# ---- N6 without a GPU: the tree ---------------------------------------------------------------------------------------------------

TREE_CASES = ['G1n4-s0.5', 'G2n4-s0.75', 'G1n3-P2', 'I6', 'I6c', 'I5']          # one per (mesh, element)


@pytest.mark.parametrize('name', TREE_CASES)
def test_native_planner_equals_numpy_on_graded_meshes(name):
    """the comparison of test_native_planner_equals_numpy: same clusters in the same order, same tile work lists, same far-field plan"""
    from test_plan_native import _both, PLAN_ARRAYS
    dm = _dm(name)
    minSize = _params(name)['minClusterSize']
    (r0, n0, f0, p0, h0), (r1, n1, f1, p1, h1) = _both(dm, minSize, 64 if CASES[name]['element'] == 'P1' else 32, eta=ETA)
    assert len(n0) == len(n1) == len(_setup(name)[3])
    for a, b in zip(n0, n1):
        assert np.array_equal(a.n1.dofs, b.n1.dofs) and np.array_equal(a.n2.dofs, b.n2.dofs)
        assert np.array_equal(a.n1.cells, b.n1.cells) and np.array_equal(a.cellsInter, b.cellsInter) and np.array_equal(a.cellsUnion, b.cellsUnion)
        assert np.array_equal(a.n1.box, b.n1.box)
    assert sorted(f0) == sorted(f1) and sum(len(v) for v in f0.values()) > 30
    for lvl in f0:
        assert len(f0[lvl]) == len(f1[lvl])
        for a, b in zip(f0[lvl], f1[lvl]):
            assert np.array_equal(a.n1.dofs, b.n1.dofs) and np.array_equal(a.n2.dofs, b.n2.dofs)
    for arr in PLAN_ARRAYS:
        x, y = getattr(p0, arr), getattr(p1, arr)
        assert x.shape == y.shape and np.array_equal(x, y), arr
    for s in range(3):
        assert np.array_equal(p0.sing_items[s], p1.sing_items[s])
    assert p0.nU == p1.nU and p0.num_dslots == p1.num_dslots
    assert h0.box.shape == h1.box.shape and h0.far.shape == h1.far.shape
    k0 = {tuple(np.round(h0.box[k].ravel(), 12)): k for k in range(h0.box.shape[0])}
    for k in range(h1.box.shape[0]):
        j = k0[tuple(np.round(h1.box[k].ravel(), 12))]
        assert np.abs(h0.transfer[j]-h1.transfer[k]).max() <= 1e-13
        assert h0.level[j] == h1.level[k]


def _support_boxes(dm):
    """[N, dim] lower and upper corners of the DoF supports, from the vertices of the cells that hold the DoF"""
    v = dm.mesh.vertices[dm.mesh.cells]
    lo, hi = v.min(axis=1), v.max(axis=1)
    N, dim = dm.num_dofs, dm.mesh.dim
    blo, bhi = np.full((N, dim), np.inf), np.full((N, dim), -np.inf)
    dofs = np.asarray(dm.dofs)
    for k in range(dofs.shape[1]):
        m = dofs[:, k] >= 0
        np.minimum.at(blo, dofs[m, k], lo[m])
        np.maximum.at(bhi, dofs[m, k], hi[m])
    return blo, bhi


@pytest.mark.parametrize('name', TREE_CASES)
def test_admissibility_on_graded_meshes(name):
    """plain numpy, nothing of clusters.py but the lists under test.  Boxes of the clusters from the DoF supports.  Near and far
    blocks tile DoF x DoF exactly once; every far pair is admissible (eta dist >= max diam) and as large as possible (the pair the
    recursion came from is not); no near pair is admissible, so none of its parent pairs is (asserted on its own); below a near
    pair of non-leaves no pair of leaves is admissible (why the block was merged).  Where h is graded (G1, the intervals) the leaf boxes differ in
    size by more than a factor of 2."""
    dm = _dm(name)
    root, Pnear, Pfar = _setup(name)[2:]
    N = dm.num_dofs
    blo, bhi = _support_boxes(dm)
    slack = 1e-12

    def box(n):
        d = np.asarray(n.dofs)
        return blo[d].min(axis=0), bhi[d].max(axis=0)

    def fails(n1, n2, sign=-1.):
        (l1, h1), (l2, h2) = box(n1), box(n2)
        gap = np.maximum(0., np.maximum(l1-h2, l2-h1))
        dist = np.sqrt((gap**2).sum())
        diam = max(np.sqrt(((h1-l1)**2).sum()), np.sqrt(((h2-l2)**2).sum()))
        return ETA*dist < diam*(1.+slack) if sign < 0 else ETA*dist >= diam*(1.-slack)

    def leaves(n):
        return [n] if n.is_leaf else [l for c in n.children for l in leaves(c)]

    cover = np.zeros((N, N), dtype=np.int32)
    for cp in list(Pnear)+[cp for v in Pfar.values() for cp in v]:
        cover[np.ix_(cp.n1.dofs, cp.n2.dofs)] += 1
    assert cover.min() == 1 and cover.max() == 1
    assert np.array_equal(box(root)[0], np.asarray(root.box)[:, 0]) and np.array_equal(box(root)[1], np.asarray(root.box)[:, 1])
    nfar = 0
    for lvl, plist in Pfar.items():
        for cp in plist:
            nfar += 1
            assert fails(cp.n1, cp.n2, +1.), (lvl, cp.n1.dofs, cp.n2.dofs)
            assert lvl >= 1 and max(cp.n1.levelNo, cp.n2.levelNo) == lvl
            p1 = cp.n1.parent if cp.n1.levelNo == lvl else cp.n1
            p2 = cp.n2.parent if cp.n2.levelNo == lvl else cp.n2
            assert fails(p1, p2), (lvl, cp.n1.dofs, cp.n2.dofs)
    merged = 0
    for cp in Pnear:
        assert fails(cp.n1, cp.n2)
        for p1, p2 in ((cp.n1.parent, cp.n2.parent), (cp.n1, cp.n2.parent), (cp.n1.parent, cp.n2)):
            if p1 is not None and p2 is not None:
                assert fails(p1, p2)
        if not (cp.n1.is_leaf and cp.n2.is_leaf):
            merged += 1
            for a in leaves(cp.n1):
                for b in leaves(cp.n2):
                    assert fails(a, b)
    diam = [np.sqrt(((box(l)[1]-box(l)[0])**2).sum()) for l in leaves(root)]
    print('{}: {} near pairs ({} of non-leaves), {} far pairs on levels {}..{}, diameters of the leaf boxes {:.2e} .. {:.2e}'.format(
        name, len(Pnear), merged, nfar, min(Pfar), max(Pfar), min(diam), max(diam)))
    assert nfar > 30 and len(Pfar) >= 2
    if not name.startswith('G2'):
        assert max(diam) > 2.*min(diam)


# ---- N1 .. N3: the near field against the oracle ----------------------------------------------------------------------------------

def _compare_near(name, Anear, symmetric, exact_counters, what):
    """pattern, counters, 1e-11 max|data| and the per-entry bound on every separated stored entry; prints the figures first"""
    ref = _reference(name, symmetric)
    assert np.array_equal(Anear.indptr, ref['indptr']) and np.array_equal(Anear.indices, ref['indices'])
    data, diag, sep = ref['data'], ref['diag'], ref['sep']
    scale = max(np.abs(data).max(), np.abs(diag).max() if symmetric else 0.)
    got = np.asarray(Anear.data)
    err = np.abs(got-data).max()/scale
    errd = np.abs(np.asarray(Anear.diagonal)-diag).max()/scale if symmetric else 0.
    ratio = np.abs(got[sep]-data[sep])/(ref['tol']*ref['mag'])
    literal = (np.abs(got[sep]-data[sep])/(ref['tol']*np.abs(data[sep]))).max()
    k = int(ratio.argmax())
    cnt, want = Anear.info['counters'], ref['cnt']
    print('{} {}: {} stored entries, max err {:.2e} max|data| (diagonal {:.2e}), {} separated entries, worst err/tol {:.3e} (P_ij {}, '
          '|ref| {:.1e} max|data|; against |ref| itself {:.3e}), numCellPairs {} / {}, numAssembledCellPairs {} / {}'.format(
              name, what, data.size, err, errd, sep.sum(), ratio[k], ref['P'][k], abs(data[sep][k])/scale, literal, cnt['numCellPairs'],
              want['numCellPairs'], cnt['numAssembledCellPairs'], want['numAssembledCellPairs']))
    if Anear.info.get('mode') == 'tiles':
        assert cnt['numAssembledCellPairs'] >= want['numAssembledCellPairs']
    else:
        for key in ('numCellPairs', 'numAssembledCellPairs'):
            assert (cnt[key] == want[key]) if exact_counters else (cnt[key] >= want[key]), (key, cnt[key], want[key])
    assert err <= TOL and errd <= TOL, (err, errd)
    assert ratio[k] <= 1., (ratio[k], ref['rows'][sep][k], ref['indices'][sep][k], data[sep][k], got[sep][k], ref['P'][k])
    return ratio[k]


@gpu
@pytest.mark.parametrize('symmetric', [True, False], ids=['sss', 'csr'])
@pytest.mark.parametrize('mode', ['tiles', 'masks'])
@pytest.mark.parametrize('name', NEAR_CASES)
def test_gpu_graded_near_field_against_oracle(name, mode, symmetric):
    """N1"""
    b = _builder(name, nearFieldAssembly=mode)
    Pnear = _setup(name)[3]
    Anear = b.assembleClusters(Pnear, forceUnsymmetricMatrix=not symmetric)
    assert Anear.info.get('mode', 'masks') == mode
    _compare_near(name, Anear, symmetric, True, mode+(' sss' if symmetric else ' csr'))


@gpu
@pytest.mark.parametrize('symmetric', [True, False], ids=['sss', 'csr'])
def test_gpu_graded_near_field_in_chunks(symmetric):
    """N2"""
    from pynucleus_amd import clusters
    name = 'G1n4-s0.5'
    b = _builder(name, maxMasksNNZ=CHUNK_NNZ)
    Pnear = _setup(name)[3]
    nchunks = sum(1 for _ in clusters.iterMasksForClusters(b.dm, Pnear, CHUNK_NNZ))
    assert nchunks >= 4, nchunks
    Anear = b.assembleClusters(Pnear, forceUnsymmetricMatrix=not symmetric)
    assert Anear.info.get('mode', 'masks') == 'masks'
    _compare_near(name, Anear, symmetric, False, '{} chunks'.format(nchunks))


def _heavy_items(name):
    """the (cell, facet) items of the tiled cluster-local boundary term: per UNORDERED cluster pair {n1, n2} (clusters.nearFieldPlan
    takes the pairs (n1, n2) and (n2, n1) of the list as one, with one diagonal-block slot per cell of cellsInter) every cell of
    cellsInter x the boundary facets of cellsUnion"""
    from pynucleus_amd import clusters
    b, op, root, Pnear, Pfar = _setup(name)
    cc, ff, seen = [], [], set()
    for cp in Pnear:
        # a node of the tree is known by its smallest DoF and its size
        key = frozenset((int(n.dofs.min()), int(n.dofs.shape[0])) for n in (cp.n1, cp.n2))
        ci = np.asarray(cp.cellsInter)
        if ci.shape[0] == 0 or key in seen:
            continue
        seen.add(key)
        facets = clusters.boundaryFacetsOfCells(b.dm.mesh, cp.cellsUnion)
        cc.append(np.repeat(ci, facets.shape[0]))
        ff.append(np.tile(facets, (ci.shape[0], 1)))
    return np.concatenate(cc), np.concatenate(ff)


def test_heavy_boundary_items_take_both_routes():
    """N3 without a GPU: by the facet formula, items on both sides of the 200 point pairs above which k_cluster_boundary hands an item
    to k_boundary_items, all of them with the tie margin"""
    name = 'G2n3-heavy'
    op = _setup(name)[1]
    cc, ff = _heavy_items(name)
    ev, distant = facet_item_evaluations(op, cc, ff)
    margin = near_tie_margin(op, np.zeros((0, 2)), cc, ff)[2]
    print('{}: {} items, {} touching, {} of <= 200 point pairs, {} of more, {} point pairs, margin {:.2e}'.format(
        name, cc.size, (~distant).sum(), (ev[distant] <= 200).sum(), (ev[distant] > 200).sum(), ev.sum(), margin))
    assert margin >= MARGIN
    assert (ev[distant] <= 200).sum() > 1000 and (ev[distant] > 200).sum() > 1000 and (~distant).sum() > 500


@gpu
def test_gpu_graded_near_field_heavy_boundary_items():
    """N3"""
    name = 'G2n3-heavy'
    b = _builder(name, nearFieldAssembly='tiles')
    op, Pnear = _setup(name)[1], _setup(name)[3]
    Anear = b.assembleClusters(Pnear)
    assert Anear.info['mode'] == 'tiles'
    c = Anear.info['counters']
    cc, ff = _heavy_items(name)
    ev, distant = facet_item_evaluations(op, cc, ff)
    # 200: `defer` of clusters_tiled_impl (csrc/pnl_hip.hip), the point pairs above which k_cluster_boundary leaves an item, uncounted,
    # to k_boundary_items; each kernel counts the items it integrates itself
    lane, wave = ev[distant & (ev <= 200)], ev[distant & (ev > 200)]
    print('{}: numBoundaryPairs {} (items {}), numBoundaryIntegrations {} (formula {}: in the lane {} items / {} point pairs, one per wave '
          '{} / {}, touching {} / {})'.format(name, c['numBoundaryPairs'], cc.size, c['numBoundaryIntegrations'], ev.sum(), lane.size,
                                              lane.sum(), wave.size, wave.sum(), (~distant).sum(), ev[~distant].sum()))
    # both routes ran: the counters hold every item and every point pair, and neither route alone accounts for them
    assert lane.size > 0 and wave.size > 0
    assert c['numBoundaryPairs'] == cc.size and c['numBoundaryIntegrations'] == ev.sum()
    _compare_near(name, Anear, True, True, 'tiles sss, target_order 3.5')


# ---- N4: the dense operator on graded intervals -----------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', INTERVAL_CASES)
def test_gpu_graded_interval_dense_against_oracle(name):
    from graded_meshes import strip_evaluations
    b, op = _setup(name)[:2]
    A = _builder(name).getDense().toarray()
    Aref = _dense_reference(name)
    sep = separated(b.dm)
    tol = entry_tolerance(strip_evaluations(op, 0, b.dm.mesh.num_cells)[sep])
    err = np.abs(A-Aref).max()/np.abs(Aref).max()
    ratio = np.abs(A[sep]-Aref[sep])/(tol*np.abs(Aref[sep]))
    print('{} getDense: max err {:.2e} max|A|, {} separated entries, worst err/tol {:.3e}, |entry| from {:.1e} max|A|'.format(
        name, err, sep.sum(), ratio.max(), np.abs(Aref[sep]).min()/np.abs(Aref).max()))
    assert np.abs(Aref-Aref.T).max() == 0. and np.linalg.eigvalsh(Aref).min() > 0.
    assert err <= TOL, err
    assert ratio.max() <= 1., ratio.max()


# ---- N5: the H2 product -----------------------------------------------------------------------------------------------------------

def _same_pairs(P0, P1):
    return len(P0) == len(P1) and all(np.array_equal(a.n1.dofs, b.n1.dofs) and np.array_equal(a.n2.dofs, b.n2.dofs) for a, b in zip(P0, P1))


@gpu
@pytest.mark.parametrize('name', H2_CASES)
def test_gpu_graded_h2_product(name):
    from pynucleus_amd.quadrature import simplexXiaoGimbutas
    from pynucleus_amd.h2 import H2Matrix
    from oracle import h2_oracle
    b = _builder(name)
    dm = b.dm
    N, dim = dm.num_dofs, dm.mesh.dim
    h2, Pnear, root = b.getH2(returnNearField=True, returnTree=True)
    assert isinstance(h2, H2Matrix) and h2.farField == 'atomic' and h2.plan.far.shape[0] >= 60
    # the tree of getH2 is the tree of the case: the oracle's near field of N1 is the reference of this one
    assert _same_pairs(Pnear, _setup(name)[3])
    far0 = [cp for lvl in sorted(_setup(name)[4]) for cp in _setup(name)[4][lvl]]
    assert _same_pairs([cp for lvl in sorted(h2.Pfar) for cp in h2.Pfar[lvl]], far0)
    m = h2.plan.m
    if name not in _far:
        _far[name] = (m, h2_oracle.far_field_dense(dm, b.kernel, root, h2.Pfar, m, simplexXiaoGimbutas(m+dm.polynomialOrder+1, dim, dim)))
    assert _far[name][0] == m
    F = _far[name][1]
    ref = _reference(name, False)
    near = _to_dense(N, ref['indptr'], ref['indices'], ref['data'], None)
    Ao = _dense_reference(name)
    A = b.getDense().toarray()
    rng = np.random.default_rng(20261021)
    X = rng.standard_normal((16, N))
    # (a) the far part of the product, atomic and ordered
    bound = 1e-11*np.abs(F).max()*N
    worst = {}
    for mode in ('atomic', 'ordered'):
        h2.farField = mode
        worst[mode] = max(np.abs(h2.matvec(X[v])-h2.Anear.matvec(X[v])-F@X[v]).max() for v in range(3))/bound
    print('{}: m = {}, {} far pairs, max|F| {:.3e}, far part against the oracle / bound: atomic {:.3e}, ordered {:.3e}'.format(
        name, m, h2.plan.far.shape[0], np.abs(F).max(), worst['atomic'], worst['ordered']))
    # (b) against the dense operator
    h2.farField = 'atomic'
    e_oracle = [np.linalg.norm((near+F)@X[v]-Ao@X[v])/np.linalg.norm(Ao@X[v]) for v in range(3)]
    e_each = [np.linalg.norm(h2.matvec(X[v])-A@X[v])/np.linalg.norm(A@X[v]) for v in range(3)]
    print('{}: e_gpu {} e_oracle {} largest ratio {:.4f}'.format(name, ['%.4e' % e for e in e_each], ['%.4e' % e for e in e_oracle],
                                                                 max(g/o for g, o in zip(e_each, e_oracle))))
    # (c) blocks of vectors, ordered far field: the bits of matvec
    h2.farField = 'ordered'
    same = True
    for nvec in (1, 16):
        Y = h2.matvec_multi(X[:nvec])
        assert Y.shape == (nvec, N)
        same = same and all(np.array_equal(Y[v], h2.matvec(X[v])) for v in range(nvec))
    assert worst['atomic'] <= 1. and worst['ordered'] <= 1., worst
    for g, o in zip(e_each, e_oracle):
        assert g <= 2.*o+1e-9, (g, o)
    assert same, 'matvec_multi and matvec differ in the ordered mode'


# ---- N6 on the device -------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', ['G1n4-s0.5', 'G2n4-s0.75', 'I6c'])
def test_gpu_device_planner_equals_host_planner_on_graded_meshes(name):
    """the comparison of test_device_planner_equals_host_planner"""
    from pynucleus_amd import clusters
    dm = _dm(name)
    minSize = _params(name)['minClusterSize']
    H = clusters._nativeTree(dm, ETA, minSize, 200, 1, refinementType='MEDIAN', planner='host')
    D = clusters._nativeTree(dm, ETA, minSize, 200, 1, refinementType='MEDIAN', planner='device')
    assert H.planner == 'host' and D.planner == 'device'
    for arr in ('range', 'parent', 'children', 'level', 'perm'):
        assert np.array_equal(getattr(H, arr), getattr(D, arr)), arr
    assert np.array_equal(H.box, D.box)
    assert H.near.shape[0] == len(_setup(name)[3]) and np.array_equal(H.near, D.near)
    assert H.far.shape[0] > 30 and np.array_equal(H.far, D.far)
    print('{}: {} nodes on levels 0..{}, {} near and {} far pairs'.format(name, H.level.shape[0], H.level.max(), H.near.shape[0], H.far.shape[0]))
