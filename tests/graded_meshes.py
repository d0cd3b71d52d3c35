"""Helpers of tests/test_graded_tiles.py: graded discs, single matrix entries from the oracle, the tie margin of the order formula.

The graded discs keep the cells of disc(noRef) and move its vertices, so the block structure of the tile plan is that of the
quasi-uniform disc while the longest edge h varies over the mesh (kind 'centre') or the cells at the rim are flat (kind 'boundary').
Nothing here needs a GPU; the CPU tests of these helpers are in tests/test_graded_tiles.py."""
import copy

import numpy as np
import scipy.sparse as sp

from oracle.oracle import OracleProblem, IGNORED
from test_small_entries import _separated
from test_device_math import _order_args


def graded_disc(noRef, kind, mu):
    """disc(noRef) with every vertex moved along its ray: 'centre' v -> v |v|^(mu - 1) (r -> r^mu, cells shrink towards the
    origin), 'boundary' r -> 1 - (1 - r)^mu (cells flatten towards the rim).  Cells, their order and the boundary lists are kept."""
    from pynucleus_amd import disc
    base = disc(noRef)
    v = np.array(base.vertices, dtype=np.float64)
    r = np.sqrt((v**2).sum(axis=1))
    if kind == 'centre':
        new_r = r**mu
    elif kind == 'boundary':
        new_r = 1.-(1.-np.minimum(r, 1.))**mu
    else:
        raise ValueError(kind)
    scale = np.where(r > 0., new_r/np.where(r > 0., r, 1.), 0.)
    mesh = copy.copy(base)
    mesh.vertices = np.ascontiguousarray(v*scale[:, None])
    mesh.setMeshTransformation(None)
    mesh.resetMeshInfo()
    return mesh


def signed_areas(mesh):
    v = mesh.vertices[mesh.cells]
    a, b = v[:, 1]-v[:, 0], v[:, 2]-v[:, 0]
    return 0.5*(a[:, 0]*b[:, 1]-a[:, 1]*b[:, 0])


def edge_lengths(mesh):
    """[nc, 3] edge lengths of the cells"""
    v = mesh.vertices[mesh.cells]
    return np.stack([np.linalg.norm(v[:, a]-v[:, b], axis=1) for a, b in ((0, 1), (0, 2), (1, 2))], axis=1)


def cell_quality(mesh):
    """4 sqrt(3) area / sum of the squared edges: 1 for the equilateral triangle"""
    return 4.*np.sqrt(3.)*np.abs(signed_areas(mesh))/(edge_lengths(mesh)**2).sum(axis=1)


def separated(dm):
    """mask of the DoF pairs whose supports share no vertex (tests/test_small_entries.py)"""
    return _separated(dm)


def supports(dm):
    """list over the DoFs of (cells, local indices) of the support, cells ascending"""
    dofs = np.asarray(dm.dofs)
    nc, dpe = dofs.shape
    c, k = np.nonzero(dofs >= 0)
    d = dofs[c, k]
    order = np.lexsort((c, d))
    c, k, d = c[order], k[order], d[order]
    cut = np.searchsorted(d, np.arange(dm.num_dofs+1))
    return [(c[cut[i]:cut[i+1]], k[cut[i]:cut[i+1]]) for i in range(dm.num_dofs)]


def as_oracle(T):
    return T if isinstance(T, OracleProblem) else OracleProblem(T)


def evaluations(op, panel):
    """kernel evaluations of one cell pair of that panel (the oracle's numIntegrations counts them)"""
    T = op.tables
    if panel >= 1:
        return int(T.dist_off[panel+1]-T.dist_off[panel])**2
    return int(T.singular[panel].num_nodes)


def oracle_entries(T, ij, cell_range=None, with_pairs=False):
    """Reference values A[i, j] for DoF pairs (i, j) that share no cell, and P_ij, the number of kernel evaluations behind each.

    The entry is the sum over the cell pairs (ca, cb), ca in the support of i, cb in the support of j, of the oracle's contribution of
    the pair (c1, c2) = (min, max) at the local position (i's or j's place in c1, dpe + the other's place in c2), times 2 for
    c1 != c2: the scatter of nl_oracle.c (scatter_elem_elem_sym), walked in the order of its loops (c1 ascending, then c2), so
    the sum has the bits of get_dense.  cell_range = (c0, c1) keeps the pairs whose first cell lies in it, like get_dense(c0, c1).
    No boundary term reaches such an entry (the Omega x Omega^c term couples the DoFs of one cell only).
    with_pairs: also the list of (c1, c2, panel) per entry."""
    op = as_oracle(T)
    dm = op.tables.dm
    dpe = int(np.asarray(dm.dofs).shape[1])
    n2 = 2*dpe
    sup = supports(dm)
    lo, hi = (0, dm.mesh.num_cells) if cell_range is None else cell_range
    cache = {}
    vals, evals, pairs_out = np.zeros(len(ij)), np.zeros(len(ij), dtype=np.int64), []
    for n, (i, j) in enumerate(ij):
        (ci, ki), (cj, kj) = sup[int(i)], sup[int(j)]
        assert np.intersect1d(ci, cj).size == 0, 'DoFs {} and {} share a cell'.format(i, j)
        terms = []
        for a, ka in zip(ci, ki):
            for b, kb in zip(cj, kj):
                terms.append((int(a), int(b), int(ka), int(kb)) if a < b else (int(b), int(a), int(kb), int(ka)))
        terms.sort()
        acc, count, plist = 0., 0, []
        for c1, c2, p, q in terms:
            if not lo <= c1 < hi:
                continue
            if (c1, c2) not in cache:
                cache[(c1, c2)] = op.eval(c1, c2)
            panel, contrib = cache[(c1, c2)]
            if panel == IGNORED:
                continue
            q += dpe
            acc += 2.*contrib[n2*p-(p*(p+1) >> 1)+q]
            count += evaluations(op, panel)
            plist.append((c1, c2, panel))
        vals[n], evals[n] = acc, count
        pairs_out.append(plist)
    return (vals, evals, pairs_out) if with_pairs else (vals, evals)


def oracle_centres(mesh):
    """cell centres as nl_oracle.c forms them: (v0 + v1 + v2) * (1 / 3); on an interval (v0 + v1) * (1 / 2)"""
    v = mesh.vertices[mesh.cells]
    if v.shape[1] == 2:
        return (v[:, 0]+v[:, 1])*(1./2.)
    return (v[:, 0]+v[:, 1]+v[:, 2])*(1./3.)


def _dist2(diff):
    """squared length of the rows, summed over the coordinates in the order of nl_oracle.c"""
    d2 = diff[:, 0]*diff[:, 0]
    for j in range(1, diff.shape[1]):
        d2 = d2+diff[:, j]*diff[:, j]
    return d2


def _margin(a1, a2):
    return np.minimum(np.abs(a1-np.rint(a1)), np.abs(a2-np.rint(a2)))


def pair_tie_margin(T, c1, c2):
    """distance to the nearest integer of the two ceil() arguments of the oracle's order formula (its d = distance of the cell
    centres, its h = longest edges, its H0), per cell pair"""
    op = as_oracle(T)
    mesh = op.tables.dm.mesh
    cen, h = oracle_centres(mesh), mesh.hVector
    return _margin(*_order_args(op.tables.qo, h[c1], h[c2], _dist2(cen[c1]-cen[c2]), op.tables.H0))


def _cell_vertex_incidence(mesh):
    nc, nV = np.asarray(mesh.cells).shape
    return sp.csr_matrix((np.ones(nV*nc), (np.repeat(np.arange(nc), nV), np.asarray(mesh.cells).ravel())), shape=(nc, mesh.num_vertices))


def strip_distant_pairs(T, c0, c1):
    """the distant cell pairs (a, b) of the oracle's strip get_dense(c0, c1): c0 <= a < c1, a < b, no common vertex"""
    mesh = as_oracle(T).tables.dm.mesh
    inc = _cell_vertex_incidence(mesh)
    a, b = np.nonzero(~((inc[c0:c1]@inc.T).toarray() > 0))
    keep = b > a+c0
    return a[keep]+c0, b[keep]


def formula_orders(T, a, b):
    """max(ceil(a1), ceil(a2), 2) of the oracle's formula arguments for the cell pairs (a, b): the oracle's order wherever
    pair_tie_margin is far above the rounding of a logarithm"""
    op = as_oracle(T)
    mesh = op.tables.dm.mesh
    cen, h = oracle_centres(mesh), mesh.hVector
    a1, a2 = _order_args(op.tables.qo, h[a], h[b], _dist2(cen[a]-cen[b]), op.tables.H0)
    return np.maximum(np.maximum(np.ceil(a1), np.ceil(a2)), 2.).astype(np.int64)


def strip_evaluations(T, c0, c1):
    """P[i, j] for every DoF pair: the kernel evaluations of the distant cell pairs of the strip that reach the entry (i, j) --
    what oracle_entries(T, ij, (c0, c1)) returns per entry, for the whole matrix at once.  Exact for separated DoF pairs (all
    their cell pairs are distant)."""
    op = as_oracle(T)
    dm = op.tables.dm
    nc, N = dm.mesh.num_cells, dm.num_dofs
    a, b = strip_distant_pairs(op, c0, c1)
    q = formula_orders(op, a, b)
    off = np.asarray(op.tables.dist_off, dtype=np.int64)
    E = np.zeros((c1-c0, nc))
    E[a-c0, b] = (off[q+1]-off[q])**2
    dofs = np.asarray(dm.dofs)
    c, k = np.nonzero(dofs >= 0)
    S = sp.csr_matrix((np.ones(c.size), (c, dofs[c, k])), shape=(nc, N))
    half = S[c0:c1].T@(S.T@E.T).T                       # [N, N]: a in the support of the row DoF, b in that of the column DoF
    return np.rint(half+half.T).astype(np.int64)


def formula_counters(T, rows=512):
    """The integer counters of the oracle's whole get_dense() without its kernel evaluations: every cell pair a <= b with a DoF is
    classified by its common vertices (identical / touching pairs) or, without one, by formula_orders.  Returns (counters,
    smallest tie margin over the distant pairs); the counters are the oracle's wherever that margin is far above the rounding of a
    logarithm (a CPU test compares them with get_dense on a small mesh)."""
    op = as_oracle(T)
    Tb = op.tables
    dm, mesh = Tb.dm, Tb.dm.mesh
    nc = mesh.num_cells
    inc = _cell_vertex_incidence(mesh)
    has = (np.asarray(dm.dofs) >= 0).any(axis=1)
    cen, h = oracle_centres(mesh), mesh.hVector
    off = np.asarray(Tb.dist_off, dtype=np.int64)
    hist = np.zeros(off.shape[0], dtype=np.int64)
    sing = {-1: 0, -2: 0, -3: 0}
    margin = np.inf
    for c0 in range(0, nc, rows):
        c1 = min(nc, c0+rows)
        common = np.rint((inc[c0:c1]@inc.T).toarray()).astype(np.int64)
        A, B = np.arange(c0, c1)[:, None], np.arange(nc)[None, :]
        valid = (B >= A) & (has[A] | has[B])
        for k in (1, 2, 3):
            sing[-k] += int((valid & (common == k)).sum())
        a, b = np.nonzero(valid & (common == 0))
        a += c0
        diff = cen[a]-cen[b]
        a1, a2 = _order_args(Tb.qo, h[a], h[b], diff[:, 0]*diff[:, 0]+diff[:, 1]*diff[:, 1], Tb.H0)
        margin = min(margin, float(_margin(a1, a2).min()))
        q = np.maximum(np.maximum(np.ceil(a1), np.ceil(a2)), 2.).astype(np.int64)
        assert q.max() <= Tb.qcap
        hist += np.bincount(q, minlength=hist.shape[0])
    npts = off[1:]-off[:-1]
    orders = {int(q): int(n) for q, n in enumerate(hist) if n}
    evals = sum(n*int(npts[q])**2 for q, n in orders.items())+sum(n*evaluations(op, p) for p, n in sing.items())
    return dict(numAssembledCellPairs=sum(orders.values())+sum(sing.values()), numIntegrations=evals, orders=orders, singular=sing), margin


def strip_tie_margin(T, c0, c1):
    """smallest margin over the distant pairs the oracle's strip get_dense(c0, c1) classifies: cell pairs (a, b), c0 <= a < c1,
    a < b, without a common vertex, and (with the Omega x Omega^c term) cell x boundary facet without a common vertex.  Returns
    (margin, number of pairs)."""
    op = as_oracle(T)
    Tb = op.tables
    mesh = Tb.dm.mesh
    nv = mesh.num_vertices
    inc = _cell_vertex_incidence(mesh)
    a, b = strip_distant_pairs(op, c0, c1)
    worst, count = pair_tie_margin(op, a, b).min(), a.size
    if Tb.zeroExterior:
        bc = np.asarray(Tb.bcells)
        finc = sp.csr_matrix((np.ones(bc.size), (np.repeat(np.arange(bc.shape[0]), 2), bc.ravel())), shape=(bc.shape[0], nv))
        a, f = np.nonzero(~((inc[c0:c1]@finc.T).toarray() > 0))
        a = a+c0
        v = mesh.vertices[bc]
        fcen = (v[:, 0]+v[:, 1])*0.5
        flen = np.sqrt((v[:, 1, 0]-v[:, 0, 0])**2+(v[:, 1, 1]-v[:, 0, 1])**2)
        diff = oracle_centres(mesh)[a]-fcen[f]
        d2 = diff[:, 0]*diff[:, 0]+diff[:, 1]*diff[:, 1]
        worst = min(worst, _margin(*_order_args(Tb.bqo, mesh.hVector[a], flen[f], d2, Tb.H0)).min())
        count += a.size
    return float(worst), int(count)


def strips(mesh, block, pad):
    """the two cell strips of a mesh: two full blocks of `block` cells plus `pad` cells on either side, (c0, c1) =
    (block k - pad, block (k + 2) + pad); one holds a cell of the smallest h (the first such cell whose strip fits), one nc // 2"""
    nc, h = mesh.num_cells, mesh.hVector
    nb = nc//block
    small = [int(c)//block for c in np.nonzero(h <= h.min()*(1.+1e-9))[0]]
    ks = [k for k in small if 1 <= k <= nb-3]+[k-1 for k in small if 1 <= k-1 <= nb-3]
    out = []
    for k in (ks[0], (nc//2)//block):
        out.append((block*k-pad, block*(k+2)+pad))
    c0, c1 = out[0]
    assert h[c0+pad:c1-pad].min() <= h.min()*(1.+1e-9)
    return out


# ---- helpers of tests/test_graded_nearfield.py: graded intervals, the masked cell pairs and boundary items of a near field ----------

def graded_interval(noRef, mu):
    """interval(noRef) on [-1, 1] with every vertex moved by x -> sign(x) (1 - (1 - |x|)^mu): cells shrink towards both end points
    (longest over shortest cell: 2^noRef - 1 for mu = 2).  Cells, their order and the boundary vertices are kept."""
    from pynucleus_amd import interval
    base = interval(noRef)
    x = np.array(base.vertices, dtype=np.float64)
    mesh = copy.copy(base)
    mesh.vertices = np.ascontiguousarray(np.sign(x)*(1.-(1.-np.minimum(np.abs(x), 1.))**mu))
    mesh.setMeshTransformation(None)
    mesh.resetMeshInfo()
    return mesh


def distant_pair_mask(mesh, pairs):
    """per cell pair (a, b): the two cells share no vertex (a == b shares all)"""
    cells = np.asarray(mesh.cells)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return ~(cells[pairs[:, 0]][:, :, None] == cells[pairs[:, 1]][:, None, :]).any(axis=(1, 2))


def pair_evaluations(T, pairs):
    """kernel evaluations per cell pair of the list, as the oracle's numIntegrations counts them: n_q^2 for a distant pair of order q
    (formula_orders: the oracle's order wherever near_tie_margin is far above the rounding of a logarithm), the size of the rule of
    the touching panel otherwise.  Returns (evaluations [np], distant [np])."""
    op = as_oracle(T)
    mesh = op.tables.dm.mesh
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    cells = np.asarray(mesh.cells)
    common = (cells[pairs[:, 0]][:, :, None] == cells[pairs[:, 1]][:, None, :]).any(axis=2).sum(axis=1)
    distant = common == 0
    out = np.zeros(pairs.shape[0], dtype=np.int64)
    off = np.asarray(op.tables.dist_off, dtype=np.int64)
    q = formula_orders(op, pairs[distant, 0], pairs[distant, 1])
    assert q.size == 0 or q.max() <= op.tables.qcap
    out[distant] = (off[q+1]-off[q])**2
    for k in np.unique(common[~distant]):
        out[common == k] = evaluations(op, -int(k))
    return out, distant


def near_evaluations(T, pairs, masks):
    """P[i, j] for every DoF pair: the kernel evaluations of the DISTANT masked cell pairs whose masked local entries reach (i, j) --
    what oracle_entries returns per separated entry (all the cell pairs of a separated DoF pair are distant, and a near-field cluster
    pair that holds the DoF pair requests all of them), for the whole near field at once.  pairs [np, 2] with a <= b and masks
    [np, 4] uint64 over the (2 dpe)(2 dpe + 1) / 2 entries of the symmetric local matrix as clusters.buildMasksForClusters makes
    them: bit k(p, q), p <= q, sends the pair's contribution to (ld[p], ld[q]) and to (ld[q], ld[p])."""
    op = as_oracle(T)
    dm = op.tables.dm
    N = dm.num_dofs
    dofs = np.asarray(dm.dofs)
    dpe = dofs.shape[1]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    masks = np.asarray(masks, dtype=np.uint64).reshape(-1, 4)
    ev, distant = pair_evaluations(op, pairs)
    pairs, masks, ev = pairs[distant], masks[distant], ev[distant].astype(np.float64)
    ld = np.concatenate([dofs[pairs[:, 0]], dofs[pairs[:, 1]]], axis=1)
    P = np.zeros(N*N)
    k = 0
    for p in range(2*dpe):
        for q in range(p, 2*dpe):
            bit = ((masks[:, k >> 6] >> np.uint64(k & 63)) & np.uint64(1)).astype(bool)
            sel = bit & (ld[:, p] >= 0) & (ld[:, q] >= 0)
            k += 1
            if not sel.any():
                continue
            I, J = ld[sel, p].astype(np.int64), ld[sel, q].astype(np.int64)
            P += np.bincount(I*N+J, weights=ev[sel], minlength=N*N)
            if p != q:
                P += np.bincount(J*N+I, weights=ev[sel], minlength=N*N)
    assert P.max() < 2.**53
    return np.rint(P).astype(np.int64).reshape(N, N)


def near_magnitudes(T, pairs):
    """M[i, j] for every DoF pair: a bound of the sum of the ABSOLUTE values of the quadrature terms behind a separated entry, for
    elements whose shape functions change sign (P2), where the terms of an entry are not of one sign and |A_ij| is no measure of them.
    The shape functions of a cell sum to 1 and |phi| <= 1, so the absolute terms of the cell pair (a, b) for any (p, q) sum to at most
    S_ab = 2 vol sum_kl w_k w_l gamma(x_k, y_l) = 2 |sum_pq contrib_ab[p, dpe + q]| of the oracle's own contribution (nlo_eval), and
    M_ij = sum of S_ab over the distant cell pairs of the list with a in the support of i and b in that of j, in either order."""
    op = as_oracle(T)
    dm = op.tables.dm
    dofs = np.asarray(dm.dofs)
    nc, dpe = dofs.shape
    n2 = 2*dpe
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pairs = pairs[distant_pair_mask(dm.mesh, pairs)]
    cross = np.array([n2*p-(p*(p+1) >> 1)+dpe+q for p in range(dpe) for q in range(dpe)])
    S = np.array([2.*abs(op.eval(int(a), int(b))[1][cross].sum()) for a, b in pairs])
    E = sp.csr_matrix((S, (pairs[:, 0], pairs[:, 1])), shape=(nc, nc))
    c, k = np.nonzero(dofs >= 0)
    inc = sp.csr_matrix((np.ones(c.size), (c, dofs[c, k])), shape=(nc, dm.num_dofs))
    half = (inc.T@E@inc).toarray()
    return half+half.T


def near_tie_margin(T, pairs, bcells=None, bfacets=None):
    """smallest distance to an integer of the two ceil() arguments of the oracle's order formulas over what a near field classifies:
    the masked cell pairs without a common vertex (nlo_panel: centres, longest edges h, formula qo) and the (cell, facet) items
    without a common vertex (nlo_panel_boundary, which nlo_assemble_boundary_masked calls with the item's facet as its only boundary
    facet: cell centre against facet centre, h of the cell against the length of the facet -- 1 on an interval --, formula bqo: the
    facet formula of strip_tie_margin).  In 1-D and 2-D.  Returns (margin of the pairs, their number, margin of the items, their
    number); the margin of an empty set is inf."""
    op = as_oracle(T)
    Tb = op.tables
    mesh = Tb.dm.mesh
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    keep = distant_pair_mask(mesh, pairs)
    a, b = pairs[keep, 0], pairs[keep, 1]
    mp = float(pair_tie_margin(op, a, b).min()) if a.size else np.inf
    mi, ni = np.inf, 0
    if bcells is not None and len(bcells):
        c = np.asarray(bcells, dtype=np.int64)
        f = np.asarray(bfacets, dtype=np.int64).reshape(c.shape[0], -1)
        cells = np.asarray(mesh.cells)
        keep = ~(cells[c][:, :, None] == f[:, None, :]).any(axis=(1, 2))
        c, f = c[keep], f[keep]
        ni = int(c.size)
        if ni:
            v = mesh.vertices[f]                                         # [ni, dim, dim]
            if f.shape[1] == 2:
                fcen = (v[:, 0]+v[:, 1])*0.5
                flen = np.sqrt((v[:, 1, 0]-v[:, 0, 0])**2+(v[:, 1, 1]-v[:, 0, 1])**2)
            else:
                fcen, flen = v[:, 0]*1., np.ones(ni)
            d2 = _dist2(oracle_centres(mesh)[c]-fcen)
            mi = float(_margin(*_order_args(Tb.bqo, mesh.hVector[c], flen, d2, Tb.H0)).min())
    return mp, int(a.size), mi, ni


def facet_item_evaluations(T, bcells, bfacets):
    """point pairs per (cell, facet) item as the oracle's nlo_eval_boundary counts them: n_q nf_q for an item without a common vertex
    (order q by the facet formula bqo), the size of the touching rule otherwise.  Returns (evaluations [ni], distant [ni])."""
    op = as_oracle(T)
    Tb = op.tables
    mesh = Tb.dm.mesh
    c = np.asarray(bcells, dtype=np.int64)
    f = np.asarray(bfacets, dtype=np.int64).reshape(c.shape[0], -1)
    cells = np.asarray(mesh.cells)
    common = (cells[c][:, :, None] == f[:, None, :]).any(axis=2).sum(axis=1)
    distant = common == 0
    out = np.zeros(c.shape[0], dtype=np.int64)
    cd, fd = c[distant], f[distant]
    v = mesh.vertices[fd]
    if f.shape[1] == 2:
        fcen = (v[:, 0]+v[:, 1])*0.5
        flen = np.sqrt((v[:, 1, 0]-v[:, 0, 0])**2+(v[:, 1, 1]-v[:, 0, 1])**2)
    else:
        fcen, flen = v[:, 0]*1., np.ones(cd.size)
    a1, a2 = _order_args(Tb.bqo, mesh.hVector[cd], flen, _dist2(oracle_centres(mesh)[cd]-fcen), Tb.H0)
    q = np.maximum(np.maximum(np.ceil(a1), np.ceil(a2)), 2.).astype(np.int64)
    off, foff = np.asarray(Tb.dist_off, dtype=np.int64), np.asarray(Tb.bfacet_off, dtype=np.int64)
    out[distant] = (off[q+1]-off[q])*(foff[q+1]-foff[q])
    for k in np.unique(common[~distant]):
        out[common == k] = int(Tb.bsingular[-int(k)].num_nodes)
    return out, distant
