"""Matrix entries far below max|A|: the parity tests bound |A_gpu - A_oracle| by 1e-11 max|A|, so an entry of 1e-6 max|A| could be
wrong by a relative 1e-5 unnoticed.  Here, besides that bound and the counters:

- integrable kernels whose far entries underflow (Gaussian of small variance, exponential of large rate): every far pair evaluates
  exp(y) with y far below -708, where pnl_exp used to return huge values of either sign;
- a per-entry relative bound on the separated DoF pairs: (i, j) such that no cell of the support of i shares a vertex with a cell of
  the support of j.  Every contribution to such an entry is a distant cross block -sum phi_i K phi_j of one sign (P0, P1), so the
  entry has no cancellation and |A_gpu - A_oracle| <= 1e-12 |A_oracle| must hold entry by entry."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TOL = 1e-11
REL = 1e-12


def _separated(dm):
    """mask of the separated DoF pairs: the vertex sets of the two supports are disjoint"""
    cells = dm.mesh.cells
    nc, nV = cells.shape
    d = dm.dofs
    rows, cols = [], []
    for k in range(d.shape[1]):
        m = d[:, k] >= 0
        for v in range(nV):
            rows.append(d[m, k])
            cols.append(cells[m, v])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    B = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(dm.num_dofs, dm.mesh.num_vertices))
    B.data[:] = 1.
    return (B@B.T).toarray() == 0.


def _compare(builder, floor=0.):
    """counters and the 1e-11 max|A| bound as the parity tests, then the per-entry bound on the separated pairs with |A_oracle| >=
    floor; returns the worst ratio |A_gpu - A_oracle| / |A_oracle| there"""
    from oracle.oracle import OracleProblem
    A = builder.getDense()
    Aref, cnt, _ = OracleProblem(builder.tables).get_dense()
    got = A.info['counters']
    for key in ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'numBoundaryPairs', 'numBoundaryIntegrations',
                'orders', 'singular'):
        assert got[key] == cnt[key], (key, got[key], cnt[key])
    Ag = A.toarray()
    assert np.all(np.isfinite(Ag))
    scale = np.abs(Aref).max()
    err = np.abs(Ag-Aref).max()/scale
    assert err < TOL, err
    sep = _separated(builder.dm if hasattr(builder, 'dm') else builder.tables.dm)
    m = sep & (np.abs(Aref) >= floor) & (Aref != 0.)
    assert m.sum() > 0
    # one sign: the separated entries of the oracle are all <= 0
    assert np.all(Aref[sep] <= 0.)
    ratio = np.abs(Ag[m]-Aref[m])/np.abs(Aref[m])
    print('separated pairs: {}, worst |A_gpu - A_oracle| / |A_oracle| {:.2e}'.format(m.sum(), ratio.max()))
    assert ratio.max() <= REL, (ratio.max(), np.argwhere(m)[ratio.argmax()], Aref[m][ratio.argmax()])
    return ratio.max()


def _fractional(domain, noRef, s, element='P1', params=None):
    from pynucleus_amd import disc, interval, PHYSICAL, dofmapFactory, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    mesh = disc(noRef) if domain == 'disc' else interval(noRef)
    dm = dofmapFactory(element, mesh, PHYSICAL)
    return nonlocalBuilder(dm, getFractionalKernel(mesh.dim, s), params or {}, zeroExterior=True)


@pytest.mark.parametrize('domain,noRef,s,element', [('disc', 4, 0.25, 'P1'), ('disc', 4, 0.5, 'P1'), ('disc', 4, 0.75, 'P1'),
                                                    ('disc', 4, 0.4, 'P1'), ('disc', 3, 0.3, 'P0'), ('interval', 6, 0.25, 'P1')])
def test_separated_entries_fractional(domain, noRef, s, element):
    """per-entry 1e-12 on the separated pairs of the fractional kernels: rsq / quarter-power (s = 1/4, 1/2, 3/4), the LDS power tables
    (s = 0.4, 0.3).  Observed worst ratio on an MI355X: 1.2e-15 .. 2.3e-15 (disc P1 / P0), 4.7e-16 (interval)."""
    b = _fractional(domain, noRef, s, element, {'target_order': 0.5} if element == 'P0' else None)
    _compare(b)


def _integrable(dim, name, par, zeroExterior=True, noRef=None):
    from pynucleus_amd import disc, interval, PHYSICAL, P1_DoFMap, getKernel
    from pynucleus_amd.builder import nonlocalBuilder
    mesh = disc(noRef or 3) if dim == 2 else interval(noRef or 5)
    kw = {'variance': par} if name == 'gaussian' else {'exponentialRate': par}
    k = getKernel(dim, kernel=name, horizon=np.inf, **kw)
    return nonlocalBuilder(P1_DoFMap(mesh, PHYSICAL), k, {}, zeroExterior=zeroExterior)


@pytest.mark.parametrize('case', ['gaussian_2d_var0.02', 'gaussian_1d_var1e-3', 'gaussian_1d_var1e-3_noext', 'exponential_1d_rate500'])
def test_underflowing_integrable_kernels(case):
    """Gaussian of variance 0.02 on the disc (2D, y = -d2 / (2 0.02^2) down to -5000), of variance 1e-3 on the interval (1D, the twins
    5 and 7 of zeroExterior=False run too), the exponential kernel at rate 500 (1D): against the oracle with the counters, the 1e-11
    max|A| bound and the per-entry bound on the separated pairs with |A_oracle| >= 1e-290.  Observed worst ratio on an MI355X: 3.4e-13
    (2D), 2.3e-13 (1D Gaussian), 1.1e-13 (exponential) -- exp(y) at |y| up to 700 carries the rounding of y, |y| 2^-53, in both.
    With pnl_exp in place of pnl_exp_ranged the far values are garbage of order 1e300 (pnl_common.h)."""
    name, dimtag, par = case.split('_')[:3]
    dim = 2 if dimtag == '2d' else 1
    par = float(par.replace('var', '').replace('rate', ''))
    _compare(_integrable(dim, name, par, zeroExterior=not case.endswith('noext')), floor=1e-290)


def test_underflowing_gaussian_h2_matches_dense():
    """getH2 of the 1D Gaussian of variance 1e-3 (its near field and the kernel interpolants of the admissible blocks evaluate the
    same branch of kern_eval) against getDense"""
    b = _integrable(1, 'gaussian', 1e-3, noRef=7)
    Ad = b.getDense().toarray()
    H = b.getH2()
    x = np.random.default_rng(3).standard_normal(Ad.shape[0])
    y = H*x
    assert np.all(np.isfinite(y))
    yd = Ad@x
    assert np.abs(y-yd).max() <= 3e-2*np.abs(yd).max(), np.abs(y-yd).max()/np.abs(yd).max()       # tests/test_h2.py: epsRelDense
