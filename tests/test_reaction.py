"""Device assembly of pointwise nonlinearities (pynucleus_amd/reaction.py, csrc/pnl_reaction.hip) against a numpy restatement of

    u_j(c, q) = sum_m U[j, dof(c, m)] phi_m(xi_q)           (local DoFs with dof < 0 contribute 0)
    R[o, I]   = sum_{(c, m): dof(c, m) = I} vol_c sum_q w_q f_o(u(c, q)) phi_m(xi_q)

written here from the formulas: rules (two Gauss points on an interval; edge midpoints for P1 and Radon's seven points for P2 on a
triangle), shape functions and the two functions.  The restatement also returns T[o, I] = the sum of the absolute values of the
terms of an entry; the device result may differ from it by reordering and FMA contraction of at most nterms products, so the bound
per entry is 64 * 2^-53 * nterms * T with nterms = (largest number of cells at a DoF) * (points) * (local shape functions), which is
at most 8 * 7 * 6 on these meshes."""
import numpy as np
import pytest

EPS = 2.0**-53


# ---- the restatement ---------------------------------------------------------------------------------------------------
def rule_and_shapes(dm):
    """(phi[dofs_per_cell, nq], w[nq]) of the DoF map's element with the rule the assembly uses"""
    md = dm.mesh.manifold_dim
    p = dm.polynomialOrder
    if md == 1:
        g = 1./np.sqrt(3.)
        l1 = np.array([.5*(1.-g), .5*(1.+g)])
        bary, w = np.stack([1.-l1, l1]), np.array([.5, .5])
    elif p == 1:
        bary, w = np.array([[.5, 0., .5], [.5, .5, 0.], [0., .5, .5]]), np.full(3, 1./3.)
    else:
        r = np.sqrt(15.)
        pts, w = [(1./3., 1./3., 1./3.)], [9./40.]
        for a, wa in (((6.-r)/21., (155.-r)/1200.), ((6.+r)/21., (155.+r)/1200.)):
            pts += [(1.-2.*a, a, a), (a, 1.-2.*a, a), (a, a, 1.-2.*a)]
            w += [wa]*3
        bary, w = np.array(pts).T, np.array(w)
    if p == 1:
        phi = bary.copy()
    elif md == 1:
        l0, l1 = bary
        phi = np.stack([l0*(2*l0-1), l1*(2*l1-1), 4*l0*l1])
    else:
        l0, l1, l2 = bary
        phi = np.stack([l0*(2*l0-1), l1*(2*l1-1), l2*(2*l2-1), 4*l0*l1, 4*l1*l2, 4*l0*l2])
    return phi, w


def f_brusselator(B, Q):
    def f(u):
        x, y = u
        z = B*x+Q*Q*y+(B/Q)*x*x+2.*Q*x*y+x*x*y
        return np.stack([-x+z, -z])
    return f


def f_cubic(u):
    return np.stack([u[0]**3-u[0]])


def restated_nonlinearity(dm, f, U):
    """(R, T, nterms): R[o, I] as in the module docstring, T[o, I] = sum of |terms|, nterms = the most terms any entry has"""
    phi, w = rule_and_shapes(dm)
    n = dm.num_dofs
    U = np.atleast_2d(np.asarray(U, dtype=np.float64))[:, :n]
    d = dm.dofs
    Ue = np.concatenate([U, np.zeros((U.shape[0], 1))], axis=1)
    ul = Ue[:, np.where(d >= 0, d, n)]                               # [nin, nc, dpc]
    uq = np.einsum('jcm,mq->jcq', ul, phi)
    fq = f(uq)                                                       # [nout, nc, nq]
    terms = dm.mesh.volVector[None, :, None, None]*w[None, None, :, None]*fq[:, :, :, None]*phi.T[None, None, :, :]   # [o, c, q, m]
    loc, aloc = terms.sum(axis=2), np.abs(terms).sum(axis=2)         # [o, c, m]
    R, T = np.zeros((fq.shape[0], n)), np.zeros((fq.shape[0], n))
    m = d >= 0
    for o in range(fq.shape[0]):
        np.add.at(R[o], d[m], loc[o][m])
        np.add.at(T[o], d[m], aloc[o][m])
    deg = np.bincount(d[m], minlength=max(n, 1)).max() if m.any() else 0
    return R, T, int(deg)*w.shape[0]*d.shape[1]


# ---- cases -------------------------------------------------------------------------------------------------------------
MESHES = ['interval1', 'interval3', 'interval67', 'interval300', 'disc1', 'disc2']
B0, Q0 = 1.22, 0.1


def make_mesh(name):
    from pynucleus_amd import simpleInterval, disc
    if name.startswith('interval'):
        return simpleInterval(-1., 1., numCells=int(name[8:]))
    return disc(int(name[4:]), radius=50.)


_dms = {}


def dofmap(name, element, tag):
    from pynucleus_amd import dofmapFactory, PHYSICAL, NO_BOUNDARY
    key = (name, element, tag)
    if key not in _dms:
        _dms[key] = dofmapFactory(element, make_mesh(name), PHYSICAL if tag == 'PHYSICAL' else NO_BOUNDARY)
    return _dms[key]


def functions(which):
    from pynucleus_amd.reaction import brusselator, cubic
    return (brusselator(B0, Q0), f_brusselator(B0, Q0)) if which == 'brusselator' else (cubic(), f_cubic)


def seeded_inputs(nin, n, seed=0):
    return np.random.default_rng(seed).uniform(-2., 2., size=(nin, n))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to('cuda:0')


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def _monomials_triangle(qr, degree):
    """largest error of the rule over x^a y^b, a + b <= degree, on the triangle (0,0), (1,0), (0,1): exact a! b! / (a + b + 2)!; the
    rule's weights sum to 1 = twice the area"""
    from math import factorial
    x, y = qr.nodes[1], qr.nodes[2]
    return max(abs(0.5*np.dot(qr.weights, x**a*y**b)-factorial(a)*factorial(b)/factorial(a+b+2))
               for a in range(degree+1) for b in range(degree+1-a))


def test_gauss2d_orders():
    from pynucleus_amd.quadrature import Gauss2D
    q2, q5 = Gauss2D(2), Gauss2D(5)
    assert q2.num_nodes == 3 and q5.num_nodes == 7
    assert abs(q2.weights.sum()-1.) < 1e-15 and abs(q5.weights.sum()-1.) < 1e-15
    assert _monomials_triangle(q2, 2) < 1e-15
    assert _monomials_triangle(q5, 5) < 1e-15
    assert _monomials_triangle(q2, 3) > 1e-4                        # the midpoint rule is not exact for cubics


def test_gauss1d_order():
    from pynucleus_amd.quadrature import Gauss1D
    q = Gauss1D(3)
    assert q.num_nodes == 2 and abs(q.weights.sum()-1.) < 1e-15
    x = q.nodes[1]                                                   # the unit interval
    for k in range(4):
        assert abs(np.dot(q.weights, x**k)-1./(k+1)) < 1e-15, k
    assert abs(np.dot(q.weights, x**4)-1./5.) > 1e-4


def test_package_rules_are_the_restated_ones():
    """the rule and shape values handed to the library equal the restatement's as sets of (node, weight) (the order of the points
    is free)"""
    from pynucleus_amd.reaction import volumeRule
    for name in ('interval3', 'disc1'):
        for element in ('P1', 'P2'):
            dm = dofmap(name, element, 'NO_BOUNDARY')
            qr = volumeRule(dm)
            phi, w = rule_and_shapes(dm)
            got = np.concatenate([dm.evalShapeFunctions(qr.nodes), qr.weights[None]]).T
            want = np.concatenate([phi, w[None]]).T
            assert got.shape == want.shape
            dist = np.abs(got[:, None, :]-want[None, :, :]).max(axis=2)        # [package point, restated point]
            match = dist.argmin(axis=1)
            assert sorted(match) == list(range(want.shape[0])) and dist.min(axis=1).max() < 1e-15, (name, element)


def test_unsupported_elements_raise():
    from pynucleus_amd import dofmapFactory, simpleInterval, NO_BOUNDARY
    from pynucleus_amd.reaction import volumeRule
    mesh = simpleInterval(-1., 1., numCells=3)
    for element in ('P0', 'P3'):
        with pytest.raises(NotImplementedError):
            volumeRule(dofmapFactory(element, mesh, NO_BOUNDARY))


def test_host_functions_match_the_restated_ones():
    u = seeded_inputs(2, 50, seed=3)
    for which in ('brusselator', 'cubic'):
        fun, f = functions(which)
        x = u[:fun.numInputs]
        # both are sums of at most six monomials evaluated in different orders: a few roundings of the sum of their magnitudes
        mag = (np.abs(x[0])+B0*np.abs(x[0])+Q0**2*np.abs(x[1])+B0/Q0*x[0]**2+2.*Q0*np.abs(x[0]*x[1])+x[0]**2*np.abs(x[1])
               if which == 'brusselator' else np.abs(x[0])**3+np.abs(x[0]))
        assert fun(x).shape == (fun.numOutputs, 50)
        assert (np.abs(fun(x)-f(x)) <= 16.*EPS*mag).all()


@pytest.mark.parametrize('name', ['interval67', 'disc2'])
@pytest.mark.parametrize('element', ['P1', 'P2'])
def test_restatement_on_constants(name, element):
    """numpy only: for constant inputs the restated assembly is f(u, v) * (M @ 1) -- the rules integrate the shape functions
    exactly, and on all vertices (NO_BOUNDARY) the shape functions sum to 1"""
    dm = dofmap(name, element, 'NO_BOUNDARY')
    rowsum = np.asarray(dm.assembleMass()@np.ones(dm.num_dofs))
    for which, c in (('brusselator', (0.3, -1.1)), ('cubic', (0.7,))):
        _, f = functions(which)
        U = np.array(c)[:, None]*np.ones((len(c), dm.num_dofs))
        R, T, _ = restated_nonlinearity(dm, f, U)
        want = f(np.array(c))[:, None]*rowsum[None, :]
        assert np.abs(R-want).max() <= 1e-14*np.abs(want).max(), (which, np.abs(R-want).max())


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('which', ['brusselator', 'cubic'])
@pytest.mark.parametrize('tag', ['PHYSICAL', 'NO_BOUNDARY'])
@pytest.mark.parametrize('element', ['P1', 'P2'])
@pytest.mark.parametrize('name', MESHES)
def test_nonlinearity_against_restatement(name, element, tag, which):
    import torch
    from pynucleus_amd.reaction import assembleNonlinearity
    dm = dofmap(name, element, tag)
    if tag == 'PHYSICAL':
        assert (dm.dofs < 0).any()
    fun, f = functions(which)
    U = seeded_inputs(fun.numInputs, dm.num_dofs, seed=len(name)+dm.num_dofs)
    R, T, nterms = restated_nonlinearity(dm, f, U)
    out = assembleNonlinearity(dm, fun, dev(U))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == R.shape
    bound = 64.*EPS*nterms*T
    assert nterms <= 8*7*6
    worst = (np.abs(got-R)-bound).max() if R.size else -1.
    print(name, element, tag, which, 'n', dm.num_dofs, 'nterms', nterms, 'max err', np.abs(got-R).max() if R.size else 0.,
          'min bound', bound.min() if R.size else 0.)
    assert worst <= 0., (worst, np.abs(got-R).max())
    if R.size:
        assert np.abs(got).max() > 0.
    # bitwise reproducible
    again = assembleNonlinearity(dm, fun, dev(U))
    assert torch.equal(out, again)


@pytest.mark.gpu
@pytest.mark.parametrize('name,element', [('interval67', 'P1'), ('disc2', 'P2')])
def test_alpha_beta_and_leading_dimensions(name, element):
    """R = beta R + alpha N(U) with beta = 1 onto a non-zero R and alpha = -dt, the vectors being rows of wider blocks (ldU, ldR >
    ndofs) whose padding must stay untouched.  Bound: that of N(U) times |alpha|, plus the rounding of the product beta R and of the
    final fused multiply-add, 2 * 2^-53 (|alpha N| + |beta R|) <= 64 * 2^-53 |beta R| with room."""
    import torch
    from pynucleus_amd.reaction import assembleNonlinearity
    dm = dofmap(name, element, 'PHYSICAL')
    fun, f = functions('brusselator')
    n, dt = dm.num_dofs, 0.0371
    U = seeded_inputs(2, n+7, seed=5)
    R0 = seeded_inputs(2, n+3, seed=6)
    N, T, nterms = restated_nonlinearity(dm, f, U)
    out = dev(R0)
    ret = assembleNonlinearity(dm, fun, dev(U), out=out, alpha=-dt, beta=1.)
    torch.cuda.synchronize()
    assert ret is out
    got = out.cpu().numpy()
    assert np.array_equal(got[:, n:], R0[:, n:])
    want = R0[:, :n]-dt*N
    bound = 64.*EPS*(nterms*dt*T+np.abs(R0[:, :n]))
    assert ((np.abs(got[:, :n]-want)-bound) <= 0.).all(), np.abs(got[:, :n]-want).max()
    # beta = 0 overwrites whatever the block held (NaN included)
    out2 = torch.full((2, n+3), float('nan'), dtype=torch.float64, device='cuda:0')
    assembleNonlinearity(dm, fun, dev(U), out=out2, alpha=2., beta=0.)
    got2 = out2.cpu().numpy()
    assert np.isnan(got2[:, n:]).all()
    assert ((np.abs(got2[:, :n]-2.*N)-64.*EPS*nterms*2.*T) <= 0.).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['interval67', 'disc2'])
def test_constant_input_gives_mass_row_sums(name):
    """P1 on all vertices: N(const) = f(u, v) * rowsum(M), M from dm.assembleMass() (both rules integrate the linear shape functions
    exactly).  Bound: that of the assembly plus the rounding of the row sums of M, at most (entries per row) * 2^-53 * rowsum each,
    covered by the same factor 64 * nterms."""
    import torch
    from pynucleus_amd.reaction import assembleNonlinearity
    dm = dofmap(name, 'P1', 'NO_BOUNDARY')
    M = dm.assembleMass()
    rowsum = np.asarray(M@np.ones(dm.num_dofs))
    for which, c in (('brusselator', (0.3, -1.1)), ('cubic', (0.7,))):
        fun, f = functions(which)
        U = np.array(c)[:, None]*np.ones((len(c), dm.num_dofs))
        _, T, nterms = restated_nonlinearity(dm, f, U)
        got = assembleNonlinearity(dm, fun, dev(U)).cpu().numpy()
        want = f(np.array(c))[:, None]*rowsum[None, :]
        bound = 64.*EPS*nterms*(T+np.abs(want))
        assert ((np.abs(got-want)-bound) <= 0.).all(), (which, np.abs(got-want).max())


@pytest.mark.gpu
def test_bad_arguments_raise():
    from pynucleus_amd._lib import PnlError, Context
    from pynucleus_amd.reaction import assembleNonlinearity, brusselator, cubic, multi_function, getSpace, _default_context
    import torch
    dm = dofmap('interval67', 'P1', 'PHYSICAL')
    n = dm.num_dofs
    with pytest.raises(PnlError):
        assembleNonlinearity(dm, brusselator(B0, Q0), dev(seeded_inputs(1, n)))          # one input row for a 2 -> 2 function
    with pytest.raises(PnlError):
        assembleNonlinearity(dm, cubic(), dev(seeded_inputs(2, n)), out=dev(np.zeros((1, n))))

    class unknown(multi_function):
        numInputs = numOutputs = 1
        fun = 99
    with pytest.raises(PnlError):
        assembleNonlinearity(dm, unknown(), dev(seeded_inputs(1, n)))
    with pytest.raises(PnlError):
        assembleNonlinearity(dm, cubic(), dev(seeded_inputs(1, n-1)))                    # a vector shorter than the space
    # the library still works after the refusals, and the space is cached per (DoF map, context)
    ctx = _default_context(torch.device('cuda', 0))
    assert isinstance(ctx, Context) and getSpace(dm, ctx) is getSpace(dm, ctx)
    U = seeded_inputs(1, n)
    R, T, nterms = restated_nonlinearity(dm, f_cubic, U)
    got = assembleNonlinearity(dm, cubic(), dev(U)).cpu().numpy()
    assert ((np.abs(got-R)-64.*EPS*nterms*T) <= 0.).all()
