"""The block eigensolver: pnl_eigb_gram / _combine / _residual (csrc/pnl_eig_block.hip) through the C ABI on synthetic blocks, and
solvers.lobpcg on synthetic and assembled operators.  Helpers come from tests/test_apply_kernels.py, tests/test_block_products.py and
tests/test_cg_block.py.

No assertion of the contracts (a)-(f) uses a measured tolerance.  Two sanity tests beside them (test_ritz_survives_a_rank_deficient_basis,
and the maxiter = 0 part of test_lobpcg_start_and_maxiter) compare with a second host computation under loose margins that their
docstrings state: a mistake there is an error of order one, the margins are many orders above the rounding level and carry no contract.

(a) gram, exact.  U and V hold integers |u| <= 8: every product and every partial sum is an integer below 2^53, so G equals the int64
    numpy product bit for bit whatever the order of the sums.  On standard-normal data: G[a][b] of a 48 x 48 call has the bits of the
    1 x 1 call on (U[a], V[b]) (made on an aligned copy: the 16-byte and the 8-byte loads give the same bits), a sub-block call
    repeats them, two calls repeat, and G is bitwise symmetric when U is V.  The whole allocations of U, V and G are compared: the
    padding keeps its poison.
(b) combine and residual, exact.  Dyadic C, S, theta, dinv (small integers times powers of two): every fma is exact, so the outputs
    equal numpy's bit for bit, and the sums equal int64 sums.  Columns outside the mask and all padding keep their fill.
(c) the stopping contract of solvers.lobpcg: passes < maxiter, residuals <= tol, theta ascending, shapes and types.
(d) true residual.  With x_v, theta_v as returned and r = A x - theta M x in longdouble on the host,
        rho_true = ||r||_2 / (|theta| ||M x||_2) <= residuals[v] (1 + (n + 4) u) + gap_v,
        gap_v = 4 u [(m_A + 2) || |A| |x_v| ||_2 + (m_M + 3) |theta_v| || |M| |x_v| ||_2] / (|theta_v| ||M x_v||_2),   u = 2^-53,
    m_A, m_M the entries per row: one product's rounding for each of A x and M x in any summation order, the multiply and the
    subtraction; the factor 4 covers the constants as in (4) of test_cg_block.py.  It is ONE product's rounding because the returned
    residual is an explicit recomputation.  Largest (rho_true - residuals[v]) / gap_v measured on an MI355X over all cases of this
    file: 0.0024 (see test_lobpcg_on_synthetic_matrices).
(e) the right eigenvalues, orthogonality, normalisation, with lam = scipy.linalg.eigh(A, M) on the host:
        |theta_v - lam_v| <= ||r_v||_2 / (sqrt(lambda_min(M)) ||x_v||_M)            (the residual bound of the symmetric pencil)
        |x_a^T M x_b| <= (||x_a||_2 ||r_b||_2 + ||x_b||_2 ||r_a||_2) / |theta_a - theta_b|,  a != b
                                                (from (theta_a - theta_b) x_a^T M x_b = x_a^T r_b - x_b^T r_a)
        |x_v^T M x_v - 1| <= (n + m_M + 4) u |x_v|^T |M| |x_v|                        (the worst case of the final normalisation)
(f) the same contracts on assembled operators: interval and disc, dense with Jacobi and multigrid, H2 in both far-field modes.

The solver inputs are shown to be solvable without the code under test: a numpy restatement of the driver (lobpcg_numpy) converges on
every one of them in at most a quarter of the maxiter the GPU tests use and meets (c)-(e).

Edges: 256 elements per workgroup and chunk and at most 256 workgroups (n = 255 / 256 / 257 and 65535 / 65536 / 65537 / 131073: one
trip, the cap, two and three trips of the chunk loop); the steps of 16 and the runs of 4 elements of k_eigb_gram (n = 1, 2, 63, 64, 65);
16 rows per group (15 / 16 / 17, 31 / 32 / 33, 47 / 48).
"""
import ctypes as C

import numpy as np
import pytest

from test_apply_kernels import U, LD, _context, _context_with_dofs
from test_block_products import block_image, _dev_block
from test_cg_block import dom, lap, LAYOUTS, _dense_operator, _csr_operator

gpu = pytest.mark.gpu

TOL = 1e-8
MAXITER = 400
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 65535, 65536, 65537, 131073)
KS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48)
KM = ((1, 1), (1, 4), (4, 8), (6, 16))
# (matrix, n, with the mass matrix): the inputs of the issue's table
INPUTS = tuple((name, n, withM) for name, n in (('dom', 63), ('dom', 257), ('dom', 1025), ('lap', 63)) for withM in (False, True))


def km_of(name):
    """lap with m = 1 and with m = 16 is not an input (400+ passes, or a stall near 1e-7, in the prototype)"""
    return KM if name == 'dom' else KM[1:3]


def mass(n):
    """the 1D P1 mass matrix h tridiag(1, 4, 1) / 6, h = 1 / (n + 1)"""
    h = 1./(n+1)
    return h*(4.*np.eye(n)+np.eye(n, k=1)+np.eye(n, k=-1))/6.


def start_block(m, n):
    return np.random.default_rng(9400+m+n).standard_normal((m, n))


_PROBLEMS = {}


def problem(name, n, withM):
    """(A, M or None, ascending eigenvalues of the pencil, lambda_min(M)), computed once"""
    import scipy.linalg as sla
    key = (name, n, withM)
    if key not in _PROBLEMS:
        A = dom(n) if name == 'dom' else lap(n)
        M = mass(n) if withM else None
        lam = sla.eigh(A, M, eigvals_only=True)
        _PROBLEMS[key] = (A, M, lam, float(np.linalg.eigvalsh(M)[0]) if withM else 1.)
    return _PROBLEMS[key]


# ---- the yardstick: the driver in numpy ------------------------------------------------------------------------------------------

def ritz_numpy(GA, GM, idx, m, rank_tol=1e-10):
    GA, GM = GA[np.ix_(idx, idx)], GM[np.ix_(idx, idx)]
    GA, GM = .5*(GA+GA.T), .5*(GM+GM.T)
    d = 1./np.sqrt(np.diagonal(GM))
    GA, GM = d[:, None]*GA*d[None, :], d[:, None]*GM*d[None, :]
    lam, V = np.linalg.eigh(GM)
    keep = lam > rank_tol*lam[-1]
    B = V[:, keep]/np.sqrt(lam[keep])
    th, Z = np.linalg.eigh(B.T@GA@B)
    return th[:m], d[:, None]*(B@Z[:, :m])


def lobpcg_numpy(A, M, X0, k, tol, maxiter, dinv):
    """LOBPCG with soft locking on the basis [X; W; P] as solvers.lobpcg runs it: carried AX, MX; explicit recomputation before a
    column counts as converged; W made M-orthogonal to X and scaled; the scaled, rank-revealing Rayleigh-Ritz problem"""
    m, n = X0.shape
    prod = lambda Mat, V: V@Mat.T if Mat is not None else V.copy()                       # noqa: E731
    S, AS, MS = (np.zeros((3*m, n)) for _ in range(3))
    AX, MX = prod(A, X0), prod(M, X0)
    th, Cx = ritz_numpy(X0@AX.T, X0@MX.T, np.arange(m), m)
    S[:m], AS[:m], MS[:m] = Cx.T@X0, Cx.T@AX, Cx.T@MX
    haveP, active, res, passes = False, np.ones(m, dtype=bool), np.full(m, np.inf), 0

    def residual(mask):
        R = AS[:m]-th[:, None]*MS[:m]
        r = np.sqrt((R*R).sum(axis=1))/(np.abs(th)*np.sqrt((MS[:m]*MS[:m]).sum(axis=1)))
        res[mask] = r[mask]
        return R
    while True:
        R = residual(active)
        active &= res > tol
        if (res[:k] <= tol).all() or passes == maxiter:
            AS[:m], MS[:m] = prod(A, S[:m]), prod(M, S[:m])
            xmx = np.einsum('ij,ij->i', S[:m], MS[:m])
            th = np.einsum('ij,ij->i', S[:m], AS[:m])/xmx
            R = residual(np.ones(m, dtype=bool))
            if (res[:k] <= tol).all() or passes == maxiter:
                break
            active = res > tol
        W = dinv*R
        nrm = np.sqrt((W*W).sum(axis=1))
        sc = np.where(active & (nrm > 0.), 1./np.where(nrm > 0., nrm, 1.), 0.)
        W = sc[:, None]*(W-(W@MS[:m].T)@S[:m])
        S[m:2*m], AS[m:2*m], MS[m:2*m] = W, prod(A, W), prod(M, W)
        act = np.nonzero(active)[0]
        idx = np.concatenate([np.arange(m), m+act, 2*m+act if haveP else act[:0]])
        th, Cs = ritz_numpy(S@AS.T, S@MS.T, idx, m)
        Cx = np.zeros((3*m, m))
        Cx[idx] = Cs
        Cp = Cx.copy()
        Cp[:m] = 0.
        new = []
        for T in (S, AS, MS):
            Tn = np.zeros_like(T)
            Tn[:m], Tn[2*m:] = Cx.T@T, Cp.T@T
            new.append(Tn)
        S, AS, MS = new
        haveP = True
        passes += 1
    order = np.argsort(th[:k], kind='stable')
    return th[order], S[order]/np.sqrt(xmx[order])[:, None], passes, res[order]


# ---- the contracts (c), (d), (e) on the host -------------------------------------------------------------------------------------

WORST = {'ratio': -np.inf}


def entries_per_row(Mat):
    return int((Mat != 0.).sum(axis=1).max())


def assert_contracts(A, M, lam, lmin, theta, X, passes, res, k, maxiter, what, mA=None, mM=None, skew=0.):
    """(c), (d), (e) for what a solver returned; A, M (None: the identity) host matrices.  skew = ||A - A^T||_F / 2 of an A that is
    symmetric up to rounding only (an H2 operator's matrix), lam then being the eigenvalues of the pencil of its symmetric part A_s: (d)
    is about the A that the operator applies, the bounds of (e) take ||A_s x - theta M x|| <= ||r|| + skew ||x||"""
    theta, X, res = np.asarray(theta), np.asarray(X), np.asarray(res)
    n = A.shape[0]
    Mh = np.eye(n) if M is None else M
    mA = entries_per_row(A) if mA is None else mA
    mM = (0 if M is None else entries_per_row(M)) if mM is None else mM
    # (c)
    assert theta.shape == res.shape == (k,) and X.shape == (k, n) and isinstance(passes, int), (what, theta.shape, X.shape, res.shape)
    assert passes < maxiter and (res <= TOL).all() and np.isfinite(X).all(), (what, passes, res)
    assert (np.diff(theta) >= 0.).all() and (theta > 0.).all(), (what, theta)
    Al, Ml, Xl = A.astype(LD), Mh.astype(LD), X.astype(LD)
    AXl, MXl = Xl@Al.T, Xl@Ml.T
    Rl = AXl-theta.astype(LD)[:, None]*MXl
    rn = np.sqrt((Rl*Rl).sum(axis=1)).astype(np.float64)
    xn = np.sqrt((Xl*Xl).sum(axis=1)).astype(np.float64)
    rs = rn+skew*xn                                              # residual norms against the symmetric part, for (e)
    mxn = np.sqrt((MXl*MXl).sum(axis=1)).astype(np.float64)
    xmx = (Xl*MXl).sum(axis=1).astype(np.float64)
    aAx = np.sqrt(((np.abs(Xl)@np.abs(Al).T)**2).sum(axis=1)).astype(np.float64)
    aMx = np.sqrt(((np.abs(Xl)@np.abs(Ml).T)**2).sum(axis=1)).astype(np.float64)
    xaMx = (np.abs(Xl)*(np.abs(Xl)@np.abs(Ml).T)).sum(axis=1).astype(np.float64)
    for v in range(k):
        # (d)
        rho = rn[v]/(abs(theta[v])*mxn[v])
        gap = 4.*U*((mA+2)*aAx[v]+(mM+3)*abs(theta[v])*aMx[v])/(abs(theta[v])*mxn[v])
        WORST['ratio'] = max(WORST['ratio'], (rho-res[v])/gap)
        print('{} column {}: theta {:.15e} passes {} residual {:.3e} rho_true {:.3e} gap {:.3e} (rho - res) / gap {:.3e}'.format(
            what, v, theta[v], passes, res[v], rho, gap, (rho-res[v])/gap))
        assert rho <= res[v]*(1.+(n+4)*U)+gap, (what, v, rho, res[v], gap)
        # (e)
        assert abs(theta[v]-lam[v]) <= rs[v]/(np.sqrt(lmin)*np.sqrt(xmx[v])), (what, v, theta[v], lam[v], rs[v])
        assert abs(xmx[v]-1.) <= (n+mM+4)*U*xaMx[v], (what, v, xmx[v]-1., (n+mM+4)*U*xaMx[v])
        for w in range(v):
            if theta[v] == theta[w]:
                continue                                             # the identity bounds nothing inside an eigenspace
            off = abs(float((Xl[v]*MXl[w]).sum()))
            assert off <= (xn[v]*rs[w]+xn[w]*rs[v])/abs(theta[v]-theta[w]), (what, v, w, off)


# ---- CPU tests -------------------------------------------------------------------------------------------------------------------

def test_abi_declares_the_block_eigensolver():
    """the header, the binding and the library agree on the new symbols (tests/test_abi.py checks the whole list)"""
    import os
    from pynucleus_amd import _lib, solvers
    from test_abi import declared_symbols
    new = {'pnl_eigb_gram', 'pnl_eigb_combine', 'pnl_eigb_residual'}
    assert new <= set(declared_symbols()) and new <= set(_lib.EXPORTS)
    assert os.path.exists(_lib.LIB_PATH), 'build the HIP library first (__graft_entry__.build())'
    L = _lib.load()                 # not a bare dlopen: torch's HIP runtime has to be in the process first (see _lib.load)
    for name in new:
        assert hasattr(L, name), name
    assert _lib.PNL_EIGB_MAXBASIS == 48 == 3*_lib.PNL_CGB_MAXVEC
    for name in ('eigb_gram', 'eigb_combine', 'eigb_residual'):
        assert callable(getattr(_lib.Context, name))
    assert callable(solvers.lobpcg)


@pytest.mark.parametrize('name,n,withM', INPUTS)
def test_numpy_driver_solves_the_inputs(name, n, withM):
    """every solver input of this file is solvable: the numpy driver converges in at most MAXITER / 4 passes and meets (c)-(e); its
    Rayleigh-Ritz step is the one of the package (solvers._ritz is plain numpy)"""
    from pynucleus_amd import solvers
    A, M, lam, lmin = problem(name, n, withM)
    for k, m in km_of(name):
        X0 = start_block(m, n)
        theta, X, passes, res = lobpcg_numpy(A, M, X0, k, TOL, MAXITER, 1./np.diagonal(A))
        assert passes <= MAXITER//4, (name, n, withM, k, m, passes)
        assert_contracts(A, M, lam, lmin, theta, X, passes, res, k, MAXITER, 'numpy {}({}) M={} k={} m={}'.format(name, n, withM, k, m))
    S = start_block(12, n)
    GA, GM = S@A@S.T, S@(S if M is None else S@M).T
    th, idx, Cs = solvers._ritz(GA, GM, np.arange(12), 4)
    th2, C2 = ritz_numpy(GA, GM, np.arange(12), 4)
    assert np.array_equal(idx, np.arange(12)) and np.array_equal(th, th2) and np.array_equal(Cs, C2)


def test_ritz_survives_a_rank_deficient_basis():
    """a basis with a repeated and a zero row: the dependent directions are dropped, the Ritz values are those of the independent rows
    and C^T G_M C = I.  Sanity margins, not contracts: the nearly dependent row perturbs the kept subspace by 1e-13 and the Gram
    matrices carry n u = 7e-15, so 1e-6 is seven orders above what is expected; a direction that is not dropped gives a Ritz value
    or a C^T G_M C that is off by order one"""
    from pynucleus_amd import solvers
    n = 63
    A, M, lam, lmin = problem('dom', n, True)
    S = start_block(6, n)
    S = np.vstack([S, S[2]*3., np.zeros(n), S[0]+1e-13*S[1]])
    GA, GM = S@A@S.T, S@M@S.T
    th, idx, Cs = solvers._ritz(GA, GM, np.arange(9), 3)
    assert list(idx) == [0, 1, 2, 3, 4, 5, 6, 8]
    th6, _, _ = solvers._ritz(GA, GM, np.arange(6), 3)
    assert np.allclose(th, th6, rtol=1e-6, atol=0.)
    assert np.abs(Cs.T@GM[np.ix_(idx, idx)]@Cs-np.eye(3)).max() < 1e-6


# ---- (a) pnl_eigb_gram -----------------------------------------------------------------------------------------------------------

def _gram(ctx, Uh, Vh, dU=0, dV=0, dG=0, oU=0, oV=0, oG=0, same=False):
    """one call; returns G [ku][kv] after checking the whole allocations of G (padding, guards) and U, V (unchanged)"""
    (ku, n), kv = Uh.shape, Vh.shape[0]
    us, up = _dev_block(Uh, n+dU, oU)
    vs, vp = (us, up) if same else _dev_block(Vh, n+dV, oV)
    ldv = n+dU if same else n+dV
    gs, gp = _dev_block(np.full((ku, kv), 7.), kv+dG, oG)
    ctx.eigb_gram(n, ku, up, n+dU, kv, vp, ldv, gp, kv+dG)
    ctx.synchronize()
    img = gs.cpu().numpy()
    G = img[oG:oG+ku*(kv+dG)].reshape(ku, kv+dG)[:, :kv].copy()
    assert np.array_equal(img, block_image(G, kv+dG, oG)), 'padding of G'
    assert np.array_equal(us.cpu().numpy(), block_image(Uh, n+dU, oU)) and np.array_equal(vs.cpu().numpy(), block_image(Vh, ldv, oU if same else oV))
    return G


@gpu
@pytest.mark.parametrize('i,n', tuple(enumerate(SIZES)))
def test_gram_exact(i, n):
    """(a) integer blocks: G is the int64 product bit for bit; every row count appears on each side over the sizes, every layout too"""
    ctx = _context()
    rng = np.random.default_rng(9500+n)
    for j in (i, i+5):
        ku, kv = KS[j % 10], KS[(3*j+7) % 10]
        dU, dV, dG, oU, oV, oG = LAYOUTS[j % 6]
        Uh, Vh = (rng.integers(-8, 9, size=(kk, n)).astype(np.float64) for kk in (ku, kv))
        G = _gram(ctx, Uh, Vh, dU, dV, dG, oU, oV, oG)
        ref = (Uh.astype(np.int64)@Vh.astype(np.int64).T).astype(np.float64)
        assert np.array_equal(G, ref), (n, ku, kv, np.argwhere(G != ref)[:4])
    ctx.close()


@gpu
@pytest.mark.parametrize('n', (1, 63, 255, 1025, 65537))
def test_gram_bits_do_not_depend_on_the_block(n):
    """(a) standard-normal rows: the bits of G[a][b] are those of the 1 x 1 call on (U[a], V[b]), of a sub-block call and of a second
    call; G is bitwise symmetric when U is V; the values are dot products"""
    ctx = _context()
    rng = np.random.default_rng(9600+n)
    Uh, Vh = rng.standard_normal((48, n)), rng.standard_normal((48, n))
    G = _gram(ctx, Uh, Vh, 1, 6, 1, 1, 0, 1)
    assert np.array_equal(G, _gram(ctx, Uh, Vh, 1, 6, 1, 1, 0, 1)), 'two calls'
    assert np.array_equal(G, _gram(ctx, Uh, Vh)), 'another layout'
    pairs = {(0, 0), (0, 47), (47, 0), (47, 47), (15, 16), (16, 15), (32, 33), (5, 40), (40, 5), (23, 23), (31, 32)}
    for a, b in sorted(pairs | {(17, b) for b in range(48)} | {(a, 32) for a in range(48)}):     # a whole row, a whole column
        assert np.array_equal(_gram(ctx, Uh[a:a+1], Vh[b:b+1]), G[a:a+1, b:b+1]), (a, b)
    assert np.array_equal(_gram(ctx, Uh[:17], Vh[:33], 0, 1, 6, 0, 1, 0), G[:17, :33])
    assert np.array_equal(_gram(ctx, Uh[16:47], Vh[31:48]), G[16:47, 31:48]), 'other positions'
    Gs = _gram(ctx, Uh, Uh, 1, 1, 0, 1, 1, 0, same=True)
    assert np.array_equal(Gs, Gs.T), 'U is V'
    ref = (Uh.astype(LD)@Vh.astype(LD).T).astype(np.float64)
    mag = np.abs(Uh)@np.abs(Vh).T
    assert (np.abs(G-ref) <= (n+2)*U*mag).all()
    ctx.close()


# ---- (b) pnl_eigb_combine, pnl_eigb_residual -------------------------------------------------------------------------------------

def dyadic(rng, shape, top=4, e=2):
    return rng.integers(-top, top+1, size=shape).astype(np.float64)*2.**rng.integers(-e, e+1, size=shape)


@gpu
@pytest.mark.parametrize('i,n', tuple(enumerate(SIZES)))
def test_combine_exact(i, n):
    """(b) Y = C S on dyadic data, bit for bit, with padding in S, C and Y"""
    ctx = _context()
    rng = np.random.default_rng(9700+n)
    for j in (i, i+5):
        kin, kout = KS[j % 10], (1, 2, 15, 16, 3)[j % 5]
        dS, dC, dY, oS, oC, oY = LAYOUTS[j % 6]
        Sh, Ch = rng.integers(-8, 9, size=(kin, n)).astype(np.float64), dyadic(rng, (kout, kin))
        ss, sp = _dev_block(Sh, n+dS, oS)
        cs, cp = _dev_block(Ch, kin+dC, oC)
        ys, yp = _dev_block(np.full((kout, n), 7.), n+dY, oY)
        ctx.eigb_combine(n, kin, sp, n+dS, kout, cp, kin+dC, yp, n+dY)
        ctx.synchronize()
        assert np.array_equal(ys.cpu().numpy(), block_image(Ch@Sh, n+dY, oY)), (n, kin, kout)
        assert np.array_equal(ss.cpu().numpy(), block_image(Sh, n+dS, oS)) and np.array_equal(cs.cpu().numpy(), block_image(Ch, kin+dC, oC))
    ctx.close()


@gpu
@pytest.mark.parametrize('i,n', tuple(enumerate(SIZES)))
def test_residual_exact(i, n):
    """(b) R = AX - theta MX, W = dinv R and the two sums on dyadic data, bit for bit; columns outside the mask and all padding keep
    their fill; without W, without dinv, and with MX the block that AX is"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(9800+n)
    for j, (nv, withW, withD, same) in enumerate(((16, True, True, False), (3, True, False, False), (16, False, True, False), (5, True, True, True))):
        dA, dM, dR, oA, oM, oR = LAYOUTS[(i+j) % 6]
        AXh, MXh = (rng.integers(-16, 17, size=(nv, n)).astype(np.float64) for _ in range(2))
        if same:
            MXh, dM, oM = AXh, dA, oA
        theta, dinv = dyadic(rng, nv), 2.**rng.integers(-2, 3, size=n)
        on = rng.integers(0, 2, size=nv).astype(bool)
        on[rng.integers(0, nv)] = True
        if nv > 1:
            on[(np.nonzero(on)[0][0]+1) % nv] = False
        mask = int(sum(1 << v for v in range(nv) if on[v]))
        axs, axp = _dev_block(AXh, n+dA, oA)
        mxs, mxp = (axs, axp) if same else _dev_block(MXh, n+dM, oM)
        rs, rp = _dev_block(np.full((nv, n), 7.), n+dR, oR)
        ws, wp = _dev_block(np.full((nv, n), 7.), n+dR+1, oR)
        th_d, di_d = torch.from_numpy(theta).cuda(), torch.from_numpy(dinv).cuda()
        sums = torch.full((2*nv,), 77., dtype=torch.float64, device='cuda')
        ctx.eigb_residual(n, nv, mask, axp, n+dA, mxp, n+dM, th_d.data_ptr(), di_d.data_ptr() if withD else 0, rp, n+dR, wp if withW else 0, n+dR+1,
                          sums.data_ptr())
        ctx.synchronize()
        R = AXh-theta[:, None]*MXh
        W = dinv*R if withD else R
        assert np.array_equal(rs.cpu().numpy(), block_image(np.where(on[:, None], R, 7.), n+dR, oR)), (n, nv)
        assert np.array_equal(ws.cpu().numpy(), block_image(np.where(on[:, None], W, 7.) if withW else np.full((nv, n), 7.), n+dR+1, oR)), (n, nv)
        rr = ((R*4.).astype(np.int64)**2).sum(axis=1)/16.
        mm = (MXh.astype(np.int64)**2).sum(axis=1).astype(np.float64)
        want = np.full((nv, 2), 77.)
        want[on, 0], want[on, 1] = rr[on], mm[on]
        assert np.array_equal(sums.cpu().numpy().reshape(nv, 2), want), (n, nv)
        assert np.array_equal(axs.cpu().numpy(), block_image(AXh, n+dA, oA)) and np.array_equal(mxs.cpu().numpy(), block_image(MXh, n+dM, oM))
    ctx.close()


@gpu
def test_eigb_validation():
    """every invalid argument of the header returns PNL_ERR_INVALID and nothing is written"""
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    n, k = 7, 3
    t = lambda *shape, fill=77.: torch.full(shape, fill, dtype=torch.float64, device='cuda')                   # noqa: E731
    V = [t(49, n) for _ in range(4)]
    G, Cm, th, dv, sums = t(49, 49), t(16, 49), t(16), t(n), t(32)
    P_ = [v.data_ptr() for v in V]
    L, h = ctx.L, ctx.h
    p = lambda v: C.c_void_p(v) if v else None                                                                  # noqa: E731
    gram = lambda h_=h, nn=n, ku=k, u=P_[0], ldu=n, kv=k, v=P_[1], ldv=n, g=G.data_ptr(), ldg=49: L.pnl_eigb_gram(  # noqa: E731
        h_, nn, ku, p(u), ldu, kv, p(v), ldv, p(g), ldg)
    comb = lambda h_=h, nn=n, kin=k, s=P_[0], lds=n, kout=k, c=Cm.data_ptr(), ldc=49, y=P_[2], ldy=n: L.pnl_eigb_combine(  # noqa: E731
        h_, nn, kin, p(s), lds, kout, p(c), ldc, p(y), ldy)
    resid = lambda h_=h, nn=n, nv=k, mask=5, ax=P_[0], ldax=n, mx=P_[1], ldmx=n, th_=th.data_ptr(), r=P_[2], ldr=n, w=P_[3], ldw=n, s=sums.data_ptr(): (  # noqa: E731
        L.pnl_eigb_residual(h_, nn, nv, mask, p(ax), ldax, p(mx), ldmx, p(th_), p(dv.data_ptr()), p(r), ldr, p(w), ldw, p(s)))
    cases = (
        (gram, (dict(h_=None), dict(nn=0), dict(nn=-1), dict(ku=0), dict(ku=49), dict(kv=0), dict(kv=49), dict(u=None), dict(v=None), dict(g=None),
                dict(ldu=n-1), dict(ldv=n-1), dict(ldg=k-1), dict(g=P_[0]), dict(g=P_[1]))),
        (comb, (dict(h_=None), dict(nn=0), dict(kin=0), dict(kin=49), dict(kout=0), dict(kout=17), dict(s=None), dict(c=None), dict(y=None),
                dict(lds=n-1), dict(ldy=n-1), dict(ldc=k-1), dict(y=P_[0]), dict(y=Cm.data_ptr()))),
        (resid, (dict(h_=None), dict(nn=0), dict(nv=0), dict(nv=17), dict(mask=0), dict(mask=8), dict(ax=None), dict(mx=None), dict(th_=None),
                 dict(r=None), dict(s=None), dict(ldax=n-1), dict(ldmx=n-1), dict(ldr=n-1), dict(ldw=n-1), dict(r=P_[0]), dict(r=P_[1]),
                 dict(w=P_[0]), dict(w=P_[1]), dict(w=P_[2]))),
    )
    for f, bad in cases:
        for kw in bad:
            assert f(**kw) == _lib.PNL_ERR_INVALID, kw
        ctx.synchronize()
        assert all(bool((x == 77.).all()) for x in V+[G, Cm, th, dv, sums]), f
    # the same pointers with valid arguments pass: U == V, W absent, MX == AX
    assert gram(v=P_[0]) == _lib.PNL_OK and comb() == _lib.PNL_OK and resid(w=None) == _lib.PNL_OK and resid(mx=P_[0]) == _lib.PNL_OK
    ctx.synchronize()
    ctx.close()


# ---- (c), (d), (e) solvers.lobpcg on synthetic matrices --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name,n,withM', INPUTS)
def test_lobpcg_on_synthetic_matrices(name, n, withM):
    """(c), (d), (e) on the inputs of the table, A a Dense_LinearOperator (for dom(257) a CSR_LinearOperator of the same entries as
    well), M None or the CSR mass matrix; numpy in / numpy out and torch in / torch out; a run repeats bit for bit.
    Largest (rho_true - residuals[v]) / gap_v measured on an MI355X over all cases of this file: 0.0024 (dense lap(63), M = I, k = 4, m = 8); the H2
    cases stay below 0.0002."""
    import torch
    import scipy.sparse as sp
    from pynucleus_amd import solvers
    A, M, lam, lmin = problem(name, n, withM)
    Ms = sp.csr_matrix(M) if withM else None
    ctx = _context_with_dofs(n)
    ops = [('dense', _dense_operator(ctx, A), None)]
    if (name, n) == ('dom', 257):
        ops.append(('csr', _csr_operator(ctx, A), n))
    for kind, op, mA in ops:
        for k, m in km_of(name):
            what = '{} {}({}) M={} k={} m={}'.format(kind, name, n, withM, k, m)
            X0 = start_block(m, n)
            theta, X, passes, res = solvers.lobpcg(op, k, M=Ms, X0=X0, tol=TOL, maxiter=MAXITER, blockSize=m)
            assert isinstance(X, np.ndarray) and isinstance(theta, np.ndarray) and isinstance(res, np.ndarray), what
            assert_contracts(A, M, lam, lmin, theta, X, passes, res, k, MAXITER, what, mA=mA)
            if (k, m) == (4, 8):
                Xt = solvers.lobpcg(op, k, M=Ms, X0=torch.from_numpy(X0).cuda(), tol=TOL, maxiter=MAXITER, blockSize=m)
                assert isinstance(Xt[1], torch.Tensor) and Xt[1].is_cuda and Xt[2] == passes, what
                assert np.array_equal(Xt[1].cpu().numpy(), X) and np.array_equal(Xt[0], theta) and np.array_equal(Xt[3], res), what+' repeated'
    ctx.close()


@gpu
def test_lobpcg_start_and_maxiter():
    """maxiter = 0 returns the Rayleigh-Ritz values of X0 and its explicit residuals; a small maxiter reports maxiter; X0 with k rows
    and no X0 at all are completed from the seeded draw (a run repeats); the default block size; the arguments that raise.
    The comparisons of the maxiter = 0 result with the host's float64 computation are sanity margins, not contracts (rounding is of the
    order n u cond(X0 M X0^T) = 1e-13; a wrong Ritz value, residual or scaling is off by order one); the contracts are (c)-(e)"""
    import scipy.linalg as sla
    import scipy.sparse as sp
    from pynucleus_amd import solvers
    n, k, m = 257, 4, 8
    A, M, lam, lmin = problem('dom', n, True)
    Ms = sp.csr_matrix(M)
    ctx = _context_with_dofs(n)
    op = _dense_operator(ctx, A)
    X0 = start_block(m, n)
    theta, X, passes, res = solvers.lobpcg(op, k, M=Ms, X0=X0, maxiter=0, blockSize=m)
    ritz = sla.eigh(X0@A@X0.T, X0@M@X0.T, eigvals_only=True)
    assert passes == 0 and np.allclose(theta, ritz[:k], rtol=1e-9, atol=0.) and (res > TOL).all()
    R = X@A-theta[:, None]*(X@M)
    rho = np.linalg.norm(R, axis=1)/(theta*np.linalg.norm(X@M, axis=1))
    assert np.allclose(res, rho, rtol=1e-6, atol=0.) and np.allclose(np.einsum('ij,ij->i', X@M, X), 1., rtol=1e-9, atol=0.)
    t3, X3, p3, r3 = solvers.lobpcg(op, k, M=Ms, X0=X0, maxiter=3, blockSize=m)
    assert p3 == 3 and (r3 > TOL).any() and np.isfinite(X3).all() and np.isfinite(r3).all()
    a = solvers.lobpcg(op, k, M=Ms, X0=X0[:k], maxiter=MAXITER)
    b = solvers.lobpcg(op, k, M=Ms, X0=X0[:k], maxiter=MAXITER)
    c = solvers.lobpcg(op, k, M=Ms, maxiter=MAXITER)
    for out in (a, b, c):
        assert_contracts(A, M, lam, lmin, *out[:2], out[2], out[3], k, MAXITER, 'start')
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'a run repeats'
    none = solvers.lobpcg(op, 2, M=Ms, preconditioner=None, maxiter=MAXITER)
    assert_contracts(A, M, lam, lmin, *none[:2], none[2], none[3], 2, MAXITER, 'no preconditioner')
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(op, 17)
    with pytest.raises(ValueError):
        solvers.lobpcg(op, 4, blockSize=3)
    with pytest.raises(ValueError):
        solvers.lobpcg(op, 2, X0=X0[:3])
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(op, 2, preconditioner=lambda r: r)
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(op, 2, preconditioner='ilu')
    ctx.close()


# ---- (f) assembled operators -------------------------------------------------------------------------------------------------------

_CASES = {}


def _assembled(domain):
    """(hierarchy with mass matrices, host A, host M, eigenvalues, lambda_min(M)) of (-Delta)^0.75, P1: the interval with 127 DoFs,
    disc(2)"""
    import scipy.linalg as sla
    if domain not in _CASES:
        from pynucleus_amd import getFractionalKernel
        from pynucleus_amd.multigrid import fractionalHierarchy
        dim, noRef = (1, 6) if domain == 'interval' else (2, 2)
        H = fractionalHierarchy(domain, noRef, getFractionalKernel(dim, 0.75), {'target_order': 1.25} if dim == 1 else {'target_order': 0.5},
                                buildMass=True)
        Ah = np.array(H.finest['A'].toarray(), dtype=np.float64)
        Mh = np.asarray(H.finest['M'].toarray(), dtype=np.float64)
        _CASES[domain] = (H, Ah, Mh, sla.eigh(.5*(Ah+Ah.T), Mh, eigvals_only=True), float(np.linalg.eigvalsh(Mh)[0]))
    return _CASES[domain]


@gpu
@pytest.mark.parametrize('domain', ('interval', 'disc'))
def test_lobpcg_on_assembled_operators(domain):
    """(f) dense A with M = dm.assembleMass(), k = 4, Jacobi and the multigrid of the hierarchy (the object and its asPreconditioner());
    the Chebyshev smoother, a distributed operator and a plain callable raise"""
    from pynucleus_amd import solvers
    from pynucleus_amd.multigrid import multigrid
    from pynucleus_amd.linear_operators import DistributedDense_LinearOperator
    H, Ah, Mh, lam, lmin = _assembled(domain)
    A, M = H.finest['A'], H.finest['M']
    n = A.num_rows
    assert 63 <= n <= 127 or domain == 'disc'
    mg = multigrid(H)
    for pre, name in (('jacobi', 'jacobi'), (mg, 'mg'), (mg.asPreconditioner(), 'mg callable')):
        theta, X, passes, res = solvers.lobpcg(A, 4, M=M, tol=TOL, maxiter=MAXITER, preconditioner=pre)
        assert_contracts(Ah, Mh, lam, lmin, theta, X, passes, res, 4, MAXITER, '{} {}'.format(domain, name), mA=n)
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(A, 4, M=M, preconditioner=multigrid(H, smoother=('chebyshev', {'degree': 2})))
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(DistributedDense_LinearOperator(A.A, A.ctx), 4, M=M)
    with pytest.raises(NotImplementedError):
        solvers.lobpcg(A, 4, M=M, preconditioner=lambda r: r)


@gpu
@pytest.mark.parametrize('farField', ('ordered', None))
def test_lobpcg_on_the_h2_operator(farField):
    """(f) the H2 operator of the disc in both far-field modes, M = dm.assembleMass(), against the eigenvalues of its own matrix
    A.toarray().  disc(3), 169 DoFs: on the 37 DoFs of disc(2) no cluster pair is admissible and getH2 returns the dense operator"""
    import scipy.linalg as sla
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel, solvers
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.h2 import H2Matrix
    dm = P1_DoFMap(disc(3), PHYSICAL)
    M = dm.assembleMass()
    Mh = np.asarray(M.toarray(), dtype=np.float64)
    params = {'target_order': 0.5, 'eta': 3., 'minClusterSize': 12}
    if farField is not None:
        params['farField'] = farField
    A = nonlocalBuilder(dm, getFractionalKernel(2, 0.75), params, zeroExterior=True).getH2()
    assert isinstance(A, H2Matrix) and (farField is None or A.farField == farField)
    n = A.num_rows
    Ah = np.array(A.toarray(), dtype=np.float64)
    print('H2 {}: asymmetry of toarray() {:.3e}'.format(A.farField, np.abs(Ah-Ah.T).max()))
    lam = sla.eigh(.5*(Ah+Ah.T), Mh, eigvals_only=True)
    theta, X, passes, res = solvers.lobpcg(A, 4, M=M, tol=TOL, maxiter=MAXITER)
    assert_contracts(Ah, Mh, lam, float(np.linalg.eigvalsh(Mh)[0]), theta, X, passes, res, 4, MAXITER, 'H2 {}'.format(A.farField), mA=n,
                     skew=.5*float(np.linalg.norm(Ah-Ah.T)))
