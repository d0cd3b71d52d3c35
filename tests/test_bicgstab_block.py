"""BiCGStab for a block of right-hand sides of a GENERAL operator: pnl_bicgstab_block and its steps (pnl_bcgb_init / _start / _alpha /
_omega / _direction, csrc/pnl_bicgstab_block.hip) through the C ABI on SYNTHETIC non-symmetric matrices,
Dense_LinearOperator.solve_bicgstab_block, solvers.bicgstab_multi and the 2-D case of solvers.bicgstab.  Helpers come from
tests/test_cg_block.py, tests/test_apply_kernels.py and tests/test_block_products.py.  The yardstick is oracle.solver_oracle.bicgstab,
the numpy restatement of the reference's bicgstab_solver.solve.

No assertion uses a tolerance tuned on the code under test:

(1) exact.  A = dense storage of diag(d), d powers of two in [2^-3, 2^3], B small integers, x0 = 0, Jacobi: every sum is an exact dyadic
    number, alpha = 1, S = 0, T2 = 0 and omega := 0 by the lucky-breakdown rule, so X == B / d bit for bit with 0 iterations and
    residual exactly 0, at every size, number of columns and layout.  (The oracle divides 0 / 0 there and returns NaN.)  Without a
    preconditioner the same matrix must still converge and obey (4).
(2) independence.  X[v], iterations[v] and residuals[v] of a block solve have the bits of the solve of B[v] alone, wherever the column
    stands and whatever the others are (a zero column, a column scaled by 1e6, a column that breaks down); two calls repeat bit for
    bit; a converged column is bit-identical before and after further passes (it is converged while its slower neighbours go on).
(3) the stopping contract, judged against the oracle: a column must report residual < tol and iterations < maxiter wherever the oracle
    converges on the same data within maxiter // 2 passes.  With maxiter = 100 for nsdom, 160 for cd(63) / cd(65) and 600 for cd(257)
    that is every non-zero column of the first six of every block (the three scales twice) at n > 2:
    test_oracle_converges_within_half_the_cap asserts it without a GPU.  The GPU tests apply the rule itself to all 33 columns: up to
    n = 257 the demanded columns are computed with the oracle (demanded); of the 33 columns of this file that leaves out two of cd(257),
    which the oracle solves in 302 and 303 passes, and those of nsdom(2) on which the oracle hits the solution exactly and returns NaN.
    Above n = 257, where the oracle takes at most 36 passes, every non-zero column is demanded.  Every other
    column must report consistently: maxiter with a finite residual >= tol, or fewer passes with a residual >= tol (a breakdown).  A
    small maxiter cuts columns off at maxiter; maxiter = 0 returns the start residual and leaves X alone; the zero column reports 0
    iterations and residual 0.
(4) true residual.  For every column that reports convergence rho_v = || b_v - A x_v ||_2, in np.longdouble on the host (mpmath where
    that has 64 bits), must satisfy rho_v <= tol + gap_v,
        gap_v = 4 (k_v + 2) (m + 6) u (|| |A| |x_v| ||_2 + || b_v ||_2),   u = 2^-53, m = entries per row, k_v = the iteration count.
    Per pass the recursive residual r and the true residual b - A x drift apart by: the two products, T = A P2 and T2 = A S2, each with
    an error of at most (m + 2) u |A| |.| ; the roundings of S = R - alpha T and R = S - omega T2 (2 u each per element with the fma);
    the roundings of the two updates of X, multiplied by |A|: 2 x 2 u |A| |x|; and the preconditioner's rounding u |P2|, u |S2| inside
    the products.  With |alpha P2| + |omega S2| of the order of |x| over the pass this is at most about (2 (m + 2) + 8) u
    (|A| |x| + |b|) per pass; the factor 4 covers the constants and the growth of the intermediate iterates.  The sum over k_v passes
    (Greenbaum 1997, Theorem 2.2, in the simplified form of the sum of the per-step errors) is NOT capped at 50: this solver never
    recomputes its residual.  The drift term is measured, not derived, so the condition that keeps the bound honest is that the numpy
    restatement (the oracle) stays under 1 % of the gap on these matrices: test_oracle_meets_the_bound_far_inside, on the first six
    columns of every block (measured there: at most 1e-5 of the gap for nsdom, 0.0064 for cd(257) at 300 passes).  It does not on
    every one of the 33 columns: see the spiking column below, where the oracle itself uses most of the gap.  A wrong index, a missed tail element, A^T in place of A or a
    column mix-up gives rho of the order of ||b||.  Largest (rho_v - residuals[v]) / gap_v measured on an MI355X over all cases of
    this file: 0.873, on column 29 of cd(65), whose residual history spikes to 2200 times the start residual in a pass with a small
    omega; the oracle has 0.883 on the same column, so this is the recurrence and not the kernels.  Every other case: at most 0.019.
(5) the steps on integer blocks: the dot products read back from the state (T.R0, T2.S, T2.T2, R.R, R.R0) equal int64 numpy sums bit
    for bit, including n = 65535 / 65536 / 65537 / 131073; the external mode leaves P2 / S2 untouched; an engineered T.R0 == 0 freezes
    the column with the breakdown code and leaves its blocks bit-identical and finite.
(6) validation: every PNL_ERR_INVALID case of the header returns before any launch, outputs stay poisoned.

Edges: 256 threads per workgroup and at most 256 workgroups for the vector kernels; 128 rows, 64 and 2048 columns of k_gemv_block; 16
columns per group (15 / 16 / 17 / 33).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import solver_oracle as SO
from test_apply_kernels import U, LD, LD_OK, hp_dot, _context, _context_with_dofs, _dev, _dev_matrix
from test_block_products import block_image, _dev_block
from test_cg_block import LAYOUTS, NVECS, DOM_SIZES, SCALES, rhs_block, _assert_same, _csr_operator

gpu = pytest.mark.gpu

TOL = 1e-8
CD_SIZES = (63, 65, 257)
ST = 12                                        # PNL_BCGB_STATE
ST_KAPPA, ST_ALPHA, ST_OMEGA, ST_RES, ST_ACTIVE, ST_KAPPA_NEW, ST_CODE, ST_TR0, ST_T2S, ST_T2T2, ST_RR, ST_BETA = range(12)
CODE_TR0 = 1


# ---- synthetic problems and the yardstick (plain numpy; tested below without a GPU) ----------------------------------------------

def nsdom(n, seed=0):
    """S = G H^T with two independent standard_normal((n, min(n, 8))) factors, the diagonal replaced by
    uniform(1.5, 4) (1 + sum_j!=i |S_ij|): strictly row-dominant, the off-diagonal part genuinely non-symmetric"""
    rng = np.random.default_rng(9500+n+seed)
    G, H = rng.standard_normal((n, min(n, 8))), rng.standard_normal((n, min(n, 8)))
    S = G@H.T
    np.fill_diagonal(S, 0.)
    np.fill_diagonal(S, rng.uniform(1.5, 4., size=n)*(1.+np.abs(S).sum(axis=1)))
    return S


def cd(n):
    """tridiag(-1.5, 2, -0.5) stored dense: a convection-diffusion stencil, strongly non-symmetric, slow to converge"""
    return 2.*np.eye(n)-0.5*np.eye(n, k=1)-1.5*np.eye(n, k=-1)


def matrix(name, n):
    return nsdom(n) if name == 'nsdom' else cd(n)


def maxiter_of(name, n):
    return 100 if name == 'nsdom' else (600 if n == 257 else 160)


def entries_per_row(name, n):
    return n if name == 'nsdom' else min(n, 3)


def jac(A):
    dinv = 1./np.diagonal(A)
    return lambda r: dinv*r


def true_residual(A, b, x):
    """rho = || b - A x ||_2 in np.longdouble (mpmath where that has 64 bits)"""
    if LD_OK:
        r = b.astype(LD)-A.astype(LD)@x.astype(LD)
        return float(np.sqrt((r*r).sum()))
    import mpmath
    r = [mpmath.mpf(float(b[i]))-hp_dot(A[i], x)[0] for i in range(A.shape[0])]
    return float(mpmath.sqrt(mpmath.fsum(ri*ri for ri in r)))


def gap(A, b, x, k, m, x0=None):
    """the gap of (4); from a non-zero guess || |A| |x| || is the larger of the guess's and the solution's"""
    ax = np.linalg.norm(np.abs(A)@np.abs(x))
    if x0 is not None:
        ax = max(ax, np.linalg.norm(np.abs(A)@np.abs(x0)))
    return 4.*(int(k)+2)*(m+6)*U*float(ax+np.linalg.norm(b))


WORST = {'ratio': -np.inf}


def assert_true_residual(A, B, X, its, res, tol, what, m, cols=None, X0=None):
    """assertion (4) for every column (of cols: those that report convergence); prints the largest (rho - residual) / gap it has seen"""
    for v in (range(B.shape[0]) if cols is None else np.nonzero(cols)[0]):
        rho = true_residual(A, B[v], X[v])
        g = gap(A, B[v], X[v], its[v], m, None if X0 is None else X0[v])
        if g > 0.:
            WORST['ratio'] = max(WORST['ratio'], (rho-res[v])/g)
        assert rho <= tol+g, '{} column {}: true residual {:.3e} > tol {:.1e} + gap {:.3e} ({} iterations, reported {:.3e})'.format(
            what, v, rho, tol, g, its[v], res[v])
    print('BCGB_GAP_RATIO {} largest (rho - residual) / gap so far: {:.3e}'.format(what, WORST['ratio']))


_DEMANDED = {}


def demanded(name, n, jacobi):
    """(3): the columns of rhs_block(n, 33) on which the oracle converges within maxiter // 2 passes; above n = 257 every non-zero one"""
    key = (name, n, bool(jacobi))
    if key not in _DEMANDED:
        kmax = max(NVECS)
        B = rhs_block(n, kmax)
        need = B.any(axis=1)
        if n <= 257:
            A = matrix(name, n)
            mi = maxiter_of(name, n)
            with np.errstate(all='ignore'):
                for v in np.nonzero(need)[0]:
                    x, it, res = SO.bicgstab(A, B[v], tol=TOL, maxiter=mi, B=jac(A) if jacobi else None)
                    need[v] = bool(res[-1] < TOL) and it <= mi//2
        _DEMANDED[key] = need
    return _DEMANDED[key]


def assert_stopping(its, res, need, maxiter, what):
    """(3): the needed columns converge below maxiter; every column reports consistently.  Returns the columns that report convergence"""
    its, res = np.asarray(its), np.asarray(res)
    assert (res[need] < TOL).all() and (its[need] < maxiter).all(), (what, its, res)
    assert np.isfinite(res).all() and (its <= maxiter).all() and (its >= 0).all(), (what, its, res)
    done = res < TOL
    assert (its[done] < maxiter).all(), (what, its, res)                 # the others: maxiter, or a breakdown (fewer passes), residual >= tol
    return done


# ---- CPU-only -------------------------------------------------------------------------------------------------------------------

def test_nsdom_is_row_dominant_and_not_symmetric():
    for n in (2, 65, 257):
        A = nsdom(n)
        d = np.diagonal(A)
        off = np.abs(A).sum(axis=1)-np.abs(d)
        assert (d > off).all()
        offd = A-np.diag(d)
        assert np.abs(A-A.T).max() > 0.5*np.abs(offd).max(), n         # of the order of the off-diagonal entries
    A = cd(65)
    assert A[1, 0] == -1.5 and A[0, 1] == -0.5 and A[0, 0] == 2. and np.count_nonzero(A) == 3*65-2


@pytest.mark.parametrize('name,n', tuple(('nsdom', n) for n in DOM_SIZES if n > 1)+tuple(('cd', n) for n in CD_SIZES))
def test_oracle_converges_within_half_the_cap(name, n):
    """(3) the demand of the GPU tests: the oracle converges within maxiter // 2 passes on the first six columns (the three scales, twice)
    of the block the GPU tests use, with and without Jacobi.  n = 2: the second pass hits the solution exactly on some columns, S = 0,
    and the oracle returns NaN: such a column is not demanded (the library's lucky-breakdown rule solves it).  n = 1 likewise:
    test_bicgstab_block_exact.  demanded() agrees and leaves out only what the module docstring lists"""
    A = matrix(name, n)
    B = rhs_block(n, max(NVECS))[:6]
    mi = maxiter_of(name, n)
    for prec in (None, jac(A)):
        for v in range(6):
            assert B[v].any()
            with np.errstate(all='ignore'):
                x, it, res = SO.bicgstab(A, B[v], tol=TOL, maxiter=mi, B=prec)
            if n == 2 and np.isnan(res[-1]):
                continue
            assert res[-1] < TOL and it <= mi//2, (name, n, v, it, res[-1])
        need = demanded(name, n, prec is not None)
        out = np.nonzero(~need)[0].tolist()
        assert need[:6].all() or n == 2
        assert out == [max(NVECS)//2] or n == 2 or (name, n, out) == ('cd', 257, [8, 14, 16]), (name, n, out)


@pytest.mark.parametrize('name,n', (('nsdom', 65), ('nsdom', 1025), ('cd', 65), ('cd', 257)))
def test_oracle_meets_the_bound_far_inside(name, n):
    """(4) the yardstick itself: the oracle's true residual exceeds tol by less than 1 % of the gap, with and without Jacobi; a wrong
    column or A^T in place of A is far outside"""
    A = matrix(name, n)
    B = rhs_block(n, max(NVECS))[:6]
    m = entries_per_row(name, n)
    for prec in (None, jac(A)):
        for v in range(6):
            x, it, res = SO.bicgstab(A, B[v], tol=TOL, maxiter=maxiter_of(name, n), B=prec)
            rho, g = true_residual(A, B[v], x), gap(A, B[v], x, it, m)
            assert res[-1] < TOL and rho-TOL <= 0.01*g, (name, n, v, it, rho, g)
    x, it, res = SO.bicgstab(A, B[0], tol=TOL, maxiter=maxiter_of(name, n))
    assert true_residual(A, B[3], x) > 1e3*(TOL+gap(A, B[3], x, it, m))
    assert true_residual(A.T, B[0], x) > 1e3*(TOL+gap(A, B[0], x, it, m))


def test_oracle_breaks_down_where_the_rules_apply():
    """the cases the library's breakdown rules are for: the oracle returns NaN on the exact diagonal case and on a 1 x 1 system"""
    with np.errstate(all='ignore'):
        x, it, res = SO.bicgstab(np.array([[2.]]), np.array([3.]), tol=TOL, maxiter=5)
        assert it == 5 and np.isnan(x).all()
        d = 2.**np.arange(-3, 4)
        x, it, res = SO.bicgstab(np.diag(d), np.arange(1., 8.), tol=TOL, maxiter=5, B=lambda r: r/d)
        assert np.isnan(x).all()


def test_abi_declares_the_block_bicgstab():
    """the header, the binding and the library agree on the new symbols (tests/test_abi.py checks the whole list)"""
    import os
    from pynucleus_amd import _lib
    from test_abi import declared_symbols
    new = {'pnl_bicgstab_block', 'pnl_bcgb_init', 'pnl_bcgb_start', 'pnl_bcgb_alpha', 'pnl_bcgb_omega', 'pnl_bcgb_direction'}
    assert new <= set(declared_symbols()) and new <= set(_lib.EXPORTS)
    assert os.path.exists(_lib.LIB_PATH), 'build the HIP library first (__graft_entry__.build())'
    L = C.CDLL(_lib.LIB_PATH)
    for name in new:
        assert hasattr(L, name), name
    assert _lib.PNL_BCGB_STATE == ST


# ---- pnl_bicgstab_block ---------------------------------------------------------------------------------------------------------

def _solve(ctx, Aptr, ldA, n, B, X0, tol, maxiter, jacobi, dB=0, dX=0, oB=0, oX=0):
    """one call; returns (X, iterations, residuals) after checking the whole allocations of X (padding, guards) and B (unchanged)"""
    k = B.shape[0]
    bs, bp = _dev_block(B, n+dB, oB)
    xs, xp = _dev_block(np.zeros((k, n)) if X0 is None else X0, n+dX, oX)
    its, res = ctx.bicgstab_block(Aptr, ldA, n, k, jacobi, bp, n+dB, xp, n+dX, tol, maxiter)
    ctx.synchronize()
    got = xs.cpu().numpy()
    X = got[oX:oX+k*(n+dX)].reshape(k, n+dX)[:, :n].copy()
    assert np.array_equal(got, block_image(X, n+dX, oX)), 'padding column or guard element of X overwritten'
    assert np.array_equal(bs.cpu().numpy(), block_image(B, n+dB, oB)), 'B was written'
    return X, its, res


@gpu
@pytest.mark.parametrize('n', DOM_SIZES)
def test_bicgstab_block_exact(n):
    """(1) at every size, layout and number of columns; column nrhs // 2 is zero and stays zero; no NaN anywhere.  Without a
    preconditioner the diagonal system converges and obeys (4)"""
    ctx = _context()
    rng = np.random.default_rng(9600+n)
    d = 2.**rng.integers(-3, 4, size=n)
    core = _dev(np.diag(d))
    Bfull = rng.integers(-8, 9, size=(max(NVECS), n)).astype(np.float64)
    for dA, dB, dX, oA, oB, oX in LAYOUTS:
        store, Av = _dev_matrix(core, n+dA, oA)
        for k in NVECS:
            B = Bfull[:k].copy()
            if k >= 2:
                B[k//2] = 0.
            X, its, res = _solve(ctx, Av.data_ptr(), n+dA, n, B, None, TOL, 50, True, dB, dX, oB, oX)
            tag = 'n={} nrhs={} layout {}'.format(n, k, (dA, dB, dX, oA, oB, oX))
            assert np.array_equal(X, B/d[None, :]), tag
            assert not its.any() and not res.any() and its.shape == res.shape == (k,), (tag, its, res)
        assert np.array_equal(store.cpu().numpy(), block_image(np.diag(d), n+dA, oA)), 'A was written'
    # no preconditioner: BiCGStab on a diagonal matrix with up to seven distinct eigenvalues
    store, Av = _dev_matrix(core, n+1, 1)
    B = Bfull[:17].copy()
    B[8] = 0.
    X, its, res = _solve(ctx, Av.data_ptr(), n+1, n, B, None, TOL, 50, False, 1, 6, 0, 1)
    done = assert_stopping(its, res, np.zeros(17, dtype=bool), 50, 'diag({}) without preconditioner'.format(n))
    nz = B.any(axis=1)
    assert np.isfinite(X).all() and done[nz].all() and its[8] == 0 and res[8] == 0. and not X[8].any(), (its, res)
    assert_true_residual(np.diag(d), B, X, its, res, TOL, 'diag({})'.format(n), 1, cols=done)
    ctx.close()


@gpu
@pytest.mark.parametrize('jacobi', (True, False))
@pytest.mark.parametrize('name,n', tuple(('nsdom', n) for n in DOM_SIZES)+tuple(('cd', n) for n in CD_SIZES))
def test_bicgstab_block_columns_are_independent(name, n, jacobi):
    """(2), (3), (4) on nsdom(n) and cd(n): every column of blocks of 1 .. 33 right-hand sides, of a permuted block and of a repeated
    call has the bits of its solo solve; every non-zero column converges below maxiter (the oracle does within maxiter // 2:
    test_oracle_converges_within_half_the_cap); the true residual obeys the bound"""
    A = matrix(name, n)
    kmax = max(NVECS)
    B = rhs_block(n, kmax)
    ctx = _context()
    dA, dB, dX, oA, oB, oX = LAYOUTS[n % len(LAYOUTS)]
    store, Av = _dev_matrix(_dev(A), n+dA, oA)
    maxiter = maxiter_of(name, n)

    def run(Bk, X0=None):
        return _solve(ctx, Av.data_ptr(), n+dA, n, Bk, X0, TOL, maxiter, jacobi, dB, dX, oB, oX)
    solo = [run(B[v:v+1]) for v in range(kmax)]
    assert np.isfinite(np.stack([s[0][0] for s in solo])).all()
    for v in (0, kmax//2):
        _assert_same(run(B[v:v+1]), solo[v], 'repeated solo solve {}'.format(v))
    for k in NVECS:
        X, its, res = run(B[:k])
        for v in range(k):
            _assert_same((X[v], its[v], res[v]), (solo[v][0][0], solo[v][1][0], solo[v][2][0]), '{}({}) nrhs={} column {}'.format(name, n, k, v))
    X, its, res = run(B)
    _assert_same(run(B), (X, its, res), 'repeated call')
    # (3): n = 1 is solved by the lucky-breakdown rule in the first pass
    need = demanded(name, n, jacobi) if n > 1 else np.arange(kmax) != kmax//2
    done = assert_stopping(its, res, need, maxiter, '{}({})'.format(name, n))
    assert its[kmax//2] == 0 and res[kmax//2] == 0. and not X[kmax//2].any()
    if n > 2:
        assert need.sum() >= kmax-3 and len(set(its[need].tolist())) > 1, its                 # columns froze at different times: frozen ones were carried along
    perm = np.random.default_rng(n).permutation(kmax)
    _assert_same(run(B[perm]), (X[perm], its[perm], res[perm]), 'permuted block')
    # (4)
    assert_true_residual(A, B, X, its, res, TOL, '{}({}){}'.format(name, n, ' jacobi' if jacobi else ''), entries_per_row(name, n), cols=done)
    ctx.close()


@gpu
def test_bicgstab_block_maxiter_and_initial_guess():
    """(3) on cd(257): maxiter = 2 cuts every column off (iterations == 2, residual >= tol, finite X, the solo bits) but the zero one,
    which is frozen from the start; maxiter = 0 returns the start residual sqrt(|r . M^-1 r|) and leaves X (a non-zero guess) untouched;
    a solve from a non-zero guess obeys (2), (3) and (4) too"""
    n, k = 257, 17
    A, B = cd(n), rhs_block(n, 17)
    ctx = _context()
    store, Av = _dev_matrix(_dev(A), n+1, 1)
    X, its, res = _solve(ctx, Av.data_ptr(), n+1, n, B, None, TOL, 2, True, 1, 6, 0, 1)
    cut = np.arange(k) != k//2
    assert (its[cut] == 2).all() and (res[cut] >= TOL).all() and its[k//2] == 0 and res[k//2] == 0. and not X[k//2].any(), (its, res)
    assert np.isfinite(X).all() and np.isfinite(res).all()
    for v in range(k):
        _assert_same(_solve(ctx, Av.data_ptr(), n+1, n, B[v:v+1], None, TOL, 2, True, 0, 1, 1, 0), (X[v:v+1], its[v:v+1], res[v:v+1]),
                     'maxiter = 2, column {}'.format(v))
    X0 = np.random.default_rng(5).standard_normal((k, n))
    Xz, iz, rz = _solve(ctx, Av.data_ptr(), n+1, n, B, X0, TOL, 0, True, 1, 6, 0, 1)
    assert np.array_equal(Xz, X0) and not iz.any()
    for v in range(k):
        r = B[v]-A@X0[v]
        want = np.sqrt(r@(r/2.))
        assert abs(rz[v]-want) <= 1e-12*want, (v, rz[v], want)         # the start residual (a sanity check of its meaning only)
    Xg, ig, rg = _solve(ctx, Av.data_ptr(), n+1, n, B, X0, TOL, 600, True, 6, 0, 1, 1)
    scale1 = np.array(SCALES)[np.arange(k) % 3] != 1e-6                # from a guess of size 1 every column is a size-1 problem; demand
    done = assert_stopping(ig, rg, scale1, 600, 'from a guess')         # those whose right-hand side is not dwarfed by it as well
    _assert_same(_solve(ctx, Av.data_ptr(), n+1, n, B[3:4], X0[3:4], TOL, 600, True), (Xg[3:4], ig[3:4], rg[3:4]), 'solo from a guess')
    assert_true_residual(A, B, Xg, ig, rg, TOL, 'cd(257) from a guess', 3, cols=done, X0=X0)
    ctx.close()


@gpu
def test_bicgstab_block_breakdown_column_is_frozen_and_alone():
    """(2) with a column that breaks down: nsdom(65) with A[0, 0] = 0, no preconditioner, b = 3 e_0 gives T = 3 A[:, 0], T . R0 = 9 A[0, 0]
    = 0 in the first pass: 0 iterations, the start residual 3 >= tol, X untouched and finite.  The other columns keep the bits of
    their solo solves and report consistently"""
    n = 65
    A = nsdom(n)
    A[0, 0] = 0.
    B = rhs_block(n, 5)
    B[1] = 0.
    B[1, 0] = 3.
    ctx = _context()
    store, Av = _dev_matrix(_dev(A), n+1, 0)
    X, its, res = _solve(ctx, Av.data_ptr(), n+1, n, B, None, TOL, 100, False, 1, 6, 0, 1)
    assert its[1] == 0 and res[1] == 3. and not X[1].any(), (its, res)
    assert np.isfinite(X).all() and np.isfinite(res).all()
    done = assert_stopping(its, res, np.zeros(5, dtype=bool), 100, 'breakdown block')
    assert not done[1] and its[2] == 0 and res[2] == 0.
    for v in range(5):
        _assert_same(_solve(ctx, Av.data_ptr(), n+1, n, B[v:v+1], None, TOL, 100, False), (X[v:v+1], its[v:v+1], res[v:v+1]), 'solo {}'.format(v))
    assert_true_residual(A, B, X, its, res, TOL, 'nsdom(65) with a zero pivot', n, cols=done)
    ctx.close()


# ---- the steps ------------------------------------------------------------------------------------------------------------------

def _state(t):
    return t.cpu().numpy().reshape(-1, ST).copy()


def _isum(a, b, scale):
    """sum a*b of arrays whose entries are multiples of 1 / scale, in int64, as a double"""
    return ((a*scale).astype(np.int64)*(b*scale).astype(np.int64)).sum(axis=1)/float(scale*scale)


@gpu
@pytest.mark.parametrize('n', (1, 255, 256, 257, 65535, 65536, 65537, 131073))
def test_bcgb_steps_on_integer_blocks(n):
    """(5): init, start, alpha, omega and direction on integer blocks (dinv powers of two), nvec = 16 and 3, with padding, in both
    preconditioner modes.  The state is crafted on the host between the calls so that alpha, omega and beta are dyadic: every vector is
    then exact and compared bit for bit, the dots with int64 sums.  Column 1 is frozen from the start (zero residual) and column 2 (of
    16) is engineered to T . R0 == 0: nothing of them changes."""
    import torch
    ctx = _context()
    rng = np.random.default_rng(9700+n)
    for nv, pad in ((16, 3), (3, 0)):
        ld = n+pad
        dinv = 2.**rng.integers(-2, 3, size=n)
        ints = lambda lo=-16, hi=17: rng.integers(lo, hi, size=(nv, n)).astype(np.float64)
        blk = lambda core: _dev_block(core, ld, 1)
        img = lambda store: store.cpu().numpy()
        same = lambda store, core: np.array_equal(img(store), block_image(core, ld, 1))
        seven = np.full((nv, n), 7.)
        dv = _dev(dinv)
        Bh, AXh = ints(), ints()
        AXh[1] = Bh[1]                                                # column 1: zero residual, never active
        (bs, bp), (axs, axp) = blk(Bh), blk(AXh)
        # ---- init, Jacobi mode: R, P, R0, P2 and the state
        (rs, rp), (ps, pp), (r0s, r0p), (p2s, p2p) = blk(seven), blk(seven), blk(seven), blk(seven)
        state = torch.full((nv*ST,), 77., dtype=torch.float64, device='cuda')
        ctx.bcgb_init(n, nv, False, dv.data_ptr(), bp, ld, axp, ld, rp, ld, pp, ld, r0p, ld, p2p, ld, state.data_ptr())
        ctx.synchronize()
        Rh = Bh-AXh
        R0h = dinv*Rh
        kap = _isum(Rh, R0h, 4)
        st = _state(state)
        assert same(rs, Rh) and same(ps, Rh) and same(r0s, R0h) and same(p2s, R0h)
        assert np.array_equal(st[:, ST_KAPPA], kap) and np.array_equal(st[:, ST_RES], np.sqrt(np.abs(kap)))
        assert np.array_equal(st[:, ST_ACTIVE], (kap != 0.).astype(np.float64)) and st[1, ST_ACTIVE] == 0.
        rest = [k for k in range(ST) if k not in (ST_KAPPA, ST_RES, ST_ACTIVE)]
        assert not st[:, rest].any()
        # ---- init, external mode: R and P only; then start from the caller's R0 (integers of either sign: kappa may be negative)
        (rs, rp), (ps, pp), (r0s, r0p), (p2s, p2p) = blk(seven), blk(seven), blk(seven), blk(seven)
        state.fill_(77.)
        ctx.bcgb_init(n, nv, True, 0, bp, ld, axp, ld, rp, ld, pp, ld, r0p, ld, p2p, ld, state.data_ptr())
        ctx.synchronize()
        assert same(rs, Rh) and same(ps, Rh) and same(r0s, seven) and same(p2s, seven) and bool((state == 77.).all())
        R0h = ints()
        R0h[1] = 0.
        r0s, r0p = blk(R0h)
        ctx.bcgb_start(n, nv, rp, ld, r0p, ld, state.data_ptr())
        ctx.synchronize()
        kap = _isum(Rh, R0h, 1)
        st = _state(state)
        assert np.array_equal(st[:, ST_KAPPA], kap) and np.array_equal(st[:, ST_RES], np.sqrt(np.abs(kap)))
        assert np.array_equal(st[:, ST_ACTIVE], (kap != 0.).astype(np.float64)) and not st[:, rest].any()
        assert same(rs, Rh) and same(r0s, R0h)
        # ---- alpha: T from the host; kappa crafted so that alpha = 2^e; column 2 of 16 has T = 0: T . R0 == 0
        Th = ints()
        bad = 2 if nv > 3 else None
        if bad is not None:
            Th[bad] = 0.
        tr0 = _isum(Th, R0h, 1)
        act = np.ones(nv)
        act[1] = 0.
        act[(tr0 == 0.) & (np.arange(nv) != (bad if bad is not None else -1))] = 0.     # a chance zero (n = 1): park the column
        e = rng.integers(-2, 3, size=nv)
        st[:, ST_KAPPA], st[:, ST_ACTIVE] = tr0*2.**e, act
        if bad is not None:
            st[bad, ST_KAPPA] = 5.
        on = act != 0.
        if bad is not None:
            on[bad] = False                                           # active, but it breaks down
        on2 = on[:, None]
        Sh = np.where(on2, Rh-2.**e[:, None]*Th, Rh)
        for ext in (True, False):
            state.copy_(torch.from_numpy(st.reshape(-1)))
            (rs, rp), (s2s, s2p), (ts, tp) = blk(Rh), blk(seven), blk(Th)
            ctx.bcgb_alpha(n, nv, ext, dv.data_ptr(), tp, ld, r0p, ld, rp, ld, s2p, ld, state.data_ptr())
            ctx.synchronize()
            st1 = _state(state)
            S2h = seven if ext else np.where(on2, dinv*Sh, 7.)
            assert same(rs, Sh) and same(s2s, S2h) and same(ts, Th) and same(r0s, R0h), ext
            assert np.array_equal(st1[on, ST_ALPHA], 2.**e[on]) and np.array_equal(st1[act != 0., ST_TR0], tr0[act != 0.])
            assert np.array_equal(st1[1], st[1]), 'state of the frozen column changed'
            if bad is not None:
                assert st1[bad, ST_CODE] == CODE_TR0 and st1[bad, ST_TR0] == 0. and st1[bad, ST_KAPPA] == 5.
            assert not st1[on, ST_CODE].any() and np.array_equal(st1[:, ST_KAPPA], st[:, ST_KAPPA])
        S2h = np.where(on2, dinv*Sh, 7.)
        # ---- omega (i): T2 random integers: the sums T2 . S and T2 . T2 over every element, omega by the same IEEE division
        T2h = ints()
        P2h, Xh = ints(), ints()
        (t2s_, t2p), (p2s, p2p), (xs, xp) = blk(T2h), blk(P2h), blk(Xh)
        base = st1.copy()
        ctx.bcgb_omega(n, nv, p2p, ld, s2p, ld, t2p, ld, r0p, ld, xp, ld, rp, ld, 0., state.data_ptr())
        ctx.synchronize()
        st2 = _state(state)
        t2s, t2t2 = _isum(T2h, Sh, 4), _isum(T2h, T2h, 1)
        assert np.array_equal(st2[on, ST_T2S], t2s[on]) and np.array_equal(st2[on, ST_T2T2], t2t2[on])
        with np.errstate(all='ignore'):
            assert np.array_equal(st2[on, ST_OMEGA], np.where(t2t2 == 0., 0., t2s/t2t2)[on])
        assert np.array_equal(st2[1], st[1])
        if bad is not None:                                            # frozen by the step behind the breakdown: code kept, res kept, blocks kept
            assert st2[bad, ST_ACTIVE] == 0. and st2[bad, ST_CODE] == CODE_TR0 and st2[bad, ST_RES] == base[bad, ST_RES]
            got = img(xs)[1:1+nv*ld].reshape(nv, ld)[bad, :n], img(rs)[1:1+nv*ld].reshape(nv, ld)[bad, :n]
            assert np.array_equal(got[0], Xh[bad]) and np.array_equal(got[1], Rh[bad]) and np.isfinite(got[0]).all()
        # ---- omega (ii): T2 = +-1 in at most four places (first, last, two inside): omega is a multiple of 1/16, every vector exact
        T2h = np.zeros((nv, n))
        for pos in sorted({0, n//3, (2*n)//3, n-1}):
            T2h[:, pos] = rng.choice([-1., 1.], size=nv)
        K = float(np.count_nonzero(T2h[0]))
        if K == 3.:                                                   # keep T2 . T2 a power of two
            T2h[:, (2*n)//3] = 0.
            K = 2.
        t2s, t2t2 = _isum(T2h, Sh, 4), np.full(nv, K)
        om = t2s/t2t2
        al = st1[:, ST_ALPHA]
        live = on.copy()
        Xn = np.where(live[:, None], Xh+al[:, None]*P2h+om[:, None]*S2h, Xh)
        Rn = np.where(live[:, None], Sh-om[:, None]*T2h, Sh)
        rr, kn = _isum(Rn, Rn, 16), _isum(Rn, R0h, 16)
        res = np.sqrt(rr)
        pos_res = np.sort(res[live & (res > 0.)])
        tol = float(pos_res[len(pos_res)//2]) if len(pos_res) else 0.5       # strict: the column with this residual goes on
        state.copy_(torch.from_numpy(base.reshape(-1)))
        (rs, rp), (t2s_, t2p), (xs, xp) = blk(Sh), blk(T2h), blk(Xh)
        ctx.bcgb_omega(n, nv, p2p, ld, s2p, ld, t2p, ld, r0p, ld, xp, ld, rp, ld, tol, state.data_ptr())
        ctx.synchronize()
        st3 = _state(state)
        assert same(xs, Xn) and same(rs, Rn) and same(p2s, P2h) and same(s2s, S2h) and same(t2s_, T2h) and same(r0s, R0h)
        assert np.array_equal(st3[live, ST_RR], rr[live]) and np.array_equal(st3[live, ST_KAPPA_NEW], kn[live])
        assert np.array_equal(st3[live, ST_RES], res[live]) and np.array_equal(st3[live, ST_OMEGA], om[live])
        conv = live & (res < tol)
        with np.errstate(all='ignore'):
            beta = kn/base[:, ST_KAPPA]*al/om
        brk = live & ~conv & ((om == 0.) | (kn == 0.) | ~np.isfinite(beta))
        go = live & ~conv & ~brk
        assert np.array_equal(st3[:, ST_ACTIVE], go.astype(np.float64)), (st3[:, ST_ACTIVE], go)
        assert np.array_equal(st3[go, ST_BETA], beta[go]) and np.array_equal(st3[go, ST_KAPPA], kn[go])
        assert not st3[conv, ST_CODE].any() and (st3[brk, ST_CODE] != 0.).all() and np.array_equal(st3[~go, ST_KAPPA], base[~go, ST_KAPPA])
        assert np.array_equal(st3[1], st[1])
        if n > 255 and nv == 16:
            assert go.any() and conv.any()
        # ---- direction: beta and omega crafted as powers of two; both modes
        f, g = rng.integers(-2, 3, size=nv), rng.integers(-2, 3, size=nv)
        st3[:, ST_BETA], st3[:, ST_OMEGA] = 2.**f, 2.**g
        Ph, Th = ints(), ints()
        Pn = np.where(go[:, None], Rn+2.**f[:, None]*(Ph-2.**g[:, None]*Th), Ph)
        for ext in (False, True):
            state.copy_(torch.from_numpy(st3.reshape(-1)))
            (ps, pp), (p2s, p2p), (ts, tp) = blk(Ph), blk(seven), blk(Th)
            ctx.bcgb_direction(n, nv, ext, dv.data_ptr(), rp, ld, tp, ld, pp, ld, p2p, ld, state.data_ptr())
            ctx.synchronize()
            assert same(ps, Pn) and same(p2s, seven if ext else np.where(go[:, None], dinv*Pn, 7.)) and same(ts, Th) and same(rs, Rn), ext
            assert np.array_equal(_state(state), st3), 'direction wrote the state'
        for s_, core in ((bs, Bh), (axs, AXh)):
            assert same(s_, core), 'an input block was written'
    ctx.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

@gpu
def test_bicgstab_block_validation():
    """(6) every invalid argument of the header returns PNL_ERR_INVALID and leaves X (a sentinel) untouched"""
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    n, k = 7, 3
    t = lambda *shape, fill=1.: torch.full(shape, fill, dtype=torch.float64, device='cuda')
    A, B, X = torch.eye(n, dtype=torch.float64, device='cuda')*2., t(k, n), t(k, n, fill=77.)
    its, res = (C.c_int*k)(), (C.c_double*k)()
    p = lambda v: C.c_void_p(v) if v else None
    good = dict(ctx=ctx.h, A=A.data_ptr(), ldA=n, n=n, nrhs=k, B=B.data_ptr(), ldb=n, X=X.data_ptr(), ldx=n, tol=TOL, maxiter=10)

    def call(**kw):
        a = dict(good, **kw)
        rc = ctx.L.pnl_bicgstab_block(a['ctx'], p(a['A']), a['ldA'], a['n'], a['nrhs'], 1, p(a['B']), a['ldb'], p(a['X']), a['ldx'], a['tol'],
                                      a['maxiter'], its, res)
        ctx.synchronize()
        return rc
    for kw in (dict(ctx=None), dict(A=None), dict(B=None), dict(X=None), dict(n=0), dict(n=-1), dict(nrhs=0), dict(nrhs=-2), dict(ldA=n-1),
               dict(ldb=n-1), dict(ldx=n-1), dict(maxiter=-1), dict(B=X.data_ptr()), dict(A=X.data_ptr())):
        assert call(**kw) == _lib.PNL_ERR_INVALID, kw
        assert bool((X == 77.).all()), kw
    X.zero_()
    assert call() == _lib.PNL_OK and bool((X == 0.5).all()) and list(its) == [0]*k and list(res) == [0.]*k
    # the steps: nvec out of range, n < 1, a leading dimension below n, null blocks, a null state, aliased blocks
    V = [t(17, n, fill=77.) for _ in range(7)]
    state = t(17*ST, fill=77.)
    dv = t(n)
    P_ = [v.data_ptr() for v in V]
    L, h, sp, dp = ctx.L, ctx.h, p(state.data_ptr()), p(dv.data_ptr())
    steps = {
        'init': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n, w=P_[2]: L.pnl_bcgb_init(h, nn, nv, 0, dp, p(a), ld, p(P_[1]), n, p(w), n, p(P_[3]), n, p(P_[4]), n,
                                                                                  p(P_[5]), n, s),
        'start': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n, w=None: L.pnl_bcgb_start(h, nn, nv, p(a), ld, p(P_[1]), n, s),
        'alpha': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n, w=P_[2]: L.pnl_bcgb_alpha(h, nn, nv, 0, dp, p(a), ld, p(P_[1]), n, p(w), n, p(P_[3]), n, s),
        'omega': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n, w=P_[4]: L.pnl_bcgb_omega(h, nn, nv, p(a), ld, p(P_[1]), n, p(P_[2]), n, p(P_[3]), n, p(w), n,
                                                                                    p(P_[5]), n, TOL, s),
        'direction': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n, w=P_[2]: L.pnl_bcgb_direction(h, nn, nv, 0, dp, p(a), ld, p(P_[1]), n, p(w), n, p(P_[3]), n, s),
    }
    for name, f in steps.items():
        cases = [dict(nv=17), dict(nv=0), dict(ld=n-1), dict(a=None), dict(s=None), dict(nn=0)]
        if name != 'start':
            cases.append(dict(w=P_[0]))                               # a written block that is also read
        for kw in cases:
            assert f(**kw) == _lib.PNL_ERR_INVALID, (name, kw)
        ctx.synchronize()
        assert all(bool((v == 77.).all()) for v in V) and bool((state == 77.).all()), name
    assert L.pnl_bcgb_init(None, n, 3, 0, dp, p(P_[0]), n, None, 0, p(P_[2]), n, p(P_[3]), n, p(P_[4]), n, p(P_[5]), n, sp) == _lib.PNL_ERR_INVALID
    # external mode: the blocks of the caller's preconditioner may be null, the others not
    assert L.pnl_bcgb_init(h, n, 3, 1, None, p(P_[0]), n, None, 0, None, n, p(P_[3]), n, None, 0, None, 0, None) == _lib.PNL_ERR_INVALID
    assert L.pnl_bcgb_init(h, n, 3, 1, None, p(P_[0]), n, None, 0, p(P_[2]), n, p(P_[3]), n, None, 0, None, 0, None) == _lib.PNL_OK
    assert steps['init']() == _lib.PNL_OK
    ctx.synchronize()
    ctx.close()


# ---- the Python layers ----------------------------------------------------------------------------------------------------------

def bicgstab_as_before(A, b, tol=1e-8, maxiter=50, dinv=None):
    """the body of solvers.bicgstab for a 1-D b, restated on A.matvec and torch vectors: what bicgstab(A, b) has returned since before
    bicgstab_multi existed"""
    import torch
    bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    x = torch.zeros_like(bd)
    Bp = (lambda r: dinv*r) if dinv is not None else None
    r = bd.clone()
    p = r.clone()
    r0 = Bp(r).clone() if Bp is not None else r.clone()
    kappa = float(torch.dot(r, r0))
    residuals = [float(np.sqrt(abs(kappa)))]
    its = maxiter
    for k in range(maxiter):
        p2 = Bp(p) if Bp is not None else p
        temp = A.matvec(p2.contiguous())
        alpha = kappa/float(torch.dot(temp, r0))
        s_ = r-alpha*temp
        s2 = Bp(s_) if Bp is not None else s_
        temp2 = A.matvec(s2.contiguous())
        omega = float(torch.dot(temp2, s_))/float(torch.dot(temp2, temp2))
        x = x+alpha*p2+omega*s2
        r = s_-omega*temp2
        residuals.append(float(torch.linalg.norm(r)))
        if residuals[-1] < tol:
            its = k
            break
        kappaNew = float(torch.dot(r, r0))
        beta = kappaNew/kappa*alpha/omega
        kappa = kappaNew
        p = r+beta*(p-omega*temp)
    return x.cpu().numpy(), its, residuals


_HIER = {}


def _hierarchy():
    """the smallest real non-symmetric operator of tests/test_solver_side.py: interval, noRef 6, smoothedLeftRight(0.25, 0.75)"""
    if 'H' not in _HIER:
        from pynucleus_amd import getFractionalKernel
        from pynucleus_amd.fractionalOrders import smoothedLeftRightFractionalOrder
        from pynucleus_amd.multigrid import fractionalHierarchy
        _HIER['H'] = fractionalHierarchy('interval', 6, getFractionalKernel(1, smoothedLeftRightFractionalOrder(0.25, 0.75)), {'target_order': 5.})
    return _HIER['H']


def _residual_ok(A, X, B):
    nz = B.any(axis=1)
    return (np.abs(X@A.T-B).max(axis=1)[nz] <= 1e-7*np.abs(B).max(axis=1)[nz]).all() and not X[~nz].any()


@gpu
def test_bicgstab_multi_on_the_nonsymmetric_operator():
    """solvers.bicgstab_multi on the assembled non-symmetric dense operator: the library call and the loop over the steps agree bit
    for bit; every row meets | A x - b |_inf <= 1e-7 | b |_inf and is within one pass of the oracle's count (the criteria of
    tests/test_solver_side.py for bicgstab); with the multigrid cycle as preconditioner every row needs fewer passes than with
    Jacobi; bicgstab with a 2-D b is bicgstab_multi; with a 1-D b it is the code and the bits of before; the cases that are not
    built raise NotImplementedError"""
    import torch
    from pynucleus_amd import solvers
    from pynucleus_amd.multigrid import multigrid
    from pynucleus_amd.linear_operators import DistributedDense_LinearOperator
    H = _hierarchy()
    Aop = H.finest['A']
    A = Aop.toarray().copy()
    n = A.shape[0]
    assert np.abs(A-A.T).max() > 1e-3*np.abs(A).max() and not Aop.symmetric
    b = np.asarray(H.finest['DoFMap'].assembleRHS(1.0))
    B = np.stack([b, 0.5*b[::-1], np.zeros(n), (1.+0.5*np.random.default_rng(1).standard_normal(n))*b, 10.*b])
    tol, mi = 1e-10, 200
    X, its, res = solvers.bicgstab_multi(Aop, B, tol=tol, maxiter=mi, preconditioner='jacobi')
    assert isinstance(X, np.ndarray) and X.shape == B.shape and its.shape == res.shape == (5,)
    _assert_same(solvers._bicgstab_steps(Aop, B, None, tol, mi, 'jacobi'), (X, its, res), 'library call against the step loop')
    _assert_same(Aop.solve_bicgstab_block(B, None, tol, mi, 'jacobi'), (X, its, res), 'operator method')
    _assert_same(solvers.bicgstab(Aop, B, tol=tol, maxiter=mi, preconditioner='jacobi'), (X, its, res), 'bicgstab with a 2-D b')
    Xt, it_t, rt = solvers.bicgstab_multi(Aop, torch.from_numpy(B).cuda(), tol=tol, maxiter=mi, preconditioner='jacobi')
    assert isinstance(Xt, torch.Tensor) and Xt.is_cuda
    _assert_same((Xt.cpu().numpy(), it_t, rt), (X, its, res), 'torch in / out')
    assert (res[[0, 1, 3, 4]] < tol).all() and (its < mi).all() and its[2] == 0 and res[2] == 0. and _residual_ok(A, X, B), (its, res)
    dinv = 1./np.diag(A)
    for v in (0, 1, 3, 4):
        xo, ito, reso = SO.bicgstab(A, B[v], tol=tol, maxiter=mi, B=lambda r: dinv*r)
        assert abs(int(its[v])-ito) <= 1, (v, its[v], ito)
    # no preconditioner through the library, X0 through both paths
    Xn, in_, rn = solvers.bicgstab_multi(Aop, B, tol=tol, maxiter=mi)
    _assert_same(solvers._bicgstab_steps(Aop, B, None, tol, mi, None), (Xn, in_, rn), 'unit diagonal: library call against the step loop')
    assert _residual_ok(A, Xn, B) and (in_ < mi).all()
    X0 = np.random.default_rng(2).standard_normal(B.shape)
    _assert_same(solvers._bicgstab_steps(Aop, B, X0, tol, mi, 'jacobi'), solvers.bicgstab_multi(Aop, B, X0=X0, tol=tol, maxiter=mi, preconditioner='jacobi'),
                 'X0')
    # multigrid between the steps: fewer passes on every row, the same criterion; the object and its asPreconditioner() alike
    mg = multigrid(H)
    Xm, im, rm = solvers.bicgstab_multi(Aop, B, tol=tol, maxiter=mi, preconditioner=mg)
    nz = B.any(axis=1)
    assert (im[nz] < its[nz]).all() and (rm[nz] < tol).all() and im[2] == 0 and _residual_ok(A, Xm, B), (im, its, rm)
    _assert_same(solvers.bicgstab_multi(Aop, B, tol=tol, maxiter=mi, preconditioner=mg.asPreconditioner()), (Xm, im, rm), 'asPreconditioner()')
    _assert_same(solvers.bicgstab_multi(Aop, B[3:4], tol=tol, maxiter=mi, preconditioner=mg), (Xm[3:4], im[3:4], rm[3:4]), 'multigrid, solo')
    # 1-D: the code and the bits of before
    for prec, dv in ((None, None), ('jacobi', 1./torch.from_numpy(np.ascontiguousarray(np.diag(A))).cuda())):
        x1, it1, res1 = solvers.bicgstab(Aop, b, tol=tol, maxiter=mi, preconditioner=prec)
        xw, itw, resw = bicgstab_as_before(Aop, b, tol, mi, dv)
        assert x1.shape == (n,) and isinstance(res1, list) and np.array_equal(x1, xw) and it1 == itw and res1 == resw
    # not built
    with pytest.raises(NotImplementedError):
        solvers.bicgstab_multi(Aop, B, preconditioner=lambda r: r)
    with pytest.raises(NotImplementedError):
        solvers.bicgstab_multi(Aop, B, preconditioner='ilu')
    with pytest.raises(NotImplementedError):
        solvers.bicgstab_multi(DistributedDense_LinearOperator(Aop.A, Aop.ctx), B)
    with pytest.raises(NotImplementedError):
        solvers.bicgstab_multi(object(), B)


@gpu
def test_bicgstab_multi_over_the_steps_on_csr_and_h2():
    """a CSR operator (cd(65), nsdom(300)) and the ordered H2 operator of tests/test_cg_block.py go through the loop over the steps:
    the residual criterion, (3), (4) for the synthetic ones, and (2) -- their products have no float atomics"""
    from pynucleus_amd import solvers
    from test_cg_block import _assembled
    for name, nn in (('cd', 65), ('nsdom', 300)):
        M = matrix(name, nn)
        cctx = _context_with_dofs(nn)
        cop = _csr_operator(cctx, M)
        Bc = rhs_block(nn, 17)
        mi = maxiter_of(name, nn)
        for prec in ('jacobi', None):
            Xc, ic, rc = solvers.bicgstab_multi(cop, Bc, tol=TOL, maxiter=mi, preconditioner=prec)
            done = assert_stopping(ic, rc, np.arange(17) != 8, mi, 'CSR {}({})'.format(name, nn))
            assert ic[8] == 0 and not Xc[8].any()
            assert_true_residual(M, Bc, Xc, ic, rc, TOL, 'CSR {}({})'.format(name, nn), entries_per_row(name, nn), cols=done)
            _assert_same(solvers.bicgstab_multi(cop, Bc, tol=TOL, maxiter=mi, preconditioner=prec), (Xc, ic, rc), 'CSR repeated')
            for v in (0, 2, 16):
                _assert_same(solvers.bicgstab_multi(cop, Bc[v:v+1], tol=TOL, maxiter=mi, preconditioner=prec), (Xc[v:v+1], ic[v:v+1], rc[v:v+1]),
                             'CSR solo {}'.format(v))
            _assert_same(solvers.bicgstab(cop, Bc[:3], tol=TOL, maxiter=mi, preconditioner=prec), (Xc[:3], ic[:3], rc[:3]), 'CSR nrhs = 3')
        cctx.close()
    A = _assembled('h2-ordered')
    Ah = np.array(A.toarray(), dtype=np.float64)
    B = rhs_block(A.num_rows, 5, scales=(1., 1e-2, 10.))                # 1e-7 |b|_inf stays above the absolute tol for every row
    X, its, res = solvers.bicgstab_multi(A, B, tol=1e-10, maxiter=200, preconditioner='jacobi')
    assert (its < 200).all() and its[2] == 0 and _residual_ok(Ah, X, B), (its, res)
    _assert_same(solvers.bicgstab_multi(A, B[3:4], tol=1e-10, maxiter=200, preconditioner='jacobi'), (X[3:4], its[3:4], res[3:4]), 'H2 solo')
