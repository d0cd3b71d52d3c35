"""The Python layer of the direct solver: solvers.chol / solvers.lu / CholeskyFactor, Dense_LinearOperator.solve_direct and the
solver='chol' time stepper, on assembled interval operators.  The kernels themselves are pinned by tests/test_cholesky.py; the bound
used here is its (R) solve bound, evaluated on the host copy of the operator."""
import os
import numpy as np
import pytest

from test_cholesky import solve_violations, seeded_rows

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_exist():
    """the public names and the two ABI entry points"""
    from pynucleus_amd import _lib, solvers, multigrid, linear_operators
    import inspect
    assert callable(solvers.chol) and callable(solvers.lu) and hasattr(solvers, 'CholeskyFactor')
    hdr = open(os.path.join(ROOT, 'include', 'pnl_hip.h')).read()
    for name in ('pnl_potrf', 'pnl_potrs'):
        assert name in _lib.EXPORTS and 'int {}('.format(name) in hdr
    assert hasattr(linear_operators.Dense_LinearOperator, 'solve_direct')
    for f in (multigrid.CrankNicolson.__init__, multigrid.solveFractionalHeat):
        assert inspect.signature(f).parameters['solver'].default == 'cg-mg'


def _operator(s, noRef=5):
    from pynucleus_amd import getFractionalKernel
    from pynucleus_amd.multigrid import fractionalHierarchy
    H = fractionalHierarchy('interval', noRef, getFractionalKernel(1, s), {'target_order': 2.-s})
    return H, H.finest['A']


@gpu
@pytest.mark.parametrize('s', [0.25, 0.75])
def test_chol_solves_an_assembled_operator(s):
    import torch
    from pynucleus_amd import solvers
    H, A = _operator(s)
    assert A.symmetric
    n = A.num_rows
    Ah = A.toarray().copy()
    F = solvers.chol(A)
    assert isinstance(F, solvers.CholeskyFactor) and F.num_rows == n
    assert np.array_equal(A.toarray(), Ah) and np.array_equal(A.refresh(), Ah)         # the operator is untouched
    L = F.L
    assert L.shape == (n, n) and not np.triu(L, 1).any() and (np.diagonal(L) > 0).all()
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x = F.solve(b)
    assert isinstance(x, np.ndarray) and x.shape == (n,)
    bad, worst = solve_violations(Ah, L, b, x, seeded_rows(n))
    assert not bad, (bad, worst)
    # torch in, torch out; the factor is a callable r -> A^-1 r; solve_direct is the same solve
    bt = torch.from_numpy(b).cuda()
    xt = F.solve(bt)
    assert isinstance(xt, torch.Tensor) and xt.is_cuda and np.array_equal(xt.cpu().numpy(), x)
    assert np.array_equal(F(bt).cpu().numpy(), x)
    assert np.array_equal(A.solve_direct(b), x)
    # a 2-D block of right-hand sides, one per row, equals the row-by-row solves bit for bit
    Bm = rng.standard_normal((5, n))
    X = F.solve(Bm)
    assert X.shape == (5, n)
    for r in range(5):
        assert np.array_equal(X[r], F.solve(Bm[r])), r
    # lu is the reference's name for it
    F2 = solvers.lu(A)
    assert np.array_equal(F2.L, L)
    # as a preconditioner the factor makes CG converge in one iteration
    xc, its, res = solvers.cg(A, b, tol=1e-8*np.linalg.norm(b), maxiter=20, preconditioner=F)
    assert its <= 1 and len(res) <= 2+1 and res[-1] <= 1e-8*np.linalg.norm(b), (its, res)
    assert np.abs(xc-x).max() <= 1e-9*np.abs(x).max()


@gpu
def test_chol_refusals_overwrite_and_indefinite():
    import torch
    from pynucleus_amd import solvers
    from pynucleus_amd.linear_operators import Dense_LinearOperator, CSR_LinearOperator
    H, A = _operator(0.75, noRef=4)
    n = A.num_rows
    Ah = A.toarray().copy()
    N = Dense_LinearOperator(A.A.clone(), A.ctx, symmetric=False)
    with pytest.raises(NotImplementedError):
        solvers.chol(N)
    with pytest.raises(NotImplementedError, match='LU with pivoting'):
        solvers.lu(N)
    with pytest.raises(NotImplementedError):
        solvers.chol(object())
    # overwrite: the operator's own storage holds the factor afterwards and its host snapshot is dropped
    B = Dense_LinearOperator(A.A.clone(), A.ctx, symmetric=True)
    assert np.array_equal(B.toarray(), Ah) and B._host is not None
    F = solvers.chol(B, overwrite=True)
    assert B._host is None and F._L.data_ptr() == B.A.data_ptr()
    now = B.toarray()
    assert np.array_equal(np.tril(now), F.L) and np.array_equal(np.triu(now, 1), np.triu(Ah, 1))
    assert np.abs(F.L@F.L.T-Ah).max() <= 1e-13*np.abs(Ah).max()
    # indefinite: the leading minor of order 3 is the first that is not positive definite
    Bad = Ah.copy()
    Bad[2, 2] = -1.
    I = Dense_LinearOperator(torch.from_numpy(Bad).cuda(), A.ctx, symmetric=True)
    with pytest.raises(np.linalg.LinAlgError, match='order 3'):
        solvers.chol(I)
    assert n > 3


@gpu
def test_heat_run_with_the_direct_solver():
    """solveFractionalHeat(solver='chol') on the interval, noRef 6, s = 0.25, problem constant: the reference's stored errors
    0.01455872... / 0.03218338... within the tolerance of test_solver_side.test_gpu_fractional_heat_reproduces_the_stored_errors"""
    from pynucleus_amd.multigrid import solveFractionalHeat
    from test_solver_side import device_hierarchy, heat_setup, HEAT_FIXTURES, SO
    s, problem = 0.25, 'constant'
    H = device_hierarchy('interval', 6, s, {'target_order': 2.-s}, mass=True)
    L = H.finest
    uss, load, z_ss, L2ex2 = heat_setup(H.getLevelList(), s, problem)
    times, us, stepper = solveFractionalHeat(H, uss, load, finalTime=1.0, tol=1e-10, solver='chol')
    M = L['M'].toarray()
    e_final, e_l2, norm = SO.transient_errors(us, times, M, lambda t: np.cos(t)*z_ss, lambda t: np.cos(t)**2*L2ex2)
    ref = HEAT_FIXTURES[(s, problem)]
    print('heat, chol: final error {!r}, L2(0,T;L2) error {!r}, norm {!r}'.format(e_final, e_l2, norm))
    assert abs(e_final-ref[0]) <= ref[3]*ref[0] and abs(e_l2-ref[1]) <= ref[3]*ref[1], (e_final, e_l2, ref)
    assert abs(norm-ref[2]) <= 1e-6*ref[2]
    assert len(us) == 9 and stepper.iterations == [0]*8
    # the operator of the hierarchy was not touched by the factorisation of M/dt + theta S
    times2, us2, stepper2 = solveFractionalHeat(H, uss, load, finalTime=1.0, tol=1e-10)
    assert max(np.abs(a-b).max() for a, b in zip(us, us2)) <= 1e-9*np.abs(us2[0]).max()


@gpu
def test_chol_stepper_needs_a_symmetric_dense_finest_level():
    from pynucleus_amd.multigrid import CrankNicolson, ImplicitEuler
    from pynucleus_amd.linear_operators import Dense_LinearOperator
    from test_solver_side import device_hierarchy
    H = device_hierarchy('interval', 3, 0.25, {'target_order': 1.75}, mass=True)
    levels = [dict(L) for L in H.getLevelList()]

    class NotDense:
        num_rows = levels[-1]['A'].num_rows
    levels[-1]['A'] = NotDense()
    with pytest.raises(NotImplementedError):
        CrankNicolson(levels, 0.125, solver='chol')
    A = H.finest['A']
    levels[-1]['A'] = Dense_LinearOperator(A.A, A.ctx, symmetric=False)
    with pytest.raises(NotImplementedError):
        ImplicitEuler(levels, 0.125, solver='chol')
    with pytest.raises(NotImplementedError):
        CrankNicolson(H, 0.125, solver='gmres')
    assert ImplicitEuler(H, 0.125, solver='chol').theta == 1.
