"""The Python layer of the pivoted direct solver: solvers.plu / LUFactor, Dense_LinearOperator.solve_direct for non-symmetric operators and
the solver='lu' time stepper, on assembled interval operators of a non-symmetric order.  The kernels themselves are pinned by
tests/test_lu.py; the bounds used here are its (R) bounds, evaluated on the host copy of the operator."""
import os
import numpy as np
import pytest

from test_lu import factor_violations, solve_violations, seeded_rows, valid_swaps, perm_of

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_exist():
    """the public names and the two ABI entry points"""
    from pynucleus_amd import _lib, solvers
    assert callable(solvers.plu) and hasattr(solvers, 'LUFactor')
    for name in ('solve', '__call__', 'L', 'U', 'piv', 'perm'):
        assert hasattr(solvers.LUFactor, name), name
    hdr = open(os.path.join(ROOT, 'include', 'pnl_hip.h')).read()
    for name in ('pnl_getrf', 'pnl_getrs'):
        assert name in _lib.EXPORTS and 'int {}('.format(name) in hdr
    assert hasattr(_lib.Context, 'getrf') and hasattr(_lib.Context, 'getrs')
    assert 'plu' in solvers.lu.__doc__


def _nonsym_hierarchy(noRef, mass=False):
    from pynucleus_amd import getFractionalKernel
    from pynucleus_amd.fractionalOrders import smoothedLeftRightFractionalOrder
    from pynucleus_amd.multigrid import fractionalHierarchy
    return fractionalHierarchy('interval', noRef, getFractionalKernel(1, smoothedLeftRightFractionalOrder(0.25, 0.75)), {'target_order': 5.},
                               buildMass=mass)


@gpu
@pytest.mark.parametrize('noRef', [5, 6])
def test_plu_solves_a_non_symmetric_assembled_operator(noRef):
    import torch
    from pynucleus_amd import solvers
    H = _nonsym_hierarchy(noRef)
    A = H.finest['A']
    n = A.num_rows
    Ah = A.toarray().copy()
    assert not A.symmetric and np.abs(Ah-Ah.T).max() > 1e-3*np.abs(Ah).max()
    F = solvers.plu(A)
    assert isinstance(F, solvers.LUFactor) and F.num_rows == n
    assert np.array_equal(A.toarray(), Ah) and np.array_equal(A.refresh(), Ah)         # the operator is untouched
    L, U, piv, perm = F.L, F.U, F.piv, F.perm
    assert valid_swaps(piv, n) and np.array_equal(perm, perm_of(piv))
    assert not np.triu(L, 1).any() and np.array_equal(np.diagonal(L), np.ones(n)) and not np.tril(U, -1).any()
    assert np.abs(np.tril(L, -1)).max() <= 1.
    rows = seeded_rows(n)
    bad, worst = factor_violations(Ah, L, U, perm, rows)
    assert not bad, (bad, worst)
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x = F.solve(b)
    assert isinstance(x, np.ndarray) and x.shape == (n,)
    bad, worst = solve_violations(Ah, L, U, perm, b, x, rows)
    assert not bad, (bad, worst)
    xg, its, res = solvers.gmres(A, b, tol=1e-10, maxiter=2*n, preconditioner='jacobi')
    assert np.abs(xg-x).max() <= 1e-8*np.abs(x).max(), np.abs(xg-x).max()/np.abs(x).max()
    # torch in, torch out; the factors are a callable r -> A^-1 r; solve_direct is the same solve
    bt = torch.from_numpy(b).cuda()
    xt = F.solve(bt)
    assert isinstance(xt, torch.Tensor) and xt.is_cuda and np.array_equal(xt.cpu().numpy(), x)
    assert np.array_equal(F(bt).cpu().numpy(), x)
    assert np.array_equal(A.solve_direct(b), x)
    assert isinstance(A._chol, solvers.LUFactor)
    A.invalidate()
    assert A._chol is None
    # a 2-D block of right-hand sides, one per row, equals the row-by-row solves bit for bit
    Bm = rng.standard_normal((5, n))
    X = F.solve(Bm)
    assert X.shape == (5, n)
    for r in range(5):
        assert np.array_equal(X[r], F.solve(Bm[r])), r
    # as a preconditioner the factors make GMRES converge at once
    xc, its, res = solvers.gmres(A, b, tol=1e-8*np.linalg.norm(b), maxiter=20, preconditioner=F)
    assert its <= 1, (its, res)
    assert np.abs(xc-x).max() <= 1e-9*np.abs(x).max()


@gpu
def test_plu_of_a_symmetric_operator_overwrite_singular_and_refusals():
    import torch
    from pynucleus_amd import solvers, getFractionalKernel
    from pynucleus_amd.multigrid import fractionalHierarchy
    from pynucleus_amd.linear_operators import Dense_LinearOperator
    H = fractionalHierarchy('interval', 5, getFractionalKernel(1, 0.75), {'target_order': 1.25})
    A = H.finest['A']
    n = A.num_rows
    Ah = A.toarray().copy()
    assert A.symmetric
    F = solvers.plu(A)
    b = np.random.default_rng(4).standard_normal(n)
    x = F.solve(b)
    bad, worst = solve_violations(Ah, F.L, F.U, F.perm, b, x, seeded_rows(n))
    assert not bad, (bad, worst)
    xc = solvers.chol(A).solve(b)
    assert np.abs(xc-x).max() <= 1e-10*np.abs(x).max()
    assert isinstance(A.solve_direct(b), np.ndarray) and isinstance(A._chol, solvers.CholeskyFactor)      # symmetric: still Cholesky
    # overwrite: the operator's own storage holds the factors afterwards and its host snapshot is dropped
    B = Dense_LinearOperator(A.A.clone(), A.ctx, symmetric=False)
    assert np.array_equal(B.toarray(), Ah) and B._host is not None
    G = solvers.plu(B, overwrite=True)
    assert B._host is None and G._LU.data_ptr() == B.A.data_ptr()
    assert np.array_equal(np.tril(B.toarray(), -1)+np.eye(n), G.L) and np.array_equal(np.triu(B.toarray()), G.U)
    assert np.array_equal(G.L, F.L) and np.array_equal(G.U, F.U) and np.array_equal(G.piv, F.piv)
    # singular: a zeroed row stays zero through every update and is the last pivot
    Bad = Ah.copy()
    Bad[3, :] = 0.
    S = Dense_LinearOperator(torch.from_numpy(Bad).cuda(), A.ctx, symmetric=False)
    with pytest.raises(np.linalg.LinAlgError, match='column {}'.format(n)):
        solvers.plu(S)
    with pytest.raises(NotImplementedError):
        solvers.plu(object())
    R = Dense_LinearOperator(A.A[:, :n-1].clone(), A.ctx)
    with pytest.raises(NotImplementedError):
        solvers.plu(R)


@gpu
def test_heat_run_with_the_pivoted_direct_solver():
    """solveFractionalHeat(solver='lu') on the interval, noRef 6, s = 0.25, problem constant: the reference's stored errors within the
    tolerance of test_solver_side.test_gpu_fractional_heat_reproduces_the_stored_errors"""
    from pynucleus_amd.multigrid import solveFractionalHeat
    from test_solver_side import device_hierarchy, heat_setup, HEAT_FIXTURES, SO
    s, problem = 0.25, 'constant'
    H = device_hierarchy('interval', 6, s, {'target_order': 2.-s}, mass=True)
    L = H.finest
    Ah = L['A'].toarray().copy()
    uss, load, z_ss, L2ex2 = heat_setup(H.getLevelList(), s, problem)
    times, us, stepper = solveFractionalHeat(H, uss, load, finalTime=1.0, tol=1e-10, solver='lu')
    M = L['M'].toarray()
    e_final, e_l2, norm = SO.transient_errors(us, times, M, lambda t: np.cos(t)*z_ss, lambda t: np.cos(t)**2*L2ex2)
    ref = HEAT_FIXTURES[(s, problem)]
    print('heat, lu: final error {!r}, L2(0,T;L2) error {!r}, norm {!r}'.format(e_final, e_l2, norm))
    assert abs(e_final-ref[0]) <= ref[3]*ref[0] and abs(e_l2-ref[1]) <= ref[3]*ref[1], (e_final, e_l2, ref)
    assert abs(norm-ref[2]) <= 1e-6*ref[2]
    assert len(us) == 9 and stepper.iterations == [0]*8
    assert np.array_equal(L['A'].refresh(), Ah)               # the operator of the hierarchy was not touched


@gpu
def test_implicit_euler_lu_on_a_non_symmetric_operator():
    """each step's result satisfies the step's linear system (M/dt + S) u_new = (M/dt) u_old + f, rebuilt on the host, within the (R)
    solve bound of the stepper's own factors"""
    import torch
    from pynucleus_amd import solvers
    from pynucleus_amd.multigrid import ImplicitEuler, CrankNicolson
    H = _nonsym_hierarchy(4, mass=True)
    Lv = H.finest
    S, M = Lv['A'].toarray().copy(), Lv['M'].toarray()
    n = S.shape[0]
    assert not Lv['A'].symmetric and np.abs(S-S.T).max() > 1e-3*np.abs(S).max()
    with pytest.raises(NotImplementedError):
        CrankNicolson(H, 0.125, solver='chol')               # Cholesky keeps refusing the non-symmetric operator
    dt = 0.125
    stepper = ImplicitEuler(H, dt, solver='lu')
    assert stepper.theta == 1. and isinstance(stepper.factor, solvers.LUFactor)
    T = S+M*(1./dt)
    F = stepper.factor
    Lf, Uf, perm = F.L, F.U, F.perm
    bad, worst = factor_violations(T, Lf, Uf, perm, seeded_rows(n))
    assert not bad, (bad, worst)
    rng = np.random.default_rng(5)
    u = torch.from_numpy(rng.standard_normal(n)).cuda()
    t = 0.
    for k in range(3):
        f = rng.standard_normal(n)
        old = u.cpu().numpy().copy()
        t = stepper.step(t, u, f)
        new = u.cpu().numpy()
        rhs = np.asarray((M.astype(np.longdouble)@old.astype(np.longdouble))/np.longdouble(dt)+f.astype(np.longdouble), dtype=np.float64)
        bad, worst = solve_violations(T, Lf, Uf, perm, rhs, new, seeded_rows(n))
        assert not bad, (k, bad, worst)
    assert abs(t-3*dt) < 1e-14 and stepper.iterations == [0]*3
    assert np.array_equal(Lv['A'].refresh(), S)
