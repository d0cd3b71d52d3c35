"""Krylov solvers for the operators of this package (dense, CSR / SSS, H2, distributed): vectors stay in HBM, the operator
is whatever ``A.matvec`` does (GEMV, SpMV, H2 passes, all-reduce).

``cg`` follows the reference's cg_solver.solve (base/PyNucleus_base/solvers.pyx:363-444) step by step: preconditioned
residual norm sqrt(r.Br) as convergence criterion, the residual recomputed from scratch every 50 iterations, update order
x, r, (refresh), Br, beta, p.  ``jacobi`` = the reference's jacobi_solver as a preconditioner (solvers.pyx:229-245).
The dense operator additionally has this loop as one library call (pnl_cg_jacobi, Dense_LinearOperator.solve_cg_jacobi).
``cg_multi`` is that loop for a 2-D block of right-hand sides: every row its own recurrence, the operator product shared
(matvec_multi); the dense operator has it as one library call (pnl_cg_jacobi_block), the others run it over the library's steps.
``gmres`` follows gmres_solver.solve (solvers.pyx:504-659; the drivers' gmres-jacobi / gmres-mg for non-symmetric orders):
left (default) or right preconditioner, modified Gram-Schmidt, Givens rotations, the rotated right-hand side as residual
estimate, restarts; the Krylov basis stays in HBM, the small Hessenberg problem lives on the host.
``bicgstab`` follows bicgstab_solver.solve (solvers.pyx:716-787); ``bicgstab_multi`` is that recurrence for a 2-D block of right-hand
sides of a general operator: every row its own recurrence, the two operator products of a pass shared (matvec_multi); the dense
operator has it as one library call (pnl_bicgstab_block), the others run it over the library's steps (pnl_bcgb_*).
``chol`` / ``lu`` are the direct solver of the symmetric dense operators (lu_solver, solvers.pyx:80-186): the Cholesky factor is
computed once in HBM (pnl_potrf), every solve is two triangular sweeps (pnl_potrs).  ``plu`` is the same solver for any square dense
operator, symmetric or not: P A = L U with partial pivoting (pnl_getrf), every solve the swaps and two sweeps (pnl_getrs)."""
import numpy as np


def _dev_vector(v, device):
    import torch
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).to(device)


def cg(A, b, x0=None, tol=1e-8, maxiter=1000, preconditioner='jacobi'):
    """Solve A x = b for a symmetric positive definite operator.  Returns (x, iterations, residuals); x is a torch tensor
    on the operator's device if b is one, else a numpy array.  A 2-D b [nrhs, n] is a block of right-hand sides: ``cg_multi``."""
    if getattr(b, 'ndim', None) == 2 or (not hasattr(b, 'ndim') and np.ndim(b) == 2):
        return cg_multi(A, b, x0, tol, maxiter, preconditioner)
    import torch
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else torch.device('cuda', torch.cuda.current_device())
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    dinv = None
    B = None
    if preconditioner == 'jacobi':
        d = A.diagonal
        d = d() if callable(d) else d
        dinv = 1./_dev_vector(d, device)
    elif callable(preconditioner):
        # r -> B r on device vectors, e.g. multigrid.asPreconditioner() (multigridPreconditioner, multigrid_{SCALAR}.pxi:470-497)
        B = preconditioner
    elif preconditioner is not None:
        raise NotImplementedError(preconditioner)
    r = bd-A.matvec(x) if x0 is not None else bd.clone()
    residuals = []
    if B is not None:
        p = B(r).clone()
        betaOld = float(torch.dot(r, p))
    elif dinv is None:
        p = r.clone()
        betaOld = float(torch.dot(r, p))
    else:
        p = dinv*r
        betaOld = float(torch.dot(r, p))
    conv = float(np.sqrt(abs(betaOld)))
    residuals.append(conv)
    its = 0
    if conv > tol:
        k = 0
        for i in range(maxiter):
            Ap = A.matvec(p)
            alpha = betaOld/float(torch.dot(p, Ap))
            x.add_(p, alpha=alpha)
            r.add_(Ap, alpha=-alpha)
            if k == 50:
                r = bd-A.matvec(x)                      # recalculate the residual to avoid rounding errors
                k = 0
            Br = B(r) if B is not None else (r if dinv is None else dinv*r)
            beta = float(torch.dot(r, Br))
            conv = float(np.sqrt(abs(beta)))
            residuals.append(conv)
            its = i
            if conv <= tol:
                break
            p = Br+(beta/betaOld)*p
            betaOld = beta
            k += 1
        else:
            its = maxiter
    import torch as _t
    if isinstance(b, _t.Tensor):
        return x, its, residuals
    return x.cpu().numpy(), its, residuals


def _cg_group(A, ctx, dinv, B, X, have_x0, tol, maxiter, its, res):
    """the loop of pnl_cg_jacobi_block (csrc/pnl_cg_block.hip) for at most 16 rows of B, with ``A.matvec_multi`` as the product and the
    library's step calls on device blocks; X [nv, n] contiguous holds the guesses and the results, its / res are filled"""
    import torch
    from ._lib import PNL_CGB_STATE
    nv, n = B.shape
    dev = B.device
    R, P, Z = (torch.empty((nv, n), dtype=torch.float64, device=dev) for _ in range(3))
    state = torch.zeros(nv*PNL_CGB_STATE, dtype=torch.float64, device=dev)
    dp = dinv.data_ptr() if dinv is not None else 0
    ldb = max(int(B.stride(0)), n)

    def product(V):
        ctx.synchronize()
        W = A.matvec_multi(V)
        torch.cuda.current_stream(dev).synchronize()
        return W

    def read_state():
        ctx.synchronize()
        return state.cpu().numpy().reshape(nv, PNL_CGB_STATE)

    AX = product(X) if have_x0 else None
    torch.cuda.current_stream(dev).synchronize()
    ctx.cgb_init(n, nv, dp, B.data_ptr(), ldb, AX.data_ptr() if AX is not None else 0, n, R.data_ptr(), n, P.data_ptr(), n, tol, state.data_ptr())
    st = read_state()
    res[:] = st[:, 3]
    its[:] = 0
    active = st[:, 4] != 0.
    k = 0
    for it in range(maxiter):
        if not active.any():
            break
        AP = product(P)
        ctx.cgb_update(n, nv, dp, P.data_ptr(), n, AP.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, Z.data_ptr(), n, state.data_ptr())
        if k == 50:
            AX = product(X)                             # recalculate the residual to avoid rounding errors
            ctx.cgb_refresh(n, nv, dp, B.data_ptr(), ldb, AX.data_ptr(), n, R.data_ptr(), n, Z.data_ptr(), n, state.data_ptr())
            k = 0
        ctx.cgb_direction(n, nv, Z.data_ptr(), n, P.data_ptr(), n, tol, state.data_ptr())
        st = read_state()
        res[active] = st[active, 3]
        done = active & (st[:, 4] == 0.)
        its[done] = it
        active &= ~done
        k += 1
    its[active] = maxiter


def _cg_group_mg(A, ctx, cycle, B, X, have_x0, tol, maxiter, its, res):
    """the loop of pnl_mg_cg_block (csrc/pnl_mg_block.hip) for at most 16 rows of B, with ``A.matvec_multi`` as the product, ``cycle``
    (R [nv, n] -> Z, one V cycle from a zero guess for every row: multigrid.cycle on a block) as the preconditioner and the library's
    external-preconditioner steps on device blocks; X [nv, n] contiguous holds the guesses and the results, its / res are filled"""
    import torch
    from ._lib import PNL_CGB_STATE
    nv, n = B.shape
    dev = B.device
    R, P = (torch.empty((nv, n), dtype=torch.float64, device=dev) for _ in range(2))
    state = torch.zeros(nv*PNL_CGB_STATE, dtype=torch.float64, device=dev)
    ldb = max(int(B.stride(0)), n)

    def product(V):
        ctx.synchronize()
        W = A.matvec_multi(V)
        torch.cuda.current_stream(dev).synchronize()
        return W

    def precondition():
        ctx.synchronize()
        Z = cycle(R).contiguous()
        torch.cuda.current_stream(dev).synchronize()
        return Z

    def read_state():
        ctx.synchronize()
        return state.cpu().numpy().reshape(nv, PNL_CGB_STATE)

    AX = product(X) if have_x0 else None
    torch.cuda.current_stream(dev).synchronize()
    ctx.cgb_residual(n, nv, B.data_ptr(), ldb, AX.data_ptr() if AX is not None else 0, n, R.data_ptr(), n, 0)
    Z = precondition()
    ctx.cgb_start(n, nv, R.data_ptr(), n, Z.data_ptr(), n, P.data_ptr(), n, tol, state.data_ptr())
    st = read_state()
    res[:] = st[:, 3]
    its[:] = 0
    active = st[:, 4] != 0.
    k = 0
    for it in range(maxiter):
        if not active.any():
            break
        AP = product(P)
        ctx.cgb_step(n, nv, P.data_ptr(), n, AP.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, state.data_ptr())
        if k == 50:
            AX = product(X)                             # recalculate the residual to avoid rounding errors
            ctx.cgb_residual(n, nv, B.data_ptr(), ldb, AX.data_ptr(), n, R.data_ptr(), n, state.data_ptr())
            k = 0
        Z = precondition()
        ctx.cgb_beta(n, nv, R.data_ptr(), n, Z.data_ptr(), n, state.data_ptr())
        ctx.cgb_direction(n, nv, Z.data_ptr(), n, P.data_ptr(), n, tol, state.data_ptr())
        st = read_state()
        res[active] = st[active, 3]
        done = active & (st[:, 4] == 0.)
        its[done] = it
        active &= ~done
        k += 1
    its[active] = maxiter


def cg_multi(A, B, X0=None, tol=1e-8, maxiter=1000, preconditioner='jacobi'):
    """Solve A X[v] = B[v] for the rows of a 2-D B [nrhs, n], A symmetric positive definite.  Every row runs the recurrence of ``cg``
    on its own (own step lengths, own convergence test sqrt(r.Br) <= tol, frozen once it has converged) and the rows share the
    operator product: one ``matvec_multi`` per iteration and 16 rows.  A symmetric Dense_LinearOperator on one GPU with the Jacobi
    preconditioner is one library call (pnl_cg_jacobi_block); any other operator with ``matvec_multi`` and ``diagonal`` (CSR, SSS, H2,
    interpolated) runs the same loop here over the library's step calls.  ``preconditioner``: 'jacobi', None (the unit diagonal), or a
    ``multigrid`` object / its ``asPreconditioner()`` (dense levels, Jacobi smoother): one V cycle from a zero guess per iteration for the
    whole block.  A dense A of the hierarchy's size is then one library call (pnl_mg_cg_block); any other operator with ``matvec_multi``
    runs the loop here over the external-preconditioner steps (pnl_cgb_residual / _start / _step / _beta / _direction) and
    ``multigrid.cycle`` on the block.
    Returns (X, iterations[nrhs], residuals[nrhs]): the final sqrt(r.Br) of every row; X is a torch tensor on the operator's device if
    B is one, else a numpy array."""
    import torch
    from ._lib import PNL_CGB_MAXVEC
    from .linear_operators import Dense_LinearOperator, _as_block
    from .multigrid import multigrid as _multigrid
    # a multigrid object, or the callable of its asPreconditioner(): the block cycle of that hierarchy
    mg = preconditioner if isinstance(preconditioner, _multigrid) else getattr(preconditioner, 'multigrid', None)
    if mg is None and callable(preconditioner):
        raise NotImplementedError('cg_multi: a plain callable as preconditioner for a block of right-hand sides is not built '
                                  '(pass a multigrid object or its asPreconditioner())')
    if mg is None and preconditioner not in ('jacobi', None):
        raise NotImplementedError(preconditioner)
    from .linear_operators import DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator
    from .distributed_h2 import DistributedH2Matrix_localData
    if isinstance(A, (DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator,
                      DistributedH2Matrix_localData)):
        raise NotImplementedError('cg_multi: the block products of the distributed operators loop their matvec; solve row by row with cg')
    if not hasattr(A, 'matvec_multi'):
        raise NotImplementedError('cg_multi needs an operator with matvec_multi; got {!r}'.format(A))
    if mg is not None:
        mg._require_block()                                 # NotImplementedError for a Chebyshev smoother, H2 / sparse levels
        cycles = getattr(preconditioner, 'maxIter', 1)
        if isinstance(A, Dense_LinearOperator) and A.num_rows == A.num_columns == mg.num_rows and cycles == 1:
            return mg._cg_block(B, X0, tol, maxiter, None if A is mg.A else A)          # one library call (pnl_mg_cg_block)
    elif isinstance(A, Dense_LinearOperator) and A.symmetric and preconditioner == 'jacobi':
        return A.solve_cg_jacobi_block(B, X0, tol, maxiter)
    if hasattr(A, 'assure_constructed'):
        A.assure_constructed()
    ctx = A.ctx if hasattr(A, 'ctx') else A.ops[0].ctx
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else A._device()
    Bd = _as_block(B, device)
    nrhs, n = Bd.shape
    assert nrhs >= 1 and n == A.num_rows == A.num_columns, (tuple(Bd.shape), A.shape)
    X = torch.zeros((nrhs, n), dtype=torch.float64, device=device) if X0 is None else _as_block(X0, device).clone(
        memory_format=torch.contiguous_format)
    assert X.shape == Bd.shape, (tuple(X.shape), tuple(Bd.shape))
    dinv = None
    if preconditioner == 'jacobi':
        d = A.diagonal
        d = d() if callable(d) else d
        dinv = 1./_dev_vector(d, device)
    its, res = np.zeros(nrhs, dtype=np.int32), np.zeros(nrhs)
    for v0 in range(0, nrhs, PNL_CGB_MAXVEC):
        v1 = min(nrhs, v0+PNL_CGB_MAXVEC)
        if mg is not None:
            _cg_group_mg(A, ctx, preconditioner if callable(preconditioner) else mg.cycle, Bd[v0:v1], X[v0:v1], X0 is not None, tol, maxiter,
                         its[v0:v1], res[v0:v1])
        else:
            _cg_group(A, ctx, dinv, Bd[v0:v1], X[v0:v1], X0 is not None, tol, maxiter, its[v0:v1], res[v0:v1])
    if isinstance(B, torch.Tensor):
        return X, its, res
    return X.cpu().numpy(), its, res


def gmres(A, b, x0=None, tol=1e-8, maxiter=50, restarts=1, preconditioner=None, left=True):
    """Solve A x = b for a general operator.  ``preconditioner``: 'jacobi', None or a callable r -> B r on device vectors
    (multigrid.asPreconditioner()).  Returns (x, iterations, residuals): the residuals are the norms of the (left-
    preconditioned) residual, the first one computed, the others from the rotated right-hand side like the reference."""
    import torch
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else torch.device('cuda', torch.cuda.current_device())
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    B = None
    if preconditioner == 'jacobi':
        d = A.diagonal
        d = d() if callable(d) else d
        dinv = 1./_dev_vector(d, device)
        B = lambda r: dinv*r                                   # noqa: E731
    elif callable(preconditioner):
        B = preconditioner
    elif preconditioner is not None:
        raise NotImplementedError(preconditioner)
    L = B if left else None
    R = B if not left else None
    n = bd.shape[0]
    Q = torch.empty((maxiter+1, n), dtype=torch.float64, device=device)
    H = np.zeros((maxiter+1, maxiter))
    c, sn, gamma, y = np.zeros(maxiter), np.zeros(maxiter), np.zeros(maxiter+1), np.zeros(maxiter+1)
    residuals, allIter, breakout, eps = [], 0, False, 1e-15
    for _ in range(restarts):
        if breakout:
            break
        r = bd-A.matvec(x)
        if L is not None:
            r = L(r)
        gamma[0] = float(torch.linalg.norm(r))
        if not residuals:
            residuals.append(abs(gamma[0]))
        if abs(gamma[0]) < tol:
            break
        Q[0] = r/gamma[0]
        i = -1
        for i in range(maxiter):
            # Arnoldi step
            if L is not None:
                w = L(A.matvec(Q[i].contiguous()))
            elif R is not None:
                w = A.matvec(R(Q[i].contiguous()))
            else:
                w = A.matvec(Q[i].contiguous())
            w = w.clone()
            for j in range(i+1):
                H[j, i] = float(torch.dot(Q[j], w))
                w.add_(Q[j], alpha=-H[j, i])
            H[i+1, i] = float(torch.linalg.norm(w))
            if not abs(H[i+1, i]) > eps:
                breakout = True
                break
            Q[i+1] = w/H[i+1, i]
            # previous Givens rotations on the new column, then the new rotation
            for j in range(i):
                rho, sigma = H[j, i], H[j+1, i]
                H[j, i] = c[j]*rho+sn[j]*sigma
                H[j+1, i] = -sn[j]*rho+c[j]*sigma
            beta = np.sqrt(H[i, i]**2+H[i+1, i]**2)
            c[i], sn[i] = H[i, i]/beta, H[i+1, i]/beta
            H[i, i] = beta
            gamma[i+1] = -sn[i]*gamma[i]
            gamma[i] = c[i]*gamma[i]
            residuals.append(abs(gamma[i+1]))
            if abs(gamma[i+1]) < tol:
                breakout = True
                break
        allIter += i
        # back substitution and update
        for j in range(i, -1, -1):
            t = gamma[j]
            for l in range(j+1, i+1):
                t -= H[j, l]*y[l]
            y[j] = t/H[j, j]
        upd = torch.from_numpy(y[:i+1].copy()).to(device)@Q[:i+1]
        x.add_(R(upd) if R is not None else upd)
    if isinstance(b, torch.Tensor):
        return x, allIter, residuals
    return x.cpu().numpy(), allIter, residuals


def _bicgstab_group(A, ctx, dinv, cycle, B, X, have_x0, tol, maxiter, its, res):
    """the loop of pnl_bicgstab_block (csrc/pnl_bicgstab_block.hip) for at most 16 rows of B, with ``A.matvec_multi`` as the product and
    the library's step calls on device blocks.  ``cycle`` None: the preconditioner is ``dinv`` (None: the unit diagonal), applied by the
    steps; else the external mode, ``cycle`` (a block [nv, n] -> M^-1 of every row: multigrid.cycle) applied here between the steps.
    X [nv, n] contiguous holds the guesses and the results, its / res are filled"""
    import torch
    from ._lib import PNL_BCGB_STATE
    nv, n = B.shape
    dev = B.device
    ext = cycle is not None
    R, P, R0, P2, S2 = (torch.empty((nv, n), dtype=torch.float64, device=dev) for _ in range(5))
    state = torch.zeros(nv*PNL_BCGB_STATE, dtype=torch.float64, device=dev)
    dp = dinv.data_ptr() if dinv is not None else 0
    ldb = max(int(B.stride(0)), n)

    def product(V):
        ctx.synchronize()
        W = A.matvec_multi(V)
        torch.cuda.current_stream(dev).synchronize()
        return W

    def precondition(V, out):
        ctx.synchronize()
        out.copy_(cycle(V))
        torch.cuda.current_stream(dev).synchronize()

    def read_state():
        ctx.synchronize()
        return state.cpu().numpy().reshape(nv, PNL_BCGB_STATE)

    AX = product(X) if have_x0 else None
    torch.cuda.current_stream(dev).synchronize()
    ctx.bcgb_init(n, nv, ext, dp, B.data_ptr(), ldb, AX.data_ptr() if AX is not None else 0, n, R.data_ptr(), n, P.data_ptr(), n, R0.data_ptr(), n,
                  P2.data_ptr(), n, state.data_ptr())
    if ext:
        precondition(R, R0)
        P2.copy_(R0)                                    # P = R at the start
        torch.cuda.current_stream(dev).synchronize()
        ctx.bcgb_start(n, nv, R.data_ptr(), n, R0.data_ptr(), n, state.data_ptr())
    st = read_state()
    res[:] = st[:, 3]
    its[:] = 0
    active = st[:, 4] != 0.
    for it in range(maxiter):
        if not active.any():
            break
        T = product(P2)
        ctx.bcgb_alpha(n, nv, ext, dp, T.data_ptr(), n, R0.data_ptr(), n, R.data_ptr(), n, S2.data_ptr(), n, state.data_ptr())
        if ext:
            precondition(R, S2)                         # S lives in R between the two steps
        T2 = product(S2)
        ctx.bcgb_omega(n, nv, P2.data_ptr(), n, S2.data_ptr(), n, T2.data_ptr(), n, R0.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, tol,
                       state.data_ptr())
        ctx.bcgb_direction(n, nv, ext, dp, R.data_ptr(), n, T.data_ptr(), n, P.data_ptr(), n, P2.data_ptr(), n, state.data_ptr())
        if ext:
            precondition(P, P2)
        st = read_state()
        res[active] = st[active, 3]
        done = active & (st[:, 4] == 0.)
        its[done] = it
        active &= ~done
    its[active] = maxiter


def bicgstab_multi(A, B, X0=None, tol=1e-8, maxiter=50, preconditioner=None):
    """Solve A X[v] = B[v] for the rows of a 2-D B [nrhs, n], A a general (non-symmetric) operator.  Every row runs the recurrence of
    ``bicgstab`` on its own (own alpha, omega, beta, own convergence test ||r||_2 < tol, frozen once it has converged) and the rows
    share the two operator products of a pass: two ``matvec_multi`` per pass and 16 rows.  A square Dense_LinearOperator on one GPU with
    ``preconditioner`` None or 'jacobi' is one library call (pnl_bicgstab_block); any other operator with ``matvec_multi`` (CSR, SSS, H2
    in either far-field mode, interpolated, non-symmetric H2) runs the same loop here over the library's step calls.  A ``multigrid``
    object or its ``asPreconditioner()`` (dense levels, Jacobi smoother) is applied between the steps: one V cycle from a zero guess
    for the whole block, twice per pass and once at the start.
    Unlike the reference, which divides and returns NaN, a row whose recurrence breaks down (T.R0, omega or kappa 0, a sum that is not
    finite) is frozen before anything that is not finite is written: it reports the pass of the breakdown and its last residual, so
    iterations < maxiter with residual >= tol identifies it.  A zero right-hand side with a zero guess reports 0 iterations and
    residual 0.
    Returns (X, iterations[nrhs], residuals[nrhs]): the final ||r||_2 of every row (for maxiter = 0 the start value sqrt(|r.M^-1 r|)); X
    is a torch tensor on the operator's device if B is one, else a numpy array."""
    from .linear_operators import Dense_LinearOperator
    from .multigrid import multigrid as _multigrid
    mg = preconditioner if isinstance(preconditioner, _multigrid) else getattr(preconditioner, 'multigrid', None)
    if mg is None and callable(preconditioner):
        raise NotImplementedError('bicgstab_multi: a plain callable as preconditioner for a block of right-hand sides is not built '
                                  '(pass a multigrid object or its asPreconditioner())')
    if mg is None and preconditioner not in ('jacobi', None):
        raise NotImplementedError(preconditioner)
    from .linear_operators import DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator
    from .distributed_h2 import DistributedH2Matrix_localData
    if isinstance(A, (DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator,
                      DistributedH2Matrix_localData)):
        raise NotImplementedError('bicgstab_multi: the block products of the distributed operators loop their matvec; solve row by row '
                                  'with bicgstab')
    if not hasattr(A, 'matvec_multi'):
        raise NotImplementedError('bicgstab_multi needs an operator with matvec_multi; got {!r}'.format(A))
    if mg is not None:
        mg._require_block()                                 # NotImplementedError for a Chebyshev smoother, H2 / sparse levels
    elif isinstance(A, Dense_LinearOperator) and A.num_rows == A.num_columns:
        return A.solve_bicgstab_block(B, X0, tol, maxiter, preconditioner)          # one library call (pnl_bicgstab_block)
    return _bicgstab_steps(A, B, X0, tol, maxiter, preconditioner)


def _bicgstab_steps(A, B, X0, tol, maxiter, preconditioner):
    """bicgstab_multi over the library's step calls, groups of 16 rows; the arguments have been checked"""
    import torch
    from ._lib import PNL_CGB_MAXVEC
    from .linear_operators import _as_block
    from .multigrid import multigrid as _multigrid
    mg = preconditioner if isinstance(preconditioner, _multigrid) else getattr(preconditioner, 'multigrid', None)
    if hasattr(A, 'assure_constructed'):
        A.assure_constructed()
    ctx = A.ctx if hasattr(A, 'ctx') else A.ops[0].ctx
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else A._device()
    Bd = _as_block(B, device)
    nrhs, n = Bd.shape
    assert nrhs >= 1 and n == A.num_rows == A.num_columns, (tuple(Bd.shape), A.shape)
    X = torch.zeros((nrhs, n), dtype=torch.float64, device=device) if X0 is None else _as_block(X0, device).clone(
        memory_format=torch.contiguous_format)
    assert X.shape == Bd.shape, (tuple(X.shape), tuple(Bd.shape))
    dinv = None
    if preconditioner == 'jacobi':
        d = A.diagonal
        d = d() if callable(d) else d
        dinv = 1./_dev_vector(d, device)
    cycle = None
    if mg is not None:
        cycle = preconditioner if callable(preconditioner) else mg.cycle
    its, res = np.zeros(nrhs, dtype=np.int32), np.zeros(nrhs)
    for v0 in range(0, nrhs, PNL_CGB_MAXVEC):
        v1 = min(nrhs, v0+PNL_CGB_MAXVEC)
        _bicgstab_group(A, ctx, dinv, cycle, Bd[v0:v1], X[v0:v1], X0 is not None, tol, maxiter, its[v0:v1], res[v0:v1])
    if isinstance(B, torch.Tensor):
        return X, its, res
    return X.cpu().numpy(), its, res


def bicgstab(A, b, x0=None, tol=1e-8, maxiter=50, preconditioner=None):
    """bicgstab_solver.solve (solvers.pyx:716-787): right-preconditioned stabilised BiCG, r0 = B r, stopping on the 2-norm of
    the residual.  Returns (x, iterations, residuals).  A 2-D b [nrhs, n] is a block of right-hand sides: ``bicgstab_multi``."""
    if getattr(b, 'ndim', None) == 2 or (not hasattr(b, 'ndim') and np.ndim(b) == 2):
        return bicgstab_multi(A, b, x0, tol, maxiter, preconditioner)
    import torch
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else torch.device('cuda', torch.cuda.current_device())
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    B = None
    if preconditioner == 'jacobi':
        d = A.diagonal
        d = d() if callable(d) else d
        dinv = 1./_dev_vector(d, device)
        B = lambda r: dinv*r                                   # noqa: E731
    elif callable(preconditioner):
        B = preconditioner
    elif preconditioner is not None:
        raise NotImplementedError(preconditioner)
    r = bd.clone() if x0 is None else bd-A.matvec(x)
    p = r.clone()
    r0 = B(r).clone() if B is not None else r.clone()
    kappa = float(torch.dot(r, r0))
    residuals = [float(np.sqrt(abs(kappa)))]
    its = maxiter
    for k in range(maxiter):
        p2 = B(p) if B is not None else p
        temp = A.matvec(p2.contiguous())
        alpha = kappa/float(torch.dot(temp, r0))
        s_ = r-alpha*temp
        s2 = B(s_) if B is not None else s_
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
    if isinstance(b, torch.Tensor):
        return x, its, residuals
    return x.cpu().numpy(), its, residuals


class _DenseFactor:
    """What the factors of a square dense operator share: the shape, the device and ``solve``.  A subclass keeps the device block
    [n, ld] under its own name and supplies ``_trs(B_ptr, ldb, nrhs)``, the library's triangular solves in place on a device block
    of right-hand sides."""

    def __init__(self, F_dev, ctx):
        self.ctx = ctx
        self.device = F_dev.device
        self.num_rows = self.num_columns = int(F_dev.shape[0])
        self.shape = (self.num_rows, self.num_columns)

    def _solve_dev(self, X):
        """in place on the rows of the contiguous device block X [nrhs, n]"""
        import torch
        torch.cuda.current_stream(self.device).synchronize()
        self._trs(X.data_ptr(), X.stride(0) if X.shape[0] > 1 else max(X.shape[1], 1), X.shape[0])
        self.ctx.synchronize()
        return X

    def solve(self, b):
        """x with A x = b for a vector, or row by row for a 2-D array of right-hand sides; torch in, torch out, else numpy"""
        import torch
        X = _dev_vector(b, self.device)
        if X.ndim not in (1, 2) or X.shape[-1] != self.num_rows:
            raise AssertionError('right-hand side of shape {} for an operator with {} rows'.format(tuple(X.shape), self.num_rows))
        shape = tuple(X.shape)
        X = X.reshape(-1, self.num_rows).contiguous().clone()
        self._solve_dev(X)
        X = X.reshape(shape)
        return X if isinstance(b, torch.Tensor) else X.cpu().numpy()

    def __call__(self, r):
        return self.solve(r)


def _ld(F):
    """row stride of the square device block F as the library wants it"""
    return F.stride(0) if F.shape[0] > 1 else F.shape[1]


def _factor_block(A, overwrite, name, accepts, needs):
    """The device block that ``chol`` / ``plu`` (``name``) factor in place: the operator's own storage with ``overwrite``, else a
    contiguous copy; both quiescent.  ``accepts(A)`` says whether A is a dense operator this factorisation takes, ``needs`` is the
    text of the error if not."""
    import torch
    from .linear_operators import Dense_LinearOperator
    if not isinstance(A, Dense_LinearOperator) or not accepts(A):
        raise NotImplementedError('{}: {}; got {!r}'.format(name, needs, A))
    A.ctx.synchronize()
    torch.cuda.current_stream(A.A.device).synchronize()
    if overwrite:
        return A.A
    try:
        F = A.A.clone(memory_format=torch.contiguous_format)
    except torch.cuda.OutOfMemoryError as e:
        raise MemoryError('{0}: no room in HBM for a copy of the {1} x {2} operator ({3:.1f} GB); '
                          '{0}(A, overwrite=True) factors it in place'.format(name, A.num_rows, A.num_columns,
                                                                              8e-9*A.num_rows*A.A.stride(0))) from e
    torch.cuda.current_stream(A.A.device).synchronize()
    return F


class CholeskyFactor(_DenseFactor):
    """A = L L^T of a symmetric positive definite dense operator, L in the lower triangle of a device block (the strict upper
    triangle holds whatever the operator had there and is never read).  ``solve(b)`` = lu_solver.solve (solvers.pyx:80-186);
    calling the object applies A^-1 to a device vector, so it can be the ``preconditioner=`` of cg / gmres / bicgstab."""

    def __init__(self, L_dev, ctx):
        super().__init__(L_dev, ctx)
        self._L = L_dev

    @property
    def L(self):
        """the factor as a lower-triangular numpy array (a copy; tests)"""
        self.ctx.synchronize()
        return np.tril(self._L.cpu().numpy())

    def _trs(self, B, ldb, nrhs):
        self.ctx.potrs(self._L.data_ptr(), _ld(self._L), self.num_rows, B, ldb, nrhs)

    def __repr__(self):
        return '<Cholesky factor of a {}x{} dense operator on {}>'.format(self.num_rows, self.num_columns, self.device)


def chol(A, overwrite=False):
    """Cholesky factorisation of a symmetric dense operator on its device (pnl_potrf).  Without ``overwrite`` a device copy of the
    block is factored; with it the operator's own storage becomes the factor (its lower triangle; the operator is invalidated and
    must not be applied any more).  Raises numpy.linalg.LinAlgError if a leading minor is not positive definite."""
    Ld = _factor_block(A, overwrite, 'chol', lambda A: A.symmetric,
                       'a symmetric Dense_LinearOperator is needed (direct solves of H2, sparse, distributed or '
                       'non-symmetric operators are not built)')
    info = A.ctx.potrf(Ld.data_ptr(), _ld(Ld), A.num_rows)
    if overwrite:
        A.invalidate()
    if info > 0:
        raise np.linalg.LinAlgError('chol: the leading minor of order {} is not positive definite'.format(info))
    return CholeskyFactor(Ld, A.ctx)


class LUFactor(_DenseFactor):
    """P A = L U of a square dense operator: L (unit diagonal, not stored) below the diagonal of a device block, U on and above it,
    and the swap sequence (int32, LAPACK's ipiv 0-based) on the device.  ``solve(b)`` = lu_solver.solve (solvers.pyx:80-186);
    calling the object applies A^-1 to a device vector, so it can be the ``preconditioner=`` of cg / gmres / bicgstab."""

    def __init__(self, LU_dev, piv_dev, ctx):
        super().__init__(LU_dev, ctx)
        self._LU = LU_dev
        self._piv = piv_dev

    def _host(self):
        self.ctx.synchronize()
        return self._LU.cpu().numpy()

    @property
    def L(self):
        """the unit lower triangular factor as a numpy array (a copy; tests)"""
        return np.tril(self._host(), -1)+np.eye(self.num_rows)

    @property
    def U(self):
        """the upper triangular factor as a numpy array (a copy; tests)"""
        return np.triu(self._host())

    @property
    def piv(self):
        """the swap sequence: at step k the rows k and piv[k] were exchanged (a copy; tests)"""
        self.ctx.synchronize()
        return self._piv.cpu().numpy().copy()

    @property
    def perm(self):
        """the row order with A[perm] = L U"""
        perm = np.arange(self.num_rows)
        for k, p in enumerate(self.piv):
            perm[k], perm[p] = perm[p], perm[k]
        return perm

    def _trs(self, B, ldb, nrhs):
        self.ctx.getrs(self._LU.data_ptr(), _ld(self._LU), self.num_rows, self._piv.data_ptr(), B, ldb, nrhs)

    def __repr__(self):
        return '<LU factors of a {}x{} dense operator on {}>'.format(self.num_rows, self.num_columns, self.device)


def plu(A, overwrite=False):
    """LU factorisation with partial pivoting of a square dense operator, symmetric or not, on its device (pnl_getrf).  Without
    ``overwrite`` a device copy of the block is factored; with it the operator's own storage becomes the factors (the operator is
    invalidated and must not be applied any more).  Raises numpy.linalg.LinAlgError if a pivot is zero."""
    import torch
    Ld = _factor_block(A, overwrite, 'plu', lambda A: A.num_rows == A.num_columns,
                       'a square Dense_LinearOperator on one GPU is needed (direct solves of H2, sparse or distributed '
                       'operators are not built)')
    n = A.num_rows
    piv = torch.empty(max(n, 1), dtype=torch.int32, device=Ld.device)
    info = A.ctx.getrf(Ld.data_ptr(), _ld(Ld), n, piv.data_ptr())
    if overwrite:
        A.invalidate()
    if info > 0:
        raise np.linalg.LinAlgError('plu: the pivot of column {} is zero, the operator is singular'.format(info))
    return LUFactor(Ld, piv[:n], A.ctx)


def lu(A):
    """the reference's name (lu_solver): for a symmetric dense operator the Cholesky factor.  ``plu`` is the pivoted factorisation,
    for symmetric and non-symmetric operators alike."""
    if not getattr(A, 'symmetric', False):
        raise NotImplementedError('LU with pivoting')
    return chol(A)
