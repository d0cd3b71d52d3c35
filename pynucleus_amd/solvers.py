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
    device = _device_of(A)
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    dinv = None
    B = None
    if preconditioner == 'jacobi':
        dinv = _jacobi_dinv(A, device)
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


class _Group:
    """At most 16 rows of a block solve over the library's step calls: the device blocks, ``A.matvec_multi`` as the product, the fences
    between the context's stream and torch's, the read-back of the state and the record of the rows.  A recurrence supplies
    ``start(AX_ptr)`` and ``one_pass(it)`` (``run``).  B [nv, n] with a unit inner stride; X [nv, n] contiguous holds the guesses and
    the results."""

    def __init__(self, A, ctx, B, X):
        self.A, self.ctx, self.B, self.X = A, ctx, B, X
        (self.nv, self.n), self.dev = B.shape, B.device
        self.ldb = max(int(B.stride(0)), self.n)

    def blocks(self, k):
        import torch
        return tuple(torch.empty((self.nv, self.n), dtype=torch.float64, device=self.dev) for _ in range(k))

    def new_state(self, width):
        import torch
        self.width = width
        self.state = torch.zeros(self.nv*width, dtype=torch.float64, device=self.dev)
        return self.state.data_ptr()

    def fence(self):
        import torch
        torch.cuda.current_stream(self.dev).synchronize()

    def product(self, V, op=None):
        """A V, or ``op`` V for another operator of the same size (the mass matrix of lobpcg)"""
        self.ctx.synchronize()
        W = (self.A if op is None else op).matvec_multi(V)
        self.fence()
        return W

    def apply(self, cycle, V, out=None):
        """cycle(V) (a block [nv, n] -> M^-1 of every row: multigrid.cycle), contiguous or copied into ``out``"""
        self.ctx.synchronize()
        Z = cycle(V)
        Z = Z.contiguous() if out is None else out.copy_(Z)
        self.fence()
        return Z

    def read_state(self):
        self.ctx.synchronize()
        return self.state.cpu().numpy().reshape(self.nv, self.width)

    def run(self, start, one_pass, have_x0, maxiter, its, res):
        """its / res are filled: the rows that are active here and no longer on the device have ended in that pass (state slot 3 is the
        residual, slot 4 the active flag, for every solver)"""
        AX = self.product(self.X) if have_x0 else None
        self.fence()
        start(AX.data_ptr() if AX is not None else 0)
        st = self.read_state()
        res[:] = st[:, 3]
        its[:] = 0
        active = st[:, 4] != 0.
        for it in range(maxiter):
            if not active.any():
                break
            one_pass(it)
            st = self.read_state()
            res[active] = st[active, 3]
            done = active & (st[:, 4] == 0.)
            its[done] = it
            active &= ~done
        its[active] = maxiter


def _cg_recurrence(g, dinv, tol):
    """the loop of pnl_cg_jacobi_block (csrc/pnl_cg_block.hip) over its fused steps; ``dinv`` None: the unit diagonal"""
    from ._lib import PNL_CGB_STATE
    ctx, n, nv, B, X, sp = g.ctx, g.n, g.nv, g.B, g.X, g.new_state(PNL_CGB_STATE)
    R, P, Z = g.blocks(3)
    dp = dinv.data_ptr() if dinv is not None else 0

    def start(AX):
        ctx.cgb_init(n, nv, dp, B.data_ptr(), g.ldb, AX, n, R.data_ptr(), n, P.data_ptr(), n, tol, sp)

    def one_pass(it):
        AP = g.product(P)
        ctx.cgb_update(n, nv, dp, P.data_ptr(), n, AP.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, Z.data_ptr(), n, sp)
        if it > 0 and it % 50 == 0:
            AX = g.product(X)                           # recalculate the residual to avoid rounding errors
            ctx.cgb_refresh(n, nv, dp, B.data_ptr(), g.ldb, AX.data_ptr(), n, R.data_ptr(), n, Z.data_ptr(), n, sp)
        ctx.cgb_direction(n, nv, Z.data_ptr(), n, P.data_ptr(), n, tol, sp)
    return start, one_pass


def _cg_mg_recurrence(g, cycle, tol):
    """the loop of pnl_mg_cg_block (csrc/pnl_mg_block.hip) over the external-preconditioner steps, ``cycle`` (one V cycle from a zero
    guess for every row) applied between them"""
    from ._lib import PNL_CGB_STATE
    ctx, n, nv, B, X, sp = g.ctx, g.n, g.nv, g.B, g.X, g.new_state(PNL_CGB_STATE)
    R, P = g.blocks(2)

    def start(AX):
        ctx.cgb_residual(n, nv, B.data_ptr(), g.ldb, AX, n, R.data_ptr(), n, 0)
        Z = g.apply(cycle, R)
        ctx.cgb_start(n, nv, R.data_ptr(), n, Z.data_ptr(), n, P.data_ptr(), n, tol, sp)

    def one_pass(it):
        AP = g.product(P)
        ctx.cgb_step(n, nv, P.data_ptr(), n, AP.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, sp)
        if it > 0 and it % 50 == 0:
            AX = g.product(X)                           # recalculate the residual to avoid rounding errors
            ctx.cgb_residual(n, nv, B.data_ptr(), g.ldb, AX.data_ptr(), n, R.data_ptr(), n, sp)
        Z = g.apply(cycle, R)
        ctx.cgb_beta(n, nv, R.data_ptr(), n, Z.data_ptr(), n, sp)
        ctx.cgb_direction(n, nv, Z.data_ptr(), n, P.data_ptr(), n, tol, sp)
    return start, one_pass


def _bicgstab_recurrence(g, pre, tol):
    """the loop of pnl_bicgstab_block (csrc/pnl_bicgstab_block.hip) over its steps.  ``pre`` a callable: the external mode, ``pre`` (a
    block cycle) applied here between the steps; else ``pre`` is dinv (None: the unit diagonal), applied by the steps"""
    from ._lib import PNL_BCGB_STATE
    ctx, n, nv, B, X, sp = g.ctx, g.n, g.nv, g.B, g.X, g.new_state(PNL_BCGB_STATE)
    ext = callable(pre)
    cycle = pre
    R, P, R0, P2, S2 = g.blocks(5)
    dp = pre.data_ptr() if pre is not None and not ext else 0

    def start(AX):
        ctx.bcgb_init(n, nv, ext, dp, B.data_ptr(), g.ldb, AX, n, R.data_ptr(), n, P.data_ptr(), n, R0.data_ptr(), n, P2.data_ptr(), n, sp)
        if ext:
            g.apply(cycle, R, R0)
            P2.copy_(R0)                                # P = R at the start
            g.fence()
            ctx.bcgb_start(n, nv, R.data_ptr(), n, R0.data_ptr(), n, sp)

    def one_pass(it):
        T = g.product(P2)
        ctx.bcgb_alpha(n, nv, ext, dp, T.data_ptr(), n, R0.data_ptr(), n, R.data_ptr(), n, S2.data_ptr(), n, sp)
        if ext:
            g.apply(cycle, R, S2)                       # S lives in R between the two steps
        T2 = g.product(S2)
        ctx.bcgb_omega(n, nv, P2.data_ptr(), n, S2.data_ptr(), n, T2.data_ptr(), n, R0.data_ptr(), n, X.data_ptr(), n, R.data_ptr(), n, tol, sp)
        ctx.bcgb_direction(n, nv, ext, dp, R.data_ptr(), n, T.data_ptr(), n, P.data_ptr(), n, P2.data_ptr(), n, sp)
        if ext:
            g.apply(cycle, P, P2)
    return start, one_pass


def _device_of(A, constructed=False):
    """the device of the vectors of an operator.  One that shows neither ``device`` nor a dense block is asked (``_device()``) only
    once it is ``constructed``, as the block front end has seen to; else the current device stands in"""
    import torch
    device = getattr(A, 'device', None)
    if device is None:
        device = A.A.device if hasattr(A, 'A') else (A._device() if constructed else torch.device('cuda', torch.cuda.current_device()))
    return device


def _jacobi_dinv(A, device):
    d = A.diagonal
    d = d() if callable(d) else d
    return 1./_dev_vector(d, device)


def _block_preconditioner(name, A, preconditioner):
    """what ``name`` (cg_multi, bicgstab_multi, lobpcg) takes: the multigrid behind ``preconditioner`` (None for 'jacobi' and None) if A and it
    are fit for a block of right-hand sides, NotImplementedError if not"""
    from .multigrid import multigrid as _multigrid
    from .linear_operators import DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator
    from .distributed_h2 import DistributedH2Matrix_localData
    # a multigrid object, or the callable of its asPreconditioner(): the block cycle of that hierarchy
    mg = preconditioner if isinstance(preconditioner, _multigrid) else getattr(preconditioner, 'multigrid', None)
    if mg is None and callable(preconditioner):
        raise NotImplementedError('{}: a plain callable as preconditioner for a block of right-hand sides is not built '
                                  '(pass a multigrid object or its asPreconditioner())'.format(name))
    if mg is None and preconditioner not in ('jacobi', None):
        raise NotImplementedError(preconditioner)
    if isinstance(A, (DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator,
                      DistributedH2Matrix_localData)):
        raise NotImplementedError('{}: the block products of the distributed operators loop their matvec; {}'.format(
            name, 'eigenpairs of distributed operators are not built' if name == 'lobpcg' else 'solve row by row with '+name[:-len('_multi')]))
    if not hasattr(A, 'matvec_multi'):
        raise NotImplementedError('{} needs an operator with matvec_multi; got {!r}'.format(name, A))
    if mg is not None:
        mg._require_block()                                 # NotImplementedError for a Chebyshev smoother, H2 / sparse levels
    return mg


def _block_context(A):
    """(context, device) of the operator behind a block solve, constructed if it is assembled lazily"""
    if hasattr(A, 'assure_constructed'):
        A.assure_constructed()
    return (A.ctx if hasattr(A, 'ctx') else A.ops[0].ctx), _device_of(A, constructed=True)


def _block_steps(name, A, B, X0, tol, maxiter, preconditioner, library=None):
    """``name`` (cg_multi, bicgstab_multi): the checks, then ``library(mg)`` -- the solver's fast paths into the library, which returns
    None where none applies -- and else the loop over the library's step calls, groups of 16 rows"""
    from ._lib import PNL_CGB_MAXVEC
    from .linear_operators import _rhs_blocks, _block_out
    mg = _block_preconditioner(name, A, preconditioner)
    out = library(mg) if library is not None else None
    if out is not None:
        return out
    ctx, device = _block_context(A)
    assert A.num_rows == A.num_columns, A.shape
    Bd, X = _rhs_blocks(B, X0, device, A.num_rows)
    # the preconditioner of the recurrence: the block cycle, or dinv (None: the unit diagonal)
    if mg is not None:
        pre = preconditioner if callable(preconditioner) else mg.cycle
    else:
        pre = _jacobi_dinv(A, device) if preconditioner == 'jacobi' else None
    recurrence = _bicgstab_recurrence if name == 'bicgstab_multi' else (_cg_recurrence if mg is None else _cg_mg_recurrence)
    nrhs = Bd.shape[0]
    its, res = np.zeros(nrhs, dtype=np.int32), np.zeros(nrhs)
    for v0 in range(0, nrhs, PNL_CGB_MAXVEC):
        v1 = min(nrhs, v0+PNL_CGB_MAXVEC)
        g = _Group(A, ctx, Bd[v0:v1], X[v0:v1])
        g.run(*recurrence(g, pre, tol), X0 is not None, maxiter, its[v0:v1], res[v0:v1])
    return _block_out(B, X), its, res


def _cg_steps(A, B, X0, tol, maxiter, preconditioner):
    """cg_multi without its library fast paths (tests compare the two)"""
    return _block_steps('cg_multi', A, B, X0, tol, maxiter, preconditioner)


def _bicgstab_steps(A, B, X0, tol, maxiter, preconditioner):
    """bicgstab_multi without its library fast path (tests compare the two)"""
    return _block_steps('bicgstab_multi', A, B, X0, tol, maxiter, preconditioner)


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
    from .linear_operators import Dense_LinearOperator

    def library(mg):
        if mg is not None:
            if isinstance(A, Dense_LinearOperator) and A.num_rows == A.num_columns == mg.num_rows and getattr(preconditioner, 'maxIter', 1) == 1:
                return mg._cg_block(B, X0, tol, maxiter, None if A is mg.A else A)          # one library call (pnl_mg_cg_block)
        elif isinstance(A, Dense_LinearOperator) and A.symmetric and preconditioner == 'jacobi':
            return A.solve_cg_jacobi_block(B, X0, tol, maxiter)
    return _block_steps('cg_multi', A, B, X0, tol, maxiter, preconditioner, library)


def gmres(A, b, x0=None, tol=1e-8, maxiter=50, restarts=1, preconditioner=None, left=True):
    """Solve A x = b for a general operator.  ``preconditioner``: 'jacobi', None or a callable r -> B r on device vectors
    (multigrid.asPreconditioner()).  Returns (x, iterations, residuals): the residuals are the norms of the (left-
    preconditioned) residual, the first one computed, the others from the rotated right-hand side like the reference."""
    import torch
    device = _device_of(A)
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    B = None
    if preconditioner == 'jacobi':
        dinv = _jacobi_dinv(A, device)
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

    def library(mg):
        if mg is None and isinstance(A, Dense_LinearOperator) and A.num_rows == A.num_columns:
            return A.solve_bicgstab_block(B, X0, tol, maxiter, preconditioner)          # one library call (pnl_bicgstab_block)
    return _block_steps('bicgstab_multi', A, B, X0, tol, maxiter, preconditioner, library)


def bicgstab(A, b, x0=None, tol=1e-8, maxiter=50, preconditioner=None):
    """bicgstab_solver.solve (solvers.pyx:716-787): right-preconditioned stabilised BiCG, r0 = B r, stopping on the 2-norm of
    the residual.  Returns (x, iterations, residuals).  A 2-D b [nrhs, n] is a block of right-hand sides: ``bicgstab_multi``."""
    if getattr(b, 'ndim', None) == 2 or (not hasattr(b, 'ndim') and np.ndim(b) == 2):
        return bicgstab_multi(A, b, x0, tol, maxiter, preconditioner)
    import torch
    device = _device_of(A)
    bd = _dev_vector(b, device)
    x = torch.zeros_like(bd) if x0 is None else _dev_vector(x0, device).clone()
    B = None
    if preconditioner == 'jacobi':
        dinv = _jacobi_dinv(A, device)
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


_RITZ_RANK_TOL = 1e-10


def _ritz(GA, GM, idx, m):
    """The Rayleigh-Ritz problem of lobpcg on the rows ``idx`` of the Gram matrices S A S^T and S M S^T of a basis S: the ``m`` smallest
    Ritz values and C [len(idx), m] with (C^T S) M (C^T S)^T = I.  The basis may be numerically rank deficient (P against W late in the
    iteration): it is scaled to a unit diagonal of G_M, and the directions of the scaled G_M below _RITZ_RANK_TOL times its largest
    eigenvalue -- the level of a Gram matrix's own rounding is n u -- are dropped through its eigendecomposition."""
    idx = np.asarray(idx, dtype=np.int64)
    dg = np.diagonal(GM)[idx]
    idx = idx[np.isfinite(dg) & (dg > 0.)]
    GA, GM = GA[np.ix_(idx, idx)], GM[np.ix_(idx, idx)]
    GA, GM = .5*(GA+GA.T), .5*(GM+GM.T)
    d = 1./np.sqrt(np.diagonal(GM))
    GA, GM = d[:, None]*GA*d[None, :], d[:, None]*GM*d[None, :]
    lam, V = np.linalg.eigh(GM)
    keep = lam > _RITZ_RANK_TOL*lam[-1]
    if int(keep.sum()) < m:
        raise np.linalg.LinAlgError('lobpcg: the basis has rank {} < {} (linearly dependent start vectors?)'.format(int(keep.sum()), m))
    B = V[:, keep]/np.sqrt(lam[keep])
    theta, Z = np.linalg.eigh(B.T@GA@B)
    return theta[:m], idx, d[:, None]*(B@Z[:, :m])


def _mass_operator(M, ctx, device, n):
    """``M`` of lobpcg as an operator with matvec_multi: None stays None, a scipy.sparse matrix becomes a CSR_LinearOperator in ``ctx``
    (which must know the n DoFs, as every context that a builder has used does)"""
    import torch
    if M is None or hasattr(M, 'matvec_multi'):
        return M
    import scipy.sparse as sp
    from .linear_operators import CSR_LinearOperator
    if not sp.issparse(M):
        raise NotImplementedError('lobpcg: M is None, a scipy.sparse matrix or an operator with matvec_multi; got {!r}'.format(type(M)))
    Mc = sp.csr_matrix(M, dtype=np.float64)
    Mc.sum_duplicates()
    Mc.sort_indices()
    assert Mc.shape == (n, n), (Mc.shape, n)
    op = CSR_LinearOperator(Mc.indptr, Mc.indices, n, ctx, device)
    op.data_dev[:Mc.nnz] = torch.from_numpy(np.ascontiguousarray(Mc.data)).to(device)
    return op


def lobpcg(A, k=1, M=None, X0=None, tol=1e-8, maxiter=200, preconditioner='jacobi', blockSize=None):
    """The ``k`` smallest eigenvalues theta[0] <= ... <= theta[k-1] of A x = theta M x and their eigenvectors X [k, n] by LOBPCG
    (Knyazev 2001) with soft locking.  ``A``: symmetric positive definite, any operator with ``matvec_multi`` (dense, CSR, SSS, H2 in
    either far-field mode, interpolated).  ``M``: None (the identity), a scipy.sparse matrix (wrapped into a CSR_LinearOperator in A's
    context) or an operator with ``matvec_multi``; symmetric positive definite.  A block of m = ``blockSize`` (default
    min(16, n, k + max(2, k // 2)); k <= m <= 16) vectors is iterated: the rows beyond k are guard vectors, which speed up convergence
    and are never required to converge.  ``X0`` [m or k, n] is the start; without it, and for the rows it lacks, the rows of a
    standard-normal block drawn on the CPU with seed 0, so that a run repeats.  ``preconditioner``: 'jacobi', None, or a ``multigrid``
    object / its ``asPreconditioner()`` (dense levels, Jacobi smoother: the block V cycle on the residuals of the active columns).

    One pass: R = AX - theta MX, W = T R and the residual sums (pnl_eigb_residual; T the preconditioner); W made M-orthogonal to X and
    scaled (pnl_eigb_gram, pnl_eigb_combine); one ``A.matvec_multi(W)`` and, with M, one ``M.matvec_multi(W)``; the Gram matrices of
    the basis [X; W; P] against [AX; AW; AP] and [MX; MW; MP] (pnl_eigb_gram, at most 48 x 48), read back once; the small generalised
    eigenproblem on the host (``_ritz``); X, AX, MX and P, AP, MP as combinations of the basis (pnl_eigb_combine).

    residuals[v] = ||A x_v - theta_v M x_v||_2 / (|theta_v| ||M x_v||_2).  The AX and MX that the passes carry drift like a recursive
    CG residual, so a column counts as converged only on recomputed data: when the carried residuals of the first k columns are all
    <= tol, or maxiter is reached, AX = A X and MX = M X are formed afresh, theta become the Rayleigh quotients and the residuals are
    recomputed; then the solver returns, or goes on from these blocks if passes remain.  The returned residuals are always of that
    kind.  ``passes < maxiter`` with all residuals <= tol is success; else passes == maxiter and the residuals say how far each
    column got.  maxiter = 0 returns the Rayleigh-Ritz values of X0 and their residuals.  The rows of X are scaled to x^T M x = 1.
    Returns (theta [k], X [k, n], passes, residuals [k]); X is a torch tensor on the operator's device if X0 is one, else numpy."""
    import torch
    from ._lib import PNL_CGB_MAXVEC, PNL_EIGB_MAXBASIS
    from .linear_operators import _as_block
    mg = _block_preconditioner('lobpcg', A, preconditioner)
    k = int(k)
    if k > PNL_CGB_MAXVEC or (blockSize is not None and blockSize > PNL_CGB_MAXVEC):
        raise NotImplementedError('lobpcg: more than {} vectors are not built (k = {}, blockSize = {})'.format(PNL_CGB_MAXVEC, k, blockSize))
    ctx, device = _block_context(A)
    n = A.num_rows
    assert A.num_rows == A.num_columns, A.shape
    m = int(blockSize) if blockSize is not None else min(PNL_CGB_MAXVEC, n, k+max(2, k//2))
    if not 1 <= k <= m <= n:
        raise ValueError('lobpcg: 1 <= k <= blockSize <= n is needed (k = {}, blockSize = {}, n = {})'.format(k, m, n))
    if maxiter < 0:
        raise ValueError('lobpcg: maxiter < 0')
    Mop = _mass_operator(M, ctx, device, n)
    if mg is not None:
        cycle = preconditioner if callable(preconditioner) else mg.cycle
        dinv = None
    else:
        cycle = None
        dinv = _jacobi_dinv(A, device).contiguous() if preconditioner == 'jacobi' else None
    f64 = dict(dtype=torch.float64, device=device)
    LDG = PNL_EIGB_MAXBASIS

    # two sets of blocks [4 m, n], rows [raw W; X; W; P]: the basis [X; W; P] and [raw W; X] are contiguous, a combination is
    # written to the other set
    S = [torch.zeros((4*m, n), **f64) for _ in range(2)]
    AS = [torch.zeros((4*m, n), **f64) for _ in range(2)]
    MS = [torch.zeros((4*m, n), **f64) for _ in range(2)] if Mop is not None else S
    Rb = torch.zeros((m, n), **f64)
    Gd = torch.zeros((2, LDG, LDG), **f64)
    Cd = torch.zeros((2, PNL_CGB_MAXVEC, LDG), **f64)
    theta_d, sums_d = torch.zeros(m, **f64), torch.zeros(2*m, **f64)
    start = torch.randn((m, n), generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(device)
    if X0 is not None:
        X0d = _as_block(X0, device)
        if X0d.shape[1] != n or X0d.shape[0] not in (k, m):
            raise ValueError('lobpcg: X0 of shape {} for k = {}, blockSize = {}, n = {}'.format(tuple(X0d.shape), k, m, n))
        start[:X0d.shape[0]] = X0d
    cur = 0
    S[cur][m:2*m] = start
    rows = lambda T, b: T[b*m:(b+1)*m]                       # noqa: E731  block b of a set: 0 raw W, 1 X, 2 W, 3 P
    g = _Group(A, ctx, Rb, Rb)                              # the fences and the products of the block solvers
    fence = g.fence

    def product(op, V, out):
        out.copy_(g.product(V, None if op is A else op))
        fence()
    ptr = lambda T, b: T.data_ptr()+8*b*m*n                 # noqa: E731

    def grams(ka, kb, b):
        """(S A S^T, S M S^T) of the rows [b m, b m + ka) of the current set against the same rows of AS and MS, on the host"""
        ctx.eigb_gram(n, ka, ptr(S[cur], b), n, kb, ptr(AS[cur], b), n, Gd[0].data_ptr(), LDG)
        ctx.eigb_gram(n, ka, ptr(S[cur], b), n, kb, ptr(MS[cur], b), n, Gd[1].data_ptr(), LDG)
        ctx.synchronize()
        G = Gd.cpu().numpy()
        return G[0, :ka, :kb], G[1, :ka, :kb]

    def upload(theta, Cx=None, Cp=None):
        """theta and the coefficients of X (and P), as [m, kin] row-major blocks, to the device"""
        Ch = np.zeros((2, PNL_CGB_MAXVEC, LDG))
        if Cx is not None:
            Ch[0, :Cx.shape[1], :Cx.shape[0]] = Cx.T
        if Cp is not None:
            Ch[1, :Cp.shape[1], :Cp.shape[0]] = Cp.T
        Cd.copy_(torch.from_numpy(Ch))
        theta_d.copy_(torch.from_numpy(np.ascontiguousarray(theta)))
        fence()

    def rotate(kin, withP):
        """X, AX, MX (and P, AP, MP) of the other set from kin rows of the basis of the current one"""
        nonlocal cur
        for T in (S, AS)+((MS,) if Mop is not None else ()):
            ctx.eigb_combine(n, kin, ptr(T[cur], 1), n, m, Cd[0].data_ptr(), LDG, ptr(T[cur ^ 1], 1), n)
            if withP:
                ctx.eigb_combine(n, kin, ptr(T[cur], 1), n, m, Cd[1].data_ptr(), LDG, ptr(T[cur ^ 1], 3), n)
        cur ^= 1

    def residual(active, res, W):
        """R (and, with W, the raw W = dinv R) of the active columns; their carried or explicit residuals into res"""
        mask = int(sum(1 << v for v in range(m) if active[v]))
        ctx.eigb_residual(n, m, mask, ptr(AS[cur], 1), n, ptr(MS[cur], 1), n, theta_d.data_ptr(), dinv.data_ptr() if dinv is not None else 0,
                          Rb.data_ptr(), n, ptr(S[cur], 0) if W else 0, n, sums_d.data_ptr())
        ctx.synchronize()
        s = sums_d.cpu().numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.sqrt(s[0::2])/(np.abs(theta)*np.sqrt(s[1::2]))
        res[active] = np.where(np.isfinite(r), r, np.inf)[active]

    fence()
    product(A, rows(S[cur], 1), rows(AS[cur], 1))
    if Mop is not None:
        product(Mop, rows(S[cur], 1), rows(MS[cur], 1))
    GA, GM = grams(m, m, 1)
    theta, idx, C = _ritz(GA, GM, np.arange(m), m)
    upload(theta, C)
    rotate(m, False)
    haveP = False
    everyone = np.ones(m, dtype=bool)
    active = everyone.copy()
    res = np.full(m, np.inf)
    passes = 0
    ownW = cycle is None
    while True:
        residual(active, res, ownW)
        active &= res > tol
        if (res[:k] <= tol).all() or passes == maxiter:
            # the carried AX, MX say so: recompute them, theta as Rayleigh quotients and the residuals of every column
            product(A, rows(S[cur], 1), rows(AS[cur], 1))
            if Mop is not None:
                product(Mop, rows(S[cur], 1), rows(MS[cur], 1))
            GA, GM = grams(m, m, 1)
            theta, xmx = np.diagonal(GA)/np.diagonal(GM), np.diagonal(GM).copy()
            upload(theta)
            residual(everyone, res, ownW)
            if (res[:k] <= tol).all() or passes == maxiter:
                break
            active = res > tol
        if not ownW:
            # the block V cycle on the active residuals only; the raw W of the other rows stays what it was (they get weight 0)
            rows_on = torch.from_numpy(np.nonzero(active)[0]).to(device)
            rows(S[cur], 0).index_copy_(0, rows_on, g.apply(cycle, Rb.index_select(0, rows_on)))
            fence()
        # W <- D (W - (W MX^T) X), D = 1 / ||W||_2 for the active rows and 0 for the others: the coefficients stay on the device
        ctx.eigb_gram(n, m, ptr(S[cur], 0), n, m, ptr(MS[cur], 1), n, Gd[0].data_ptr(), LDG)
        ctx.eigb_gram(n, m, ptr(S[cur], 0), n, m, ptr(S[cur], 0), n, Gd[1].data_ptr(), LDG)
        ctx.synchronize()
        on = torch.from_numpy(active).to(device)
        nrm2 = torch.diagonal(Gd[1])[:m]
        sc = torch.where(on & (nrm2 > 0.), torch.rsqrt(torch.where(nrm2 > 0., nrm2, torch.ones_like(nrm2))), torch.zeros_like(nrm2))
        Cd[0].zero_()
        Cd[0, :m, :m] = torch.diag(sc)
        Cd[0, :m, m:2*m] = -sc[:, None]*torch.where(on[:, None], Gd[0, :m, :m], torch.zeros_like(Gd[0, :m, :m]))
        fence()
        ctx.eigb_combine(n, 2*m, ptr(S[cur], 0), n, m, Cd[0].data_ptr(), LDG, ptr(S[cur], 2), n)
        product(A, rows(S[cur], 2), rows(AS[cur], 2))
        if Mop is not None:
            product(Mop, rows(S[cur], 2), rows(MS[cur], 2))
        GA, GM = grams(3*m, 3*m, 1)
        act = np.nonzero(active)[0]
        theta, idx, C = _ritz(GA, GM, np.concatenate([np.arange(m), m+act, 2*m+act if haveP else act[:0]]), m)
        Cx = np.zeros((3*m, m))
        Cx[idx] = C
        Cp = Cx.copy()
        Cp[:m] = 0.
        upload(theta, Cx, Cp)
        rotate(3*m, True)
        haveP = True
        passes += 1
    # the rows that are returned: x^T M x = 1, and ascending theta (Rayleigh quotients of a cluster may have left the order of the
    # Ritz values by a rounding)
    order = np.argsort(theta[:k], kind='stable')
    Cn = np.zeros((k, k))
    Cn[order, np.arange(k)] = 1./np.sqrt(xmx[order])
    upload(theta, Cn)
    X = torch.empty((k, n), **f64)
    ctx.eigb_combine(n, k, ptr(S[cur], 1), n, k, Cd[0].data_ptr(), LDG, X.data_ptr(), n)
    ctx.synchronize()
    return theta[order], (X if isinstance(X0, torch.Tensor) else X.cpu().numpy()), passes, res[order]


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
