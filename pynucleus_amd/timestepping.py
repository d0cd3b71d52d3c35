"""IMEX Runge-Kutta time stepping for reaction-diffusion systems with a nonlocal operator,

    m_c M u_c' + S u_c - N_c(u) = g_c(t),      c = 0 .. ncomp - 1,

the operator implicit, the pointwise nonlinearity explicit, Picard iteration on top.

Host-side mirror of ``IMEX`` / ``EulerIMEX`` / ``ARS3`` / ``koto`` (base/PyNucleus_base/timestepping.py:377-682) with the sign
conventions of ``_stepOfPicard``: E = -N(U), I = S U.  One sweep is one library call (csrc/pnl_reaction.hip: pnl_imex_sweep)
that composes pnl_csr_matvec, pnl_gemv_axpby, pnl_assemble_nonlinearity, pnl_mg_cg or pnl_potrs and pnl_csr_cg_jacobi; the
vectors never leave HBM.  This module builds the implicit systems m_c M + dt gamma S once per dt (``buildTransientHierarchy``),
keeps them alive and hands pointers over.  No CPU fallback.
"""
import numpy as np
from . import _lib


class IMEX:
    """IMEX(hierarchy, fun, dt, c, AExpl, AImpl, bExpl, bImpl, massScales): ``hierarchy`` is a fractionalHierarchy (or its level
    list) built with buildMass=True whose finest operator S is dense and symmetric; ``fun`` a reaction.multi_function with as
    many inputs and outputs as there are components.  solver='cg-mg': multigrid-preconditioned CG on the hierarchy of
    m_c M + dt gamma S per component; 'chol': that matrix on the finest level factored once per component.  The mass solve at
    the end of a sweep is Jacobi-CG on m_c M to massTol."""
    gamma = None

    def __init__(self, hierarchy, fun, dt, c, AExpl, AImpl, bExpl, bImpl, massScales=None, solver='cg-mg', tol=1e-8, maxiter=100,
                 massTol=None, massMaxiter=1000, smoother=('jacobi', {'omega': 2.0/3.0})):
        from .linear_operators import Dense_LinearOperator
        if solver not in ('cg-mg', 'chol'):
            raise NotImplementedError('solver {!r}: cg-mg and chol are built'.format(solver))
        levels = hierarchy.getLevelList() if hasattr(hierarchy, 'getLevelList') else list(hierarchy)
        for L in levels[:-1] if solver == 'cg-mg' else []:
            if not isinstance(L['A'], Dense_LinearOperator):
                raise NotImplementedError('IMEX stepping needs dense levels; got {!r}'.format(L['A']))
        S = levels[-1]['A']
        if not isinstance(S, Dense_LinearOperator) or S.num_rows != S.num_columns:
            raise NotImplementedError('IMEX stepping needs a dense operator on the finest level (H2 and sparse operators are not built); '
                                      'got {!r}'.format(S))
        if not S.symmetric:
            raise NotImplementedError('IMEX stepping needs a symmetric operator (CG and Cholesky solves)')
        if 'M' not in levels[-1]:
            raise AssertionError('the hierarchy has no mass matrices (buildMass=True)')
        self.c = np.asarray(c, dtype=np.float64)
        self.AExpl, self.AImpl = np.asarray(AExpl, dtype=np.float64), np.asarray(AImpl, dtype=np.float64)
        self.bExpl, self.bImpl = np.asarray(bExpl, dtype=np.float64), np.asarray(bImpl, dtype=np.float64)
        self.s = s = self.AExpl.shape[0]
        assert self.AImpl.shape == (s, s) and self.AExpl.shape == (s, s) and self.bExpl.shape == self.bImpl.shape == self.c.shape == (s,)
        if s > _lib.PNL_IMEX_MAX_STAGES:
            raise NotImplementedError('{} stages (at most {})'.format(s, _lib.PNL_IMEX_MAX_STAGES))
        diag = [self.AImpl[k, k] for k in range(s) if np.abs(self.AExpl[k]).max() != 0.]
        if not diag or min(diag) != max(diag) or not diag[0] > 0.:
            raise NotImplementedError('the implicit stages must share one positive diagonal entry of AImpl; got {}'.format(diag))
        self.gamma = float(diag[0])
        self.fun = fun
        self.ncomp = int(fun.numInputs)
        if fun.numOutputs != self.ncomp or self.ncomp > _lib.PNL_IMEX_MAX_COMP:
            raise NotImplementedError('a nonlinearity with {} inputs and {} outputs'.format(fun.numInputs, fun.numOutputs))
        self.massScales = np.ones(self.ncomp) if massScales is None else np.asarray(massScales, dtype=np.float64)
        assert self.massScales.shape == (self.ncomp,) and (self.massScales > 0.).all()
        self.solverType, self.tol, self.maxiter = solver, float(tol), int(maxiter)
        self.massTol, self.massMaxiter = float(tol if massTol is None else massTol), int(massMaxiter)
        self.smoother = smoother
        self.levels = levels
        self.S, self.dm = S, levels[-1]['DoFMap']
        self.ctx, self.device, self.n = S.ctx, S.A.device, S.num_rows
        from .multigrid import _DevCSR
        from .reaction import getSpace
        self.M = _DevCSR(levels[-1]['M'], self.device)
        self.space = getSpace(self.dm, self.ctx)
        self.iterations = []             # per sweep: [(s + 1), ncomp] iterations of the stage solves and of the mass solves
        self.picardNorms = []            # per picardStep: the norms of the Picard updates
        self.dt = None
        self._imex = None
        self._setup(float(dt))

    # -- the implicit systems, once per dt -----------------------------------------------------------------------------
    def _release(self):
        if getattr(self, '_imex', None) and getattr(self.ctx, 'h', None):
            self.ctx.imex_destroy(self._imex)
        self._imex = None
        self.solvers = []

    def _setup(self, dt):
        import torch
        from .multigrid import buildTransientHierarchy, multigrid
        assert dt > 0.
        self._release()
        self.dt = dt
        d = _lib.pnl_imex_desc()
        d.s, d.ncomp, d.n, d.fun = self.s, self.ncomp, self.n, int(self.fun.fun)
        d.nparams = len(self.fun.params)
        for i, p in enumerate(self.fun.params):
            d.params[i] = float(p)
        d.solver = _lib.PNL_IMEX_CHOL if self.solverType == 'chol' else _lib.PNL_IMEX_CG_MG
        d.maxiter, d.mass_maxiter = self.maxiter, self.massMaxiter
        for k in range(self.s):
            d.bE[k], d.bI[k] = self.bExpl[k], self.bImpl[k]
            for j in range(self.s):
                d.AE[k*self.s+j], d.AI[k*self.s+j] = self.AExpl[k, j], self.AImpl[k, j]
        d.dt, d.tol, d.mass_tol = dt, self.tol, self.massTol
        d.S_dev, d.ldS = self.S.A.data_ptr(), self.S.A.stride(0) if self.n > 1 else self.S.A.shape[1]
        d.M_indptr_dev, d.M_indices_dev, d.M_data_dev = self.M.indptr.data_ptr(), self.M.indices.data_ptr(), self.M.data.data_ptr()
        d.space = self.space._h
        for c in range(self.ncomp):
            d.mass_scale[c] = self.massScales[c]
            if self.solverType == 'chol':
                from .solvers import chol
                T = buildTransientHierarchy(self.levels[-1:], self.massScales[c], dt*self.gamma)[-1]['A']
                T.symmetric = True
                F = chol(T, overwrite=True)
                self.solvers.append(F)
                d.chol_dev[c], d.ldchol[c] = F._L.data_ptr(), F._L.stride(0) if self.n > 1 else F._L.shape[1]
            else:
                mg = multigrid(buildTransientHierarchy(self.levels, self.massScales[c], dt*self.gamma), smoother=self.smoother, ctx=self.ctx)
                if not getattr(mg, '_native', False):
                    raise NotImplementedError('IMEX stepping needs the library multigrid (dense levels, Jacobi smoother); '
                                              'got smoother={!r} / a level that is not dense'.format(self.smoother))
                self.solvers.append(mg)
                d.mg[c] = mg._mg.value
        torch.cuda.current_stream(self.device).synchronize()
        self.ctx.synchronize()
        self._desc = d
        self._imex = self.ctx.imex_create(d)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # -- stepping ------------------------------------------------------------------------------------------------------
    def _check(self, u):
        import torch
        if not (isinstance(u, torch.Tensor) and u.device == self.device and u.dtype == torch.float64 and u.is_contiguous()
                and u.numel() == self.ncomp*self.n):
            raise AssertionError('u must be a contiguous fp64 device tensor [{}, {}]'.format(self.ncomp, self.n))

    def _force(self, force):
        import torch
        if force is None:
            return None
        if isinstance(force, torch.Tensor):
            f = force.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(force, dtype=np.float64))).to(self.device)
        assert f.numel() == self.s*self.ncomp*self.n, 'force: the values of g at the stages, [s, ncomp, n]'
        return f

    def _sweep(self, u_prev, u, f):
        import torch
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        its = self.ctx.imex_sweep(self._imex, u_prev.data_ptr(), u.data_ptr(), f.data_ptr() if f is not None else None, (self.s+1)*self.ncomp)
        self.iterations.append(its.reshape(self.s+1, self.ncomp))

    def step(self, t, dt, u, force=None):
        """one sweep with u_prev = u; u (device tensor [ncomp, n]) is overwritten; returns t + dt"""
        self._check(u)
        if dt is not None and float(dt) != self.dt:
            self._setup(float(dt))
        self._sweep(u, u, self._force(force))
        return t+self.dt

    def picardStep(self, t, dt, u, tol=1e-3, force=None, maxPicard=1000):
        """sweeps from (u_prev, u) with u_prev fixed at the entry value of u until the 2-norm over all components of the update is
        <= tol; returns (t + dt, number of sweeps)"""
        import torch
        self._check(u)
        if dt is not None and float(dt) != self.dt:
            self._setup(float(dt))
        f = self._force(force)
        u_prev = u.clone()
        its, norms = 0, []
        while True:
            old = u.clone()
            self._sweep(u_prev, u, f)
            its += 1
            norms.append(float(torch.linalg.norm((u-old).reshape(-1))))
            if norms[-1] <= tol:
                break
            if not np.isfinite(norms[-1]) or its >= maxPicard:
                raise RuntimeError('Picard iteration did not converge: update norms {}'.format(norms[-5:]))
        self.picardNorms.append(norms)
        return t+self.dt, its


_G = (3.+np.sqrt(3.))/6.
# name -> (c, AExpl, AImpl, bExpl, bImpl), timestepping.py:599-682
_TABLEAUX = {
    'euler_imex': ([0., 1.], [[0., 0.], [1., 0.]], [[0., 0.], [0., 1.]], [1., 0.], [0., 1.]),
    'ars3': ([0., _G, 1.-_G], [[0., 0., 0.], [_G, 0., 0.], [_G-1., 2.*(1.-_G), 0.]], [[0., 0., 0.], [0., _G, 0.], [0., 1.-2.*_G, _G]],
             [0., .5, .5], [0., .5, .5]),
    'koto': ([0., 1., .5, 1.], [[0., 0., 0., 0.], [1., 0., 0., 0.], [.5, 0., 0., 0.], [0., 0., 1., 0.]],
             [[0., 0., 0., 0.], [0., 1., 0., 0.], [0., -.5, 1., 0.], [0., -1., 1., 1.]], [0., 0., 1., 0.], [0., -1., 1., 1.]),
}


def tableau(name):
    """(c, AExpl, AImpl, bExpl, bImpl) of 'euler_imex', 'ars3' or 'koto' as numpy arrays"""
    return tuple(np.asarray(a, dtype=np.float64) for a in _TABLEAUX[name])


class EulerIMEX(IMEX):
    gamma = 1.

    def __init__(self, hierarchy, fun, dt, **kwargs):
        super().__init__(hierarchy, fun, dt, *tableau('euler_imex'), **kwargs)


class ARS3(IMEX):
    gamma = _G

    def __init__(self, hierarchy, fun, dt, **kwargs):
        super().__init__(hierarchy, fun, dt, *tableau('ars3'), **kwargs)


class koto(IMEX):
    gamma = 1.

    def __init__(self, hierarchy, fun, dt, **kwargs):
        super().__init__(hierarchy, fun, dt, *tableau('koto'), **kwargs)


_STEPPERS = {'euler_imex': EulerIMEX, 'ars3': ARS3, 'koto': koto}


def timestepperFactory(name, *args, **kwargs):
    """timestepperFactory('euler_imex' | 'ars3' | 'koto', hierarchy, fun, dt, ...)"""
    if name not in _STEPPERS:
        raise NotImplementedError('time stepper {!r}: {} are built here (the theta methods live in multigrid.py)'.format(name, sorted(_STEPPERS)))
    return _STEPPERS[name](*args, **kwargs)
