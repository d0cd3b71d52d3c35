"""Pointwise nonlinearities assembled against the test functions on the device.

Host-side mirror of ``multi_function`` / ``brusselator`` (fem/PyNucleus_fem/femCy.pyx:3025-3041) and ``assembleNonlinearity``
(femCy.pyx:3087-3178): for input vectors U[j, :] and f: R^nin -> R^nout,

    u_j(c, q) = sum_m U[j, dof(c, m)] phi_m(xi_q),      R[o, I] = sum_{dof(c, m) = I} vol_c sum_q w_q f_o(u(c, q)) phi_m(xi_q),

with the volume rules the reference picks (1D: two Gauss points; triangles: edge midpoints for P1, Radon's seven points for
P2).  The cell loop and the per-DoF sums run inside libpnl_hip.so (csrc/pnl_reaction.hip: pnl_assemble_nonlinearity); this
module keeps one ``fe_space`` per (DoF map, context) and hands device pointers over.  No CPU fallback.
"""
import weakref
import numpy as np
from . import _lib


class multi_function:
    """f: R^numInputs -> R^numOutputs, known to the library by ``fun`` (pnl_function) and ``params``; ``__call__`` evaluates it with
    numpy on arrays of shape [numInputs, ...] (host-side use: tests, initial data)"""
    numInputs = numOutputs = 0
    fun = -1
    params = ()

    def __call__(self, u):
        raise NotImplementedError()


class brusselator(multi_function):
    """z = B u + Q^2 v + (B/Q) u^2 + 2 Q u v + u^2 v,  f = (-u + z, -z)"""
    numInputs = numOutputs = 2
    fun = _lib.PNL_FUN_BRUSSELATOR

    def __init__(self, B, Q):
        self.B, self.Q = float(B), float(Q)
        self.params = (self.B, self.Q)

    def __call__(self, u):
        x, y = np.asarray(u[0], dtype=np.float64), np.asarray(u[1], dtype=np.float64)
        z = self.B*x+self.Q**2*y+self.B/self.Q*x**2+2.*self.Q*x*y+x**2*y
        return np.stack([-x+z, -z])


class cubic(multi_function):
    """u^3 - u (the derivative of the double-well potential, CahnHilliard_F_prime)"""
    numInputs = numOutputs = 1
    fun = _lib.PNL_FUN_CUBIC

    def __call__(self, u):
        x = np.asarray(u[0], dtype=np.float64)
        return np.stack([x**3-x])


def volumeRule(dm):
    """the rule of the nonlinearity assembly for this DoF map"""
    from .dofmap import P1_DoFMap, P2_DoFMap
    from .quadrature import Gauss1D, Gauss2D
    if not isinstance(dm, (P1_DoFMap, P2_DoFMap)):
        raise NotImplementedError('nonlinearities are assembled for P1 and P2 elements; got {}'.format(type(dm).__name__))
    md = dm.mesh.manifold_dim
    if md == 1:
        return Gauss1D(3)
    if md == 2:
        return Gauss2D(2 if isinstance(dm, P1_DoFMap) else 5)
    raise NotImplementedError('dimension {}'.format(md))


class fe_space:
    """pnl_fe_space of a DoF map in one context: cell -> DoF table, cell volumes, shape functions at the rule's nodes, and the
    library's inverted index and workspace"""

    def __init__(self, dm, ctx):
        qr = volumeRule(dm)
        self.ctx, self.num_dofs = ctx, int(dm.num_dofs)
        self.rule = qr
        self._h = ctx.fe_space_create(dm.dofs, dm.mesh.volVector, dm.evalShapeFunctions(qr.nodes), qr.weights, dm.num_dofs)

    def __del__(self):
        try:
            if getattr(self, '_h', None) and getattr(self.ctx, 'h', None):
                self.ctx.fe_space_destroy(self._h)
                self._h = None
        except Exception:
            pass


_spaces = weakref.WeakKeyDictionary()       # DoF map -> {id(context): fe_space}
_contexts = {}                              # device index -> Context for callers that bring none


def getSpace(dm, ctx):
    per = _spaces.setdefault(dm, {})
    sp = per.get(id(ctx))
    if sp is None or sp.ctx is not ctx:
        sp = per[id(ctx)] = fe_space(dm, ctx)
    return sp


def _default_context(device):
    idx = device.index if device.index is not None else 0
    if idx not in _contexts:
        _contexts[idx] = _lib.Context(idx)
    return _contexts[idx]


def assembleNonlinearity(dm, fun, U, out=None, alpha=1., beta=0., ctx=None):
    """out = beta out + alpha N(U) for device tensors U [numInputs, >= num_dofs] and out [numOutputs, >= num_dofs] (fp64, unit
    stride along a row; a 1-D tensor is one row).  Runs on torch's current stream; returns ``out``."""
    import torch
    if not isinstance(U, torch.Tensor) or not U.is_cuda or U.dtype != torch.float64:
        raise TypeError('U must be an fp64 tensor on the GPU')
    U2 = U if U.ndim == 2 else U.unsqueeze(0)
    if U2.stride(1) != 1:
        U2 = U2.contiguous()
    volumeRule(dm)                          # P0 / P3: NotImplementedError
    n = int(dm.num_dofs)
    if out is None:
        if beta != 0.:
            raise ValueError('beta != 0 needs out')
        out = torch.empty((fun.numOutputs, n), dtype=torch.float64, device=U.device)
    if n == 0:
        return out                          # a space without DoFs (one cell, Dirichlet): nothing to assemble
    ctx = ctx or _default_context(U.device)
    sp = getSpace(dm, ctx)
    R2 = out if out.ndim == 2 else out.unsqueeze(0)
    if not out.is_cuda or out.dtype != torch.float64 or R2.stride(1) != 1:
        raise TypeError('out must be an fp64 tensor on the GPU with unit stride along its rows')
    ldU = U2.stride(0) if U2.shape[0] > 1 else U2.shape[1]
    ldR = R2.stride(0) if R2.shape[0] > 1 else R2.shape[1]
    if U2.shape[1] < n or R2.shape[1] < n:
        raise _lib.PnlError('vectors of length {} / {} for a space with {} DoFs'.format(U2.shape[1], R2.shape[1], n))
    ctx.set_stream(torch.cuda.current_stream(U.device).cuda_stream)
    ctx.assemble_nonlinearity(sp._h, fun.fun, fun.params, U2.shape[0], U2.data_ptr(), ldU, R2.shape[0], alpha, beta, R2.data_ptr(), ldR)
    return out
