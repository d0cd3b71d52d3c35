#!/usr/bin/env python3
"""A sweep over the fractional order with ONE set of assembled operators: (-Delta)^s u = f for a dozen orders s, then the
recovery of an order from a solution.

The kernel is a ranged fractional kernel (getFractionalKernel(dim, admissibleSet([s_left, s_right]))): assembleNonlocal cuts the range
into intervals, assembles the operator at a few Chebyshev nodes per interval when the interval is first visited, and
A(s) = sum_k w_k(s) A(s_k) afterwards costs a weight update (``set``), one pass over the node blocks (``materialize``) and the solve.
Per order the example prints that time against a fresh assembly (getDense) plus the same solve, and the difference of the two
solutions; then it recovers s* from u(s*) by a scalar minimisation over s that touches only the interpolated operator.

    python examples/fractional_order_sweep.py [interval|disc] [noRef]
"""
import sys
import time
import numpy as np
sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__))))
from pynucleus_amd import driverMesh, P1_DoFMap, PHYSICAL, getFractionalKernel, admissibleSet  # noqa: E402

domain = sys.argv[1] if len(sys.argv) > 1 else 'interval'
dim = 1 if domain == 'interval' else 2
noRef = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if dim == 1 else 4)
s_left, s_right = (0.2, 0.8) if dim == 1 else (0.3, 0.7)

mesh = driverMesh(domain, noRef)
dm = P1_DoFMap(mesh, PHYSICAL)
f = np.asarray(dm.assembleRHS(1.0))
kernel = getFractionalKernel(dim, admissibleSet([s_left, s_right]))
A = dm.assembleNonlocal(kernel, 'dense')
print('{}: {} DoFs, h = {:.4g}; {}'.format(domain, dm.num_dofs, mesh.h, A))


def solve_interpolated(s):
    A.set(s)
    return A.materialize().solve_direct(f)


def solve_fresh(s):
    return dm.assembleNonlocal(kernel.getFrozenKernel(s), 'dense').solve_direct(f)


def clock(fn, s):
    t0 = time.perf_counter()
    u = fn(s)                                     # solve_direct returns a host vector: the device work has finished
    return u, time.perf_counter()-t0


solve_fresh(0.5*(s_left+s_right))                 # warm the kernels of both paths outside the timed sweep
print('{:>8s} {:>10s} {:>16s} {:>12s} {:>14s}'.format('s', 'interval', 'interpolated [s]', 'fresh [s]', 'rel. difference'))
totals, visited = [0., 0.], set()
for s in np.linspace(s_left, s_right, 12):
    u, t_int = clock(solve_interpolated, s)       # includes the assembly of an interval's node operators on its first visit
    first = '' if A.selected in visited else '   first visit: {} node operators assembled'.format(A.getSelectedOp().numInterpolationNodes)
    visited.add(A.selected)
    v, t_fresh = clock(solve_fresh, s)
    totals[0] += t_int
    totals[1] += t_fresh
    print('{:8.4f} {:10d} {:16.4f} {:12.4f} {:14.3e}{}'.format(s, A.selected, t_int, t_fresh, np.abs(u-v).max()/np.abs(v).max(), first))
print('sweep: interpolated {:.3f} s (node operators assembled on the way: {} of {}), fresh assemblies {:.3f} s'.format(
    totals[0], sum(op.numInterpolationNodes for op in A.ops if op.constructed), A.numInterpolationNodes, totals[1]))
t0 = time.perf_counter()
for s in np.linspace(s_left, s_right, 12):
    solve_interpolated(s)
print('the same sweep again, every node operator in place: {:.3f} s'.format(time.perf_counter()-t0))

# order identification: s* from u(s*), with the interpolated operator only
from scipy.optimize import minimize_scalar  # noqa: E402
s_star = s_left+0.618*(s_right-s_left)
u_star = solve_fresh(s_star)
evals = [0]


def misfit(s):
    evals[0] += 1
    d = solve_interpolated(s)-u_star
    return float(d@d)


t0 = time.perf_counter()
res = minimize_scalar(misfit, bounds=(s_left, s_right), method='bounded', options=dict(xatol=1e-6))
print('order identification: s* = {:.6f}, recovered {:.6f} (error {:.2e}) in {} solves, {:.3f} s'.format(
    s_star, res.x, abs(res.x-s_star), evals[0], time.perf_counter()-t0))
