#!/usr/bin/env python3
"""The first six eigenvalues of (-Delta)^s with zero exterior values on the interval and on the disc, on the GPU.

One nonlocal operator per refinement level (assembled on the device, with the P1 mass matrices), then solvers.lobpcg on the finest
level for A x = lambda M x, preconditioned by the block V cycle of the hierarchy (the 'cg-mg' preconditioner of the solves).  For the
interval the values are printed beside Kwasnicki's asymptotics for (-1, 1) (J. Funct. Anal. 262 (2012)):
lambda_j = (j pi / 2 - (2 - 2 s) pi / 8)^(2 s) + O(1 / j), rescaled by (2 / length)^(2 s) if the mesh's interval is not (-1, 1).
A printout, not an assertion: the asymptotics are not sharp for small j, and the P1 values lie above the exact ones.

    python examples/fractional_eigenvalues.py [interval|disc|both] [noRef] [s]
"""
import os
import sys
import time
from math import pi
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynucleus_amd import getFractionalKernel, solvers  # noqa: E402
from pynucleus_amd.multigrid import fractionalHierarchy, multigrid  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else 'both'
s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
K = 6

for domain in (('interval', 'disc') if which == 'both' else (which,)):
    dim = 1 if domain == 'interval' else 2
    noRef = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if dim == 1 else 4)
    params = {'target_order': 2.-s} if dim == 1 else {'target_order': 0.5}
    t0 = time.time()
    H = fractionalHierarchy(domain, noRef, getFractionalKernel(dim, s), params, buildMass=True)
    t1 = time.time()
    A, M = H.finest['A'], H.finest['M']
    theta, X, passes, residuals = solvers.lobpcg(A, K, M=M, tol=1e-8, maxiter=200, preconditioner=multigrid(H))
    t2 = time.time()
    print('{}, s = {}: levels {} DoFs, hierarchy assembled in {:.2f} s; {} eigenpairs in {} LOBPCG passes, {:.2f} s, largest residual {:.2e}'.format(
        domain, s, [L['DoFMap'].num_dofs for L in H.getLevelList()], t1-t0, K, passes, t2-t1, float(np.max(residuals))))
    if dim == 1:
        v = np.asarray(H.finest['mesh'].vertices).ravel()
        scale = (2./(v.max()-v.min()))**(2.*s)
        print('   j   lambda_j (P1, h = {:.2e})   Kwasnicki (j pi/2 - (2 - 2s) pi/8)^(2s)'.format(float(np.max(H.finest['mesh'].hVector))))
        for j in range(1, K+1):
            print('  {:2d}   {:.10f}                {:.10f}'.format(j, theta[j-1], scale*(j*pi/2.-(2.-2.*s)*pi/8.)**(2.*s)))
    else:
        print('   j   lambda_j (P1, h = {:.2e})'.format(float(np.max(H.finest['mesh'].hVector))))
        for j in range(1, K+1):
            print('  {:2d}   {:.10f}'.format(j, theta[j-1]))
