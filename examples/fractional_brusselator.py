#!/usr/bin/env python3
"""The reference's Brusselator driver in miniature (drivers/brusselator.py): the two-species fractional reaction-diffusion system

          dU/dt = -(-Delta)^alpha U + (B - 1) U + Q^2 V + B/Q U^2 + 2 Q U V + U^2 V
    eta^2 dV/dt = -(-Delta)^beta  V -      B  U - Q^2 V - B/Q U^2 - 2 Q U V - U^2 V

with zero-flux conditions on a disc of radius 50 (or the interval (-50, 50)), alpha = beta = 0.75, stepped by an IMEX Runge-Kutta
scheme with Picard iteration: the operator implicit, the nonlinearity explicit.  The operator is assembled on the device once per
level; every sweep is one call into libpnl_hip.so (pnl_imex_sweep), the vectors stay in HBM.

    python examples/fractional_brusselator.py [disc|interval] [noRef] [euler_imex|ars3|koto] [chol|cg-mg] [steps]
"""
import sys
import time
import numpy as np
sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__))))
from pynucleus_amd.nonlocalProblems import brusselatorProblem  # noqa: E402
from pynucleus_amd.timestepping import timestepperFactory  # noqa: E402

domain = sys.argv[1] if len(sys.argv) > 1 else 'disc'
noRef = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stepperType = sys.argv[3] if len(sys.argv) > 3 else 'ars3'
solver = sys.argv[4] if len(sys.argv) > 4 else 'cg-mg'
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 5

import torch  # noqa: E402

problem = brusselatorProblem(domain, 'Neumann', noRef, 'spots')
t0 = time.time()
H = problem.hierarchy()
t1 = time.time()
dm = H.finest['DoFMap']
# the driver's defaults: dt = 0.01, linear solves to 1e-6, Picard iteration to 1e-4
dt = 0.01
ts = timestepperFactory(stepperType, H, problem.nonlinearity, dt, massScales=problem.massScales, solver=solver, tol=1e-6)
t2 = time.time()
print('{}: levels {} DoFs, hierarchy assembled in {:.2f} s, {} with solver {} set up in {:.2f} s; B = {:.4f}, Q = {:.4f}, dt = {}'.format(
    domain, [L['DoFMap'].num_dofs for L in H.getLevelList()], t1-t0, stepperType, solver, t2-t1, problem.B, problem.Q, dt))
u = torch.from_numpy(problem.initial(dm)).to(ts.device)
t = 0.
for k in range(steps):
    torch.cuda.synchronize()
    s0 = time.time()
    t, its = ts.picardStep(t, dt, u, tol=1e-4)
    torch.cuda.synchronize()
    s1 = time.time()
    uh = u.cpu().numpy()
    print('t = {:.4f}: {} Picard iterations ({:.1f} ms per sweep), U in [{:.6f}, {:.6f}], V in [{:.6f}, {:.6f}]'.format(
        t, its, 1e3*(s1-s0)/its, uh[0].min(), uh[0].max(), uh[1].min(), uh[1].max()))
