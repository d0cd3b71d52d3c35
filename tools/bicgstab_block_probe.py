"""Micro-benchmark of the block BiCGStab against sequential single-vector solves, in one process.

  The dense non-symmetric operator of fractionalHierarchy('disc', --noRef, smoothedLeftRightFractionalOrder(0.25, 0.75)) (P1,
  target_order 0.5; the finest level).  For nrhs in {1, 2, 4, 16}: solvers.bicgstab_multi (pnl_bicgstab_block: two pnl_gemv_block
  passes over the block per pass of the loop, the scalars on the device, one read-back per pass) against nrhs calls of
  solvers.bicgstab with a 1-D right-hand side (the Python loop over torch calls: two pnl_gemv products and five scalar read-backs
  per pass and right-hand side), at the same tol, maxiter and Jacobi preconditioner.  Right-hand side 0 is f = 1, the others are
  f = 1 times seeded random factors in [0.5, 1.5] per DoF.

Wall-clock seconds of the whole solves (both are synchronous) after one warm-up solve of every shape; block and loop alternate,
five rounds, the median is reported, with the iteration counts of both, the time per pass and the largest relative difference of
the solutions.  Prints one JSON line.
usage: bicgstab_block_probe.py [--noRef R] [--tol T] [--maxiter M] [--nrhs K ...]      (defaults: --noRef 5 --tol 1e-8 --maxiter 200)"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

NRHS = (1, 2, 4, 16)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter()-t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--noRef', type=int, default=5)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--maxiter', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--nrhs', type=int, nargs='*', default=list(NRHS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bicgstab_block_probe.py needs a GPU'
    from pynucleus_amd import getFractionalKernel, solvers
    from pynucleus_amd.fractionalOrders import smoothedLeftRightFractionalOrder
    from pynucleus_amd.multigrid import fractionalHierarchy
    t0 = time.perf_counter()
    H = fractionalHierarchy('disc', a.noRef, getFractionalKernel(2, smoothedLeftRightFractionalOrder(0.25, 0.75)), {'target_order': 0.5})
    A = H.finest['A']
    A.ctx.synchronize()
    t_asm = time.perf_counter()-t0
    assert not A.symmetric
    N = A.num_rows
    b = np.asarray(H.finest['DoFMap'].assembleRHS(1.0))
    kmax = max(a.nrhs)
    fac = np.random.default_rng(0).uniform(0.5, 1.5, size=(kmax, N))
    fac[0] = 1.
    B = torch.from_numpy(b[None, :]*fac).to(A.A.device)
    out = dict(N=N, noRef=a.noRef, tol=a.tol, maxiter=a.maxiter, rounds=a.rounds, hierarchy_s=t_asm, nrhs={})
    for k in a.nrhs:
        def block():
            return solvers.bicgstab_multi(A, B[:k], tol=a.tol, maxiter=a.maxiter, preconditioner='jacobi')

        def loop():
            return [solvers.bicgstab(A, B[v], tol=a.tol, maxiter=a.maxiter, preconditioner='jacobi') for v in range(k)]
        block(); loop()
        tb, tl = [], []
        for _ in range(a.rounds):
            t, (Xb, ib, rb) = wall(block)
            tb.append(t)
            t, sols = wall(loop)
            tl.append(t)
        tb, tl = statistics.median(tb), statistics.median(tl)
        Xl = torch.stack([x for x, _, _ in sols])
        il = [int(i) for _, i, _ in sols]
        out['nrhs'][k] = dict(block_ms=1e3*tb, loop_ms=1e3*tl, loop_over_block=tl/tb, block_iterations=[int(i) for i in ib], loop_iterations=il,
                              block_ms_per_pass=1e3*tb/max(int(ib.max())+1, 1), loop_ms_per_pass=1e3*tl/max(sum(i+1 for i in il), 1),
                              block_residual_max=float(rb.max()), loop_residual_max=max(float(r[-1]) for _, _, r in sols),
                              max_rel_diff=float((Xb-Xl).abs().max()/Xl.abs().max()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
