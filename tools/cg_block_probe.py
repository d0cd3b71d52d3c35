"""Micro-benchmark of the block Jacobi-CG against sequential single-vector solves, in one process.

  The dense operator of bench.py's headline (disc refined --noRef times, P1, fractional kernel of order --s, target_order 0.5,
  zeroExterior).  For nrhs in {1, 2, 4, 8, 16}: Dense_LinearOperator.solve_cg_jacobi_block (pnl_cg_jacobi_block: one pnl_gemv_block
  pass over the full block per iteration) against nrhs calls of solve_cg_jacobi (pnl_cg_jacobi: the symmetric half-read GEMV per
  iteration and right-hand side), at the same tol and maxiter.  Right-hand side 0 is the benchmark's (f = 1), the others are f = 1
  times seeded random factors in [0.5, 1.5] per DoF.

Wall-clock seconds of the whole solves (both are synchronous calls) after one warm-up solve of every shape; block and loop alternate,
three rounds, the median is reported, with the iteration counts of both, the time per iteration and the largest relative difference of
the solutions.  Prints one JSON line.
usage: cg_block_probe.py [--noRef R] [--s S] [--tol T] [--maxiter M] [--nrhs K ...]      (defaults: --noRef 7 --s 0.5 --tol 1e-8)"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

NRHS = (1, 2, 4, 8, 16)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter()-t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--noRef', type=int, default=7)
    ap.add_argument('--s', type=float, default=0.5)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--maxiter', type=int, default=5000)
    ap.add_argument('--nrhs', type=int, nargs='*', default=list(NRHS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'cg_block_probe.py needs a GPU'
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    dm = P1_DoFMap(disc(a.noRef), PHYSICAL)
    A = nonlocalBuilder(dm, getFractionalKernel(2, a.s), {'target_order': 0.5}, zeroExterior=True).getDense()
    assert A.symmetric
    N = A.num_rows
    b = np.asarray(dm.assembleRHS(1.0))
    kmax = max(a.nrhs)
    fac = np.random.default_rng(0).uniform(0.5, 1.5, size=(kmax, N))
    fac[0] = 1.
    B = torch.from_numpy(b[None, :]*fac).to(A.A.device)
    out = dict(N=N, noRef=a.noRef, s=a.s, tol=a.tol, maxiter=a.maxiter, nrhs={})
    for k in a.nrhs:
        def block():
            return A.solve_cg_jacobi_block(B[:k], tol=a.tol, maxiter=a.maxiter)

        def loop():
            return [A.solve_cg_jacobi(B[v], tol=a.tol, maxiter=a.maxiter) for v in range(k)]
        block(); loop()
        tb, tl = [], []
        for _ in range(3):
            t, (Xb, ib, rb) = wall(block)
            tb.append(t)
            t, sols = wall(loop)
            tl.append(t)
        tb, tl = statistics.median(tb), statistics.median(tl)
        Xl = torch.stack([x for x, _, _ in sols])
        il = [int(i) for _, i, _ in sols]
        out['nrhs'][k] = dict(block_ms=1e3*tb, loop_ms=1e3*tl, loop_over_block=tl/tb, block_iterations=[int(i) for i in ib], loop_iterations=il,
                              block_ms_per_iteration=1e3*tb/max(int(ib.max())+1, 1), loop_ms_per_iteration=1e3*tl/max(sum(i+1 for i in il), 1),
                              block_residual_max=float(rb.max()), loop_residual_max=max(float(r) for _, _, r in sols),
                              max_rel_diff=float((Xb-Xl).abs().max()/Xl.abs().max()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
