"""Micro-benchmark of the block multigrid-preconditioned CG against sequential single-vector solves, in one process.

  The `disc` hierarchy whose finest level is the dense operator of bench.py's headline (levels 0 .. --noRef of the uniformly refined
  disc, P1, fractional kernel of order --s, target_order 0.5, zeroExterior; --noRef 7: 48,769 DoFs on the finest level).  For nrhs in
  {1, 2, 4, 8, 16}: multigrid.cg on the 2-D block (pnl_mg_cg_block: per iteration one pnl_gemv_block pass for A P and one block V cycle,
  two more passes over the finest operator) against nrhs calls of multigrid.cg on the rows (pnl_mg_cg: the symmetric half-read product
  where the level is large enough), at the same tol and maxiter.  Right-hand side 0 is the benchmark's (f = 1), the others are f = 1
  times seeded random factors in [0.5, 1.5] per DoF.

Wall-clock seconds of the whole solves (both are synchronous calls) after one warm-up solve of every shape; block and loop alternate,
three rounds, the median is reported, with the iteration counts of both, the time per pass of the loop (a column that reports k
iterations has made k + 1 passes; the block makes as many as its slowest column) and the largest relative difference of the solutions.
Prints one JSON line.
usage: mg_block_probe.py [--noRef R] [--s S] [--tol T] [--maxiter M] [--nrhs K ...]      (defaults: --noRef 7 --s 0.5 --tol 1e-8)"""
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
    ap.add_argument('--maxiter', type=int, default=100)
    ap.add_argument('--nrhs', type=int, nargs='*', default=list(NRHS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'mg_block_probe.py needs a GPU'
    from pynucleus_amd import getFractionalKernel
    from pynucleus_amd.multigrid import fractionalHierarchy, multigrid
    H = fractionalHierarchy('disc', a.noRef, getFractionalKernel(2, a.s), {'target_order': 0.5})
    mg = multigrid(H)
    dm, A = H.finest['DoFMap'], H.finest['A']
    N = A.num_rows
    b = np.asarray(dm.assembleRHS(1.0))
    kmax = max(a.nrhs)
    fac = np.random.default_rng(0).uniform(0.5, 1.5, size=(kmax, N))
    fac[0] = 1.
    B = torch.from_numpy(b[None, :]*fac).to(A.A.device)
    out = dict(N=N, levels=[L['A'].num_rows for L in H.getLevelList()], noRef=a.noRef, s=a.s, tol=a.tol, maxiter=a.maxiter, nrhs={})
    for k in a.nrhs:
        def block():
            return mg.cg(B[:k], tol=a.tol, maxiter=a.maxiter)

        def loop():
            return [mg.cg(B[v], tol=a.tol, maxiter=a.maxiter) for v in range(k)]
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
                              block_ms_per_pass=1e3*tb/max(int(ib.max())+1, 1), loop_ms_per_pass=1e3*tl/max(sum(i+1 for i in il), 1),
                              block_residual_max=float(rb.max()), loop_residual_max=max(float(r[-1]) for _, _, r in sols),
                              max_rel_diff=float((Xb-Xl).abs().max()/Xl.abs().max()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
