"""Micro-benchmark of solvers.lobpcg on the dense operator of bench.py's headline, in one process.

The `disc` hierarchy with mass matrices whose finest level is that operator (levels 0 .. --noRef; --noRef 7: 48,769 DoFs; P1,
fractional kernel of order --s, target_order 0.5, zeroExterior): the --k smallest eigenpairs of A x = theta M x with a block of --m
vectors, once with the Jacobi preconditioner and once with the block V cycle of the hierarchy ('cg-mg').  Beside the solves, the
pieces a pass is made of are timed alone on --m vectors: A.matvec_multi (the yardstick: tools/block_probe.py measures the same
product), M.matvec_multi, one block V cycle, and the vector side of a pass without any product (pnl_eigb_residual, two pnl_eigb_gram
and one pnl_eigb_combine for W, two pnl_eigb_gram on the 3 m rows of the basis, six pnl_eigb_combine).

Wall-clock milliseconds after one warm-up of every shape, the median of --rounds; ms per pass is the whole solve over its passes (the
start -- two products and a Rayleigh-Ritz step -- and the final recomputation are in it).  Prints one JSON line.
usage: eig_probe.py [--tree DIR] [--noRef R] [--s S] [--k K] [--m M] [--tol T] [--maxiter N] [--rounds N]
--tree DIR imports the package from another checkout (default: the one this file is in)."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--noRef', type=int, default=7)
    ap.add_argument('--s', type=float, default=0.5)
    ap.add_argument('--k', type=int, default=6)
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--maxiter', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    assert torch.cuda.is_available(), 'eig_probe.py needs a GPU'
    from pynucleus_amd import getFractionalKernel, solvers
    from pynucleus_amd.multigrid import fractionalHierarchy, multigrid

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return 1e3*(time.perf_counter()-t0), res

    def median_ms(fn):
        fn()
        return statistics.median(wall(fn)[0] for _ in range(a.rounds))

    H = fractionalHierarchy('disc', a.noRef, getFractionalKernel(2, a.s), {'target_order': 0.5}, buildMass=True)
    A, M, mg = H.finest['A'], H.finest['M'], multigrid(H)
    ctx, n, m = A.ctx, A.num_rows, a.m
    dev = A.A.device
    out = dict(N=n, levels=[L['A'].num_rows for L in H.getLevelList()], s=a.s, k=a.k, m=m, tol=a.tol, maxiter=a.maxiter, rounds=a.rounds)
    Mop = solvers._mass_operator(M, ctx, dev, n)
    V = torch.randn((4*m, n), generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    W = torch.empty_like(V)
    out['matvec_multi_ms'] = median_ms(lambda: A.matvec_multi(V[:m]))
    out['mass_matvec_multi_ms'] = median_ms(lambda: Mop.matvec_multi(V[:m]))
    out['cycle_ms'] = median_ms(lambda: mg.cycle(V[:m]))
    small = torch.zeros((4, 48, 48), dtype=torch.float64, device=dev)
    theta = torch.ones(m, dtype=torch.float64, device=dev)
    p = lambda T, b: T.data_ptr()+8*b*m*n                    # noqa: E731

    def vector_side():
        ctx.eigb_residual(n, m, (1 << m)-1, p(V, 1), n, p(V, 2), n, theta.data_ptr(), 0, p(W, 1), n, p(W, 0), n, small[3].data_ptr())
        ctx.eigb_gram(n, m, p(V, 0), n, m, p(V, 1), n, small[0].data_ptr(), 48)
        ctx.eigb_gram(n, m, p(V, 0), n, m, p(V, 0), n, small[1].data_ptr(), 48)
        ctx.eigb_combine(n, 2*m, p(V, 0), n, m, small[2].data_ptr(), 48, p(W, 2), n)
        for _ in range(2):
            ctx.eigb_gram(n, 3*m, p(V, 1), n, 3*m, p(V, 1), n, small[0].data_ptr(), 48)
        for b in range(6):
            ctx.eigb_combine(n, 3*m, p(V, 1), n, m, small[2].data_ptr(), 48, p(W, b % 4), n)
        ctx.synchronize()
    out['vector_side_ms'] = median_ms(vector_side)
    for name, pre in (('jacobi', 'jacobi'), ('cg-mg', mg)):
        solve = lambda: solvers.lobpcg(A, a.k, M=M, tol=a.tol, maxiter=a.maxiter, preconditioner=pre, blockSize=m)     # noqa: E731
        solve()
        runs = [wall(solve) for _ in range(a.rounds)]
        ms = statistics.median(t for t, _ in runs)
        theta_, _, passes, res = runs[-1][1]
        out[name] = {'passes': int(passes), 'solve_ms': ms, 'ms_per_pass': ms/max(int(passes), 1), 'residual_max': float(res.max()),
                     'theta': [float(t) for t in theta_]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
