"""Micro-benchmark of the direct solver: pnl_potrf, pnl_potrs with one and with eight right-hand sides, against torch.linalg.cholesky /
torch.cholesky_solve on the same matrix and against two pnl_gemv products of the upper triangle (symmetric_half = 2) as the HBM
yardstick of one solve; HIP events, one process.  With --heat also the noRef 6 heat run, solver='chol' against the default stepper.
usage: chol_probe.py [--heat] [N ...]   (default 4096 12097 48769)"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from pynucleus_amd import _lib

FP64_PEAK = 78.6e12          # MI355X, matrix fp64 (data sheet); the vector rate is the same


def spd(N, ld, g):
    """random symmetric matrix with a dominant diagonal, built block-wise on the device (lower triangle mirrored)"""
    A = torch.empty((N, ld), dtype=torch.float64, device='cuda')
    for i in range(0, N, 4096):
        A[i:i+4096, :N] = torch.rand((min(4096, N-i), N), dtype=torch.float64, device='cuda', generator=g)-0.5
    for i in range(0, N, 4096):
        for j in range(0, i+1, 4096):
            blk = A[i:i+4096, j:min(j+4096, N)]
            if i == j:
                blk.copy_(torch.tril(blk)+torch.tril(blk, -1).T)
            else:
                A[j:min(j+4096, N), i:i+4096] = blk.T
    A.diagonal().add_(float(N))
    return A


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)/reps


def probe(ctx, N):
    ld = (N+7) & ~7
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    A = spd(N, ld, g)
    F = torch.empty_like(A)
    out = {'N': N}
    ms = []
    for rep in range(3 if N < 20000 else 2):
        F.copy_(A)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        info = ctx.potrf(F.data_ptr(), ld, N)
        e1.record()
        torch.cuda.synchronize()
        assert info == 0, info
        ms.append(e0.elapsed_time(e1))
    out['potrf_ms'] = min(ms)
    out['potrf_frac_of_fp64_peak'] = (N**3/3.)/(1e-3*out['potrf_ms'])/FP64_PEAK
    B = torch.rand((8, N), dtype=torch.float64, device='cuda', generator=g)
    X = B.clone()
    ctx.potrs(F.data_ptr(), ld, N, X.data_ptr(), N, 8); ctx.synchronize()
    R = (A[:, :N]@X.T).T-B
    out['residual_8rhs'] = float(R.abs().max()/B.abs().max())
    del R
    for nrhs in (1, 8):
        t = timed(lambda: ctx.potrs(F.data_ptr(), ld, N, X.data_ptr(), N, nrhs), 5)
        out['potrs{}_ms'.format(nrhs)] = t
        out['potrs{}_TBs_on_8n2'.format(nrhs)] = 8.*N*N/(1e-3*t)/1e12
    x, y = B[0].contiguous(), torch.empty(N, dtype=torch.float64, device='cuda')
    ctx.gemv(A.data_ptr(), ld, N, x.data_ptr(), y.data_ptr(), 2); ctx.synchronize()
    out['two_gemv2_ms'] = 2.*timed(lambda: ctx.gemv(A.data_ptr(), ld, N, x.data_ptr(), y.data_ptr(), 2), 10)
    out['potrs1_over_two_gemv2'] = out['potrs1_ms']/out['two_gemv2_ms']
    del F, X
    torch.cuda.empty_cache()
    # the yardstick: torch on the same matrix (contiguous copy)
    try:
        At = A[:, :N].contiguous()
        del A
        torch.cuda.empty_cache()
        Lt = torch.linalg.cholesky(At)                          # warm-up (library handles, workspace)
        ms = []
        for rep in range(2):
            ms.append(timed(lambda: torch.linalg.cholesky(At, out=Lt), 1))
        out['torch_cholesky_ms'] = min(ms)
        del At
        Bt = B.T.contiguous()
        for nrhs in (1, 8):
            b = Bt[:, :nrhs].contiguous()
            torch.cholesky_solve(b, Lt)
            out['torch_cholesky_solve{}_ms'.format(nrhs)] = timed(lambda: torch.cholesky_solve(b, Lt), 3)
        out['potrf_over_torch'] = out['potrf_ms']/out['torch_cholesky_ms']
    except Exception as e:                                      # the yardstick may not fit next to the matrix: say so
        out['torch_error'] = repr(e)[:200]
    print(out, flush=True)
    return out


def heat():
    from pynucleus_amd import getFractionalKernel
    from pynucleus_amd.multigrid import fractionalHierarchy, solveFractionalHeat
    s = 0.25
    H = fractionalHierarchy('interval', 6, getFractionalKernel(1, s), {'target_order': 2.-s}, buildMass=True)
    dm = H.finest['DoFMap']
    from pynucleus_amd.quadrature import simplexXiaoGimbutas
    qr = simplexXiaoGimbutas(3, 1, 1)
    f = np.asarray(dm.assembleRHS(lambda x: 1., qr))
    out = {}
    for solver in ('cg-mg', 'chol', 'cg-mg', 'chol'):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        solveFractionalHeat(H, lambda x: 0., lambda t: np.cos(t)*f, finalTime=1.0, tol=1e-10, solver=solver)
        torch.cuda.synchronize(); out[solver] = 1e3*(time.perf_counter()-t0)
    print({'heat_noRef6_ms': out}, flush=True)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--heat']
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for N in ([int(a) for a in args] or [4096, 12097, 48769]):
        probe(ctx, N)
    if '--heat' in sys.argv:
        heat()
