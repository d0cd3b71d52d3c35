"""Micro-benchmark of the pivoted direct solver: pnl_getrf, pnl_getrs with one and with eight right-hand sides, against
torch.linalg.lu_factor / lu_solve on the same matrix and against pnl_potrf on a symmetric positive definite matrix of the same size (LU
does twice the flop of Cholesky); HIP events, one process.
usage: lu_probe.py [N ...]   (default 4096 12097 48769)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pynucleus_amd import _lib
from chol_probe import FP64_PEAK, spd, timed


def general(N, ld, g):
    """random matrix with rows scaled over six decades (real pivoting), built block-wise on the device"""
    A = torch.empty((N, ld), dtype=torch.float64, device='cuda')
    for i in range(0, N, 4096):
        m = min(4096, N-i)
        A[i:i+m, :N] = torch.rand((m, N), dtype=torch.float64, device='cuda', generator=g)-0.5
        A[i:i+m, :N] *= 10.**(6.*torch.rand((m, 1), dtype=torch.float64, device='cuda', generator=g)-3.)
    if ld > N:
        A[:, N:] = 0.
    return A


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def probe(ctx, N):
    ld = (N+7) & ~7
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    A = general(N, ld, g)
    F = torch.empty_like(A)
    piv = torch.empty(N, dtype=torch.int32, device='cuda')
    out = {'N': N}
    ms = []
    for rep in range(3 if N < 20000 else 2):
        F.copy_(A)
        t, info = once(lambda: ctx.getrf(F.data_ptr(), ld, N, piv.data_ptr()))
        assert info == 0, info
        ms.append(t)
    out['getrf_ms'] = min(ms)
    out['getrf_frac_of_fp64_peak'] = (2.*N**3/3.)/(1e-3*out['getrf_ms'])/FP64_PEAK
    B = torch.rand((8, N), dtype=torch.float64, device='cuda', generator=g)
    X = B.clone()
    ctx.getrs(F.data_ptr(), ld, N, piv.data_ptr(), X.data_ptr(), N, 8); ctx.synchronize()
    R = (A[:, :N]@X.T).T-B
    out['residual_8rhs'] = float(R.abs().max()/((A[:, :N].abs()@X.abs().T).max()))
    del R
    for nrhs in (1, 8):
        t = timed(lambda: ctx.getrs(F.data_ptr(), ld, N, piv.data_ptr(), X.data_ptr(), N, nrhs), 5)
        out['getrs{}_ms'.format(nrhs)] = t
        out['getrs{}_TBs_on_8n2'.format(nrhs)] = 8.*N*N/(1e-3*t)/1e12
    # Cholesky on a symmetric positive definite matrix of the same size, in the storage of the factors
    del A
    F.copy_(spd(N, ld, g))
    t, info = once(lambda: ctx.potrf(F.data_ptr(), ld, N))
    assert info == 0, info
    out['potrf_ms'] = t
    out['getrf_over_2x_potrf'] = out['getrf_ms']/(2.*t)
    del F, X
    torch.cuda.empty_cache()
    # the yardstick: torch on the same matrix (contiguous copy)
    try:
        g.manual_seed(1)
        At = general(N, N, g)
        LUt, pt = torch.linalg.lu_factor(At)                       # warm-up (library handles, workspace)
        del LUt, pt
        ms = []
        for rep in range(2):
            t, (LUt, pt) = once(lambda: torch.linalg.lu_factor(At))
            ms.append(t)
        out['torch_lu_factor_ms'] = min(ms)
        del At
        Bt = B.T.contiguous()
        for nrhs in (1, 8):
            b = Bt[:, :nrhs].contiguous()
            torch.linalg.lu_solve(LUt, pt, b)
            out['torch_lu_solve{}_ms'.format(nrhs)] = timed(lambda: torch.linalg.lu_solve(LUt, pt, b), 3)
        out['getrf_over_torch'] = out['getrf_ms']/out['torch_lu_factor_ms']
    except Exception as e:                                      # the yardstick may not fit next to the matrix: say so
        out['torch_error'] = repr(e)[:200]
    print(out, flush=True)
    return out


if __name__ == '__main__':
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for N in ([int(a) for a in sys.argv[1:]] or [4096, 12097, 48769]):
        probe(ctx, N)
