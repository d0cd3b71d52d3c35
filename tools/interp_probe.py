"""Micro-benchmark of the fused kernels of csrc/pnl_interp.hip on m random N x N blocks: pnl_gemv_multi (m 8 N ld bytes) and pnl_lincomb
((m + 1) 8 N ld bytes) against what the generic path does -- m one-sided pnl_gemv calls and m torch axpys -- and against a single
one-sided pnl_gemv (8 N ld bytes), all in one run, alternating, timed with device events.  usage: interp_probe.py [N] [m ...]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from pynucleus_amd import _lib  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
MS = [int(v) for v in sys.argv[2:]] or [3, 10]
ROUNDS, REPS = 5, 10
ld = (N+7) & ~7
ctx = _lib.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
g = torch.Generator(device='cuda')
g.manual_seed(1)
blocks = []
for k in range(max(MS)):
    A = torch.empty((N, ld), dtype=torch.float64, device='cuda')
    for i in range(0, N, 4096):
        A[i:i+4096] = torch.rand((min(4096, N-i), ld), dtype=torch.float64, device='cuda', generator=g)-0.5
    blocks.append(A)
B = torch.empty((N, ld), dtype=torch.float64, device='cuda')
x = torch.rand(N, dtype=torch.float64, device='cuda', generator=g)
y, t, acc = (torch.empty(N, dtype=torch.float64, device='cuda') for _ in range(3))
torch.cuda.synchronize()


def timed(fn):
    """ms per call over REPS calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)/REPS


for m in MS:
    ptrs = [A.data_ptr() for A in blocks[:m]]
    c = np.cos(np.arange(m)+0.5)

    def fused():
        ctx.gemv_multi(ptrs, ld, N, N, c, x.data_ptr(), 1., 0., None, y.data_ptr())

    def combine():
        ctx.lincomb(ptrs, ld, N, N, c, B.data_ptr(), ld)

    def loop():
        for k in range(m):
            ctx.gemv(ptrs[k], ld, N, x.data_ptr(), t.data_ptr(), 0)
            if k == 0:
                torch.mul(t, float(c[0]), out=acc)
            else:
                acc.add_(t, alpha=float(c[k]))

    def single():
        ctx.gemv(ptrs[0], ld, N, x.data_ptr(), t.data_ptr(), 0)

    cases = [('pnl_gemv_multi', fused, m), ('pnl_lincomb', combine, m+1), ('loop of pnl_gemv + axpy', loop, m), ('single pnl_gemv', single, 1)]
    for _, fn, _ in cases:                         # warm every shape
        fn()
        fn()
    torch.cuda.synchronize()
    diff = float((y-acc).abs().max()/acc.abs().max())
    ms = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):                        # alternate the four, keep every round: the spread is part of the result
        for name, fn, _ in cases:
            ms[name].append(timed(fn))
    print('N = {}, ld = {}, m = {}: fused vs loop max rel diff {:.2e}'.format(N, ld, m, diff))
    for name, _, nblocks in cases:
        v = np.array(ms[name])
        nbytes = nblocks*8.*N*ld
        print('  {:26s} ms min {:8.3f} median {:8.3f} max {:8.3f}   TB/s at median {:6.3f} (best {:6.3f}) on {} x 8 N ld bytes'.format(
            name, v.min(), np.median(v), v.max(), nbytes/np.median(v)/1e9, nbytes/v.min()/1e9, nblocks))
