"""SHA-256 digests of what the direct solvers (pnl_potrf / pnl_potrs, pnl_getrf / pnl_getrs; csrc/pnl_direct.hip) leave for seeded
inputs: one line per case with the digest of the factor block's bytes (padding columns included), of piv, and of the solutions for
nrhs = 1 and nrhs = 5.  Two builds of the library compute the same thing bit for bit exactly if their outputs are the same text:
    PNL_LIB=<one libpnl_hip.so> python tools/direct_digest.py > a.txt;  PNL_LIB=<the other> python tools/direct_digest.py > b.txt
(one process per library: PNL_LIB is read when the package is imported).

Inputs: the (R) matrices of tests/test_cholesky.py (D (G G^T + n I) D) and tests/test_lu.py (D1 G D2, rows scaled over six
decades), ld = n + 6.  n = 65: a full panel and a panel of one column; 321: a block edge and a narrow last panel; 513: two block-level
updates with K = 256 and a last panel of one column.  nrhs = 5: a full group of four right-hand sides and a remainder.  These are
the smallest sizes that pass through every kernel and both values of K.
usage: direct_digest.py [N ...]   (default 65 321 513)"""
import hashlib
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pynucleus_amd import _lib


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def matrix(kind, n):
    rng = np.random.default_rng([n, int(kind == 'lu')])
    G = rng.standard_normal((n, n))
    d1, d2 = 10.**rng.uniform(-3., 3., size=n), 10.**rng.uniform(-3., 3., size=n)
    if kind == 'lu':
        return G*d1[:, None]*d2[None, :], rng
    A = (G@G.T+n*np.eye(n))*d1[:, None]*d1[None, :]
    return np.tril(A)+np.tril(A, -1).T, rng


def digest(ctx, kind, n):
    ld = n+6
    A, rng = matrix(kind, n)
    host = np.zeros((n, ld))
    host[:, :n] = A
    F = torch.from_numpy(host).cuda()
    piv = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    info = ctx.potrf(F.data_ptr(), ld, n) if kind == 'chol' else ctx.getrf(F.data_ptr(), ld, n, piv.data_ptr())
    ctx.synchronize()
    assert info == 0, (kind, n, info)
    line = '{} n={} ld={} factor={} piv={}'.format(kind, n, ld, sha(F), sha(piv) if kind == 'lu' else '-')
    B = rng.standard_normal((5, n))
    for nrhs in (1, 5):
        X = torch.from_numpy(B[:nrhs].copy()).cuda()
        if kind == 'chol':
            ctx.potrs(F.data_ptr(), ld, n, X.data_ptr(), n, nrhs)
        else:
            ctx.getrs(F.data_ptr(), ld, n, piv.data_ptr(), X.data_ptr(), n, nrhs)
        ctx.synchronize()
        assert bool(torch.isfinite(X).all()), (kind, n, nrhs)
        line += ' x{}={}'.format(nrhs, sha(X))
    print(line, flush=True)


if __name__ == '__main__':
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for n in ([int(a) for a in sys.argv[1:]] or [65, 321, 513]):
        for kind in ('chol', 'lu'):
            digest(ctx, kind, n)
