"""The apply kernels (GEMV, two-sided GEMV, slab, SpMV, CG) through the C ABI on SYNTHETIC matrices built in numpy: no assembled
operator is involved; a context gets a mesh and a DoF map only where an entry point needs to know N.

Two kinds of check.

(E) exact.  Entries of A, x, b are integers in [-1024, 1024], alpha / beta in {1, -1, 2, 0.5, 0}; the strict lower triangle of the
    square matrices holds integers in [2^20, 2^21] (a leaked entry cannot cancel) and the matrices are NOT symmetric.  With
    n <= 2^14 every partial sum, in any order, fused or not, is an integer (a multiple of 1/2 after alpha / beta) below
    2^14 * 2^21 * 2^10 * 2 = 2^46 < 2^53: fp64 arithmetic is exact, the result does not depend on the summation order or on the
    order of the fp64 atomics.  The reference is an int64 numpy product, the assertion is bit equality.  Padding columns (ld > n)
    and the elements before / after every vector view hold 2^30: a read or write past an edge changes a sum / a guard.  One-hot
    vectors e_k at the block edges give single columns of the operator, so that a failure names the entry.
(R) rounding.  Entries standard_normal * 10^uniform(-6, 6); reference in np.longdouble where it has >= 63 mantissa bits, else
    mpmath on a seeded subset of >= 64 rows that holds every block edge.  A sum of m products in any order with one rounding
    per operation has |err_i| <= gamma_m sum_j |a_ij| |x_j|, gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, 3.1); with the scaling by alpha and the beta b term
        tol_i = (m + 4) u (|alpha| (|A_op| |x|)_i + |beta| |b_i|),
    m = the number of products that enter component i.  No other tolerance is used for a matvec.

Contracts as the code and include/pnl_hip.h state them ("Contracts of the apply kernels"):
  pnl_gemv mode 0   y = A x on the full matrix.
  pnl_gemv mode 1   y = A x + A^T x on the full matrix, literally (A + A^T) x: the diagonal counts TWICE (k_gemv takes every entry
                    of the row, k_gemv_t_add every entry of the column); one-sided PNL_FLAG_NO_MIRROR storage holds half of the
                    diagonal for that reason.  m = 2 n.
  pnl_gemv mode 2   y = triu(A) x + triu(A, 1)^T x: the upper triangle only, the diagonal once, nothing below it.
  pnl_slab_matvec   y = 0; y[rowdofs] += S x[coldofs]; y[coldofs] += M^T x[rowdofs], M = S without the entries whose row and
                    column DoF coincide.  With dblocks = NULL the entry point needs a context with a mesh, a DoF map (N) and
                    pnl_set_row_slab; nothing is assembled (no tile-order job exists before the first finalize).
  pnl_slab_diagonal diag = 0; diag[rowdofs[r]] = S[r, c] where coldofs[c] == rowdofs[r].
  pnl_gemv_axpby    y = alpha A x + beta b (b may be y; b may be NULL with beta = 0).
  pnl_csr_matvec    y = alpha A x + beta y; one thread walks a row, the column indices need NOT be sorted.
  pnl_spmv          CSR (diag NULL): y = A x.  SSS (diag given, data = strict lower triangle): y = (L + L^T + D) x.  The pattern
                    comes from pnl_upload_sparsity, which demands strictly increasing columns per row -- sorted for both.
  pnl_inv_diagonal  1 / a_ii: the build has no fast-math flag (csrc/Makefile: -O3 -munsafe-fp-atomics only, which concerns
                    atomics), so the fp64 division is IEEE-correct and must equal numpy's 1.0 / a bit for bit.
  pnl_cg_jacobi     Jacobi-preconditioned CG on the symmetrised upper triangle; stops on sqrt(r . D^-1 r) <= tol; the residual
                    is recomputed from b - A x when the counter k reaches 50 (iterations 50, 99, 148, ... counted from 0).
"""
import math
import time
from fractions import Fraction

import mpmath
import numpy as np
import pytest

gpu = pytest.mark.gpu

U = 2.**-53
LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
POISON = 2**30
LOW_LO, LOW_HI = 2**20, 2**21                  # the strict lower triangle of the (E) matrices
EDGES = (63, 64, 1023, 1024, 4095, 4096)      # one-hot positions (and n - 1)
GEMV_SIZES = (1, 2, 63, 64, 65, 127, 129, 511, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 2111, 2112, 2113, 4095, 4096,
              4097, 4159, 4160, 4161, 8191, 8193, 8257)
GEMV_R_SIZES = (1, 65, 1025, 1089, 2113, 4097, 4161, 8257)
FULL_LAYOUT_SIZES = (65, 1089, 2113, 4161)
# (ld - n, offset of the matrix base in doubles, offset of the x view in doubles)
LAYOUTS = [(dl, ao, xo) for dl in (0, 1, 6) for ao in (0, 1) for xo in (0, 1)]
MISALIGNED = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (6, 1, 0), (6, 0, 1)]
AXPBY_SHAPES = ((1, 1), (3, 257), (257, 3), (64, 511), (65, 513), (300, 1025), (1025, 2049))
ROW_LENGTHS = (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 449, 1100)
SLAB_N = 8399


# ---- expected values and tolerances (plain numpy; tested below without a GPU) -------------------------------------------------

def exact_matrix(rng, n):
    """non-symmetric integer matrix: [-1024, 1024] on and above the diagonal, [2^20, 2^21] strictly below it"""
    A = rng.integers(-1024, 1025, size=(n, n), dtype=np.int64)
    low = np.tri(n, n, -1, dtype=bool)
    A[low] = rng.integers(LOW_LO, LOW_HI+1, size=int(low.sum()), dtype=np.int64)
    return A


def exact_vector(rng, n):
    x = rng.integers(-1024, 1025, size=n, dtype=np.int64)
    x[x == 0] = 1                              # every entry of the operator takes part
    return x


def rtype(rng, shape):
    return rng.standard_normal(shape)*10.**rng.uniform(-6., 6., size=shape)


def expected_mode2(A, x):
    """triu(A) x + triu(A, 1)^T x"""
    Up = np.triu(A)
    return Up@x+x@Up-np.diagonal(A)*x


def column_mode2(A, k):
    """column k of the mode-2 operator (= its row k): A[:k, k] above the diagonal, A[k, k:] from it on"""
    return np.concatenate([A[:k, k], A[k, k:]])


def expected_slab(S, rowdofs, coldofs, x, N):
    """y[rowdofs] += S x[coldofs]; y[coldofs] += M^T x[rowdofs], M = S where rowdofs[r] != coldofs[c], else 0"""
    y = np.zeros((N,)+x.shape[1:], dtype=np.result_type(S, x))
    y[rowdofs] += S@x[coldofs]
    M = np.where(np.asarray(rowdofs)[:, None] != np.asarray(coldofs)[None, :], S, 0)
    y[coldofs] += M.T@x[rowdofs]
    return y


def expected_slab_diagonal(S, rowdofs, coldofs, N):
    d = np.zeros(N, dtype=S.dtype)
    r, c = np.nonzero(np.asarray(rowdofs)[:, None] == np.asarray(coldofs)[None, :])
    d[np.asarray(rowdofs)[r]] = S[r, c]
    return d


def csr_dense(indptr, indices, data, ncols):
    D = np.zeros((len(indptr)-1, ncols), dtype=data.dtype)
    for i in range(len(indptr)-1):
        D[i, indices[indptr[i]:indptr[i+1]]] = data[indptr[i]:indptr[i+1]]
    return D


def expected_sss(indptr, indices, data, diag, x):
    """(L + L^T + D) x for the strict lower triangle L in CSR"""
    Lo = csr_dense(indptr, indices, data, len(diag))
    return Lo@x+Lo.T@x+(diag*x.T).T


def gamma_tol(m, mag, alpha=1., beta=0., b=0.):
    """(m + 4) u (|alpha| mag + |beta| |b|), mag = sum |a| |x| over the m products of the component"""
    return (m+4)*U*(abs(alpha)*mag+abs(beta)*abs(b))


def hp(v):
    return LD(v) if LD_OK else mpmath.mpf(float(v))


def hp_fraction(v):
    """the high-precision number as an exact rational"""
    if LD_OK:
        hi = float(v)
        return Fraction(hi)+Fraction(float(v-LD(hi)))
    return Fraction(int(v.man)*(-1 if v < 0 else 1))*Fraction(2)**int(v.exp)


def hp_dot(a, b):
    """(sum a_j b_j, sum |a_j| |b_j|) in the high-precision arithmetic"""
    if LD_OK:
        p = np.asarray(a, dtype=LD)*np.asarray(b, dtype=LD)
        return p.sum(), np.abs(p).sum()
    aa, bb = [mpmath.mpf(float(v)) for v in a], [mpmath.mpf(float(v)) for v in b]
    return mpmath.fdot(aa, bb), mpmath.fdot([abs(v) for v in aa], [abs(v) for v in bb])


def hp_rows(n, seed=0):
    """all rows with longdouble; with mpmath a seeded subset of >= 64 rows (or all of them) that holds every block edge"""
    if LD_OK:
        return list(range(n))
    rows = {k+d for k in EDGES+(0, n-1) for d in (-1, 0, 1) if 0 <= k+d < n}
    rows |= set(int(i) for i in np.random.default_rng(seed+n).choice(n, size=min(n, 64), replace=False))
    return sorted(rows)


def layouts_for(n, index):
    """all twelve at FULL_LAYOUT_SIZES; elsewhere ld = n, one misaligned variant and, for odd n, ld = n + 1 on an aligned base: the
    16-byte paths (the plain strips of k_gemv_two_sided among them) need an even leading dimension, which ld = n is not"""
    return LAYOUTS if n in FULL_LAYOUT_SIZES else few_layouts(n, index)


def few_layouts(n, index):
    out = [(0, 0, 0), MISALIGNED[index % len(MISALIGNED)]]
    return out+[(1, 0, 0)] if n % 2 and (1, 0, 0) not in out else out


def hot_positions(n, extra=()):
    return sorted({k for k in EDGES+(n-1,)+tuple(extra) if 0 <= k < n})


def sparse_pattern(rng, N, ncols, strict_lower, sort):
    """CSR pattern with the row lengths ROW_LENGTHS shuffled over rows of their own, short rows elsewhere, an empty first and last
    row; strict_lower: columns < row (the long rows then sit below row 1100)"""
    lens = np.minimum(rng.integers(0, 4, size=N), np.arange(N) if strict_lower else ncols)
    special = rng.choice(np.arange(max(ROW_LENGTHS)+1 if strict_lower else 1, N-1), size=len(ROW_LENGTHS), replace=False)
    lens[special] = rng.permutation(ROW_LENGTHS)
    lens[0] = lens[N-1] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.zeros(indptr[-1], dtype=np.int32)
    for i in range(N):
        cols = rng.choice(i if strict_lower else ncols, size=lens[i], replace=False)
        indices[indptr[i]:indptr[i+1]] = np.sort(cols) if sort else cols
    return indptr, indices, special


# ---- CPU-only: the references themselves ---------------------------------------------------------------------------------------

def test_expected_mode2_against_loops_and_not_A_times_x():
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 20):
        A, x = exact_matrix(rng, n), exact_vector(rng, n)
        y = [0]*n
        for i in range(n):
            for j in range(n):
                if j >= i:
                    y[i] += int(A[i, j])*int(x[j])
                if j > i:
                    y[j] += int(A[i, j])*int(x[i])
        assert [int(v) for v in expected_mode2(A, x)] == y
        for k in range(n):
            e = np.zeros(n, dtype=np.int64); e[k] = 1
            assert np.array_equal(column_mode2(A, k), expected_mode2(A, e))
        if n > 1:
            # the structural test cannot degenerate: on this data the contract differs from A x and from (A + A^T) x, and a
            # single leaked entry of the lower triangle outweighs everything above the diagonal
            assert not np.array_equal(expected_mode2(A, x), A@x)
            assert not np.array_equal(expected_mode2(A, x), A@x+A.T@x)
            assert not np.array_equal(A, A.T)
            assert A[np.tri(n, n, -1, dtype=bool)].min() >= LOW_LO
    Af = rtype(rng, (9, 9)); xf = rtype(rng, 9)
    S = np.triu(Af)+np.triu(Af, 1).T
    assert np.allclose(expected_mode2(Af, xf), S@xf, rtol=1e-12, atol=0.)


def test_expected_slab_against_loops():
    rng = np.random.default_rng(1)
    N = 40
    for rowdofs, coldofs in (([3, 4, 5, 6], list(range(2, 30))), ([1, 3, 5], [0, 2, 4, 6]), ([30, 31], [0, 1, 2]),
                             ([2, 9, 17, 18], [1, 2, 3, 9, 18, 30])):
        S = rng.integers(-9, 10, size=(len(rowdofs), len(coldofs))).astype(np.int64)
        x = rng.integers(-9, 10, size=N).astype(np.int64)
        y, d = [0]*N, [0]*N
        for r, I in enumerate(rowdofs):
            for c, J in enumerate(coldofs):
                y[I] += int(S[r, c])*int(x[J])
                if I != J:
                    y[J] += int(S[r, c])*int(x[I])
                else:
                    d[I] = int(S[r, c])
        assert [int(v) for v in expected_slab(S, rowdofs, coldofs, x, N)] == y
        assert [int(v) for v in expected_slab_diagonal(S, rowdofs, coldofs, N)] == d


def test_expected_sss_against_loops():
    rng = np.random.default_rng(2)
    N = 30
    lens = np.minimum(rng.integers(0, 6, size=N), np.arange(N))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(i, size=lens[i], replace=False)) for i in range(N)]).astype(np.int32)
    data = rng.integers(-9, 10, size=indptr[-1]).astype(np.int64)
    diag, x = rng.integers(-9, 10, size=N).astype(np.int64), rng.integers(-9, 10, size=N).astype(np.int64)
    y = [int(diag[i])*int(x[i]) for i in range(N)]
    for i in range(N):
        for t in range(indptr[i], indptr[i+1]):
            J = indices[t]
            assert J < i
            y[i] += int(data[t])*int(x[J])
            y[J] += int(data[t])*int(x[i])
    assert [int(v) for v in expected_sss(indptr, indices, data, diag, x)] == y


def test_sparse_pattern_has_every_row_length():
    for strict_lower in (False, True):
        indptr, indices, special = sparse_pattern(np.random.default_rng(3), 1400, 1400, strict_lower, True)
        lens = np.diff(indptr)
        assert sorted(lens[special]) == sorted(ROW_LENGTHS) and lens[0] == 0 and lens[-1] == 0
        for i in range(1400):
            row = indices[indptr[i]:indptr[i+1]]
            assert np.all(np.diff(row) > 0) and (not strict_lower or len(row) == 0 or row.max() < i)


def test_gamma_tolerance_holds_for_fp64_in_any_order_and_not_for_fp32():
    """the bound of (R) against exact rational arithmetic: forward, backward, pairwise and four-chain fp64 sums stay inside it, a
    sum with an fp32 accumulator does not"""
    rng = np.random.default_rng(4)
    worst = 0.
    for m in (1, 2, 65, 1000):
        a, x = rtype(rng, m), rtype(rng, m)
        exact = sum(Fraction(float(u))*Fraction(float(v)) for u, v in zip(a, x))
        mag = sum(abs(Fraction(float(u))*Fraction(float(v))) for u, v in zip(a, x))
        tol = Fraction(gamma_tol(m, 1.))*mag
        ref, refmag = hp_dot(a, x)
        assert abs(hp_fraction(ref)-exact) <= tol/64 and abs(hp_fraction(refmag)-mag) <= tol/64
        p = a*x
        fwd = 0.
        for v in p:
            fwd += v
        bwd = 0.
        for v in p[::-1]:
            bwd += v
        chains = sum(float(np.sum(p[k::4])) for k in range(4))
        for s in (fwd, bwd, float(np.sum(p)), chains):
            assert abs(Fraction(s)-exact) <= tol
            worst = max(worst, float(abs(Fraction(s)-exact)/tol)) if tol else worst
        if m >= 65:
            s32 = np.float32(0.)
            for v in p:
                s32 = np.float32(s32+np.float32(v))
            assert abs(Fraction(float(s32))-exact) > tol
    assert gamma_tol(10, 2., alpha=-3., beta=0.5, b=-8.) == 14*U*(6.+4.)
    assert worst <= 1.


def test_exact_data_stays_below_2_53():
    n = max(GEMV_SIZES)
    assert n <= 2**14
    rng = np.random.default_rng(5)
    A, x = exact_matrix(rng, 200), exact_vector(rng, 200)
    assert np.abs(A).max() <= LOW_HI and np.abs(np.triu(A)).max() <= 1024 and np.abs(x).max() <= 1024 and np.abs(x).min() >= 1
    worst_mode0 = n*LOW_HI*1024                # every partial sum of a row of the full matrix
    worst_mode1 = 2*worst_mode0                # A x + A^T x
    worst_scaled = 2*worst_mode1+2*POISON      # |alpha|, |beta| <= 2
    assert worst_mode0 <= 2**45 and worst_mode1 <= 2**46 and worst_scaled < 2**53
    # alpha, beta in {1, -1, 2, 0.5, 0}: the results are multiples of 1/2 and still exact
    assert float(2*worst_scaled+1)/2. == worst_scaled+0.5


def test_layout_lists():
    assert len(LAYOUTS) == 12 and all(v in LAYOUTS for v in MISALIGNED) and (0, 0, 0) not in MISALIGNED
    assert set(GEMV_R_SIZES) <= set(GEMV_SIZES) and {2113, 4161, 8257} <= set(GEMV_R_SIZES)
    assert set(FULL_LAYOUT_SIZES) <= set(GEMV_SIZES) and len(GEMV_SIZES) == 29
    for i, n in enumerate(GEMV_SIZES):
        ls = layouts_for(n, i)
        assert (0, 0, 0) in ls and any(v in MISALIGNED for v in ls)
        # a layout on which 16-byte loads are legal in every row: even ld, aligned base and x
        assert any((n+dl) % 2 == 0 and ao == 0 and xo == 0 for dl, ao, xo in ls) or n == 1


# ---- device plumbing ------------------------------------------------------------------------------------------------------------

def _context():
    import torch
    from pynucleus_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream(0).cuda_stream)
    return ctx


def _context_with_dofs(N):
    """a context that knows N: interval mesh with N + 1 cells and its P1 DoF map; nothing else is uploaded"""
    from pynucleus_amd import _lib, PHYSICAL, P1_DoFMap
    from pynucleus_amd.mesh import simpleInterval
    from pynucleus_amd.local_matrix import dof_permutation_table
    mesh = simpleInterval(0., 1., N+1)
    dm = P1_DoFMap(mesh, PHYSICAL)
    assert dm.num_dofs == N
    ctx = _context()
    keep = [_lib._hp(mesh.vertices, np.float64), _lib._hp(mesh.cells, np.int32), _lib._hp(mesh.volVector, np.float64),
            _lib._hp(mesh.hVector, np.float64), _lib._hp(dm.dofs, np.int32), _lib._hp(dof_permutation_table(dm), np.int32)]
    p = [k[1] for k in keep]
    ctx.check(ctx.L.pnl_upload_mesh(ctx.h, 1, mesh.num_vertices, p[0], mesh.num_cells, p[1], p[2], p[3], 1./math.sqrt(8.)))
    ctx.check(ctx.L.pnl_upload_dofmap(ctx.h, dm.dofs_per_element, dm.dofs_per_vertex, dm.dofs_per_edge, N, p[4], p[5]))
    return ctx


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_matrix(core_d, ld, off):
    """(storage, view): the nrows x ncols device matrix core_d inside a poisoned allocation, leading dimension ld, base offset off"""
    import torch
    nr, nc = core_d.shape
    store = torch.full((off+nr*ld+1,), float(POISON), dtype=torch.float64, device='cuda')
    view = store[off:off+nr*ld].view(nr, ld)
    view[:, :nc] = core_d
    return store, view


def _dev_vector(v, off, dtype=np.float64):
    """(storage, view): v at offset off of an allocation with one poisoned element after it (and before it for off = 1)"""
    import torch
    v = np.ascontiguousarray(v, dtype=dtype)
    host = np.full(v.shape[0]+2, POISON, dtype=dtype)
    host[off:off+v.shape[0]] = v
    store = torch.from_numpy(host).cuda()
    return store, store[off:off+v.shape[0]]


def _result(ctx, ys, yv, off):
    """the output view as numpy; the elements around it must still hold the poison"""
    ctx.synchronize()
    h = ys.cpu().numpy()
    n = yv.shape[0]
    assert h[off+n] == POISON and (off == 0 or h[off-1] == POISON), 'write outside the output vector'
    return h[off:off+n].copy()


def _assert_exact(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    if not np.array_equal(got, ref):
        bad = np.nonzero(got != ref)[0]
        raise AssertionError('{}: {} of {} components differ, first at {}: got {!r}, expected {!r}'.format(
            what, bad.size, ref.size, bad[:8].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist()))


def _assert_rounding(got, rows, ref, tol, what):
    for i, r, t in zip(rows, ref, tol):
        err = abs(hp(got[i])-r)
        assert err <= t, '{}: component {}: got {!r}, reference {!r}, error {:.3e} > tol {:.3e}'.format(
            what, i, got[i], float(r), float(err), float(t))


def _gemv(ctx, Av, n, xv, mode, yoff):
    ys, yv = _dev_vector(np.full(n, POISON), yoff)
    ctx.gemv(Av.data_ptr(), Av.stride(0) if n > 1 else Av.shape[1], n, xv.data_ptr(), yv.data_ptr(), mode)
    return _result(ctx, ys, yv, yoff)


# ---- pnl_gemv modes 0, 1, 2 ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', GEMV_SIZES)
def test_gemv_exact(n):
    """(E) for k_gemv (+ k_gemv_t_add) and k_gemv_two_sided<false>: random integer x and one-hot x at the block edges, every layout
    of layouts_for(n).  Mode 2 must equal triu(A) x + triu(A, 1)^T x although the lower triangle holds 2^20 .. 2^21."""
    import torch
    ctx = _context()
    rng = np.random.default_rng(1000+n)
    A, x = exact_matrix(rng, n), exact_vector(rng, n)
    Ax, xA = A@x, x@A
    ref = {0: Ax, 1: Ax+xA, 2: expected_mode2(A, x)}
    hot = hot_positions(n)
    col = {0: lambda k: A[:, k], 1: lambda k: A[:, k]+A[k, :], 2: lambda k: column_mode2(A, k)}
    core = _dev(A.astype(np.float64))
    for dl, ao, xo in layouts_for(n, GEMV_SIZES.index(n)):
        store, Av = _dev_matrix(core, n+dl, ao)
        xs, xv = _dev_vector(x, xo)
        for mode in (0, 1, 2):
            tag = 'n={} mode={} ld=n+{} A offset {} x offset {}'.format(n, mode, dl, ao, xo)
            _assert_exact(_gemv(ctx, Av, n, xv, mode, xo), ref[mode], tag)
            for k in hot:
                e = np.zeros(n); e[k] = 1.
                es, ev = _dev_vector(e, xo)
                _assert_exact(_gemv(ctx, Av, n, ev, mode, xo), col[mode](k), tag+' x=e_{} (component i = entry (i, {}))'.format(k, k))
        del store, Av
    del core
    ctx.close()
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize('n', GEMV_R_SIZES)
def test_gemv_rounding(n):
    """(R) for the three modes, the two or three layouts of few_layouts: per component within (m + 4) u (|A_op| |x|)_i, m = n
    (modes 0, 2) or 2 n (mode 1: A x and A^T x are 2 n products)"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(2000+n)
    A, x = rtype(rng, (n, n)), rtype(rng, n)
    At = np.ascontiguousarray(A.T)
    rows = hp_rows(n)
    terms = {0: lambda i: (A[i], x), 1: lambda i: (np.concatenate([A[i], At[i]]), np.concatenate([x, x])),
             2: lambda i: (np.concatenate([At[i, :i], A[i, i:]]), x)}
    refs = {}
    for mode in (0, 1, 2):
        rt = [hp_dot(*terms[mode](i)) for i in rows]
        refs[mode] = ([r for r, _ in rt], [gamma_tol(2*n if mode == 1 else n, mag) for _, mag in rt])
    core = _dev(A)
    for dl, ao, xo in few_layouts(n, GEMV_R_SIZES.index(n)):
        store, Av = _dev_matrix(core, n+dl, ao)
        xs, xv = _dev_vector(x, xo)
        for mode in (0, 1, 2):
            got = _gemv(ctx, Av, n, xv, mode, xo)
            _assert_rounding(got, rows, refs[mode][0], refs[mode][1], 'n={} mode={} ld=n+{} A offset {} x offset {}'.format(n, mode, dl, ao, xo))
        del store, Av
    del core
    ctx.close()
    torch.cuda.empty_cache()


# ---- pnl_gemv_axpby -------------------------------------------------------------------------------------------------------------

# (alpha, beta, b): b = None (null pointer, beta = 0), 'b' (distinct from y), 'y' (aliased to y)
AXPBY_COEFFS = ((1., 0., None), (-1., 1., 'b'), (2., -1., 'y'), (0.5, 0.5, 'b'), (0., 2., 'y'), (-1., 0., 'b'), (0.5, 1., 'y'))


def _axpby(ctx, Av, ld, nr, nc, xv, alpha, beta, bkind, b, yoff):
    bs, bv = _dev_vector(b, 1-yoff)
    ys, yv = _dev_vector(b if bkind == 'y' else np.full(nr, POISON), yoff)
    bp = 0 if bkind is None else (yv.data_ptr() if bkind == 'y' else bv.data_ptr())
    ctx.gemv_axpby(Av.data_ptr(), ld, nr, nc, xv.data_ptr(), alpha, beta, bp, yv.data_ptr())
    return _result(ctx, ys, yv, yoff)


@gpu
@pytest.mark.parametrize('shape', AXPBY_SHAPES)
def test_gemv_axpby_exact(shape):
    """(E) for k_gemv_axpby: all twelve layouts, null / distinct / aliased b, alpha and beta from {1, -1, 2, 0.5, 0} (products with
    0.5 are multiples of 1/2: still exact), one-hot x at the column edges"""
    nr, nc = shape
    ctx = _context()
    rng = np.random.default_rng(3000+nr+nc)
    A = rng.integers(-1024, 1025, size=(nr, nc), dtype=np.int64)
    x, b = exact_vector(rng, nc), exact_vector(rng, nr)
    core = _dev(A.astype(np.float64))
    for dl, ao, xo in LAYOUTS:
        store, Av = _dev_matrix(core, nc+dl, ao)
        xs, xv = _dev_vector(x, xo)
        for alpha, beta, bkind in AXPBY_COEFFS:
            tag = '{}x{} ld=ncols+{} A offset {} x offset {} alpha={} beta={} b={}'.format(nr, nc, dl, ao, xo, alpha, beta, bkind)
            ref = alpha*(A@x).astype(np.float64)+beta*b.astype(np.float64)
            _assert_exact(_axpby(ctx, Av, nc+dl, nr, nc, xv, alpha, beta, bkind, b, xo), ref, tag)
        for k in hot_positions(nc, (nc//2, 127, 128, 511, 512)):
            e = np.zeros(nc); e[k] = 1.
            es, ev = _dev_vector(e, xo)
            _assert_exact(_axpby(ctx, Av, nc+dl, nr, nc, ev, -1., 1., 'b', b, xo), b-A[:, k],
                          '{}x{} ld=ncols+{} A offset {} x offset {} x=e_{}'.format(nr, nc, dl, ao, xo, k))
    ctx.close()


@gpu
@pytest.mark.parametrize('shape', ((3, 257), (65, 513), (1025, 2049)))
def test_gemv_axpby_rounding(shape):
    """(R): |y_i - ref_i| <= (ncols + 4) u (|alpha| (|A| |x|)_i + |beta| |b_i|)"""
    nr, nc = shape
    ctx = _context()
    rng = np.random.default_rng(3500+nr+nc)
    A, x, b = rtype(rng, (nr, nc)), rtype(rng, nc), rtype(rng, nr)
    rows = hp_rows(nr)
    rt = [hp_dot(A[i], x) for i in rows]
    core = _dev(A)
    for dl, ao, xo in ((0, 0, 0), (1, 1, 0), (6, 0, 1)):
        store, Av = _dev_matrix(core, nc+dl, ao)
        xs, xv = _dev_vector(x, xo)
        for alpha, beta, bkind in ((1., 0., None), (-1., 1., 'b'), (0.5, -1., 'y'), (2., 0.5, 'b')):
            got = _axpby(ctx, Av, nc+dl, nr, nc, xv, alpha, beta, bkind, b, xo)
            ref = [hp(alpha)*r+hp(beta)*hp(b[i]) for i, (r, _) in zip(rows, rt)]
            tol = [gamma_tol(nc, mag, alpha, beta, b[i]) for i, (_, mag) in zip(rows, rt)]
            _assert_rounding(got, rows, ref, tol, '{}x{} ld=ncols+{} A offset {} x offset {} alpha={} beta={} b={}'.format(
                nr, nc, dl, ao, xo, alpha, beta, bkind))
    ctx.close()


# ---- pnl_csr_matvec, pnl_spmv -------------------------------------------------------------------------------------------------

def _sparse_case(seed, N, ncols, strict_lower, sort, exact):
    rng = np.random.default_rng(seed)
    indptr, indices, special = sparse_pattern(rng, N, ncols, strict_lower, sort)
    nnz = int(indptr[-1])
    if exact:
        data, x = exact_vector(rng, nnz), exact_vector(rng, ncols)
        y0, diag = exact_vector(rng, N), exact_vector(rng, N)
    else:
        data, x, y0, diag = rtype(rng, nnz), rtype(rng, ncols), rtype(rng, N), rtype(rng, N)
    return indptr, indices, special, data, x, y0, diag


def _hot_matrix(n, ks, dtype):
    X = np.zeros((n, len(ks)), dtype=dtype)
    X[ks, np.arange(len(ks))] = 1
    return X


@gpu
def test_csr_matvec_exact_and_rounding():
    """k_csr_axpby, y = alpha A x + beta y: rows of 0 .. 1100 entries, empty first and last row, UNSORTED columns (one thread walks
    a row: no order is needed), views at offset 1.  (E) for every alpha / beta pair and one-hot x; (R) with m = the row length."""
    ctx = _context()
    N, ncols = 1400, 1300
    indptr, indices, special, data, x, y0, _ = _sparse_case(4000, N, ncols, False, False, True)
    assert any(np.any(np.diff(indices[indptr[i]:indptr[i+1]]) < 0) for i in special)
    D = csr_dense(indptr, indices, data, ncols)
    ips, ipv = _dev_vector(indptr, 1, np.int32)
    ixs, ixv = _dev_vector(indices, 1, np.int32)
    ds, dv = _dev_vector(data, 1)

    def run(xh, alpha, beta, y0h, off):
        xs, xv = _dev_vector(xh, off)
        ys, yv = _dev_vector(y0h, 1-off)
        ctx.csr_matvec(N, ipv.data_ptr(), ixv.data_ptr(), dv.data_ptr(), xv.data_ptr(), alpha, beta, yv.data_ptr())
        return _result(ctx, ys, yv, 1-off)
    for off in (0, 1):
        for alpha in (1., -1., 2., 0.5, 0.):
            for beta in (1., -1., 2., 0.5, 0.):
                ref = alpha*(D@x).astype(np.float64)+beta*y0.astype(np.float64)
                _assert_exact(run(x, alpha, beta, y0, off), ref, 'csr alpha={} beta={} x offset {}'.format(alpha, beta, off))
        for k in hot_positions(ncols, (0, 191, 192, 255, 256)):
            e = np.zeros(ncols); e[k] = 1.
            _assert_exact(run(e, 1., 0., y0, off), D[:, k], 'csr x=e_{} x offset {}'.format(k, off))
    indptr, indices, special, data, x, y0, _ = _sparse_case(4001, N, ncols, False, False, False)
    ips, ipv = _dev_vector(indptr, 1, np.int32)
    ixs, ixv = _dev_vector(indices, 1, np.int32)
    ds, dv = _dev_vector(data, 1)
    rows = list(range(N))
    rt = [hp_dot(data[indptr[i]:indptr[i+1]], x[indices[indptr[i]:indptr[i+1]]]) for i in rows]
    for alpha, beta in ((1., 0.), (-1., 1.), (0.5, 2.)):
        got = run(x, alpha, beta, y0, 1)
        ref = [hp(alpha)*r+hp(beta)*hp(y0[i]) for i, (r, _) in zip(rows, rt)]
        tol = [gamma_tol(int(indptr[i+1]-indptr[i]), mag, alpha, beta, y0[i]) for i, (_, mag) in zip(rows, rt)]
        _assert_rounding(got, rows, ref, tol, 'csr (R) alpha={} beta={}'.format(alpha, beta))
    ctx.close()


@gpu
@pytest.mark.parametrize('sss', (False, True), ids=('csr', 'sss'))
def test_spmv_exact_and_rounding(sss):
    """k_spmv on the pattern of pnl_upload_sparsity (sorted columns are demanded there) in a context with N = 1400 DoFs (interval,
    P1; the smallest N that lets an SSS row hold 1100 entries left of the diagonal with rows to spare): CSR, y = A x, the four-chain
    loop from 193 entries on; SSS, y = (L + L^T + D) x with the mirrored entries through atomics.  (E) with random and one-hot x,
    (R) with m = the number of products of the component (row entries; for SSS also the column entries and the diagonal)."""
    N = 1400
    ctx = _context_with_dofs(N)
    for exact in (True, False):
        indptr, indices, special, data, x, _, diag = _sparse_case(5000+sss, N, N, sss, True, exact)
        ctx.upload_sparsity(indptr, indices)
        ds, dv = _dev_vector(data, 1)
        gs, gv = _dev_vector(diag, 1)

        def run(xh, off):
            xs, xv = _dev_vector(xh, off)
            ys, yv = _dev_vector(np.full(N, POISON), 1-off)
            ctx.spmv(dv.data_ptr(), gv.data_ptr() if sss else 0, xv.data_ptr(), yv.data_ptr())
            return _result(ctx, ys, yv, 1-off)
        D = csr_dense(indptr, indices, data, N)
        if exact:
            full = D+D.T+np.diag(diag) if sss else D
            for off in (0, 1):
                ref = expected_sss(indptr, indices, data, diag, x) if sss else D@x
                _assert_exact(run(x, off), ref, 'spmv sss={} x offset {}'.format(sss, off))
                for k in hot_positions(N, (0, 191, 192, 255, 256)+tuple(int(s) for s in special)):
                    e = np.zeros(N); e[k] = 1.
                    _assert_exact(run(e, off), full[:, k], 'spmv sss={} x=e_{} x offset {}'.format(sss, k, off))
        else:
            mask = D != 0.
            rows = list(range(N))
            ref, tol = [], []
            for i in rows:
                a, xx = D[i, mask[i]], x[mask[i]]
                if sss:
                    a = np.concatenate([a, D[mask[:, i], i], diag[i:i+1]])
                    xx = np.concatenate([xx, x[mask[:, i]], x[i:i+1]])
                r, mag = hp_dot(a, xx)
                ref.append(r); tol.append(gamma_tol(len(a), mag))
            _assert_rounding(run(x, 1), rows, ref, tol, 'spmv (R) sss={}'.format(sss))
    ctx.close()


# ---- pnl_slab_matvec / pnl_slab_diagonal --------------------------------------------------------------------------------------

def _slab_shapes():
    """(name, rowdofs, coldofs).  Contiguous rows inside / across the ends of a contiguous column range (the production shape:
    strips near the coinciding DoFs are masked, full strips far from them plain); interleaved (nothing coincides, nothing is
    plain); rows below / above every column (every full strip plain); random increasing subsets with partial overlap."""
    out = []
    c0 = 50
    i = 0
    for nrows in (1, 64, 65, 200):
        for ncols in (1000, 1024, 4096, 4097, 5121, 8200):
            r0 = (c0-min(10, nrows//2), c0+ncols//2-7, c0+ncols-(nrows+1)//2)[i % 3]
            out.append(('contiguous {}x{} rows from {}'.format(nrows, ncols, r0), np.arange(r0, r0+nrows), np.arange(c0, c0+ncols)))
            i += 1
    out.append(('interleaved 200x4097', 2*np.arange(100, 300)+1, 2*np.arange(4097)))
    out.append(('rows below 65x5121', np.arange(10, 75), np.arange(100, 100+5121)))
    out.append(('rows above 65x4097', np.arange(8300, 8365), np.arange(0, 4097)))
    rng = np.random.default_rng(6000)
    out.append(('random 200x5121', np.sort(rng.choice(np.arange(1000, 3000), 200, replace=False)),
                np.sort(rng.choice(SLAB_N, 5121, replace=False))))
    out.append(('random 64x1024', np.sort(rng.choice(np.arange(2000, 2200), 64, replace=False)),
                np.sort(rng.choice(np.arange(1500, 3500), 1024, replace=False))))
    return out


SLAB_SHAPES = _slab_shapes()
SLAB_LAYOUTS = ((0, 0), (1, 0), (0, 1))          # (ld - ncols, base offset)
SLAB_R_SHAPES = ('contiguous 200x8200 rows from 8150', 'interleaved 200x4097', 'random 200x5121')


def test_slab_shapes_are_what_they_claim():
    names = [s[0] for s in SLAB_SHAPES]
    assert all(n in names for n in SLAB_R_SHAPES) and len(SLAB_SHAPES) == 29
    for name, rd, cd in SLAB_SHAPES:
        assert np.all(np.diff(rd) > 0) and np.all(np.diff(cd) > 0) and rd.min() >= 0 and cd.min() >= 0
        assert rd.max() < SLAB_N and cd.max() < SLAB_N
        common = np.intersect1d(rd, cd).size
        if name.startswith('contiguous') or name.startswith('random'):
            assert common > 0
        else:
            assert common == 0
    # the production shape has plain strips (a full 1024-column strip whose DoFs all lie on one side of the 64 row DoFs) and masked ones
    _, rd, cd = SLAB_SHAPES[names.index('contiguous 200x8200 rows from 8150')]
    plain = [rd[63] < cd[c] or rd[0] > cd[c+1023] for c in range(0, 8200-1023, 1024)]
    assert any(plain) and not all(plain)


@gpu
@pytest.mark.parametrize('shape', SLAB_SHAPES, ids=[s[0].replace(' ', '_') for s in SLAB_SHAPES])
def test_slab_exact(shape):
    """(E) for k_gemv_two_sided<true> and k_slab_diag with dblocks = NULL in a context that holds an interval mesh, its P1 DoF map
    (N = 8399) and the row slab -- nothing else is needed: ld = ncols, ncols + 1 and a misaligned base; the entries at coinciding
    DoFs hold 2^20 .. 2^21, so that a doubled one cannot hide"""
    name, rd, cd = shape
    ctx = _context_with_dofs(SLAB_N)
    ctx.set_row_slab(rd, cd)
    rng = np.random.default_rng(6100+len(name)+int(rd[0])+int(cd[-1]))
    nr, nc = len(rd), len(cd)
    S = rng.integers(-1024, 1025, size=(nr, nc), dtype=np.int64)
    same = rd[:, None] == cd[None, :]
    S[same] = rng.integers(LOW_LO, LOW_HI+1, size=int(same.sum()), dtype=np.int64)
    x = exact_vector(rng, SLAB_N)
    ks = sorted({int(rd[0]), int(rd[-1])} | {int(cd[k]) for k in hot_positions(nc)})
    X = np.concatenate([x[:, None], _hot_matrix(SLAB_N, ks, np.int64)], axis=1)
    Y = expected_slab(S, rd, cd, X, SLAB_N)
    dref = expected_slab_diagonal(S, rd, cd, SLAB_N)
    core = _dev(S.astype(np.float64))
    for dl, ao in SLAB_LAYOUTS:
        store, Sv = _dev_matrix(core, nc+dl, ao)
        for j in range(X.shape[1]):
            xs, xv = _dev_vector(X[:, j], ao)
            ys, yv = _dev_vector(np.full(SLAB_N, POISON), 1-ao)
            ctx.slab_matvec(Sv.data_ptr(), nc+dl, 0, xv.data_ptr(), yv.data_ptr())
            _assert_exact(_result(ctx, ys, yv, 1-ao), Y[:, j], 'slab {} ld=ncols+{} offset {} {}'.format(
                name, dl, ao, 'random x' if j == 0 else 'x=e_{} (component i = operator entry (i, {}))'.format(ks[j-1], ks[j-1])))
        gs, gv = _dev_vector(np.full(SLAB_N, POISON), ao)
        ctx.slab_diagonal(Sv.data_ptr(), nc+dl, 0, gv.data_ptr())
        _assert_exact(_result(ctx, gs, gv, ao), dref, 'slab diagonal {} ld=ncols+{} offset {}'.format(name, dl, ao))
    ctx.close()


@gpu
@pytest.mark.parametrize('name', SLAB_R_SHAPES)
def test_slab_rounding(name):
    """(R): component i gathers the products of its slab row (if i is a row DoF) and of its slab column without the coinciding
    entry (if i is a column DoF); m = their number; a component that gathers nothing is exactly 0"""
    _, rd, cd = SLAB_SHAPES[[s[0] for s in SLAB_SHAPES].index(name)]
    ctx = _context_with_dofs(SLAB_N)
    ctx.set_row_slab(rd, cd)
    rng = np.random.default_rng(6500+len(name))
    nr, nc = len(rd), len(cd)
    S, x = rtype(rng, (nr, nc)), rtype(rng, SLAB_N)
    St = np.ascontiguousarray(S.T)
    rowof, colof = {int(I): r for r, I in enumerate(rd)}, {int(J): c for c, J in enumerate(cd)}
    rows = sorted(set(hp_rows(SLAB_N)) | ({int(rd[0]), int(rd[-1]), int(cd[0]), int(cd[-1])} if not LD_OK else set()))
    ref, tol = [], []
    for i in rows:
        a, xx = [], []
        if i in rowof:
            a.append(S[rowof[i]]); xx.append(x[cd])
        if i in colof:
            keep = rd != i
            a.append(St[colof[i]][keep]); xx.append(x[rd][keep])
        if a:
            a, xx = np.concatenate(a), np.concatenate(xx)
            r, mag = hp_dot(a, xx)
            ref.append(r); tol.append(gamma_tol(len(a), mag))
        else:
            ref.append(hp(0.)); tol.append(hp(0.))
    core = _dev(S)
    for dl, ao in SLAB_LAYOUTS:
        store, Sv = _dev_matrix(core, nc+dl, ao)
        xs, xv = _dev_vector(x, ao)
        ys, yv = _dev_vector(np.full(SLAB_N, POISON), 1-ao)
        ctx.slab_matvec(Sv.data_ptr(), nc+dl, 0, xv.data_ptr(), yv.data_ptr())
        _assert_rounding(_result(ctx, ys, yv, 1-ao), rows, ref, tol, 'slab (R) {} ld=ncols+{} offset {}'.format(name, dl, ao))
    ctx.close()


# ---- pnl_inv_diagonal ---------------------------------------------------------------------------------------------------------

@gpu
def test_inv_diagonal_is_correctly_rounded():
    """k_diag_inv: no fast-math flag in csrc/Makefile, so 1. / a_ii is the IEEE division and equals numpy's bit for bit; values over
    the whole normal range whose reciprocal is normal, ld > n, misaligned base"""
    ctx = _context()
    rng = np.random.default_rng(7000)
    for n, dl, ao in ((1, 0, 0), (257, 1, 1), (1025, 6, 0), (4097, 0, 1)):
        d = rng.standard_normal(n)*10.**rng.uniform(-300., 300., size=n)
        d[:min(n, 6)] = [1., -1., 3., 2.**-1000, -2.**1000, 1.+2.**-52][:min(n, 6)]
        A = rtype(rng, (n, n))
        A[np.arange(n), np.arange(n)] = d
        store, Av = _dev_matrix(_dev(A), n+dl, ao)
        os_, ov = _dev_vector(np.full(n, POISON), 1-ao)
        ctx.inv_diagonal(Av.data_ptr(), n+dl, n, ov.data_ptr())
        _assert_exact(_result(ctx, os_, ov, 1-ao), 1./d, 'inv_diagonal n={} ld=n+{} offset {}'.format(n, dl, ao))
    ctx.close()


# ---- pnl_cg_jacobi ------------------------------------------------------------------------------------------------------------

def spd_system(n, rho, seed):
    """B = diag(s) T diag(s), T_ij = rho^|i-j| (Kac-Murdock-Szego), s graded over four decades: diag(B) = s^2, so that the
    Jacobi-preconditioned matrix D^-1/2 B D^-1/2 is T itself, whatever the grading; b = B x_true.  Returns B, b and the stored
    matrix: B on and above the diagonal, integers in [2^20, 2^21] below it."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    s = 10.**np.linspace(-2., 2., n)
    B = (rho**np.abs(i[:, None]-i[None, :]))*s[:, None]*s[None, :]
    B = np.triu(B)+np.triu(B, 1).T
    stored = B.copy()
    low = np.tri(n, n, -1, dtype=bool)
    stored[low] = rng.integers(LOW_LO, LOW_HI+1, size=int(low.sum())).astype(np.float64)
    b = B@(rng.standard_normal(n)/s)
    return B, b, stored


def hp_matvec(B, x):
    """B x with B, x fp64, products and sums in the high-precision arithmetic; also |B| |x|"""
    if LD_OK:
        Bl, xl = B.astype(LD), np.asarray(x, dtype=LD)
        return Bl@xl, np.abs(Bl)@np.abs(xl)
    rt = [hp_dot(B[i], x) for i in range(B.shape[0])]
    return [r for r, _ in rt], [m for _, m in rt]


def true_residual(B, b, x, dinv):
    """sqrt(r . D^-1 r), r = b - B x, in the high-precision arithmetic; and the floor of the drift allowance,
    (n + 4) u || |B| |x| + |b| || in the D^-1 norm"""
    Bx, mag = hp_matvec(B, x)
    n = len(b)
    r = [hp(b[i])-Bx[i] for i in range(n)]
    res = sum(r[i]*r[i]*hp(dinv[i]) for i in range(n))**0.5
    fl = sum((mag[i]+abs(hp(b[i])))**2*hp(dinv[i]) for i in range(n))**0.5
    return float(res), float((n+4)*U*fl)


def refined_solution(B, b):
    import scipy.linalg
    lu = scipy.linalg.lu_factor(B)
    x = scipy.linalg.lu_solve(lu, b)
    for _ in range(4):
        Bx, _ = hp_matvec(B, x)
        x = x+scipy.linalg.lu_solve(lu, np.array([float(hp(b[i])-Bx[i]) for i in range(len(b))]))
    return x


def _cg_device(ctx, stored, b, x0, tol, maxiter, dl=1, ao=1):
    n = len(b)
    store, Av = _dev_matrix(_dev(stored), n+dl, ao)
    bs, bv = _dev_vector(b, 1)
    xs, xv = _dev_vector(x0, 1)
    it, res = ctx.cg_jacobi(Av.data_ptr(), n+dl, n, bv.data_ptr(), xv.data_ptr(), tol, maxiter)
    return _result(ctx, xs, xv, 1), it, res


# (n, rho, relative tolerance, kind): the short run stays under 50 iterations (never recomputes the residual), the long run needs
# more than 120 (the k == 50 branch runs at iterations 50 and 99 at least), one system at n = 4161 (second group of g2_upper_block)
CG_CASES = ((601, 0.3, 1e-9, 'short'), (1001, 0.97, 1e-10, 'long'), (4161, 0.6, 1e-9, 'short'))


@gpu
@pytest.mark.parametrize('n,rho,rtol,kind', CG_CASES)
def test_cg_jacobi_on_synthetic_spd(n, rho, rtol, kind):
    """pnl_cg_jacobi against oracle.solver_oracle.cg (the project's fp64 restatement of cg_solver.solve, with the same recomputation
    of the residual at k == 50 and the same stopping quantity sqrt(r . Br)), B = 1 / diag, on the symmetrised upper triangle; the
    stored matrix holds 2^20 .. 2^21 below the diagonal, so CG converging to the oracle's solution proves that it reads the upper
    triangle only.  The test computes the spectrum of the Jacobi-preconditioned matrix itself (eigvalsh) and prints it.

    (i)   maxiter = 0 and an already solved right-hand side return iters = 0 and leave x untouched bit for bit.
    (ii)  iteration count: short runs within +-1 of the oracle's; the long run within 5 % of the oracle's count (rounding in
          another summation order shifts late iterations).  Measured on an MI355X, oracle / device: 17 / 17 (n = 601), 386 / 391 and 393
          in two runs (n = 1001; the order of the atomics differs from run to run; margin 19; the oracle's own count moves with the BLAS of the host, 394 on another machine), 40 / 40
          (n = 4161).
    (iii) true preconditioned residual sqrt(r . D^-1 r), r = b - A_op x in the arithmetic of (R), against the returned one: the
          gap is the drift since the last recomputation.  Allowance = max(8 x the same gap of the oracle's fp64 run (random-walk
          spread between two summation orders), (n + 4) u || |A_op| |x| + |b| ||_{D^-1}); the true residual must be <= tol +
          allowance.  Measured, oracle gap / device gap / floor: 9.2e-17 / 2.5e-16 / 4.5e-12 (n = 601, tol 2.7e-8),
          3.7e-15 / 1.2e-15 / 1.9e-10 (n = 1001, tol 1.5e-8), 6.6e-16 / 1.2e-15 / 1.4e-10 (n = 4161, tol 9.7e-8): the floor
          decides in all three, 8 x the oracle's gap never does.
    (iv)  error against the longdouble-refined direct solution x*: with Ahat = D^-1/2 A D^-1/2 (eigenvalues lambda_min ..
          lambda_max computed here), e = x* - x and r = b - A x = A e:  D^1/2 e = Ahat^-1 D^-1/2 r, hence
          || D^1/2 e ||_2 <= || r ||_{D^-1} / lambda_min <= (tol + allowance) / lambda_min, which is itself below
          cond * tol / lambda_min (cond = lambda_max / lambda_min > 1 + allowance / tol, asserted).  x* carries the error of
          the refinement, u-level relative to x*, added as (n + 4) u || D^1/2 x* ||_2."""
    from oracle import solver_oracle
    ctx = _context()
    B, b, stored = spd_system(n, rho, 8000+n)
    d = np.diagonal(B).copy()
    dinv = 1./d
    t0 = time.time()
    lam = np.linalg.eigvalsh(B*np.sqrt(dinv)[:, None]*np.sqrt(dinv)[None, :])
    lmin, lmax = float(lam[0]), float(lam[-1])
    cond = lmax/lmin
    print('cg n={} rho={}: Jacobi-preconditioned spectrum [{:.6e}, {:.6e}], cond {:.4e} (eigvalsh {:.1f} s)'.format(
        n, rho, lmin, lmax, cond, time.time()-t0))
    assert lmin > 0.
    x0 = np.zeros(n)
    tol = rtol*math.sqrt(float(b@(dinv*b)))
    # (i)
    xs0 = np.random.default_rng(1).standard_normal(n)
    xg, it, res = _cg_device(ctx, stored, b, xs0, tol, 0)
    assert it == 0 and np.array_equal(xg, xs0) and res > tol
    bsolved = B@xs0
    xg, it, res = _cg_device(ctx, stored, bsolved, xs0, 1e-6*math.sqrt(float(bsolved@(dinv*bsolved))), 500)
    assert it == 0 and np.array_equal(xg, xs0)
    # oracle and device run
    xo, ito, reso = solver_oracle.cg(B, b, x0=x0, tol=tol, maxiter=2000, B=lambda r: dinv*r)
    xg, it, res = _cg_device(ctx, stored, b, x0, tol, 2000)
    print('cg n={} rho={}: iterations oracle {}, device {}'.format(n, rho, ito, it))
    # (ii)
    if kind == 'short':
        assert ito < 50 and abs(it-ito) <= 1, (it, ito)
    else:
        assert ito > 120 and it > 120 and abs(it-ito) <= 0.05*ito, (it, ito)
    # (iii)
    true_o, floor_o = true_residual(B, b, xo, dinv)
    true_g, floor_g = true_residual(B, b, xg, dinv)
    gap_o, gap_g = abs(true_o-reso[-1]), abs(true_g-res)
    allowance = max(8.*gap_o, floor_g)
    print('cg n={} rho={}: tol {:.6e}; oracle residual returned {:.6e} true {:.6e} gap {:.3e}; device returned {:.6e} true {:.6e} '
          'gap {:.3e}; floor {:.3e}, allowance {:.3e}'.format(n, rho, tol, reso[-1], true_o, gap_o, res, true_g, gap_g, floor_g, allowance))
    assert res <= tol
    assert gap_g <= allowance, (gap_g, gap_o, floor_g)
    assert true_g <= tol+allowance, (true_g, tol, allowance)
    # (iv)
    assert cond > 1.+allowance/tol
    xstar = refined_solution(B, b)
    sq = np.sqrt(d)
    err = float(np.linalg.norm(sq*(xg-xstar)))
    bound = (tol+allowance)/lmin+(n+4)*U*float(np.linalg.norm(sq*xstar))
    print('cg n={} rho={}: || D^1/2 (x - x*) || = {:.3e}, bound (tol + allowance) / lambda_min = {:.3e}, cond tol / lambda_min = {:.3e}'.format(
        n, rho, err, bound, cond*tol/lmin))
    assert err <= bound, (err, bound)
    assert float(np.linalg.norm(sq*(xo-xstar))) <= bound
    ctx.close()
