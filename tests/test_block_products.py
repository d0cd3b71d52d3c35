"""Products with a block of vectors: pnl_gemv_block and pnl_spmv_block through the C ABI on SYNTHETIC matrices, and matvec_multi /
dotMV / A * X of the operator classes.  The method is that of tests/test_apply_kernels.py, whose helpers are imported:

(E) exact.  Integer entries in [-1024, 1024] (X nowhere zero), alpha / beta in {1, -1, 2, 0.5, 0}: every partial sum is an integer
    (a multiple of 1/2 after alpha / beta) below 4161 * 2^20 * 2 << 2^53, so fp64 arithmetic is exact in any order, MFMA included.
    The reference is an int64 numpy product, the assertion is bit equality.  Every padding column (ld > n) and the elements before
    and after every array hold 2^30; the whole allocation of Y is compared, so a write past an edge or a sum that took a padding
    element shows.
(R) rounding.  Entries standard_normal * 10^uniform(-6, 6), reference in np.longdouble where it has >= 63 mantissa bits (every
    component is checked), else mpmath on a seeded subset of >= 64 rows that holds every tile edge (only that subset is checked).
    tol_i = (m + 4) u (|alpha| (|A| |x|)_i + |beta| |b_i|), u = 2^-53, m = products per component: it holds for any summation
    order with one rounding per fma, which is what v_mfma_f64_16x16x4_f64 does.

Tile edges of k_gemv_block (csrc/pnl_block.hip): 16 rows per wave, 128 rows per workgroup, 64 columns per staged sub-chunk,
2048 columns per workgroup (more columns: partial sums through the context's scratch, k_gb_reduce), 16 vectors per group.
"""
import numpy as np
import pytest

from test_apply_kernels import (U, LD, LD_OK, POISON, ROW_LENGTHS, exact_vector, rtype, csr_dense, expected_sss, gamma_tol, hp, hp_dot,
                                sparse_pattern, _context, _context_with_dofs, _dev, _dev_matrix, _dev_vector, _assert_exact)

gpu = pytest.mark.gpu

NVECS = (1, 2, 3, 15, 16, 17, 33)
ISSUE_SHAPES = ((1, 1), (3, 257), (257, 3), (15, 16), (16, 15), (17, 33), (64, 511), (65, 513), (300, 1025), (1025, 2049),
                (1089, 1089), (2113, 2113), (4161, 4161))
# the edges +-1 of the row tile (128), the staged sub-chunk (64 columns), the column chunk (2048; (1025, 2049) above), and
# two, three and five chunks
EDGE_SHAPES = ((127, 129), (128, 128), (129, 127), (63, 65), (65, 63), (66, 64), (17, 2047), (33, 2048), (17, 4095), (33, 4096), (130, 4097),
               (20, 8193))
BIG = ((2113, 2113), (4161, 4161))
# (ld - n of A, X, B, Y; base offset in doubles of A, X, B, Y)
BLOCK_LAYOUTS = ((0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 0, 0, 0, 0), (6, 6, 6, 6, 0, 0, 0, 0), (0, 1, 6, 0, 1, 0, 1, 0),
                 (1, 6, 0, 6, 0, 1, 0, 1), (6, 0, 1, 1, 1, 1, 1, 1))
# (alpha, beta, b): b = None (null pointer, beta = 0, Y prefilled with NaN), 'b' (distinct from Y), 'y' (B == Y)
COEFFS = ((1., 0., None), (-1., 1., 'b'), (2., -1., 'y'), (0.5, 0.5, 'b'), (0., 2., 'y'), (-1., 0., 'b'), (0.5, 1., 'y'))
TILE_EDGES = (15, 16, 17, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097)


# ---- expected values (plain numpy; tested below without a GPU) -----------------------------------------------------------------

def expected_block(A, X, alpha=1., beta=0., B=None):
    """Y[v] = alpha A X[v] + beta B[v] for the rows of X, in float64 from an integer (or float) product"""
    Y = alpha*(X@A.T).astype(np.float64)
    return Y if B is None or beta == 0. else Y+beta*np.asarray(B, dtype=np.float64)


def exact_products(A, X):
    """X A^T in int64.  Large blocks: the float64 product (exact below 2^53 in any order, and what BLAS makes fast), converted, with
    64 seeded rows and the first and last one recomputed in int64"""
    if A.size <= 2**21:
        return X@A.T
    P = X.astype(np.float64)@A.T.astype(np.float64)
    assert np.abs(X).max()*np.abs(A).max()*A.shape[1] < 2**53
    out = P.astype(np.int64)
    assert np.array_equal(out.astype(np.float64), P)
    rows = np.unique(np.concatenate([[0, A.shape[0]-1], np.random.default_rng(A.shape[0]).choice(A.shape[0], size=64, replace=False)]))
    assert np.array_equal(out[:, rows], X@A[rows].T)
    return out


def block_image(core, ld, off, fill=POISON):
    """the host image of an allocation that holds the k x n block ``core`` with leading dimension ld at offset off: poison in the
    padding columns and in the elements before and after"""
    k, n = core.shape
    img = np.full(off+k*ld+1, float(fill))
    body = img[off:off+k*ld].reshape(k, ld)
    body[:, :n] = core
    return img


def subset_rows(n, seed=0):
    """every row with longdouble; with mpmath >= 64 seeded rows and every tile edge"""
    if LD_OK:
        return list(range(n))
    rows = {k+d for k in TILE_EDGES+(0, n-1) for d in (-1, 0, 1) if 0 <= k+d < n}
    rows |= set(int(i) for i in np.random.default_rng(seed+n).choice(n, size=min(n, 64), replace=False))
    return sorted(rows)


def hp_products(A, X, rows):
    """(A X[v])_i and (|A| |X[v]|)_i for i in rows, every v, in high precision: two arrays [k][len(rows)]"""
    if LD_OK:
        Ah, Xh = A[rows].astype(LD), X.astype(LD)
        return (Ah@Xh.T).T, (np.abs(Ah)@np.abs(Xh).T).T
    ref = [[hp_dot(A[i], x) for i in rows] for x in X]
    return [[r for r, _ in row] for row in ref], [[m for _, m in row] for row in ref]


# ---- CPU-only -------------------------------------------------------------------------------------------------------------------

def test_expected_block_against_loops():
    rng = np.random.default_rng(0)
    for nr, nc, k in ((1, 1, 1), (3, 7, 2), (5, 4, 3)):
        A = rng.integers(-9, 10, size=(nr, nc), dtype=np.int64)
        X = rng.integers(-9, 10, size=(k, nc), dtype=np.int64)
        B = rng.integers(-9, 10, size=(k, nr), dtype=np.int64)
        for alpha, beta in ((1., 0.), (-1., 1.), (0.5, 2.), (0., 0.5)):
            want = [[alpha*sum(int(A[r, c])*int(X[v, c]) for c in range(nc))+beta*int(B[v, r]) for r in range(nr)] for v in range(k)]
            assert expected_block(A, X, alpha, beta, B).tolist() == want
        assert expected_block(A, X).tolist() == [[float(sum(int(A[r, c])*int(X[v, c]) for c in range(nc))) for r in range(nr)] for v in range(k)]
    Ab = rng.integers(-1024, 1025, size=(1500, 1500), dtype=np.int64)
    Xb = rng.integers(-1024, 1025, size=(3, 1500), dtype=np.int64)
    assert Ab.size > 2**21 and np.array_equal(exact_products(Ab, Xb), Xb@Ab.T)
    img = block_image(np.arange(6.).reshape(2, 3), 5, 1)
    assert img.tolist() == [POISON, 0, 1, 2, POISON, POISON, 3, 4, 5, POISON, POISON, POISON]
    ref, mag = hp_products(np.array([[1., -2.], [3., 4.]]), np.array([[1., 1.], [2., -1.]]), [0, 1])
    assert [[float(v) for v in r] for r in ref] == [[-1., 7.], [4., 2.]] and [[float(v) for v in r] for r in mag] == [[3., 7.], [4., 10.]]
    assert set(ISSUE_SHAPES) & set(EDGE_SHAPES) == set() and 4161*2**20*2 < 2**53
    for e in (127, 128, 129):
        assert any(e in s for s in EDGE_SHAPES)
    for e in (63, 64, 65, 2047, 2048, 4095, 4096, 4097, 8193):
        assert any(s[1] == e for s in EDGE_SHAPES)
    assert (1025, 2049) in ISSUE_SHAPES


def test_diagonal_operator_block_products():
    """diagonalOperator.dotMV / matvec_multi / *: the three shape cases of LinearOperator_{SCALAR}.pxi:64-76"""
    from pynucleus_amd.linear_operators import diagonalOperator
    rng = np.random.default_rng(1)
    n, k = 5, 3
    d = rng.integers(1, 9, size=n).astype(np.float64)
    D = diagonalOperator(d)
    Xr = rng.integers(-9, 10, size=(k, n)).astype(np.float64)       # rows are vectors
    assert np.array_equal(D.matvec_multi(Xr), Xr*d[None, :])
    Y = np.zeros((k, n))
    assert D.matvec_multi(Xr, Y) is Y and np.array_equal(Y, Xr*d[None, :])
    assert np.array_equal(D.dotMV(Xr), Xr*d[None, :]) and D.dotMV(Xr).shape == (k, n)
    Xc = np.ascontiguousarray(Xr.T)                                  # columns are vectors
    for got in (D.dotMV(Xc), D*Xc, D.matvec(Xc), D.dot(Xc)):
        assert got.shape == (n, k) and np.array_equal(got, d[:, None]*Xc)
    # square X: the first rule wins, the columns are the vectors
    Xs = rng.integers(-9, 10, size=(n, n)).astype(np.float64)
    assert np.array_equal(D.dotMV(Xs), d[:, None]*Xs) and np.array_equal(D*Xs, np.diag(d)@Xs)
    assert not np.array_equal(d[:, None]*Xs, Xs*d[None, :])
    with pytest.raises(ValueError):
        D.dotMV(np.zeros((n+1, n+2)))
    with pytest.raises(ValueError):
        D.dotMV(np.zeros(n))
    # 1-D arguments are what they were
    x = rng.standard_normal(n)
    assert np.array_equal(D.matvec(x), d*x) and np.array_equal(D*x, d*x)


class _StubOperator:
    """numpy matvec only; counts its calls"""

    def __init__(self, A):
        self.A = A
        self.num_rows, self.num_columns = A.shape
        self.calls = 0

    def matvec(self, x, y=None):
        self.calls += 1
        assert np.ndim(x) == 1
        return self.A@np.asarray(x)


def test_loop_helper_on_a_stub_operator():
    from pynucleus_amd.linear_operators import matvec_multi_loop, blockProducts
    rng = np.random.default_rng(2)
    A = rng.standard_normal((4, 6))
    op = _StubOperator(A)
    X = rng.standard_normal((3, 6))
    Y = matvec_multi_loop(op, X)
    assert op.calls == 3 and Y.shape == (3, 4)
    for v in range(3):
        assert np.array_equal(Y[v], A@X[v])
    out = np.zeros((3, 4))
    assert matvec_multi_loop(op, X, out) is out and np.array_equal(out, Y)
    with pytest.raises(AssertionError):
        matvec_multi_loop(op, rng.standard_normal((3, 5)))

    class Looped(blockProducts, _StubOperator):
        pass
    lo = Looped(A)
    assert np.array_equal(lo.matvec_multi(X), Y) and np.array_equal(lo.dotMV(X), Y)
    assert np.array_equal(lo.dotMV(np.ascontiguousarray(X.T)), Y.T)


# ---- pnl_gemv_block --------------------------------------------------------------------------------------------------------------

def _dev_block(core, ld, off, fill=POISON):
    """(storage, pointer of the block): core [k][n] inside a poisoned allocation"""
    import torch
    store = torch.from_numpy(block_image(core, ld, off, fill)).cuda()
    return store, store.data_ptr()+8*off


def _gemv_block(ctx, Aptr, ldA, nr, nc, X, B, alpha, beta, bkind, dX, dB, dY, oX, oB, oY):
    """one call; returns Y [k][nr] after checking the whole allocation of Y (padding, guards) against its expected image"""
    k = X.shape[0]
    xs, xp = _dev_block(X.astype(np.float64), nc+dX, oX)
    if bkind == 'y':
        dB, oB = dY, oY
        ys, yp = _dev_block(B.astype(np.float64), nr+dY, oY)
        bp = yp
    else:
        ys, yp = _dev_block(np.full((k, nr), np.nan), nr+dY, oY)
        bs, bp = _dev_block(B.astype(np.float64), nr+dB, oB) if bkind == 'b' else (None, 0)
    ctx.gemv_block(Aptr, ldA, nr, nc, k, xp, nc+dX, alpha, beta, bp, nr+dB if bp else 0, yp, nr+dY)
    ctx.synchronize()
    got = ys.cpu().numpy()
    Y = got[oY:oY+k*(nr+dY)].reshape(k, nr+dY)[:, :nr].copy()
    assert np.array_equal(got, block_image(Y, nr+dY, oY)), 'padding column or guard element of Y overwritten'
    return Y


def _assert_block_exact(got, ref, what):
    for v in range(ref.shape[0]):
        _assert_exact(got[v], ref[v], what+' vector {}'.format(v))


@gpu
@pytest.mark.parametrize('shape', ISSUE_SHAPES+EDGE_SHAPES, ids=lambda s: '{}x{}'.format(*s))
def test_gemv_block_exact(shape):
    """(E) for k_gemv_block and k_gb_reduce.  Shapes: those of the issue and the edges +-1 of this kernel's tiles -- 16 rows per wave
    and 128 per workgroup (15 / 16 / 17, 127 / 128 / 129 rows), 64 columns per staged sub-chunk (63 / 64 / 65 and 127 / 128 / 129
    columns), 2048 columns per workgroup (2047 / 2048: one chunk, direct store; 2049: two chunks through the scratch), the edges of the
    second chunk (4095 / 4096 / 4097) and five chunks (8193), 16 vectors per group (15 / 16 / 17 / 33).  Six layouts: ld - n in {0, 1, 6} and base offsets {0, 1} for each of A, X, B, Y (with
    the aligned even-ld case that takes the 16-byte loads and the scalar-load cases); B null / distinct / B == Y; Y prefilled with
    NaN where it is not B.  The two large squares take every layout at nvec in (1, 17) and every nvec on the first and last layout."""
    import torch
    nr, nc = shape
    ctx = _context()
    rng = np.random.default_rng(7000+nr+3*nc)
    A = rng.integers(-1024, 1025, size=(nr, nc), dtype=np.int64)
    kmax = max(NVECS)
    X = np.stack([exact_vector(rng, nc) for _ in range(kmax)])
    B = np.stack([exact_vector(rng, nr) for _ in range(kmax)])
    AX = exact_products(A, X)                                        # int64 [kmax][nr]
    assert np.abs(AX).max()*2+2*1024 < 2**53
    core = _dev(A.astype(np.float64))
    for li, (dA, dX, dB, dY, oA, oX, oB, oY) in enumerate(BLOCK_LAYOUTS):
        store, Av = _dev_matrix(core, nc+dA, oA)
        nvecs = NVECS if shape not in BIG or li in (0, len(BLOCK_LAYOUTS)-1) else (1, 17)
        for k in nvecs:
            for ci, (alpha, beta, bkind) in enumerate(COEFFS):
                if shape in BIG and (ci+k+li) % 3:
                    continue                                         # a third of the coefficient cases per (layout, nvec) there
                tag = '{}x{} nvec={} layout {} alpha={} beta={} b={}'.format(nr, nc, k, li, alpha, beta, bkind)
                ref = alpha*AX[:k].astype(np.float64)+(beta*B[:k].astype(np.float64) if bkind else 0.)
                got = _gemv_block(ctx, Av.data_ptr(), nc+dA, nr, nc, X[:k], B[:k], alpha, beta, bkind, dX, dB, dY, oX, oB, oY)
                _assert_block_exact(got, ref, tag)
        assert np.array_equal(store.cpu().numpy(), block_image(A.astype(np.float64), nc+dA, oA)), 'A was written'
        del store, Av
    del core
    ctx.close()
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize('shape', ((300, 1025), (130, 4097), (2113, 2113)), ids=lambda s: '{}x{}'.format(*s))
def test_gemv_block_one_hot(shape):
    """X = rows of the identity at 0, the tile edges and ncols - 1: the result is those columns of A bit for bit (component r of
    vector v = entry (r, position v)), so a failure names the entry"""
    nr, nc = shape
    ctx = _context()
    rng = np.random.default_rng(7100+nr+nc)
    A = rng.integers(-1024, 1025, size=(nr, nc), dtype=np.int64)
    A[A == 0] = 7
    ks = sorted({p for p in (0, 1, 7, 8)+TILE_EDGES+(nc-2, nc-1) if 0 <= p < nc})
    X = np.zeros((len(ks), nc), dtype=np.int64)
    X[np.arange(len(ks)), ks] = 1
    core = _dev(A.astype(np.float64))
    for dA, dX, dB, dY, oA, oX, oB, oY in (BLOCK_LAYOUTS[0], BLOCK_LAYOUTS[1], BLOCK_LAYOUTS[5]):
        store, Av = _dev_matrix(core, nc+dA, oA)
        got = _gemv_block(ctx, Av.data_ptr(), nc+dA, nr, nc, X, None, 1., 0., None, dX, dB, dY, oX, oB, oY)
        for v, p in enumerate(ks):
            _assert_exact(got[v], A[:, p], '{}x{} x=e_{} (component r = entry (r, {}))'.format(nr, nc, p, p))
    ctx.close()


_R_CACHE = {}


def _rounding_case(shape):
    """A, X (17 vectors), B, rows, reference and magnitude of A X: computed once per shape"""
    if shape not in _R_CACHE:
        nr, nc = shape
        rng = np.random.default_rng(7200+nr+nc)
        A, X, B = rtype(rng, (nr, nc)), rtype(rng, (17, nc)), rtype(rng, (17, nr))
        rows = subset_rows(nr)
        ref, mag = hp_products(A, X, rows)
        _R_CACHE[shape] = (A, X, B, rows, ref, mag)
    return _R_CACHE[shape]


def _assert_block_rounding(got, rows, ref, mag, m, alpha, beta, B, what):
    """|got[v][i] - (alpha ref + beta B)| <= (m + 4) u (|alpha| mag + |beta| |B|) for every v and every i in rows"""
    for v in range(got.shape[0]):
        if LD_OK:
            bb = B[v][rows].astype(LD) if B is not None else LD(0)
            want = LD(alpha)*np.asarray(ref[v], dtype=LD)+LD(beta)*bb
            tol = (m+4)*LD(U)*(abs(LD(alpha))*np.asarray(mag[v], dtype=LD)+abs(LD(beta))*np.abs(bb))
            err = np.abs(got[v][rows].astype(LD)-want)
            bad = np.nonzero(~(err <= tol))[0]
            assert bad.size == 0, '{} vector {}: {} components outside the bound, first row {}: error {:.3e} > tol {:.3e}'.format(
                what, v, bad.size, rows[bad[0]], float(err[bad[0]]), float(tol[bad[0]]))
        else:
            for j, i in enumerate(rows):
                bb = hp(B[v][i]) if B is not None else hp(0.)
                want = hp(alpha)*ref[v][j]+hp(beta)*bb
                tol = gamma_tol(m, mag[v][j], alpha, beta, bb)
                assert abs(hp(got[v][i])-want) <= tol, '{} vector {} row {}'.format(what, v, i)


@gpu
@pytest.mark.parametrize('nvec', (3, 16, 17))
@pytest.mark.parametrize('shape', ((65, 513), (1025, 2049), (2113, 2113)), ids=lambda s: '{}x{}'.format(*s))
def test_gemv_block_rounding(shape, nvec):
    """(R): every component (longdouble; with mpmath the seeded subset with every tile edge, and only that) within
    (ncols + 4) u (|alpha| (|A| |x|)_i + |beta| |b_i|)"""
    nr, nc = shape
    A, X, B, rows, ref, mag = _rounding_case(shape)
    ctx = _context()
    core = _dev(A)
    for (dA, dX, dB, dY, oA, oX, oB, oY), (alpha, beta, bkind) in zip((BLOCK_LAYOUTS[0], BLOCK_LAYOUTS[3], BLOCK_LAYOUTS[5]),
                                                                    ((1., 0., None), (-1., 1., 'b'), (0.5, -1., 'y'))):
        store, Av = _dev_matrix(core, nc+dA, oA)
        got = _gemv_block(ctx, Av.data_ptr(), nc+dA, nr, nc, X[:nvec], B[:nvec], alpha, beta, bkind, dX, dB, dY, oX, oB, oY)
        _assert_block_rounding(got, rows, ref, mag, nc, alpha, beta, B if bkind else None,
                               '{}x{} nvec={} alpha={} beta={} b={}'.format(nr, nc, nvec, alpha, beta, bkind))
    ctx.close()


@gpu
def test_gemv_block_bits_do_not_depend_on_the_block():
    """one A (2113^2, ld = n + 1 at offset 1) and one vector x: its result has the same bits alone (nvec = 1), at the positions 0, 7,
    15, 16 and 32 of blocks of 3, 16, 17 and 33 other random vectors (where the block is long enough), and when a call is repeated"""
    n = 2113
    rng = np.random.default_rng(7300)
    A, x = rtype(rng, (n, n)), rtype(rng, n)
    ctx = _context()
    store, Av = _dev_matrix(_dev(A), n+1, 1)

    def run(X):
        return _gemv_block(ctx, Av.data_ptr(), n+1, n, n, X, None, 1., 0., None, 1, 0, 6, 1, 0, 1)
    alone = run(x[None, :])[0]
    assert np.array_equal(alone, run(x[None, :])[0])
    assert np.abs(alone-A@x).max() <= 1e-9*np.abs(A@x).max()
    for nother in (3, 16, 17, 33):
        others = rtype(rng, (nother, n))
        for pos in (0, 7, 15, 16, 32):
            if pos > nother:
                continue
            X = np.insert(others, pos, x, axis=0)
            first, second = run(X), run(X)
            assert np.array_equal(first, second), 'repeated call differs ({} others, position {})'.format(nother, pos)
            assert np.array_equal(first[pos], alone), 'bits of x differ among {} others at position {}'.format(nother, pos)
    ctx.close()


@gpu
def test_gemv_block_validation():
    """every invalid argument of the header returns PNL_ERR_INVALID and leaves Y (a sentinel) untouched"""
    import torch
    from pynucleus_amd import _lib
    import ctypes as C
    ctx = _context()
    nr, nc, k = 5, 7, 3
    A = torch.ones((nr, nc), dtype=torch.float64, device='cuda')
    X = torch.ones((k, nc), dtype=torch.float64, device='cuda')
    B = torch.ones((k, nr), dtype=torch.float64, device='cuda')
    Y = torch.full((k, nr), 77., dtype=torch.float64, device='cuda')
    good = dict(ctx=ctx.h, A=A.data_ptr(), ldA=nc, nrows=nr, ncols=nc, nvec=k, X=X.data_ptr(), ldx=nc, alpha=1., beta=0., B=None, ldb=0,
                Y=Y.data_ptr(), ldy=nr)

    def call(**kw):
        a = dict(good, **kw)
        p = lambda v: C.c_void_p(v) if v else None
        rc = ctx.L.pnl_gemv_block(a['ctx'], p(a['A']), a['ldA'], a['nrows'], a['ncols'], a['nvec'], p(a['X']), a['ldx'], a['alpha'], a['beta'],
                                  p(a['B']), a['ldb'], p(a['Y']), a['ldy'])
        ctx.synchronize()
        return rc
    bad = [dict(ctx=None), dict(A=None), dict(X=None), dict(Y=None), dict(nvec=0), dict(nvec=-1), dict(nrows=0), dict(ncols=0), dict(ldA=nc-1),
           dict(ldx=nc-1), dict(ldy=nr-1), dict(beta=1., B=None, ldb=nr), dict(beta=1., B=B.data_ptr(), ldb=nr-1), dict(X=Y.data_ptr())]
    for kw in bad:
        assert call(**kw) == _lib.PNL_ERR_INVALID, kw
        assert bool((Y == 77.).all()), kw
    assert call() == _lib.PNL_OK and bool((Y == float(nc)).all())
    assert call(beta=1., B=B.data_ptr(), ldb=nr) == _lib.PNL_OK and bool((Y == float(nc)+1.).all())
    ctx.close()


# ---- pnl_spmv_block --------------------------------------------------------------------------------------------------------------

SP_N = 1400
SP_NVECS = (1, 3, 16, 17)


def _sparse_block_case(seed, sss, exact):
    rng = np.random.default_rng(seed)
    indptr, indices, special = sparse_pattern(rng, SP_N, SP_N, sss, True)
    nnz = int(indptr[-1])
    kmax = max(SP_NVECS)
    if exact:
        data, diag = exact_vector(rng, nnz), exact_vector(rng, SP_N)
        X = np.stack([exact_vector(rng, SP_N) for _ in range(kmax)])
    else:
        data, diag, X = rtype(rng, nnz), rtype(rng, SP_N), rtype(rng, (kmax, SP_N))
    return indptr, indices, data, diag, X


def _spmv_block(ctx, dptr, gptr, X, dX, dY, oX, oY):
    k = X.shape[0]
    xs, xp = _dev_block(X.astype(np.float64), SP_N+dX, oX)
    ys, yp = _dev_block(np.full((k, SP_N), np.nan), SP_N+dY, oY)
    ctx.spmv_block(dptr, gptr, k, xp, SP_N+dX, yp, SP_N+dY)
    ctx.synchronize()
    got = ys.cpu().numpy()
    Y = got[oY:oY+k*(SP_N+dY)].reshape(k, SP_N+dY)[:, :SP_N].copy()
    assert np.array_equal(got, block_image(Y, SP_N+dY, oY)), 'padding column or guard element of Y overwritten'
    return Y


@gpu
@pytest.mark.parametrize('sss', (False, True), ids=('csr', 'sss'))
def test_spmv_block_exact_and_rounding(sss):
    """k_spmv_block on a pattern with the row lengths (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 449, 1100) and strictly
    increasing columns, N = 1400 DoFs, nvec in (1, 3, 16, 17) (the transposed scratch of 1, 4, 16 and 16 + 1 vectors), ldx / ldy with
    padding and offsets.  (E) with guards; (R) with m = the products of the component (SSS: the row, the mirrored entries and the
    diagonal).  CSR: the bits of a vector do not depend on nvec or on its position.  SSS (atomics): value only."""
    ctx = _context_with_dofs(SP_N)
    assert set(ROW_LENGTHS) == {0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 449, 1100}
    for exact in (True, False):
        indptr, indices, data, diag, X = _sparse_block_case(7400+sss, sss, exact)
        assert set(ROW_LENGTHS) <= set(np.diff(indptr).tolist())
        ctx.upload_sparsity(indptr, indices)
        ds, dv = _dev_vector(data, 1)
        gs, gv = _dev_vector(diag, 1)
        gptr = gv.data_ptr() if sss else 0
        D = csr_dense(indptr, indices, data, SP_N)
        if exact:
            full = D+D.T+np.diag(diag) if sss else D
            ref = X@full.T
            for (dX, dY, oX, oY) in ((0, 0, 0, 0), (1, 6, 1, 0), (6, 1, 0, 1)):
                for k in SP_NVECS:
                    _assert_block_exact(_spmv_block(ctx, dv.data_ptr(), gptr, X[:k], dX, dY, oX, oY), ref[:k].astype(np.float64),
                                        'spmv_block sss={} nvec={} ldx=n+{} ldy=n+{}'.format(sss, k, dX, dY))
            if sss:
                assert np.array_equal(ref[0], expected_sss(indptr, indices, data, diag, X[0]))
        else:
            mask = D != 0.
            rows = list(range(SP_N))
            got = {k: _spmv_block(ctx, dv.data_ptr(), gptr, X[:k], 1, 6, 1, 0) for k in SP_NVECS}
            for v in range(max(SP_NVECS)):
                ref, tol = [], []
                for i in rows:
                    a, xx = D[i, mask[i]], X[v][mask[i]]
                    if sss:
                        a = np.concatenate([a, D[mask[:, i], i], diag[i:i+1]])
                        xx = np.concatenate([xx, X[v][mask[:, i]], X[v][i:i+1]])
                    r, mag = hp_dot(a, xx)
                    ref.append(r); tol.append(gamma_tol(len(a), mag))
                for k in SP_NVECS:
                    if v < k:
                        for i, r, t in zip(rows, ref, tol):
                            assert abs(hp(got[k][v][i])-r) <= t, 'spmv_block (R) sss={} nvec={} vector {} row {}'.format(sss, k, v, i)
            if not sss:
                # independence: vector 0 alone, first of 3 / 16 / 17, and at other positions of a permuted block; repeated calls
                alone = got[1][0]
                for k in SP_NVECS:
                    assert np.array_equal(got[k][0], alone), k
                    assert np.array_equal(_spmv_block(ctx, dv.data_ptr(), gptr, X[:k], 1, 6, 1, 0), got[k]), k
                for pos in (2, 7, 15, 16):
                    Xp = np.insert(X[1:], pos, X[0], axis=0)
                    assert np.array_equal(_spmv_block(ctx, dv.data_ptr(), gptr, Xp, 0, 1, 0, 1)[pos], alone), pos
    ctx.close()


@gpu
def test_spmv_block_state_and_validation():
    import torch
    import ctypes as C
    from pynucleus_amd import _lib
    N = 40
    ctx = _context_with_dofs(N)
    X = torch.ones((2, N), dtype=torch.float64, device='cuda')
    Y = torch.full((2, N), 77., dtype=torch.float64, device='cuda')
    data = torch.ones(N, dtype=torch.float64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(d=data, nvec=2, x=X, ldx=N, y=Y, ldy=N):
        rc = ctx.L.pnl_spmv_block(ctx.h, p(d), None, nvec, p(x), ldx, p(y), ldy)
        ctx.synchronize()
        return rc
    assert call() == _lib.PNL_ERR_STATE and bool((Y == 77.).all())            # no pattern yet
    indptr = np.arange(N+1, dtype=np.int32)
    ctx.upload_sparsity(indptr, np.arange(N, dtype=np.int32))                # the identity pattern
    for kw in (dict(d=None), dict(nvec=0), dict(ldx=N-1), dict(ldy=N-1), dict(x=None), dict(y=None), dict(x=Y)):
        assert call(**kw) == _lib.PNL_ERR_INVALID, kw
        assert bool((Y == 77.).all()), kw
    assert call() == _lib.PNL_OK and bool((Y == 1.).all())
    ctx.close()


# ---- the operator classes ---------------------------------------------------------------------------------------------------------

def _dense_operator(ctx, A, pad=3, symmetric=False):
    import torch
    from pynucleus_amd.linear_operators import Dense_LinearOperator
    nr, nc = A.shape
    store = torch.full((nr, nc+pad), float(POISON), dtype=torch.float64, device='cuda')
    store[:, :nc] = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).cuda()
    return Dense_LinearOperator(store[:, :nc], ctx, symmetric=symmetric)


@gpu
@pytest.mark.parametrize('shape', ((300, 1025), (1089, 1089)), ids=lambda s: '{}x{}'.format(*s))
def test_dense_operator_block_products(shape):
    """Dense_LinearOperator on a synthetic torch block with padded rows: matvec_multi, both orientations of dotMV, A * X, numpy and
    torch in / out, Y= given, a strided torch view as X (not copied: its row stride is the leading dimension), symmetric=True on a
    symmetric integer block (the full read: exact), and matvec(x) for 1-D x with the bits of a direct pnl_gemv / pnl_gemv_axpby"""
    import torch
    nr, nc = shape
    ctx = _context()
    rng = np.random.default_rng(7500+nr)
    A = rng.integers(-1024, 1025, size=(nr, nc), dtype=np.int64)
    op = _dense_operator(ctx, A)
    k = 5
    X = np.stack([exact_vector(rng, nc) for _ in range(k)]).astype(np.float64)
    ref = expected_block(A, X.astype(np.int64))                           # [k][nr]
    got = op.matvec_multi(X)
    assert isinstance(got, np.ndarray) and got.shape == (k, nr)
    _assert_block_exact(got, ref, 'matvec_multi numpy')
    out = np.zeros((k, nr))
    assert op.matvec_multi(X, out) is out and np.array_equal(out, ref)
    _assert_block_exact(op.matvec_multi(X[:1]), ref[:1], 'matvec_multi k = 1')
    Xt = torch.from_numpy(X).cuda()
    gt = op.matvec_multi(Xt)
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and gt.shape == (k, nr) and np.array_equal(gt.cpu().numpy(), ref)
    Yt = torch.zeros((k, nr), dtype=torch.float64, device='cuda')
    assert op.matvec_multi(Xt, Yt) is Yt and np.array_equal(Yt.cpu().numpy(), ref)
    # a strided view: k x nc with row stride nc + 9 inside a poisoned buffer
    big = torch.full((k, nc+9), float(POISON), dtype=torch.float64, device='cuda')
    big[:, 2:2+nc] = Xt
    view = big[:, 2:2+nc]
    assert not view.is_contiguous() and view.stride() == (nc+9, 1)
    assert np.array_equal(op.matvec_multi(view).cpu().numpy(), ref)
    # dotMV: rows are vectors / columns are vectors; A * X and matvec / dot with a 2-D argument
    if nr != nc:
        assert np.array_equal(op.dotMV(X), ref)
    Xc = np.ascontiguousarray(X.T)
    for g in (op.dotMV(Xc), op*Xc, op.matvec(Xc), op.dot(Xc)):
        assert g.shape == (nr, k) and np.array_equal(g, ref.T)
    gt = op*Xt.t()
    assert isinstance(gt, torch.Tensor) and gt.shape == (nr, k) and np.array_equal(gt.cpu().numpy(), ref.T)
    with pytest.raises(ValueError):
        op.dotMV(np.zeros((nc+1, nc+2)))
    if nr == nc:
        # the square tie: the columns are the vectors
        Xs = rng.integers(-3, 4, size=(nc, nc)).astype(np.float64)
        assert np.array_equal(op.dotMV(Xs), (A@Xs.astype(np.int64)).astype(np.float64))
        S = np.triu(A)+np.triu(A, 1).T
        sop = _dense_operator(ctx, S, symmetric=True)
        assert sop.symmetric
        _assert_block_exact(sop.matvec_multi(X), (X.astype(np.int64)@S.T).astype(np.float64), 'symmetric=True')
    # 1-D: the code and the bits of before
    x = rng.standard_normal(nc)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty(nr, dtype=torch.float64, device='cuda')
    if nr == nc:
        ctx.gemv(op.A.data_ptr(), op.A.stride(0), nr, xd.data_ptr(), yd.data_ptr(), 0)
    else:
        ctx.gemv_axpby(op.A.data_ptr(), op.A.stride(0), nr, nc, xd.data_ptr(), 1., 0., None, yd.data_ptr())
    ctx.synchronize()
    y1 = op.matvec(x)
    assert y1.shape == (nr,) and np.array_equal(y1, yd.cpu().numpy()) and np.array_equal(op*x, y1) and np.array_equal(op.dot(xd).cpu().numpy(), y1)
    ctx.close()


@gpu
@pytest.mark.parametrize('sss', (False, True), ids=('csr', 'sss'))
def test_sparse_operator_block_products(sss):
    import torch
    from pynucleus_amd.linear_operators import CSR_LinearOperator, SSS_LinearOperator
    ctx = _context_with_dofs(SP_N)
    indptr, indices, data, diag, X = _sparse_block_case(7600+sss, sss, True)
    dev = torch.device('cuda', 0)
    op = (SSS_LinearOperator if sss else CSR_LinearOperator)(indptr, indices, SP_N, ctx, dev)
    op.data_dev[:data.shape[0]] = torch.from_numpy(data.astype(np.float64)).cuda()
    if sss:
        op.diag_dev.copy_(torch.from_numpy(diag.astype(np.float64)).cuda())
    D = csr_dense(indptr, indices, data, SP_N)
    full = D+D.T+np.diag(diag) if sss else D
    X = X[:5]
    ref = (X@full.T).astype(np.float64)
    Xf = X.astype(np.float64)
    _assert_block_exact(op.matvec_multi(Xf), ref, 'sparse matvec_multi')
    Xc = np.ascontiguousarray(Xf.T)
    for g in (op.dotMV(Xc), op*Xc, op.matvec(Xc)):
        assert g.shape == (SP_N, 5) and np.array_equal(g, ref.T)
    gt = op.matvec_multi(torch.from_numpy(Xf).cuda())
    assert isinstance(gt, torch.Tensor) and np.array_equal(gt.cpu().numpy(), ref)
    assert np.array_equal(op.matvec(Xf[0]), ref[0])                       # 1-D: pnl_spmv as before, exact data
    ctx.close()


@gpu
def test_interpolation_operator_block_products():
    """three synthetic dense node operators of 513^2.  Random data, weights from lagrangeWeights: matvec_multi within
    (n + 4 + m) u (|sum_j c_j A_j| |x|)_i of the longdouble reference (m = 3 more roundings for the combination).  Integer data
    with the coefficients (2, -1, 0.5): exact."""
    from pynucleus_amd.linear_operators import interpolationOperator
    n, m, k = 513, 3, 5
    ctx = _context()
    rng = np.random.default_rng(7700)
    nodes = np.array([0.2, 0.5, 0.8])
    As = [rtype(rng, (n, n)) for _ in range(m)]
    op = interpolationOperator([_dense_operator(ctx, A, pad=7) for A in As], nodes, 0.2, 0.8)
    op.set(0.37)
    assert op._fused() is not None
    X = rtype(rng, (k, n))
    got = op.matvec_multi(X)
    assert got.shape == (k, n)
    rows = subset_rows(n)
    if LD_OK:
        Cm = sum(LD(c)*A.astype(LD) for c, A in zip(op.coeffs, As))
        ref, mag = (Cm@X.astype(LD).T).T, (np.abs(Cm)@np.abs(X).astype(LD).T).T
    else:
        import mpmath
        Cm = np.array([[mpmath.fsum(mpmath.mpf(float(c))*mpmath.mpf(float(A[i, j])) for c, A in zip(op.coeffs, As)) for j in range(n)] for i in rows])
        ref = [[mpmath.fdot(Cm[a], [mpmath.mpf(float(v)) for v in x]) for a in range(len(rows))] for x in X]
        mag = [[mpmath.fdot([abs(v) for v in Cm[a]], [abs(mpmath.mpf(float(v))) for v in x]) for a in range(len(rows))] for x in X]
    _assert_block_rounding(got, rows, ref, mag, n+m, 1., 0., None, 'interpolationOperator.matvec_multi')
    assert np.array_equal(op.dotMV(np.ascontiguousarray(X.T)), got.T)
    # integer blocks, coefficients set by hand: exact
    Ai = [rng.integers(-1024, 1025, size=(n, n), dtype=np.int64) for _ in range(m)]
    iop = interpolationOperator([_dense_operator(ctx, A, pad=7) for A in Ai], nodes, 0.2, 0.8)
    iop.set(0.5)
    iop.coeffs = np.array([2., -1., 0.5])
    Xi = np.stack([exact_vector(rng, n) for _ in range(k)])
    want = sum(c*(Xi@A.T).astype(np.float64) for c, A in zip(iop.coeffs, Ai))
    _assert_block_exact(iop.matvec_multi(Xi.astype(np.float64)), want, 'interpolationOperator integer')
    ctx.close()


@gpu
def test_assembled_operators_block_products():
    """disc(3), P1, fractional kernel s = 0.75.  getDense: dotMV against toarray() @ X within the bound; solve_direct of the block
    product returns X with the backward bound of tests/test_cholesky.py for that solve (|b - A x| <= gamma_{3n+1} |L| |L^T| |x|).
    getH2: matvec_multi is the loop of matvec, bit for bit."""
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from test_cholesky import solve_violations, seeded_rows
    dm = P1_DoFMap(disc(3), PHYSICAL)
    kernel = getFractionalKernel(2, 0.75)
    A = nonlocalBuilder(dm, kernel, {'target_order': 0.5}, zeroExterior=True).getDense()
    n = A.num_rows
    X = np.random.default_rng(7800).standard_normal((5, n))
    Ah = A.toarray().copy()
    Y = A.dotMV(X)
    assert Y.shape == (5, n)
    rows = subset_rows(n)
    ref, mag = hp_products(Ah, X, rows)
    _assert_block_rounding(Y, rows, ref, mag, n, 1., 0., None, 'assembled dotMV')
    assert np.array_equal(A.matvec_multi(X), Y) and np.array_equal(A*np.ascontiguousarray(X.T), Y.T)
    Xs = A.solve_direct(Y)
    assert Xs.shape == (5, n) and A.symmetric
    cache = {}
    for v in range(5):
        bad, worst = solve_violations(Ah, A._chol.L, Y[v], Xs[v], seeded_rows(n), cache)
        assert not bad, (v, bad, worst)
    assert np.abs(Xs-X).max() <= 1e-6*np.abs(X).max()                     # a sanity check only (the bound above is the test)
    H = nonlocalBuilder(dm, kernel, {'target_order': 0.5, 'eta': 3., 'minClusterSize': 12}, zeroExterior=True).getH2()
    YH = H.matvec_multi(X)
    assert YH.shape == (5, n)
    for v in range(5):
        assert np.array_equal(YH[v], H.matvec(X[v])), v
    assert np.array_equal(H.dotMV(np.ascontiguousarray(X.T)), YH.T)
