"""The direct solver (pnl_potrf, pnl_potrs; csrc/pnl_direct.hip) through the C ABI on SYNTHETIC matrices built in numpy, in the manner of
tests/test_apply_kernels.py: no assembled operator, a bare context.

Kernels and their constants (csrc/pnl_direct.hip): k_chol_diag / k_chol_panel work on panels of NB = 64 columns, OB = 256 columns make
a block, k_direct_update<true> works in T x T = 64 x 64 workgroup tiles (once per panel inside the block, once per block on the rest);
k_direct_trsv_diag (L y = b, then L^T x = y), k_direct_sweep, k_chol_bwd_sweep walk block columns of NB.

(E) exact.  L0 integer lower triangular, off-diagonal entries in [-3, 3] with about half of them zero, diagonal in {1, 2, 4};
    A = L0 L0^T.  Every partial sum of the factorisation of entry (i, j), in any order and with or without FMA, MFMA accumulation
    included, is an integer of magnitude <= |a_ij| + sum_k |l_ik| |l_jk| <= 2 sqrt(r_i r_j) <= 2 max r, r_i = sum_k l_ik^2
    <= 9 (n - 1) + 16 (exact_bound proves 2 max r < 2^53 per case in int64); every square root is of a perfect square and every
    quotient an integer.  The Cholesky factor with positive diagonal is unique, so the device's lower triangle must equal L0 BIT FOR
    BIT.  The strict upper triangle, the padding columns and the elements around the buffer hold 2^30 and must still hold it.
    For x0 integer in [-8, 8] and b = A x0 the sweeps pass through the integers y = L0^T x0 and x0 (bounds proved by
    solve_bound), so pnl_potrs must return x0 bit for bit for every nrhs and ldb; one-hot right-hand sides name a wrong entry.
    For n > 513 the int64 product L0 L0^T is formed by the fp64 BLAS, which the proven bound makes exact, and seeded rows are
    checked against the int64 product.
(R) rounding.  A = D (G G^T + n I) D, G standard normal, D = diag(10^U(-3, 3)).  With u = 2^-53, gamma_k = k u / (1 - k u)
    (Higham, Accuracy and Stability of Numerical Algorithms, theorems 10.3, 10.4 with lemma 8.4 for any order of summation and FMA):
        factor  |A - L L^T|_ij <= gamma_{m+3} (|L| |L^T|)_ij,  m = min(i, j) + 1 products in the entry,
        solve   |b - A x|_i   <= gamma_{3n+1} (|L| |L^T| |x|)_i.
    No other tolerance.  Both sides are evaluated in np.longdouble where it has >= 63 mantissa bits (all rows for n <= 513, else
    >= 64 seeded rows that hold the first, the last and the block-edge rows), else in mpmath on the seeded rows.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NB, OB, T = 64, 256, 64                       # NB, OB, T of csrc/pnl_direct.hip
U = 2.**-53
LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
POISON = 2**30
FULL_ROWS_MAX = 513
SIZES = (1, 2, 3, 15, 16, 17, NB-1, NB, NB+1, 2*NB-1, 2*NB, 2*NB+1, 3*NB-1, 3*NB, 3*NB+1, OB-1, OB, 4*NB+1, 5*NB+1, 2*OB+1, 4161)
assert all(v in SIZES for v in (T-1, T+1, 2*T-1, 2*T+1)) and max(SIZES) <= 4161 and any(4*NB+1 <= v for v in SIZES)
LD_PADS = (0, 1, 6)
LDB_PADS = (0, 3)
NRHS = (1, 2, 5)
FAIL_PIVOTS = (0, NB-1, NB, 2*NB+5)


# ---- host helpers (tested below without a GPU) ------------------------------------------------------------------------------------

def gamma(k):
    return k*U/(1.-k*U)


def exact_factor(rng, n):
    """L0: integer lower triangular, off-diagonal in [-3, 3] with about half zero, diagonal in {1, 2, 4}"""
    L0 = np.tril(rng.integers(-3, 4, size=(n, n), dtype=np.int64)*rng.integers(0, 2, size=(n, n), dtype=np.int64), -1)
    L0[np.arange(n), np.arange(n)] = rng.choice(np.array([1, 2, 4], dtype=np.int64), size=n)
    return L0


def exact_bound(L0):
    """an upper bound, in exact integers, of every partial sum of every entry during the factorisation of L0 L0^T"""
    r = (L0*L0).sum(axis=1)
    return 2*int(r.max())


def exact_product(L0):
    """A = L0 L0^T as int64"""
    n = L0.shape[0]
    assert exact_bound(L0) < 2**53
    if n <= FULL_ROWS_MAX:
        return L0@L0.T
    Lf = L0.astype(np.float64)
    A = (Lf@Lf.T).astype(np.int64)            # exact: integer partial sums below 2^53 in any order
    rows = seeded_rows(n, 7)[:16]
    assert np.array_equal(A[rows], L0[rows]@L0.T)
    return A


def solve_bound(L0, x0):
    """an upper bound, in exact integers, of every partial sum of both sweeps for b = L0 L0^T x0"""
    y = L0.T@x0
    b = L0@y
    aL = np.abs(L0)
    return int(max((np.abs(b)+aL@np.abs(y)).max(), (np.abs(y)+aL.T@np.abs(x0)).max()))


def seeded_rows(n, seed=0):
    """all rows for n <= FULL_ROWS_MAX, else >= 64 rows: first, last, the edges of the panels, blocks and tiles, and random ones"""
    if n <= FULL_ROWS_MAX:
        return np.arange(n)
    fixed = [0, 1, NB-1, NB, NB+1, OB-1, OB, OB+1, n-NB-1, n-2, n-1, (n//OB)*OB-1, (n//OB)*OB, (n//NB)*NB-1, (n//NB)*NB]
    rnd = np.random.default_rng(seed).choice(n, size=64, replace=False).tolist()
    return np.unique(np.array([r for r in fixed+rnd if 0 <= r < n]))


def rounding_matrix(rng, n):
    G = rng.standard_normal((n, n))
    d = 10.**rng.uniform(-3., 3., size=n)
    A = (G@G.T+n*np.eye(n))*d[:, None]*d[None, :]
    return np.tril(A)+np.tril(A, -1).T


def _hp_dot(a, b):
    if LD_OK:
        return np.dot(a.astype(LD), b.astype(LD))
    import mpmath
    return mpmath.fdot([mpmath.mpf(float(v)) for v in a], [mpmath.mpf(float(v)) for v in b])


def _hp(v):
    if LD_OK:
        return LD(v)
    import mpmath
    return mpmath.mpf(float(v))


def factor_violations(A, L, rows):
    """entries (i, j), j <= i, i in rows, with |A - L L^T|_ij > gamma_{j+4} (|L| |L^T|)_ij: [(i, j, error, bound)] (at most 8) and the
    largest error / bound"""
    bad, worst = [], 0.
    L = np.tril(L)
    aL = np.abs(L)
    if LD_OK:
        Lh, aLh = L.astype(LD), aL.astype(LD)
        g = np.array([gamma(j+4) for j in range(L.shape[0])], dtype=LD)
        for i in rows:
            err = np.abs(A[i, :i+1].astype(LD)-Lh[:i+1, :i+1]@Lh[i, :i+1])
            bnd = g[:i+1]*(aLh[:i+1, :i+1]@aLh[i, :i+1])
            with np.errstate(invalid='ignore', divide='ignore'):
                ratio = np.where(bnd > 0, err/np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.))
            worst = max(worst, float(ratio.max()))
            for j in np.nonzero(~(err <= bnd))[0][:8]:
                bad.append((int(i), int(j), float(err[j]), float(bnd[j])))
    else:
        for i in rows:
            for j in range(i+1):
                err = abs(_hp(A[i, j])-_hp_dot(L[i, :j+1], L[j, :j+1]))
                bnd = gamma(j+4)*_hp_dot(aL[i, :j+1], aL[j, :j+1])
                if not err <= bnd:
                    bad.append((int(i), j, float(err), float(bnd)))
                worst = max(worst, float(err/bnd) if bnd > 0 else (np.inf if err > 0 else 0.))
    return bad[:8], worst


def solve_violations(A, L, b, x, rows, cache=None):
    """components i in rows with |b - A x|_i > gamma_{3n+1} (|L| |L^T| |x|)_i; cache: a dict that keeps |L|^T in high precision
    between the right-hand sides of one factor"""
    n = A.shape[0]
    L = np.tril(L)
    aL = np.abs(L)
    bad, worst = [], 0.
    if LD_OK:
        cache = {} if cache is None else cache
        if 'aLT' not in cache:
            cache['aLT'] = np.ascontiguousarray(aL.T).astype(LD)
        t = cache['aLT']@np.abs(x).astype(LD)
        xh = x.astype(LD)
    else:
        t = [_hp_dot(aL[:, k], np.abs(x)) for k in range(n)]
    for i in rows:
        if LD_OK:
            err = abs(LD(b[i])-np.dot(A[i].astype(LD), xh))
            bnd = gamma(3*n+1)*np.dot(aL[i].astype(LD), t)
        else:
            import mpmath
            err = abs(_hp(b[i])-_hp_dot(A[i], x))
            bnd = gamma(3*n+1)*mpmath.fdot([_hp(v) for v in aL[i]], t)
        if not err <= bnd:
            bad.append((int(i), float(err), float(bnd)))
        worst = max(worst, float(err/bnd) if bnd > 0 else (np.inf if err > 0 else 0.))
    return bad[:8], worst


# ---- CPU tests of the helpers -------------------------------------------------------------------------------------------------------

def test_sizes_cover_the_block_edges():
    for k in (1, 2, 3):
        assert {k*NB-1, k*NB, k*NB+1} <= set(SIZES)
    assert {1, 2, 3, 15, 16, 17, T-1, T+1, 2*T-1, 2*T+1, OB-1, OB, OB+1, 4161} <= set(SIZES)
    assert max(FAIL_PIVOTS) < 4*NB+1


@pytest.mark.parametrize('n', SIZES)
def test_exact_data_is_exact_and_stays_below_2_53(n):
    rng = np.random.default_rng(4000+n)
    L0 = exact_factor(rng, n)
    assert exact_bound(L0) <= 2*(9*(n-1)+16) < 2**53
    assert set(np.unique(np.diagonal(L0))) <= {1, 2, 4} and np.abs(np.tril(L0, -1)).max(initial=0) <= 3 and not np.triu(L0, 1).any()
    if n >= 64:
        frac = (np.tril(L0, -1) == 0).sum()-n*(n+1)//2
        assert 0.4 < frac/(n*(n-1)//2) < 0.75              # about half of the strict lower triangle is zero (4 of 7 values times 1/2 ...)
    x0 = rng.integers(-8, 9, size=n, dtype=np.int64)
    assert solve_bound(L0, x0) < 2**53
    if n <= FULL_ROWS_MAX:
        A = exact_product(L0)
        # the fp64 factor of the exact data is L0 itself: numpy's Cholesky (LAPACK, another order of summation) agrees bit for bit
        assert np.array_equal(np.linalg.cholesky(A.astype(np.float64)), L0.astype(np.float64))


def test_exact_product_by_blas_equals_int64_product():
    L0 = exact_factor(np.random.default_rng(5), 600)
    assert np.array_equal(exact_product(L0), L0@L0.T)


def test_rounding_bounds_hold_for_fp64_and_not_for_fp32():
    rng = np.random.default_rng(11)
    n = 193
    A = rounding_matrix(rng, n)
    L = np.linalg.cholesky(A)
    rows = seeded_rows(n)
    bad, worst = factor_violations(A, L, rows)
    assert not bad and worst < 1., (bad, worst)
    L32 = L.astype(np.float32).astype(np.float64)
    bad32, worst32 = factor_violations(A, L32, rows)
    assert bad32 and worst32 > 1e3, worst32                 # a factor rounded to fp32 breaks the bound by orders of magnitude
    b = rng.standard_normal(n)
    import scipy.linalg as sl
    x = sl.solve_triangular(L, sl.solve_triangular(L, b, lower=True), lower=True, trans='T')
    bad, worst = solve_violations(A, L, b, x, rows)
    assert not bad and worst < 1., (bad, worst)
    x32 = x.astype(np.float32).astype(np.float64)
    assert solve_violations(A, L, b, x32, rows)[0]


def test_seeded_rows():
    assert np.array_equal(seeded_rows(513), np.arange(513))
    r = seeded_rows(4161)
    assert r.shape[0] >= 64 and {0, 4160, NB-1, NB, OB-1, OB, 4095, 4096} <= set(r.tolist())


def test_abi_names_exist():
    import os
    from pynucleus_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnl_hip.h')).read()
    for name in ('pnl_potrf', 'pnl_potrs'):
        assert name in _lib.EXPORTS and 'int {}('.format(name) in hdr, name
    assert hasattr(_lib.Context, 'potrf') and hasattr(_lib.Context, 'potrs')


# ---- device plumbing ----------------------------------------------------------------------------------------------------------------

def _context():
    import torch
    from pynucleus_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream(0).cuda_stream)
    return ctx


def _dev_lower(A, ld):
    """(storage, view): the lower triangle of A at an ODD double offset of a poisoned allocation with leading dimension ld; the strict
    upper triangle, the padding columns and the elements before / after hold 2^30"""
    import torch
    n = A.shape[0]
    host = np.full((n, ld), float(POISON))
    host[:, :n] = np.where(np.tri(n, dtype=bool), A.astype(np.float64), float(POISON))
    store = torch.full((1+n*ld+1,), float(POISON), dtype=torch.float64, device='cuda')
    view = store[1:1+n*ld].view(n, ld)
    view.copy_(torch.from_numpy(host))
    return store, view


def _lower_and_guards(ctx, store, n, ld, what):
    """the lower triangle back on the host; everything else must still hold the poison"""
    ctx.synchronize()
    h = store.cpu().numpy()
    assert h[0] == POISON and h[-1] == POISON, what+': write outside the buffer'
    M = h[1:1+n*ld].reshape(n, ld)
    assert (M[:, n:] == POISON).all(), what+': write into the padding columns'
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    assert (M[:, :n][up] == POISON).all(), what+': write above the diagonal'
    return np.tril(M[:, :n])


def _dev_rhs(Bm, ldb):
    """(storage, view): the rows of Bm [nrhs, n] with stride ldb, 2^30 between and around them"""
    import torch
    nrhs, n = Bm.shape
    host = np.full(1+nrhs*ldb+1, float(POISON))
    V = host[1:1+nrhs*ldb].reshape(nrhs, ldb)
    V[:, :n] = Bm
    store = torch.from_numpy(host).cuda()
    return store, store[1:1+nrhs*ldb].view(nrhs, ldb)


def _rhs_back(ctx, store, nrhs, n, ldb, what):
    ctx.synchronize()
    h = store.cpu().numpy()
    assert h[0] == POISON and h[-1] == POISON, what+': write outside the right-hand sides'
    V = h[1:1+nrhs*ldb].reshape(nrhs, ldb)
    assert (V[:, n:] == POISON).all(), what+': write between the right-hand sides'
    return V[:, :n].copy()


def _assert_same(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError('{}: {} of {} entries differ, first at {}: got {!r}, expected {!r}'.format(
            what, bad.shape[0], ref.size, bad[:6].tolist(), [float(got[tuple(b)]) for b in bad[:4]], [float(ref[tuple(b)]) for b in bad[:4]]))


def _potrs(ctx, Lv, n, ld, Bm, ldb, what):
    bs, bv = _dev_rhs(Bm, ldb)
    ctx.potrs(Lv.data_ptr(), ld, n, bv.data_ptr(), ldb, Bm.shape[0])
    return _rhs_back(ctx, bs, Bm.shape[0], n, ldb, what)


# ---- (E) ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', SIZES)
def test_potrf_potrs_exact(n):
    """(E): the factor equals L0 bit for bit for ld = n, n + 1, n + 6 at an odd base, the guards hold; pnl_potrs returns x0 bit for
    bit for nrhs = 1, 2, 5 and ldb = n, n + 3.  A one-hot right-hand side has no integer solution (L0^-1 e_k has denominators up to
    4^(n-k)), so the one-hot vectors at 0, NB - 1, NB, n - 1 are the SOLUTIONS here (b = A e_k, a wrong component names the entry) and
    right-hand sides in the (R) test"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(4000+n)
    L0 = exact_factor(rng, n)
    A = exact_product(L0)
    hot = sorted({k for k in (0, NB-1, NB, n-1) if 0 <= k < n})
    Xall = rng.integers(-8, 9, size=(max(NRHS), n), dtype=np.int64)
    assert max(solve_bound(L0, x) for x in Xall) < 2**53
    Ball = (Xall@A.T).astype(np.float64)
    for pad in LD_PADS:
        ld = n+pad
        tag = 'n={} ld=n+{}'.format(n, pad)
        store, Av = _dev_lower(A, ld)
        info = ctx.potrf(Av.data_ptr(), ld, n)
        assert info == 0, (tag, info)
        _assert_same(_lower_and_guards(ctx, store, n, ld, tag), L0, tag+' factor (entry (i, j) of L)')
        for nrhs in NRHS:
            for bpad in LDB_PADS:
                X0 = Xall[:nrhs]
                what = '{} nrhs={} ldb=n+{}'.format(tag, nrhs, bpad)
                _assert_same(_potrs(ctx, Av, n, ld, Ball[:nrhs], n+bpad, what), X0, what+' (vector, component)')
        E = np.zeros((len(hot), n), dtype=np.int64)
        E[np.arange(len(hot)), hot] = 1
        what = tag+' one-hot solutions at {}'.format(hot)
        _assert_same(_potrs(ctx, Av, n, ld, (E@A.T).astype(np.float64), n+3, what), E, what+' (k-th vector, component)')
        # nothing of the factor was written by the solves
        _assert_same(_lower_and_guards(ctx, store, n, ld, tag+' after the solves'), L0, tag+' factor after the solves')
        del store, Av
    ctx.close()
    torch.cuda.empty_cache()


# ---- (R) ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', SIZES)
def test_potrf_potrs_rounding(n):
    """(R): the two textbook bounds, nothing else, over the whole grid ld = n, n + 1, n + 6 x ldb = n, n + 3 x nrhs = 1, 2, 5 plus the
    one-hot right-hand sides at 0, NB - 1, NB, n - 1.  The bounds are evaluated once per distinct result: no kernel has a path that
    depends on ld, ldb, nrhs or an alignment, so the factor of every ld and the solution of a right-hand side in every (ld, ldb, nrhs)
    must repeat the bits of the first one, for which the bound was evaluated (bit equality asks more than the bound, never less)"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(6000+n)
    A = rounding_matrix(rng, n)
    rows = seeded_rows(n, n)
    hot = sorted({k for k in (0, NB-1, NB, n-1) if 0 <= k < n})
    Bm = rng.standard_normal((max(NRHS), n))*10.**rng.uniform(-3., 3., size=(max(NRHS), n))
    Eh = np.zeros((len(hot), n))
    Eh[np.arange(len(hot)), hot] = 1.                          # one-hot right-hand sides: columns of A^-1
    L, cache, seen = None, {}, {}

    def check(key, b, x, what):
        if key in seen:
            _assert_same(x, seen[key], what+': bits differ from the first solve of this right-hand side')
            return
        bad, worst = solve_violations(A, L, b, x, rows, cache)
        print('{} solve: largest error / bound {:.3e}'.format(what, worst))
        assert not bad, '{}: |b - A x| above gamma_(3n+1) |L||L^T||x| at (i, error, bound) {}'.format(what, bad)
        seen[key] = x.copy()

    for pad in LD_PADS:
        ld = n+pad
        tag = 'n={} ld=n+{}'.format(n, pad)
        store, Av = _dev_lower(A, ld)
        info = ctx.potrf(Av.data_ptr(), ld, n)
        assert info == 0, (tag, info)
        Lg = _lower_and_guards(ctx, store, n, ld, tag)
        if L is None:
            L = Lg
            assert (np.diagonal(L) > 0).all()
            bad, worst = factor_violations(A, L, rows)
            print('{} factor: largest error / bound {:.3e}'.format(tag, worst))
            assert not bad, '{}: |A - L L^T| above gamma_(m+3) |L||L^T| at (i, j, error, bound) {}'.format(tag, bad)
        else:
            _assert_same(Lg, L, tag+': bits of the factor differ from those of ld = n')
        for nrhs in NRHS:
            for bpad in LDB_PADS:
                what = '{} nrhs={} ldb=n+{}'.format(tag, nrhs, bpad)
                X = _potrs(ctx, Av, n, ld, Bm[:nrhs], n+bpad, what)
                for r in range(nrhs):
                    check(('b', r), Bm[r], X[r], what+' vector {}'.format(r))
        X = _potrs(ctx, Av, n, ld, Eh, n+3, tag+' one-hot')
        for r, k in enumerate(hot):
            check(('e', k), Eh[r], X[r], tag+' b = e_{}'.format(k))
        del store, Av
    ctx.close()
    torch.cuda.empty_cache()


# ---- failure path ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('kind', ['nonpositive', 'nan'])
@pytest.mark.parametrize('k', FAIL_PIVOTS)
def test_potrf_reports_the_first_bad_pivot(k, kind):
    """pivot k of an (E) matrix made <= 0 (0 for even k, -1 for odd k) or NaN: info = k + 1, no write outside the lower triangle, and
    the columns before k still hold L0 (they are finished before pivot k is looked at)"""
    import torch
    ctx = _context()
    n = 4*NB+1
    rng = np.random.default_rng(7000+k)
    L0 = exact_factor(rng, n)
    A = exact_product(L0).astype(np.float64)
    A[k, k] = np.nan if kind == 'nan' else A[k, k]-float(L0[k, k]**2+(k % 2))
    for pad in (0, 1):
        store, Av = _dev_lower(A, n+pad)
        info = ctx.potrf(Av.data_ptr(), n+pad, n)
        Lg = _lower_and_guards(ctx, store, n, n+pad, 'bad pivot {}'.format(k))
        assert info == k+1, (k, kind, info)
        _assert_same(Lg[:, :k], L0[:, :k], 'columns before the bad pivot {}'.format(k))
        del store, Av
    ctx.close()
    torch.cuda.empty_cache()


@gpu
def test_potrf_potrs_argument_checks():
    import ctypes as C
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    A = torch.full((8, 8), float(POISON), dtype=torch.float64, device='cuda')
    b = torch.full((8,), float(POISON), dtype=torch.float64, device='cuda')
    info = C.c_int(-7)
    P = C.c_void_p
    assert ctx.L.pnl_potrf(ctx.h, P(A.data_ptr()), 7, 8, C.byref(info)) == _lib.PNL_ERR_INVALID          # ldA < n
    assert ctx.L.pnl_potrf(ctx.h, P(A.data_ptr()), 8, -1, C.byref(info)) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrf(ctx.h, None, 8, 8, C.byref(info)) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrf(ctx.h, P(A.data_ptr()), 8, 8, None) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrf(ctx.h, None, 0, 0, C.byref(info)) == _lib.PNL_OK and info.value == 0         # n = 0: a no-op
    assert ctx.L.pnl_potrs(ctx.h, P(A.data_ptr()), 7, 8, P(b.data_ptr()), 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrs(ctx.h, P(A.data_ptr()), 8, 8, P(b.data_ptr()), 7, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrs(ctx.h, P(A.data_ptr()), 8, 8, None, 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_potrs(ctx.h, P(A.data_ptr()), 8, 0, P(b.data_ptr()), 8, 1) == _lib.PNL_OK
    ctx.synchronize()
    assert (A.cpu().numpy() == POISON).all() and (b.cpu().numpy() == POISON).all()
    ctx.close()
