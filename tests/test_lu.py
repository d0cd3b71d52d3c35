"""The pivoted direct solver (pnl_getrf, pnl_getrs; csrc/pnl_direct.hip) through the C ABI on SYNTHETIC matrices built in numpy, in the
manner of tests/test_cholesky.py: no assembled operator, a bare context.

Kernels and their constants (csrc/pnl_direct.hip): k_lu_step works on panels of NB = 64 columns, RB = 64 rows per workgroup; OB = 256
columns make a block; k_direct_update<false> works in T x T = 64 x 64 tiles and stages KC = 32 columns of k per step; k_lu_swap /
k_lu_u12 take 256 columns per workgroup; k_lu_gather, k_direct_trsv_diag (L y = P b, then U x = y), k_direct_sweep walk block columns
of NB.

(E) exact.  L0 unit lower triangular, off-diagonal entries in {0, +-1/4, +-1/2} with about half of them zero; U0 upper triangular,
    off-diagonal entries 4 {-3 .. 3} with about half of them zero, diagonal in +-{4, 8, 16}; A = (L0 U0) with its rows scattered by a
    seeded permutation.  Every product l u is an integer, so every partial sum of the factorisation, in any order and with FMA or MFMA
    accumulation, is an integer of magnitude <= 2 max(|L0| |U0|) (exact_bound proves < 2^53 per case).  At step k the candidates are
    u_kk and l_ik u_kk with |l| <= 1/2: the pivot is unique; each quotient is a dyadic number and exact.  The device must return L0 and
    U0 BIT FOR BIT, the swap sequence of that permutation, and leave the 2^30 in the padding columns and around the buffer alone.
    For x0 integer in [-8, 8] and b = A x0 the sweeps pass through multiples of 1/4 (y = U0 x0 is integer; solve_bound proves the
    magnitudes), so pnl_getrs must return x0 bit for bit for every nrhs and ldb; one-hot solutions name a wrong entry.
(R) rounding.  A = D1 G D2, G standard normal, D = diag(10^U(-3, 3)): the row scaling forces real pivoting.  piv must be a valid swap
    sequence, every |l_ik| <= 1, and with the device's own permutation, u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and
    Stability of Numerical Algorithms, theorems 9.3, 9.4):
        factor  |P A - L U|_ij <= gamma_{m+3} (|L| |U|)_ij,  m = min(i, j) + 1 products in the entry,
        solve   |P b - P A x|_i <= gamma_{3n+1} (|L| |U| |x|)_i.
    No other tolerance.  Both sides are evaluated in np.longdouble where it has >= 63 mantissa bits (all rows for n <= 513, else seeded
    rows that hold the first, the last and the block-edge rows), else in mpmath on the seeded rows.  Pivots are not compared with
    LAPACK's (near-ties may differ legitimately); factoring the same input twice gives identical bits and pivots.
"""
import numpy as np
import pytest

from test_cholesky import gamma, LD, LD_OK, POISON, _hp, _hp_dot, _context, _dev_rhs, _rhs_back, _assert_same

gpu = pytest.mark.gpu

NB, OB, T, KC, RB = 64, 256, 64, 32, 64         # NB, OB, T, KC, RB of csrc/pnl_direct.hip
FULL_ROWS_MAX = 513
LARGE = 2081                                    # 8 blocks and a narrow last panel
SIZES = tuple(sorted({1, 2, 3, 15, 16, 17, LARGE, 4*NB+1, 2*OB+1} | {v for w in (NB, OB, T, KC, RB) for v in (w-1, w, w+1, 2*w-1, 2*w+1)}))
assert max(SIZES) <= 4161
LD_PADS = (0, 1, 6)
LDB_PADS = (0, 3)
NRHS = (1, 2, 5)
FAIL_PIVOTS = (0, NB-1, NB, 2*NB+5)
PIV_GUARD = -77


# ---- host helpers (tested below without a GPU) ------------------------------------------------------------------------------------

def exact_factors(rng, n):
    """(L0, U0, perm): the (E) factors as float64 and the row order with A[perm] = L0 U0"""
    half = lambda: rng.integers(0, 2, size=(n, n))                                              # noqa: E731
    L0 = np.tril(rng.choice(np.array([-0.5, -0.25, 0.25, 0.5]), size=(n, n))*half(), -1)+np.eye(n)
    U0 = np.triu(4.*rng.integers(-3, 4, size=(n, n))*half(), 1)
    U0[np.arange(n), np.arange(n)] = rng.choice(np.array([4., 8., 16.]), size=n)*rng.choice(np.array([-1., 1.]), size=n)
    return L0, U0, rng.permutation(n)


def exact_bound(L0, U0):
    """an upper bound of every partial sum of every entry during the factorisation of L0 U0 (all of them integers)"""
    return 2.*float((np.abs(L0)@np.abs(U0)).max())


def exact_matrix(L0, U0, perm):
    """A with A[perm] = L0 U0; the fp64 product is exact: integer partial sums below 2^53 in any order"""
    assert exact_bound(L0, U0) < 2.**53
    LU = L0@U0
    assert np.array_equal(LU, np.rint(LU))
    A = np.empty_like(LU)
    A[perm] = LU
    return A


def swaps_of(perm):
    """the swap sequence piv (k <= piv[k]) that brings the rows into the order perm: rows k and piv[k] exchanged at step k"""
    n = perm.shape[0]
    at = np.arange(n)                    # at[i]: the original row now at position i
    where = np.arange(n)                 # where[r]: the position of original row r
    piv = np.empty(n, dtype=np.int32)
    for k in range(n):
        p = where[perm[k]]
        piv[k] = p
        a, b = at[k], at[p]
        at[k], at[p] = b, a
        where[a], where[b] = p, k
    return piv


def perm_of(piv):
    """the row order of a swap sequence: A[perm] = L U"""
    perm = np.arange(len(piv))
    for k, p in enumerate(piv):
        perm[k], perm[p] = perm[p], perm[k]
    return perm


def solve_bound(L0, U0, x0):
    """an upper bound of every partial sum of both sweeps for b = A x0 (all of them multiples of 1/4)"""
    y = U0@x0
    return float(max((np.abs(L0)@np.abs(y)).max(), (np.abs(U0)@np.abs(x0)).max()))*2.


def seeded_rows(n, seed=0):
    """all rows for n <= FULL_ROWS_MAX, else the first, the last, the edges of the panels and blocks, and 24 random ones"""
    if n <= FULL_ROWS_MAX:
        return np.arange(n)
    fixed = [0, 1, NB-1, NB, NB+1, OB-1, OB, OB+1, n-NB-1, n-2, n-1, (n//OB)*OB-1, (n//OB)*OB, (n//NB)*NB-1, (n//NB)*NB]
    rnd = np.random.default_rng(seed).choice(n, size=24, replace=False).tolist()
    return np.unique(np.array([r for r in fixed+rnd if 0 <= r < n]))


def rounding_matrix(rng, n):
    G = rng.standard_normal((n, n))
    return G*(10.**rng.uniform(-3., 3., size=n))[:, None]*(10.**rng.uniform(-3., 3., size=n))[None, :]


def split(M):
    """(L with its unit diagonal, U) of the block pnl_getrf leaves"""
    return np.tril(M, -1)+np.eye(M.shape[0]), np.triu(M)


def factor_violations(A, L, U, perm, rows):
    """entries (i, j), i in rows, with |P A - L U|_ij > gamma_{min(i, j) + 4} (|L| |U|)_ij: [(i, j, error, bound)] (at most 8) and the
    largest error / bound"""
    n = A.shape[0]
    bad, worst = [], 0.
    aL, aU = np.abs(L), np.abs(U)
    if LD_OK:
        Uh, aUh = U.astype(LD), aU.astype(LD)
        for i in rows:
            g = np.array([gamma(min(i, j)+4) for j in range(n)], dtype=LD)
            err = np.abs(A[perm[i]].astype(LD)-L[i, :i+1].astype(LD)@Uh[:i+1])
            bnd = g*(aL[i, :i+1].astype(LD)@aUh[:i+1])
            with np.errstate(invalid='ignore', divide='ignore'):
                ratio = np.where(bnd > 0, err/np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.))
            worst = max(worst, float(ratio.max()))
            for j in np.nonzero(~(err <= bnd))[0][:8]:
                bad.append((int(i), int(j), float(err[j]), float(bnd[j])))
    else:
        for i in rows:
            for j in range(n):
                m = min(i, j)+1
                err = abs(_hp(A[perm[i], j])-_hp_dot(L[i, :m], U[:m, j]))
                bnd = gamma(m+3)*_hp_dot(aL[i, :m], aU[:m, j])
                if not err <= bnd:
                    bad.append((int(i), j, float(err), float(bnd)))
                worst = max(worst, float(err/bnd) if bnd > 0 else (np.inf if err > 0 else 0.))
    return bad[:8], worst


def solve_violations(A, L, U, perm, b, x, rows, cache=None):
    """components i in rows with |P b - P A x|_i > gamma_{3n+1} (|L| |U| |x|)_i; cache: a dict that keeps |U| in high precision between
    the right-hand sides of one factor"""
    n = A.shape[0]
    aL, aU = np.abs(L), np.abs(U)
    bad, worst = [], 0.
    if LD_OK:
        cache = {} if cache is None else cache
        if 'aU' not in cache:
            cache['aU'] = aU.astype(LD)
        t = cache['aU']@np.abs(x).astype(LD)
        xh = x.astype(LD)
    else:
        t = [_hp_dot(aU[k], np.abs(x)) for k in range(n)]
    for i in rows:
        if LD_OK:
            err = abs(LD(b[perm[i]])-np.dot(A[perm[i]].astype(LD), xh))
            bnd = gamma(3*n+1)*np.dot(aL[i].astype(LD), t)
        else:
            import mpmath
            err = abs(_hp(b[perm[i]])-_hp_dot(A[perm[i]], x))
            bnd = gamma(3*n+1)*mpmath.fdot([_hp(v) for v in aL[i]], t)
        if not err <= bnd:
            bad.append((int(i), float(err), float(bnd)))
        worst = max(worst, float(err/bnd) if bnd > 0 else (np.inf if err > 0 else 0.))
    return bad[:8], worst


def valid_swaps(piv, n):
    return piv.shape == (n,) and bool((piv >= np.arange(n)).all() and (piv < n).all())


# ---- CPU tests of the helpers -------------------------------------------------------------------------------------------------------

def test_sizes_cover_the_block_edges():
    for w in (NB, OB, T, KC, RB):
        assert {w-1, w, w+1, 2*w-1, 2*w+1} <= set(SIZES)
    assert {1, 2, 3, 15, 16, 17} <= set(SIZES) and any(v >= 4*NB+1 for v in SIZES) and any(v >= 2*OB+1 for v in SIZES)
    assert max(FAIL_PIVOTS) < 4*NB+1


@pytest.mark.parametrize('n', [v for v in SIZES if v <= FULL_ROWS_MAX])
def test_exact_data_is_exact_and_lapack_reproduces_it(n):
    import scipy.linalg as sl
    rng = np.random.default_rng(8000+n)
    L0, U0, perm = exact_factors(rng, n)
    assert exact_bound(L0, U0) < 2.**53
    assert np.array_equal(np.diagonal(L0), np.ones(n)) and not np.triu(L0, 1).any() and not np.tril(U0, -1).any()
    assert set(np.unique(np.tril(L0, -1))) <= {-0.5, -0.25, 0., 0.25, 0.5} and set(np.unique(np.abs(np.diagonal(U0)))) <= {4., 8., 16.}
    assert set(np.unique(np.triu(U0, 1))) <= set(4.*np.arange(-3, 4))
    if n >= 64:
        for M, k in ((np.tril(L0, -1), -1), (np.triu(U0, 1).T, -1)):
            zeros = (M[np.tri(n, k=k, dtype=bool)] == 0).mean()
            assert 0.4 < zeros < 0.75, zeros
    A = exact_matrix(L0, U0, perm)
    piv = swaps_of(perm)
    assert valid_swaps(piv, n) and np.array_equal(perm_of(piv), perm)
    lu, lpiv = sl.lu_factor(A)
    assert np.array_equal(lpiv, piv)
    L, U = split(lu)
    assert np.array_equal(L, L0) and np.array_equal(U, U0)
    x0 = rng.integers(-8, 9, size=n).astype(np.float64)
    assert solve_bound(L0, U0, x0) < 2.**51
    assert np.array_equal(sl.lu_solve((lu, lpiv), A@x0), x0)


def test_rounding_bounds_hold_for_fp64_and_not_for_fp32():
    import scipy.linalg as sl
    rng = np.random.default_rng(12)
    n = 193
    A = rounding_matrix(rng, n)
    lu, piv = sl.lu_factor(A)
    L, U = split(lu)
    perm = perm_of(piv)
    rows = seeded_rows(n)
    assert np.abs(np.tril(lu, -1)).max() <= 1. and not np.array_equal(perm, np.arange(n))
    bad, worst = factor_violations(A, L, U, perm, rows)
    assert not bad and worst < 1., (bad, worst)
    bad32, worst32 = factor_violations(A, L, U.astype(np.float32).astype(np.float64), perm, rows)
    assert bad32 and worst32 > 1e3, worst32
    wrong = perm.copy()
    wrong[[0, 1]] = wrong[[1, 0]]
    assert factor_violations(A, L, U, wrong, rows)[0]                     # another permutation breaks it
    b = rng.standard_normal(n)
    x = sl.lu_solve((lu, piv), b)
    bad, worst = solve_violations(A, L, U, perm, b, x, rows)
    assert not bad and worst < 1., (bad, worst)
    assert solve_violations(A, L, U, perm, b, x.astype(np.float32).astype(np.float64), rows)[0]


def test_seeded_rows_and_swaps():
    assert np.array_equal(seeded_rows(513), np.arange(513))
    r = seeded_rows(LARGE)
    assert r.shape[0] >= 24 and {0, LARGE-1, NB-1, NB, OB-1, OB} <= set(r.tolist())
    perm = np.random.default_rng(1).permutation(50)
    x = np.arange(50.)
    y = x.copy()
    for k, p in enumerate(swaps_of(perm)):
        y[[k, p]] = y[[p, k]]
    assert np.array_equal(y, x[perm])


# ---- device plumbing ----------------------------------------------------------------------------------------------------------------

def _dev_full(A, ld):
    """(storage, view): A at an ODD double offset of a poisoned allocation with leading dimension ld"""
    import torch
    n = A.shape[0]
    host = np.full((n, ld), float(POISON))
    host[:, :n] = A
    store = torch.full((1+n*ld+1,), float(POISON), dtype=torch.float64, device='cuda')
    view = store[1:1+n*ld].view(n, ld)
    view.copy_(torch.from_numpy(host))
    return store, view


def _dev_piv(n):
    import torch
    store = torch.full((n+2,), PIV_GUARD, dtype=torch.int32, device='cuda')
    return store, store[1:1+n]


def _block_and_guards(ctx, store, pstore, n, ld, what):
    """the n x n block and the swap sequence back on the host; everything else must still hold the poison"""
    ctx.synchronize()
    h = store.cpu().numpy()
    assert h[0] == POISON and h[-1] == POISON, what+': write outside the buffer'
    M = h[1:1+n*ld].reshape(n, ld)
    assert (M[:, n:] == POISON).all(), what+': write into the padding columns'
    p = pstore.cpu().numpy()
    assert p[0] == PIV_GUARD and p[-1] == PIV_GUARD, what+': write outside piv'
    return M[:, :n].copy(), p[1:-1].copy()


def _getrf(ctx, A, ld, what):
    store, Av = _dev_full(A, ld)
    pstore, pv = _dev_piv(A.shape[0])
    info = ctx.getrf(Av.data_ptr(), ld, A.shape[0], pv.data_ptr())
    M, piv = _block_and_guards(ctx, store, pstore, A.shape[0], ld, what)
    return info, M, piv, (store, Av, pstore, pv)


def _getrs(ctx, Av, pv, n, ld, Bm, ldb, what):
    bs, bv = _dev_rhs(Bm, ldb)
    ctx.getrs(Av.data_ptr(), ld, n, pv.data_ptr(), bv.data_ptr(), ldb, Bm.shape[0])
    return _rhs_back(ctx, bs, Bm.shape[0], n, ldb, what)


# ---- (E) ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', SIZES)
def test_getrf_getrs_exact(n):
    """(E): the block equals L0 \\ U0 bit for bit and piv the swap sequence of the permutation for ld = n, n + 1, n + 6 at an odd base,
    the guards hold; pnl_getrs returns x0 bit for bit for nrhs = 1, 2, 5 and ldb = n, n + 3.  The one-hot vectors at 0, NB - 1, NB,
    n - 1 are SOLUTIONS here (b = A e_k: a wrong component names the entry) and right-hand sides in the (R) test"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(8000+n)
    L0, U0, perm = exact_factors(rng, n)
    A = exact_matrix(L0, U0, perm)
    piv0 = swaps_of(perm)
    ref = np.tril(L0, -1)+U0
    hot = sorted({k for k in (0, NB-1, NB, n-1) if 0 <= k < n})
    Xall = rng.integers(-8, 9, size=(max(NRHS), n)).astype(np.float64)
    assert max(solve_bound(L0, U0, x) for x in Xall) < 2.**51
    Ball = Xall@A.T
    for pad in LD_PADS:
        ld = n+pad
        tag = 'n={} ld=n+{}'.format(n, pad)
        info, M, piv, (store, Av, pstore, pv) = _getrf(ctx, A, ld, tag)
        assert info == 0, (tag, info)
        _assert_same(piv.astype(np.float64), piv0, tag+' swap sequence (step)')
        _assert_same(M, ref, tag+' factors (entry (i, j) of L \\ U)')
        for nrhs in NRHS:
            for bpad in LDB_PADS:
                what = '{} nrhs={} ldb=n+{}'.format(tag, nrhs, bpad)
                _assert_same(_getrs(ctx, Av, pv, n, ld, Ball[:nrhs], n+bpad, what), Xall[:nrhs], what+' (vector, component)')
        E = np.zeros((len(hot), n))
        E[np.arange(len(hot)), hot] = 1.
        what = tag+' one-hot solutions at {}'.format(hot)
        _assert_same(_getrs(ctx, Av, pv, n, ld, E@A.T, n+3, what), E, what+' (k-th vector, component)')
        # nothing of the factors was written by the solves
        M2, piv2 = _block_and_guards(ctx, store, pstore, n, ld, tag+' after the solves')
        _assert_same(M2, ref, tag+' factors after the solves')
        assert np.array_equal(piv2, piv0)
        del store, Av, pstore, pv
    ctx.close()
    torch.cuda.empty_cache()


# ---- (R) ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', SIZES)
def test_getrf_getrs_rounding(n):
    """(R): a valid swap sequence, |l| <= 1 and the two textbook bounds, nothing else, over the whole grid ld = n, n + 1, n + 6 x
    ldb = n, n + 3 x nrhs = 1, 2, 5 plus the one-hot right-hand sides at 0, NB - 1, NB, n - 1.  The bounds are evaluated once per
    distinct result: no kernel has a path that depends on ld, ldb, nrhs or an alignment, so the factors of every ld (the second
    factorisation of the same input among them) and the solution of a right-hand side in every (ld, ldb, nrhs) must repeat the bits
    of the first one, for which the bound was evaluated (bit equality asks more than the bound, never less)"""
    import torch
    ctx = _context()
    rng = np.random.default_rng(9000+n)
    A = rounding_matrix(rng, n)
    rows = seeded_rows(n, n)
    hot = sorted({k for k in (0, NB-1, NB, n-1) if 0 <= k < n})
    Bm = rng.standard_normal((max(NRHS), n))*10.**rng.uniform(-3., 3., size=(max(NRHS), n))
    Eh = np.zeros((len(hot), n))
    Eh[np.arange(len(hot)), hot] = 1.
    first, cache, seen = None, {}, {}

    def check(key, b, x, what):
        if key in seen:
            _assert_same(x, seen[key], what+': bits differ from the first solve of this right-hand side')
            return
        M, piv, L, U, perm = first
        bad, worst = solve_violations(A, L, U, perm, b, x, rows, cache)
        print('{} solve: largest error / bound {:.3e}'.format(what, worst))
        assert not bad, '{}: |P b - P A x| above gamma_(3n+1) |L||U||x| at (i, error, bound) {}'.format(what, bad)
        seen[key] = x.copy()

    for pad in LD_PADS+(0,):
        ld = n+pad
        tag = 'n={} ld=n+{}'.format(n, pad)
        info, M, piv, (store, Av, pstore, pv) = _getrf(ctx, A, ld, tag)
        assert info == 0, (tag, info)
        if first is None:
            assert valid_swaps(piv, n), piv
            L, U = split(M)
            assert np.abs(np.tril(M, -1)).max(initial=0.) <= 1., 'a multiplier above 1: the pivot was not the largest entry'
            perm = perm_of(piv)
            first = (M, piv, L, U, perm)
            bad, worst = factor_violations(A, L, U, perm, rows)
            print('{} factor: largest error / bound {:.3e}, {} interchanges'.format(tag, worst, int((piv != np.arange(n)).sum())))
            assert not bad, '{}: |P A - L U| above gamma_(m+3) |L||U| at (i, j, error, bound) {}'.format(tag, bad)
        else:
            assert np.array_equal(piv, first[1]), tag+': the swap sequence differs from that of the first factorisation'
            _assert_same(M, first[0], tag+': bits of the factors differ from those of the first factorisation')
        for nrhs in NRHS:
            for bpad in LDB_PADS:
                what = '{} nrhs={} ldb=n+{}'.format(tag, nrhs, bpad)
                X = _getrs(ctx, Av, pv, n, ld, Bm[:nrhs], n+bpad, what)
                for r in range(nrhs):
                    check(('b', r), Bm[r], X[r], what+' vector {}'.format(r))
        X = _getrs(ctx, Av, pv, n, ld, Eh, n+3, tag+' one-hot')
        for r, k in enumerate(hot):
            check(('e', k), Eh[r], X[r], tag+' b = e_{}'.format(k))
        del store, Av, pstore, pv
    ctx.close()
    torch.cuda.empty_cache()


# ---- singular input and argument checks --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('k', FAIL_PIVOTS)
def test_getrf_reports_the_first_zero_pivot(k):
    """(E) with U0[k, k] = 0: every candidate of column k is l_ik 0 = 0, so info = k + 1; the call returns PNL_OK, the guards hold, and
    the columns before k still hold their factors (they are finished before pivot k is looked at)"""
    import torch
    ctx = _context()
    n = 4*NB+1
    rng = np.random.default_rng(10000+k)
    L0, U0, perm = exact_factors(rng, n)
    U0[k, k] = 0.
    A = exact_matrix(L0, U0, perm)
    for pad in (0, 1):
        info, M, piv, keep = _getrf(ctx, A, n+pad, 'zero pivot {}'.format(k))
        assert info == k+1, (k, info)
        assert valid_swaps(piv, n), piv
        assert np.array_equal(piv[:k], swaps_of(perm)[:k])
        _assert_same(M[:k, :], (np.tril(L0, -1)+U0)[:k, :], 'rows of U before the zero pivot {}'.format(k))
        del keep
    ctx.close()
    torch.cuda.empty_cache()


@gpu
def test_getrf_getrs_argument_checks():
    import ctypes as C
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    A = torch.full((8, 8), float(POISON), dtype=torch.float64, device='cuda')
    b = torch.full((8,), float(POISON), dtype=torch.float64, device='cuda')
    piv = torch.full((8,), PIV_GUARD, dtype=torch.int32, device='cuda')
    info = C.c_int(-7)
    P = C.c_void_p
    Ap, bp, pp = P(A.data_ptr()), P(b.data_ptr()), P(piv.data_ptr())
    assert ctx.L.pnl_getrf(ctx.h, Ap, 7, 8, pp, C.byref(info)) == _lib.PNL_ERR_INVALID          # ldA < n
    assert ctx.L.pnl_getrf(ctx.h, Ap, 8, -1, pp, C.byref(info)) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrf(ctx.h, None, 8, 8, pp, C.byref(info)) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrf(ctx.h, Ap, 8, 8, None, C.byref(info)) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrf(ctx.h, Ap, 8, 8, pp, None) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrf(ctx.h, None, 0, 0, None, C.byref(info)) == _lib.PNL_OK and info.value == 0     # n = 0: a no-op
    assert ctx.L.pnl_getrs(ctx.h, Ap, 7, 8, pp, bp, 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 8, pp, bp, 7, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 8, pp, bp, 8, -1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 8, pp, None, 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 8, None, bp, 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, None, 8, 8, pp, bp, 8, 1) == _lib.PNL_ERR_INVALID
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 0, pp, bp, 8, 1) == _lib.PNL_OK
    assert ctx.L.pnl_getrs(ctx.h, Ap, 8, 8, pp, bp, 8, 0) == _lib.PNL_OK
    ctx.synchronize()
    assert (A.cpu().numpy() == POISON).all() and (b.cpu().numpy() == POISON).all() and (piv.cpu().numpy() == PIV_GUARD).all()
    ctx.close()
