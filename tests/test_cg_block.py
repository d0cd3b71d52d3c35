"""Jacobi-CG for a block of right-hand sides: pnl_cg_jacobi_block and its steps (pnl_cgb_init / _update / _refresh / _direction,
csrc/pnl_cg_block.hip) through the C ABI on SYNTHETIC matrices, Dense_LinearOperator.solve_cg_jacobi_block, solvers.cg_multi and the
2-D case of solvers.cg.  Helpers come from tests/test_apply_kernels.py and tests/test_block_products.py.

No assertion uses a measured tolerance:

(1) exact.  A = dense storage of diag(d), d powers of two in [2^-3, 2^3], B small integers, x0 = 0: every product and sum is an exact
    dyadic number and alpha = 1, so X == B / d bit for bit with 0 iterations and residual 0, at every size and layout.
(2) independence.  X[v], iterations[v] and residuals[v] of a block solve have the bits of the solve of B[v] alone, wherever the column
    stands and whatever the others are; two calls repeat bit for bit.  (Freezing, the groups of 16, the atomic-free reductions.)
(3) the stopping contract: residuals[v] <= tol and iterations[v] < maxiter where the problem is solvable; maxiter reported by the columns
    that a small maxiter cuts off; maxiter = 0 returns the initial residual and leaves X alone.
(4) true residual.  rho_v = sqrt(r^T D^-1 r), r = b_v - A x_v in high precision on the host, must satisfy rho_v <= tol + gap_v,
        gap_v = 4 (min(k_v, 50) + 2) (m + 6) u sqrt(max_i 1 / d_i) (|| |A| |x_v| ||_2 + || b_v ||_2),   u = 2^-53, m = entries per row:
    the recursive residual drifts from the true one by one matvec error (m + 2) u |A| |x| and a few vector roundings per iteration
    (Greenbaum 1997, Theorem 2.2 in the simplified form: the sum of the per-step errors), over at most 50 iterations, because the
    residual is recomputed then; the factor 4 covers the constants.  It holds for any summation order; a wrong index, a missed tail
    element or a column mix-up gives rho of the order of ||b||.  The numpy restatement of the recurrence below stays under 1 % of
    the gap on these matrices (test_numpy_recurrence_meets_the_bound).  Largest (rho_v - residuals[v]) / gap_v measured on an MI355X over
    all cases of this file: 0.012.
(5) the steps on integer blocks: the dot products read back from the state equal int64 numpy sums bit for bit, and a frozen column is
    bit-identical before and after.

Edges: 256 threads per workgroup and at most 256 workgroups for the vector kernels (n = 255 / 256 / 257 and 65535 / 65536 / 65537 /
131073: one trip, the cap, two and three trips of the grid-stride loop); 128 rows, 64 and 2048 columns of k_gemv_block; 16 columns per
group (15 / 16 / 17 / 33).
"""
import ctypes as C

import numpy as np
import pytest

from test_apply_kernels import U, LD, LD_OK, POISON, hp_dot, _context, _context_with_dofs, _dev, _dev_matrix
from test_block_products import block_image, _dev_block

gpu = pytest.mark.gpu

TOL = 1e-8
NVECS = (1, 2, 3, 15, 16, 17, 33)
DOM_SIZES = (1, 2, 63, 64, 65, 127, 129, 255, 257, 1025, 2049, 2113)
EXACT_SIZES = DOM_SIZES+(256, 511, 513)
LAP_SIZES = (63, 65, 257)
# (ld - n of A, B, X; base offset in doubles of A, B, X)
LAYOUTS = ((0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0), (6, 6, 6, 0, 0, 0), (0, 1, 6, 1, 0, 1), (1, 6, 0, 0, 1, 0), (6, 0, 1, 1, 1, 1))
ST = 8                                         # PNL_CGB_STATE
ST_BETA_OLD, ST_PAP, ST_BETA, ST_CONV, ST_ACTIVE = range(5)


# ---- synthetic problems and the yardstick (plain numpy; tested below without a GPU) ----------------------------------------------

def dom(n, seed=0):
    """S = G G^T with G = standard_normal((n, min(n, 8))), the diagonal replaced by uniform(1.5, 4) (1 + sum_j!=i |S_ij|): strictly
    diagonally dominant, Jacobi-CG converges in a few iterations"""
    rng = np.random.default_rng(9000+n+seed)
    G = rng.standard_normal((n, min(n, 8)))
    S = G@G.T
    np.fill_diagonal(S, 0.)
    np.fill_diagonal(S, rng.uniform(1.5, 4., size=n)*(1.+np.abs(S).sum(axis=1)))
    return S


def lap(n):
    """tridiag(-1, 2, -1) stored dense"""
    return 2.*np.eye(n)-np.eye(n, k=1)-np.eye(n, k=-1)


SCALES = (1., 1e-6, 1e6)


def rhs_block(n, nrhs, seed=0, scales=SCALES):
    """columns standard_normal scaled by 1, 1e-6 and 1e6 in turn; column nrhs // 2 is exactly zero if there are two or more"""
    rng = np.random.default_rng(9100+n+seed)
    B = rng.standard_normal((nrhs, n))*np.array(scales)[np.arange(nrhs) % len(scales)][:, None]
    if nrhs >= 2:
        B[nrhs//2] = 0.
    return B


def must_converge(name, nrhs):
    """the columns of rhs_block that (3) demands convergence of.  dom: all -- Jacobi-CG needs at most ten passes there, so the test
    sees the recursive residual only, which falls whatever the attainable accuracy is.  lap: all but those scaled by 1e6.  For them
    ||x|| is of the order n^2 ||b|| / 10 >= 1e9, so the residual recomputed in pass 50 cannot be expected below u ||A|| ||x|| >= 1e-7,
    above tol = 1e-8: whether the recursive residual dips under tol between two recomputations is decided by rounding (the numpy
    recurrence runs into maxiter on most of them).  Such a column must still report consistently -- maxiter with a residual above
    tol, or less with one below -- with the bits of its solo solve, and obey (4) if it reports convergence."""
    return np.ones(nrhs, dtype=bool) if name == 'dom' else np.array(SCALES)[np.arange(nrhs) % 3] != 1e6


def assert_stopping(its, res, need, maxiter, what):
    its, res = np.asarray(its), np.asarray(res)
    assert (res[need] <= TOL).all() and (its[need] < maxiter).all(), (what, its, res)
    done = res <= TOL
    assert (its[done] < maxiter).all() and (its[~done] == maxiter).all() and np.isfinite(res).all(), (what, its, res)
    return done


def cg_recurrence(A, b, x0, tol, maxiter, d):
    """pnl_cg_jacobi's loop for one column in numpy: (x, iterations, conv)"""
    dinv = 1./d
    x = x0.copy()
    r = b-A@x
    p = dinv*r
    betaOld = float(r@p)
    conv = np.sqrt(betaOld)
    it = 0
    if conv > tol and betaOld != 0.:
        k = 0
        for it in range(maxiter):
            Ap = A@p
            alpha = betaOld/float(p@Ap)
            x += alpha*p
            r -= alpha*Ap
            if k == 50:
                r = b-A@x
                k = 0
            z = dinv*r
            beta = float(r@z)
            conv = np.sqrt(beta)
            if conv <= tol:
                break
            p = z+(beta/betaOld)*p
            betaOld = beta
            k += 1
        else:
            it = maxiter
    return x, it, conv


def true_residual(A, b, x, d):
    """(rho, || |A| |x| ||_2 + || b ||_2): rho = sqrt(r^T D^-1 r), r = b - A x, in np.longdouble (mpmath where that has 64 bits)"""
    if LD_OK:
        Ah, xh, bh = A.astype(LD), x.astype(LD), b.astype(LD)
        r = bh-Ah@xh
        rho = np.sqrt((r*r/d.astype(LD)).sum())
    else:
        import mpmath
        r = [mpmath.mpf(float(b[i]))-hp_dot(A[i], x)[0] for i in range(A.shape[0])]
        rho = mpmath.sqrt(mpmath.fsum(ri*ri/mpmath.mpf(float(di)) for ri, di in zip(r, d)))
    return float(rho), float(np.linalg.norm(np.abs(A)@np.abs(x))+np.linalg.norm(b))


def gap(A, b, x, d, k, m=None, x0=None):
    """the gap of (4).  From a non-zero guess the iterates are as large as the guess before they are as small as the solution, and
    the drift is bounded through the largest iterate (Greenbaum's max_k ||x_k||): || |A| |x| || is then the larger of the two"""
    m = A.shape[1] if m is None else m
    ax = np.linalg.norm(np.abs(A)@np.abs(x))
    if x0 is not None:
        ax = max(ax, np.linalg.norm(np.abs(A)@np.abs(x0)))
    return 4.*(min(int(k), 50)+2)*(m+6)*U*np.sqrt((1./d).max())*float(ax+np.linalg.norm(b))


WORST = {'ratio': -np.inf}


def assert_true_residual(A, B, X, its, res, d, tol, what, m=None, cols=None, X0=None):
    """assertion (4) for every column (of cols: those that report convergence); prints the largest (rho - residual) / gap it has seen"""
    for v in (range(B.shape[0]) if cols is None else np.nonzero(cols)[0]):
        rho, _ = true_residual(A, B[v], X[v], d)
        g = gap(A, B[v], X[v], d, its[v], m, None if X0 is None else X0[v])
        if g > 0.:
            WORST['ratio'] = max(WORST['ratio'], (rho-res[v])/g)
        assert rho <= tol+g, '{} column {}: true residual {:.3e} > tol {:.1e} + gap {:.3e} ({} iterations, reported {:.3e})'.format(
            what, v, rho, tol, g, its[v], res[v])
    print('CGB_GAP_RATIO {} largest (rho - residual) / gap so far: {:.3e}'.format(what, WORST['ratio']))


# ---- CPU-only -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,n', (('dom', 65), ('lap', 65)))
def test_numpy_recurrence_meets_the_bound(name, n):
    """(8) the yardstick itself: the numpy recurrence solves dom(65) and lap(65) to the bound of (4), far inside it, reports the
    iteration counts the issue states (3-6; 61-256 with the 50-iteration refresh) and freezes a zero column at once"""
    A = dom(n) if name == 'dom' else lap(n)
    d = np.diagonal(A).copy()
    if name == 'dom':
        off = np.abs(A).sum(axis=1)-d
        assert (d > off).all() and np.array_equal(A, A.T)
    B = rhs_block(n, 5)
    assert not B[2].any() and B[0].any()
    for v in range(5):
        x, it, conv = cg_recurrence(A, B[v], np.zeros(n), TOL, 1000, d)
        if not B[v].any():
            assert it == 0 and conv == 0. and not x.any()
            continue
        assert conv <= TOL and it < 1000
        if v % 3 != 1:
            assert (3 <= it <= 6) if name == 'dom' else (50 < it <= 256), it
        rho, _ = true_residual(A, B[v], x, d)
        g = gap(A, B[v], x, d, it)
        assert rho <= TOL+g
        assert rho-conv <= 0.01*g, (rho, conv, g)
    # a wrong column is far outside
    x, it, conv = cg_recurrence(A, B[0], np.zeros(n), TOL, 1000, d)
    assert true_residual(A, B[3], x, d)[0] > 1e3*(TOL+gap(A, B[3], x, d, it))
    # maxiter: the count of a column that is cut off, and an untouched x for 0
    x, it, conv = cg_recurrence(lap(65), B[0], np.zeros(n), TOL, 2, np.full(n, 2.))
    assert it == 2 and conv > TOL
    x, it, conv = cg_recurrence(lap(65), B[0], np.ones(n), TOL, 0, np.full(n, 2.))
    assert it == 0 and np.array_equal(x, np.ones(n)) and conv > TOL


def test_exact_case_is_exact_in_numpy():
    """(1) in numpy: alpha = 1, X = B / d after one pass that reports 0 iterations"""
    n = 65
    rng = np.random.default_rng(1)
    d = 2.**rng.integers(-3, 4, size=n)
    b = rng.integers(-8, 9, size=n).astype(np.float64)
    x, it, conv = cg_recurrence(np.diag(d), b, np.zeros(n), TOL, 1000, d)
    assert np.array_equal(x, b/d) and it == 0 and conv == 0.


# ---- pnl_cg_jacobi_block ------------------------------------------------------------------------------------------------------

def _solve(ctx, Aptr, ldA, n, B, X0, tol, maxiter, dB=0, dX=0, oB=0, oX=0):
    """one call; returns (X, iterations, residuals) after checking the whole allocations of X (padding, guards) and B (unchanged)"""
    k = B.shape[0]
    bs, bp = _dev_block(B, n+dB, oB)
    xs, xp = _dev_block(np.zeros((k, n)) if X0 is None else X0, n+dX, oX)
    its, res = ctx.cg_jacobi_block(Aptr, ldA, n, k, bp, n+dB, xp, n+dX, tol, maxiter)
    ctx.synchronize()
    got = xs.cpu().numpy()
    X = got[oX:oX+k*(n+dX)].reshape(k, n+dX)[:, :n].copy()
    assert np.array_equal(got, block_image(X, n+dX, oX)), 'padding column or guard element of X overwritten'
    assert np.array_equal(bs.cpu().numpy(), block_image(B, n+dB, oB)), 'B was written'
    return X, its, res


@gpu
@pytest.mark.parametrize('n', EXACT_SIZES)
def test_cg_block_exact(n):
    """(1) at every size, layout and number of columns; column nrhs // 2 is zero and stays zero; no NaN anywhere"""
    ctx = _context()
    rng = np.random.default_rng(9200+n)
    d = 2.**rng.integers(-3, 4, size=n)
    core = _dev(np.diag(d))
    Bfull = rng.integers(-8, 9, size=(max(NVECS), n)).astype(np.float64)
    for dA, dB, dX, oA, oB, oX in LAYOUTS:
        store, Av = _dev_matrix(core, n+dA, oA)
        for k in NVECS:
            B = Bfull[:k].copy()
            if k >= 2:
                B[k//2] = 0.
            X, its, res = _solve(ctx, Av.data_ptr(), n+dA, n, B, None, TOL, 1000, dB, dX, oB, oX)
            tag = 'n={} nrhs={} layout {}'.format(n, k, (dA, dB, dX, oA, oB, oX))
            assert np.array_equal(X, B/d[None, :]), tag
            assert not its.any() and not res.any() and its.shape == res.shape == (k,), (tag, its, res)
        assert np.array_equal(store.cpu().numpy(), block_image(np.diag(d), n+dA, oA)), 'A was written'
    ctx.close()


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ('X', 'iterations', 'residual')):
        assert np.array_equal(np.asarray(g), np.asarray(w)), '{}: {} differs: {!r} != {!r}'.format(what, name, g, w)


@gpu
@pytest.mark.parametrize('name,n', tuple(('dom', n) for n in DOM_SIZES)+tuple(('lap', n) for n in LAP_SIZES))
def test_cg_block_columns_are_independent(name, n):
    """(2), (3), (4) on dom(n) and lap(n): every column of blocks of 1 .. 33 right-hand sides, of a permuted block and of a repeated
    call has the bits of its solo solve; every column that must converge (must_converge) does so below maxiter; the true residual
    obeys the bound"""
    A = dom(n) if name == 'dom' else lap(n)
    d = np.diagonal(A).copy()
    kmax = max(NVECS)
    B = rhs_block(n, kmax)
    ctx = _context()
    dA, dB, dX, oA, oB, oX = LAYOUTS[n % len(LAYOUTS)]
    store, Av = _dev_matrix(_dev(A), n+dA, oA)

    maxiter = 1000 if name == 'dom' else 400                       # lap(257) at scale 1 needs at most 256 passes

    def run(Bk, X0=None):
        return _solve(ctx, Av.data_ptr(), n+dA, n, Bk, X0, TOL, maxiter, dB, dX, oB, oX)
    solo = [run(B[v:v+1]) for v in range(kmax)]
    assert not np.isnan(np.stack([s[0][0] for s in solo])).any()
    for v in (0, kmax//2):
        _assert_same(run(B[v:v+1]), solo[v], 'repeated solo solve {}'.format(v))
    for k in NVECS:
        X, its, res = run(B[:k])
        for v in range(k):
            _assert_same((X[v], its[v], res[v]), (solo[v][0][0], solo[v][1][0], solo[v][2][0]), '{}({}) nrhs={} column {}'.format(name, n, k, v))
    X, its, res = run(B)
    _assert_same(run(B), (X, its, res), 'repeated call')
    # (3)
    done = assert_stopping(its, res, must_converge(name, kmax), maxiter, '{}({})'.format(name, n))
    assert its[kmax//2] == 0 and res[kmax//2] == 0. and not X[kmax//2].any()
    if name == 'lap' and n > 50:
        assert its.max() > 50, its                                # the refresh has run
    if n > 2:
        assert len(set(its.tolist())) > 1, its                       # columns froze at different times
    # a permuted block
    perm = np.random.default_rng(n).permutation(kmax)
    Xp, ip, rp = run(B[perm])
    _assert_same((Xp, ip, rp), (X[perm], its[perm], res[perm]), 'permuted block')
    # (4)
    assert_true_residual(A, B, X, its, res, d, TOL, '{}({})'.format(name, n), cols=done)
    ctx.close()


@gpu
def test_cg_block_maxiter_and_initial_guess():
    """(3) on lap(257): maxiter = 2 cuts every column off (iterations == 2, residual > tol, finite X, the solo bits) but the zero
    one, which is frozen from the start; maxiter = 0 returns the initial residual and leaves X (a non-zero guess) untouched; a solve
    from a non-zero guess obeys (2) and (4) too"""
    n, k = 257, 17
    A, B = lap(n), rhs_block(n, 17)
    d = np.full(n, 2.)
    ctx = _context()
    store, Av = _dev_matrix(_dev(A), n+1, 1)
    X, its, res = _solve(ctx, Av.data_ptr(), n+1, n, B, None, TOL, 2, 1, 6, 0, 1)
    cut = np.arange(k) != k//2
    assert (its[cut] == 2).all() and (res[cut] > TOL).all() and its[k//2] == 0 and res[k//2] == 0. and not X[k//2].any(), (its, res)
    assert np.isfinite(X).all() and np.isfinite(res).all()
    for v in range(k):
        _assert_same(_solve(ctx, Av.data_ptr(), n+1, n, B[v:v+1], None, TOL, 2, 0, 1, 1, 0), (X[v:v+1], its[v:v+1], res[v:v+1]), 'maxiter = 2, column {}'.format(v))
    X0 = np.random.default_rng(5).standard_normal((k, n))
    Xz, iz, rz = _solve(ctx, Av.data_ptr(), n+1, n, B, X0, TOL, 0, 1, 6, 0, 1)
    assert np.array_equal(Xz, X0) and not iz.any()
    for v in range(k):
        r = B[v]-A@X0[v]
        want = np.sqrt(r@(r/d))
        assert abs(rz[v]-want) <= 1e-12*want, (v, rz[v], want)         # the initial residual (a sanity check of its meaning only)
    Xg, ig, rg = _solve(ctx, Av.data_ptr(), n+1, n, B, X0, TOL, 400, 6, 0, 1, 1)
    done = assert_stopping(ig, rg, must_converge('lap', k), 400, 'from a guess')
    _assert_same(_solve(ctx, Av.data_ptr(), n+1, n, B[3:4], X0[3:4], TOL, 400), (Xg[3:4], ig[3:4], rg[3:4]), 'solo from a guess')
    assert_true_residual(A, B, Xg, ig, rg, d, TOL, 'lap(257) from a guess', cols=done, X0=X0)
    ctx.close()


# ---- the steps ----------------------------------------------------------------------------------------------------------------

def _state(t):
    return t.cpu().numpy().reshape(-1, ST).copy()


@gpu
@pytest.mark.parametrize('n', (1, 255, 256, 257, 65535, 65536, 65537, 131073))
def test_cgb_steps_on_integer_blocks(n):
    """(5): init, update, refresh and direction once each on integer blocks (dinv powers of two), nvec = 16 and 3, with padding.  The
    state is crafted on the host between the calls so that alpha and beta / betaOld are powers of two: every vector is then exact and
    compared bit for bit, the dots with int64 sums.  Column 1 is frozen: nothing of it changes."""
    import torch
    ctx = _context()
    rng = np.random.default_rng(9300+n)
    for nv, pad in ((16, 3), (3, 0)):
        ld = n+pad
        dinv = 2.**rng.integers(-2, 3, size=n)
        ints = lambda: rng.integers(-16, 17, size=(nv, n)).astype(np.float64)
        Bh, AXh, Ph = ints(), ints(), ints()
        Ph[Ph == 0.] = 1.
        APh = Ph*rng.integers(1, 4, size=(nv, n))
        Xh = ints()
        AXh[1] = Bh[1]                                                # column 1: zero residual, frozen by init
        dv = _dev(dinv)
        blk = lambda core: _dev_block(core, ld, 1)
        img = lambda store: store.cpu().numpy()
        (bs, bp), (axs, axp), (rs, rp), (ps, pp), (zs, zp), (xs, xp), (aps, app) = (blk(Bh), blk(AXh), blk(np.full((nv, n), 7.)), blk(np.full((nv, n), 7.)),
                                                                                  blk(np.full((nv, n), 7.)), blk(Xh), blk(APh))
        state = torch.full((nv*ST,), 77., dtype=torch.float64, device='cuda')
        # init
        R0 = Bh-AXh
        P0 = dinv*R0
        b0 = (R0*P0).sum(axis=1)                                      # exact: multiples of 1/4 below 2^53
        assert np.array_equal(b0, ((R0*4).astype(np.int64)*(P0*4).astype(np.int64)).sum(axis=1)/16.)
        tol = float(np.sqrt(np.sort(b0)[1 if nv > 2 else 0])) if n > 1 else 0.5     # freezes the column with the smallest residual besides column 1
        ctx.cgb_init(n, nv, dv.data_ptr(), bp, ld, axp, ld, rp, ld, pp, ld, tol, state.data_ptr())
        ctx.synchronize()
        st = _state(state)
        assert np.array_equal(img(rs), block_image(R0, ld, 1)) and np.array_equal(img(ps), block_image(P0, ld, 1))
        assert np.array_equal(st[:, ST_BETA_OLD], b0) and np.array_equal(st[:, ST_BETA], b0) and np.array_equal(st[:, ST_CONV], np.sqrt(b0))
        assert np.array_equal(st[:, ST_ACTIVE], ((np.sqrt(b0) > tol) & (b0 != 0.)).astype(np.float64)) and st[1, ST_ACTIVE] == 0.
        assert not st[:, ST_PAP].any() and not st[:, ST_ACTIVE+1:].any()
        # update: P, AP, X from the host; betaOld crafted so that alpha = 2^e
        pap = (Ph*APh).sum(axis=1)
        e = rng.integers(-2, 3, size=nv)
        act = np.ones(nv)
        act[1] = 0.
        st[:, ST_BETA_OLD], st[:, ST_ACTIVE] = pap*2.**e, act
        state.copy_(torch.from_numpy(st.reshape(-1)))
        ps, pp = blk(Ph)
        before = (img(xs).copy(), img(rs).copy(), img(zs).copy(), st.copy())
        ctx.cgb_update(n, nv, dv.data_ptr(), pp, ld, app, ld, xp, ld, rp, ld, zp, ld, state.data_ptr())
        ctx.synchronize()
        on = act[:, None] != 0.
        X1 = np.where(on, Xh+2.**e[:, None]*Ph, Xh)
        R1 = np.where(on, R0-2.**e[:, None]*APh, R0)
        Z1 = np.where(on, dinv*R1, 7.)
        b1 = (R1*Z1).sum(axis=1)
        st1 = _state(state)
        assert np.array_equal(img(xs), block_image(X1, ld, 1)) and np.array_equal(img(rs), block_image(R1, ld, 1))
        assert np.array_equal(img(zs), block_image(Z1, ld, 1)) and np.array_equal(img(ps), block_image(Ph, ld, 1))
        assert np.array_equal(st1[on[:, 0], ST_PAP], pap[on[:, 0]]) and np.array_equal(st1[on[:, 0], ST_BETA], b1[on[:, 0]])
        assert np.array_equal(st1[on[:, 0], ST_CONV], np.sqrt(b1[on[:, 0]])) and np.array_equal(st1[:, ST_BETA_OLD], st[:, ST_BETA_OLD])
        assert np.array_equal(st1[1], before[3][1]), 'state of the frozen column changed'
        # refresh
        ctx.cgb_refresh(n, nv, dv.data_ptr(), bp, ld, axp, ld, rp, ld, zp, ld, state.data_ptr())
        ctx.synchronize()
        R2 = np.where(on, Bh-AXh, R1)
        Z2 = np.where(on, dinv*R2, Z1)
        b2 = (R2*Z2).sum(axis=1)
        st2 = _state(state)
        assert np.array_equal(img(rs), block_image(R2, ld, 1)) and np.array_equal(img(zs), block_image(Z2, ld, 1))
        assert np.array_equal(st2[on[:, 0], ST_BETA], b2[on[:, 0]]) and np.array_equal(st2[1], before[3][1])
        # direction: beta / betaOld = 2^f; the active column with the smallest conv is frozen by tol, nothing of it is written
        f = rng.integers(-2, 3, size=nv)
        st2[on[:, 0], ST_BETA_OLD] = (st2[:, ST_BETA]*2.**(-f))[on[:, 0]]
        live = np.nonzero(on[:, 0] & (st2[:, ST_BETA] > 0.))[0]
        tol2 = float(st2[live, ST_CONV].min()) if live.size else 0.
        state.copy_(torch.from_numpy(st2.reshape(-1)))
        ctx.cgb_direction(n, nv, zp, ld, pp, ld, tol2, state.data_ptr())
        ctx.synchronize()
        go = on[:, 0] & ~(st2[:, ST_CONV] <= tol2)
        P3 = np.where(go[:, None], Z2+2.**f[:, None]*Ph, Ph)
        st3 = _state(state)
        assert np.array_equal(img(ps), block_image(P3, ld, 1)) and np.array_equal(img(zs), block_image(Z2, ld, 1))
        assert np.array_equal(st3[:, ST_ACTIVE], go.astype(np.float64))
        assert np.array_equal(st3[go, ST_BETA_OLD], st2[go, ST_BETA]) and np.array_equal(st3[~go, ST_BETA_OLD], st2[~go, ST_BETA_OLD])
        assert np.array_equal(st3[:, ST_BETA:ST_ACTIVE], st2[:, ST_BETA:ST_ACTIVE]) and np.array_equal(st3[1], before[3][1])
        if live.size > 1 and n > 1:
            assert go.any() and (on[:, 0] & ~go).any()
        for s_, core in ((bs, Bh), (axs, AXh), (aps, APh)):
            assert np.array_equal(img(s_), block_image(core, ld, 1)), 'an input block was written'
    ctx.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

@gpu
def test_cg_block_validation():
    """(7) every invalid argument of the header returns PNL_ERR_INVALID and leaves X (a sentinel) untouched"""
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    n, k = 7, 3
    t = lambda *shape, fill=1.: torch.full(shape, fill, dtype=torch.float64, device='cuda')
    A, B, X = torch.eye(n, dtype=torch.float64, device='cuda')*2., t(k, n), t(k, n, fill=77.)
    its, res = (C.c_int*k)(), (C.c_double*k)()
    p = lambda v: C.c_void_p(v) if v else None
    good = dict(ctx=ctx.h, A=A.data_ptr(), ldA=n, n=n, nrhs=k, B=B.data_ptr(), ldb=n, X=X.data_ptr(), ldx=n, tol=TOL, maxiter=10)

    def call(**kw):
        a = dict(good, **kw)
        rc = ctx.L.pnl_cg_jacobi_block(a['ctx'], p(a['A']), a['ldA'], a['n'], a['nrhs'], p(a['B']), a['ldb'], p(a['X']), a['ldx'], a['tol'], a['maxiter'],
                                       its, res)
        ctx.synchronize()
        return rc
    for kw in (dict(ctx=None), dict(A=None), dict(B=None), dict(X=None), dict(n=0), dict(n=-1), dict(nrhs=0), dict(nrhs=-2), dict(ldA=n-1),
               dict(ldb=n-1), dict(ldx=n-1), dict(maxiter=-1), dict(B=X.data_ptr())):
        assert call(**kw) == _lib.PNL_ERR_INVALID, kw
        assert bool((X == 77.).all()), kw
    X.zero_()
    assert call() == _lib.PNL_OK and bool((X == 0.5).all()) and list(its) == [0]*k and list(res) == [0.]*k
    # the steps: nvec > 16, a leading dimension below n, null blocks
    V = [t(17, n, fill=77.) for _ in range(6)]
    state = t(17*ST, fill=77.)
    dv = t(n)
    P_ = [v.data_ptr() for v in V]
    L, h, sp, dp = ctx.L, ctx.h, p(state.data_ptr()), p(dv.data_ptr())
    steps = {
        'init': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_init(h, nn, nv, dp, p(a), ld, p(P_[1]), n, p(P_[2]), n, p(P_[3]), n, TOL, s),
        'update': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_update(h, nn, nv, dp, p(a), ld, p(P_[1]), n, p(P_[2]), n, p(P_[3]), n, p(P_[4]), n, s),
        'refresh': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_refresh(h, nn, nv, dp, p(a), ld, p(P_[1]), n, p(P_[2]), n, p(P_[3]), n, s),
        'direction': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_direction(h, nn, nv, p(a), ld, p(P_[1]), n, TOL, s),
    }
    for name, f in steps.items():
        for kw in (dict(nv=17), dict(nv=0), dict(ld=n-1), dict(a=None), dict(s=None), dict(nn=0)):
            assert f(**kw) == _lib.PNL_ERR_INVALID, (name, kw)
        ctx.synchronize()
        assert all(bool((v == 77.).all()) for v in V) and bool((state == 77.).all()), name
    assert L.pnl_cgb_init(None, n, 3, dp, p(P_[0]), n, None, 0, p(P_[2]), n, p(P_[3]), n, TOL, sp) == _lib.PNL_ERR_INVALID
    assert steps['init']() == _lib.PNL_OK
    ctx.close()


# ---- the Python layers -----------------------------------------------------------------------------------------------------------

def _dense_operator(ctx, A, symmetric=True, pad=3):
    import torch
    from pynucleus_amd.linear_operators import Dense_LinearOperator
    n = A.shape[0]
    store = torch.full((n, n+pad), float(POISON), dtype=torch.float64, device='cuda')
    store[:, :n] = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    return Dense_LinearOperator(store[:, :n], ctx, symmetric=symmetric)


def _csr_operator(ctx, A):
    """CSR_LinearOperator with the pattern and the values of the non-zeros of the host matrix A"""
    import torch
    from pynucleus_amd.linear_operators import CSR_LinearOperator
    n = A.shape[0]
    rows, cols = np.nonzero(A)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    op = CSR_LinearOperator(indptr, cols.astype(np.int32), n, ctx, torch.device('cuda', 0))
    op.data_dev[:rows.shape[0]] = torch.from_numpy(A[rows, cols]).cuda()
    return op


def cg_as_before(A, b, tol=1e-8, maxiter=1000):
    """the loop of solvers.cg for a 1-D b and the Jacobi preconditioner, restated on A.matvec and torch vectors: what cg(A, b) has
    returned since before cg_multi existed"""
    import torch
    bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    x = torch.zeros_like(bd)
    dinv = 1./torch.from_numpy(np.ascontiguousarray(A.diagonal, dtype=np.float64)).cuda()
    r = bd.clone()
    p = dinv*r
    betaOld = float(torch.dot(r, p))
    residuals = [float(np.sqrt(abs(betaOld)))]
    its = 0
    if residuals[0] > tol:
        k = 0
        for i in range(maxiter):
            Ap = A.matvec(p)
            alpha = betaOld/float(torch.dot(p, Ap))
            x.add_(p, alpha=alpha)
            r.add_(Ap, alpha=-alpha)
            if k == 50:
                r = bd-A.matvec(x)
                k = 0
            Br = dinv*r
            beta = float(torch.dot(r, Br))
            residuals.append(float(np.sqrt(abs(beta))))
            its = i
            if residuals[-1] <= tol:
                break
            p = Br+(beta/betaOld)*p
            betaOld = beta
            k += 1
        else:
            its = maxiter
    return x.cpu().numpy(), its, residuals


@gpu
def test_dense_operator_and_cg_multi_on_synthetic_matrices():
    """Dense_LinearOperator.solve_cg_jacobi_block is the library call (numpy and torch in / out, X0); cg_multi sends a symmetric dense
    operator there, runs the loop over the steps for a CSR operator and for preconditioner=None, with (2) and (4) for each; cg with a
    2-D b is cg_multi; a callable preconditioner and a distributed operator raise NotImplementedError"""
    import torch
    from pynucleus_amd import solvers
    from pynucleus_amd.linear_operators import DistributedDense_LinearOperator
    n, k = 129, 17
    A, B = dom(n), rhs_block(n, 17)
    d = np.diagonal(A).copy()
    ctx = _context()
    op = _dense_operator(ctx, A)
    X, its, res = op.solve_cg_jacobi_block(B)
    assert isinstance(X, np.ndarray) and X.shape == (k, n) and its.shape == res.shape == (k,) and (res <= TOL).all()
    store, Av = _dev_matrix(_dev(A), n+3, 0)
    _assert_same(_solve(ctx, Av.data_ptr(), n+3, n, B, None, TOL, 1000), (X, its, res), 'operator method against the C ABI')
    Xt, it_t, rt = op.solve_cg_jacobi_block(torch.from_numpy(B).cuda(), tol=TOL)
    assert isinstance(Xt, torch.Tensor) and Xt.is_cuda
    _assert_same((Xt.cpu().numpy(), it_t, rt), (X, its, res), 'torch in / out')
    _assert_same(solvers.cg_multi(op, B), (X, its, res), 'cg_multi on a symmetric dense operator')
    _assert_same(solvers.cg(op, B), (X, its, res), 'cg with a 2-D b')
    X0 = np.random.default_rng(3).standard_normal((k, n))
    Xg, ig, rg = solvers.cg_multi(op, B, X0=X0)
    _assert_same(_solve(ctx, Av.data_ptr(), n+3, n, B, X0, TOL, 1000), (Xg, ig, rg), 'X0')
    with pytest.raises(NotImplementedError):
        solvers.cg_multi(op, B, preconditioner=lambda r: r)
    with pytest.raises(NotImplementedError):
        solvers.cg_multi(DistributedDense_LinearOperator(op.A, ctx), B)
    # the loop over the steps: no preconditioner (unit diagonal) on the dense operator, and a CSR operator; lap(65) takes the refresh
    Xn, in_, rn = solvers.cg_multi(op, B, preconditioner=None)
    assert (rn <= TOL).all() and (in_ < 1000).all()
    assert_true_residual(A, B, Xn, in_, rn, np.ones(n), TOL, 'dom(129) without preconditioner')
    for v in (0, 8, 16):
        _assert_same(solvers.cg_multi(op, B[v:v+1], preconditioner=None), (Xn[v:v+1], in_[v:v+1], rn[v:v+1]), 'unit diagonal, solo {}'.format(v))
    ctx.close()
    for M, name, m in ((lap(65), 'lap(65)', 3), (dom(300), 'dom(300)', 300)):
        nn = M.shape[0]
        cctx = _context_with_dofs(nn)
        cop = _csr_operator(cctx, M)
        Bc = rhs_block(nn, 17)
        mi = 120                                                     # lap(65) at scale 1 needs at most 65 passes
        Xc, ic, rc = solvers.cg_multi(cop, Bc, maxiter=mi)
        done = assert_stopping(ic, rc, must_converge(name[:3], 17), mi, 'CSR '+name)
        assert ic[8] == 0 and not Xc[8].any() and (name != 'lap(65)' or ic.max() > 50)
        assert_true_residual(M, Bc, Xc, ic, rc, np.diagonal(M).copy(), TOL, 'CSR '+name, m=m, cols=done)
        _assert_same(solvers.cg_multi(cop, Bc, maxiter=mi), (Xc, ic, rc), 'CSR repeated')
        for v in (0, 1, 2, 16):
            _assert_same(solvers.cg_multi(cop, Bc[v:v+1], maxiter=mi), (Xc[v:v+1], ic[v:v+1], rc[v:v+1]), 'CSR {} solo {}'.format(name, v))
        perm = np.random.default_rng(nn).permutation(17)
        _assert_same(solvers.cg_multi(cop, Bc[perm], maxiter=mi), (Xc[perm], ic[perm], rc[perm]), 'CSR permuted')
        _assert_same(solvers.cg_multi(cop, Bc[:3], maxiter=mi), (Xc[:3], ic[:3], rc[:3]), 'CSR nrhs = 3')
        Xt, it_t, rt = solvers.cg(cop, torch.from_numpy(Bc).cuda(), maxiter=mi)
        assert isinstance(Xt, torch.Tensor)
        _assert_same((Xt.cpu().numpy(), it_t, rt), (Xc, ic, rc), 'CSR torch through cg')
        cctx.close()


@gpu
@pytest.mark.parametrize('name,n,maxiter', (('dom', 257, 1000), ('lap', 65, 200)))
def test_step_loop_on_the_dense_operator_has_the_bits_of_the_library_call(name, n, maxiter):
    """solvers._cg_steps (the Python loop over pnl_cgb_init / _update / _refresh / _direction, A.matvec_multi as the product) on the
    dense operator returns the bits of solve_cg_jacobi_block (pnl_cg_jacobi_block), from a zero guess and from a seeded X0: b - 0 is b
    in every bit, both loops use pnl_gemv_block, whose bits do not depend on the leading dimensions, and the same steps.  n = 257: two
    workgroups and a tail; 17 rows: a full group and a remainder of one; lap(65) passes 50 iterations and takes the refresh"""
    from pynucleus_amd import solvers
    A = dom(n) if name == 'dom' else lap(n)
    B = rhs_block(n, 17)
    ctx = _context()
    op = _dense_operator(ctx, A)
    X, its, res = op.solve_cg_jacobi_block(B, tol=TOL, maxiter=maxiter)
    assert name != 'lap' or its.max() > 50
    _assert_same(solvers._cg_steps(op, B, None, TOL, maxiter, 'jacobi'), (X, its, res), 'library call against the step loop')
    X0 = np.random.default_rng(9300+n).standard_normal((17, n))
    _assert_same(solvers._cg_steps(op, B, X0, TOL, maxiter, 'jacobi'), op.solve_cg_jacobi_block(B, X0, tol=TOL, maxiter=maxiter),
                 'library call against the step loop, from a guess')
    ctx.close()


_OPERATORS = {}


def _assembled(kind):
    """disc(3), P1, fractional s = 0.75 as Dense / H2; the finite-horizon getSparse of tests/test_finite_horizon.py on a small square
    as CSR / SSS"""
    if kind not in _OPERATORS:
        from pynucleus_amd import disc, uniformSquare, P1_DoFMap, PHYSICAL, NO_BOUNDARY, getFractionalKernel, getKernel, INDICATOR
        from pynucleus_amd.builder import nonlocalBuilder
        if kind in ('dense', 'h2-atomic', 'h2-ordered'):
            dm = P1_DoFMap(disc(3), PHYSICAL)
            kernel = getFractionalKernel(2, 0.75)
            if kind == 'dense':
                A = nonlocalBuilder(dm, kernel, {'target_order': 0.5}, zeroExterior=True).getDense()
            else:
                A = nonlocalBuilder(dm, kernel, {'target_order': 0.5, 'eta': 3., 'minClusterSize': 12, 'farField': kind[3:]},
                                    zeroExterior=True).getH2()
        else:
            dm = P1_DoFMap(uniformSquare(17), NO_BOUNDARY)
            params = {'forceUnsymmetric': True} if kind == 'csr' else {}
            A = nonlocalBuilder(dm, getKernel(2, kernel=INDICATOR, horizon=0.2), params, zeroExterior=False).getSparse()
        _OPERATORS[kind] = A
    return _OPERATORS[kind]


@gpu
@pytest.mark.parametrize('kind', ('dense', 'csr', 'sss', 'h2-atomic', 'h2-ordered'))
def test_cg_multi_on_assembled_operators(kind):
    """(6) five right-hand sides on the assembled operators.  (4) with A.toarray() as the matrix; (2) for Dense, CSR and the ordered
    H2 (SSS and the atomic H2 add with float atomics: their contract is the value); cg with a 2-D b is cg_multi; cg with a 1-D b
    returns what the loop of solvers.py, restated here on A.matvec, returns: bit for bit where matvec has no float atomics (CSR, the
    ordered H2), else (the dense half-read, SSS, the atomic H2) both obey (4).
    The finite-horizon operator on NO_BOUNDARY DoFs annihilates the constants, so its right-hand sides are taken from its range
    (B = Y A^T for the scaled random Y): a consistent system, on which CG from a zero guess converges."""
    from pynucleus_amd import solvers
    from pynucleus_amd.linear_operators import CSR_LinearOperator, SSS_LinearOperator
    A = _assembled(kind)
    want = {'csr': CSR_LinearOperator, 'sss': SSS_LinearOperator}.get(kind)
    assert (want is None or type(A) is want) and (kind != 'dense' or A.symmetric) and (kind[:2] != 'h2' or A.farField == kind[3:])
    n = A.num_rows
    Ah = np.array(A.toarray(), dtype=np.float64)
    d = np.asarray(A.diagonal, dtype=np.float64).copy()
    B = rhs_block(n, 5, scales=(1., 1e-6, 1e2))                     # within the attainable accuracy of these operators at tol = 1e-8
    if kind in ('csr', 'sss'):
        B = B@Ah.T
    assert not B[2].any()
    X, its, res = solvers.cg_multi(A, B)
    assert X.shape == (5, n) and (res <= TOL).all() and (its < 1000).all() and its[2] == 0 and not X[2].any(), (its, res)
    assert_true_residual(Ah, B, X, its, res, d, TOL, kind)
    if kind in ('dense', 'csr', 'h2-ordered'):
        _assert_same(solvers.cg_multi(A, B), (X, its, res), kind+' repeated')
        for v in range(5):
            _assert_same(solvers.cg_multi(A, B[v:v+1]), (X[v:v+1], its[v:v+1], res[v:v+1]), '{} solo {}'.format(kind, v))
        perm = np.array([3, 0, 4, 2, 1])
        _assert_same(solvers.cg_multi(A, B[perm]), (X[perm], its[perm], res[perm]), kind+' permuted')
        _assert_same(solvers.cg(A, B), (X, its, res), kind+' cg with a 2-D b')
    else:
        X2, i2, r2 = solvers.cg(A, B)
        assert X2.shape == X.shape and (r2 <= TOL).all()
        assert_true_residual(Ah, B, X2, i2, r2, d, TOL, kind+' through cg')
    # 1-D: the code and the values of before
    x1, it1, res1 = solvers.cg(A, B[0])
    xw, itw, resw = cg_as_before(A, B[0])
    assert x1.shape == (n,) and isinstance(res1, list)
    assert len(res1) == it1+2 and res1[-1] <= TOL
    if kind in ('csr', 'h2-ordered'):
        assert np.array_equal(x1, xw) and it1 == itw and res1 == resw
    else:
        for xx, ii, rr in ((x1, it1, res1), (xw, itw, resw)):
            assert_true_residual(Ah, B[:1], xx[None, :], [ii], [rr[-1]], d, TOL, kind+' 1-D')
