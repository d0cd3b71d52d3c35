"""Multigrid for a block of right-hand sides: pnl_mg_cycle_block, pnl_mg_cg_block (csrc/pnl_mg_block.hip), the external-preconditioner
steps pnl_cgb_residual / _start / _step / _beta (csrc/pnl_cg_block.hip) through the C ABI on SYNTHETIC hierarchies, and the Python layer
(multigrid.cycle / multigrid.cg with a 2-D B, solvers.cg_multi with a multigrid preconditioner).  The yardstick is the numpy
restatement oracle/solver_oracle.py (SO.Multigrid, SO.cg), the one tests/test_solver_side.py holds the single-vector cycle to.

Synthetic hierarchies (built here from numpy, seeded): nested 1-D sizes n_l = 2 n_{l-1} + 1 on (0, 1), h = 1 / (n + 1); every level is
    A = tridiag(-1, 2, -1) / h + h^2 G,    G_ij = exp(-4 (x_i - x_j)^2) + sum_k w_k f_k(x_i) f_k(x_j),  f_k(x) = cos(k pi x + phi_k),
the P1 stiffness matrix plus a smooth dense positive semi-definite part in the scaling of a P1 discretisation of an integral operator
(it is of the size of the stiffness matrix on the smooth modes and dominated by the diagonal 2 / h; w_k, phi_k seeded, the same on
every level); P is linear interpolation, R = P^T.
    'two'   (3, 7)                            the coarse solve only
    'deep'  (3, 7, 15, 31, 63, 127, 255, 511) launch-bound levels; the finest level is handed over as kind 2 (symmetric)
    'big'   (1023, 2047, 4095)                the finest level crosses the 2048-column split of pnl_gemv_block, the coarse inverse is 1023^2
    'weak'  (15, 31, 63, 127) with the three coarser level matrices multiplied by 64: the coarse-grid correction is 64 times too small,
            a deliberately weak cycle (little more than two Jacobi sweeps) with which CG needs about 80 iterations; it is cut off at
            maxiter = 56, behind the recomputation of the residual in pass 50.  (A small omega alone does not do it: the preconditioned
            spectrum then has two clusters and CG is through in 30 iterations.)
Columns: 33 seeded right-hand sides per hierarchy, column 2 exactly zero.  A column is standard_normal (column 0: a smooth load) times a
scale chosen from the ORACLE's conv history of that column so that tol falls into the geometric middle of a gap of that history, the
gap being at a different iteration from column to column: no entry of the history then lies within a factor 2 of tol and an iteration
count cannot flip on rounding.  The slow run of 'weak' has no such gap (its history falls by a quarter per iteration), so its columns
are scaled to stand at 100 tol when maxiter cuts them off: every entry is above 2 tol and the count is maxiter whatever the rounding.
Test (1) asserts exactly that, without a GPU.  Blocks live in poisoned allocations with ld = n + 3.

Bounds (none is a measured one but the one the issue defines through a measurement):
  cycle against numpy: 1e-12 of the largest entry, the bound of tests/test_solver_side.py; for 'big' the larger of 1e-12 and four times the
      error of the existing pnl_mg_cycle against numpy on the same data (measured in the test, printed as MGB_CYCLE_ERR).
      Measured on an MI355X over the 33 columns: pnl_mg_cycle 7.1e-15 (from zero) / 1.6e-14 (from a guess), so the bound is 1e-12 there
      too; the block cycle stands at 8.7e-15 / 3.9e-14 on 'big' and at most 1.4e-14 on the smaller hierarchies.
  pnl_mg_cg_block against SO.cg: equal iteration counts, conv to rtol 1e-5 (atol 1e-13), solutions to 1e-9 of the largest entry,
      |A x - b| <= 1e-8 |b|: the bounds of the cg-mg test of tests/test_solver_side.py.  Largest solution difference measured on an MI355X
      over all cases of this file: 1.7e-10 of the largest entry.
  independence: bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import solver_oracle as SO
from test_apply_kernels import POISON, _context, _context_with_dofs, _dev
from test_block_products import block_image, _dev_block

gpu = pytest.mark.gpu

HIERARCHIES = {'two': (3, 7), 'deep': (3, 7, 15, 31, 63, 127, 255, 511), 'big': (1023, 2047, 4095), 'weak': (15, 31, 63, 127)}
COARSE_SCALE = {'weak': 64.}
TOL = 1e-8
MAXITER = {'two': 200, 'deep': 200, 'big': 200, 'weak': 56}
NVECS = (1, 3, 16, 17, 33)
KMAX = max(NVECS)
ZERO_COLUMN = 2
PAD = 3
ST = 8                                         # PNL_CGB_STATE
ST_BETA_OLD, ST_PAP, ST_BETA, ST_CONV, ST_ACTIVE = range(5)
PNL_OK, PNL_ERR_INVALID = 0, -1


# ---- synthetic hierarchies and right-hand sides (plain numpy) ------------------------------------------------------------------------

def level_matrix(n):
    h = 1./(n+1)
    x = h*np.arange(1, n+1)
    rng = np.random.default_rng(4711)                               # the same operator on every level
    G = np.exp(-4.*(x[:, None]-x[None, :])**2)
    for k in range(1, 5):
        w, phi = rng.uniform(0.2, 1.), rng.uniform(0., 2.*np.pi)
        f = np.cos(k*np.pi*x+phi)
        G += w*np.outer(f, f)
    A = (2.*np.eye(n)-np.eye(n, k=1)-np.eye(n, k=-1))/h+h*h*G
    return 0.5*(A+A.T)


def prolongation(nc):
    """linear interpolation from nc to 2 nc + 1 interior nodes"""
    P = np.zeros((2*nc+1, nc))
    j = np.arange(nc)
    P[2*j+1, j] = 1.
    P[2*j, j] = 0.5
    P[2*j+2, j] = 0.5
    return P


_HIER, _RHS, _ORACLE = {}, {}, {}


def hierarchy(name):
    if name not in _HIER:
        lv = []
        for l, n in enumerate(HIERARCHIES[name]):
            L = {'A': level_matrix(n)*(COARSE_SCALE.get(name, 1.) if l < len(HIERARCHIES[name])-1 else 1.)}
            if l > 0:
                assert n == 2*HIERARCHIES[name][l-1]+1
                L['P'] = prolongation(HIERARCHIES[name][l-1])
                L['R'] = L['P'].T.copy()
            lv.append(L)
        _HIER[name] = lv
    return _HIER[name]


def oracle_mg(name, **cycle):
    return SO.Multigrid(hierarchy(name), **cycle)


def rhs(name):
    """KMAX columns (see the module docstring); computed once per hierarchy"""
    if name not in _RHS:
        lv = hierarchy(name)
        A = lv[-1]['A']
        n = A.shape[0]
        mo = oracle_mg(name)
        rng = np.random.default_rng(5000+n)
        x = np.arange(1, n+1)/(n+1.)
        B = rng.standard_normal((KMAX, n))
        B[0] = np.sin(np.pi*x)+0.5*x
        long_run = name == 'weak'
        for v in range(KMAX):
            if v == ZERO_COLUMN:
                B[v] = 0.
                continue
            _, _, hist = SO.cg(A, B[v], tol=0., maxiter=MAXITER[name] if long_run else 20, B=mo.precondition)
            hist = np.asarray(hist)
            if long_run:
                B[v] *= 100.*TOL/hist[-1]
                continue
            # gaps of the history wide enough for tol with a factor 2 to spare on either side (and some more for the rounding of the scale)
            # among the entries small enough for a true residual below 1e-8 |b| and with the entry before them above the rounding floor
            # (n = 7 needs less for that; there CG ends exactly after 7 passes and what follows is rounding noise: not those entries)
            upper = 1e-9 if n < 10 else 1e-12
            wide = [k for k in range(1, min(len(hist)-1, n-1)) if 0. < hist[k+1] < upper*hist[0] and hist[k] > 1e-16*hist[0] and hist[:k+1].min() > 6.*hist[k+1]
                    and hist[k+1:].max() < hist[k]/6.]
            assert wide, (name, v, hist)
            k = wide[v % len(wide)]
            B[v] *= TOL/np.sqrt(hist[k]*hist[k+1])
        _RHS[name] = B
    return _RHS[name]


def oracle_cg(name, v, x0=None, maxiter=None):
    maxiter = MAXITER[name] if maxiter is None else maxiter
    key = (name, v, None if x0 is None else x0.tobytes(), maxiter)
    if key not in _ORACLE:
        _ORACLE[key] = SO.cg(hierarchy(name)[-1]['A'], rhs(name)[v], x0=x0, tol=TOL, maxiter=maxiter, B=oracle_mg(name).precondition)
    return _ORACLE[key]


def guesses(name):
    n = HIERARCHIES[name][-1]
    scale = np.abs(rhs(name)).max(axis=1)*0.5**(np.arange(KMAX) % 4)/(n+1.)          # A x0 of the size of b, differently per column
    # the zero column keeps a zero guess: from a non-zero one its result is the contracted guess, whose leading digits cancel in b - A x
    # (pnl_mg_cycle itself then stands at 6e-11 of the largest entry on 'big')
    scale[ZERO_COLUMN] = 0.
    return np.random.default_rng(77+n).standard_normal((KMAX, n))*scale[:, None]


def guess_columns(name):
    """the first three non-zero columns whose oracle history FROM THE GUESS has no entry within a factor 2 of tol either"""
    X0, out = guesses(name), []
    for v in range(KMAX):
        hist = np.asarray(oracle_cg(name, v, x0=X0[v])[2])
        if v != ZERO_COLUMN and not ((hist > TOL/2.) & (hist < 2.*TOL)).any():
            out.append(v)
        if len(out) == 3:
            break
    return out


# ---- (1) CPU: the yardstick and the inputs ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(HIERARCHIES))
def test_oracle_converges_and_no_count_can_flip(name):
    """(1) the level matrices are symmetric positive definite and dense, SO.Multigrid / SO.cg converge on them, and for the tolerance
    and the columns of tests (3) and (4) no entry of the oracle's conv history lies within a factor 2 of tol: an iteration count cannot
    flip on rounding.  The zero column converges at once; the weak cycle needs more than 50 iterations (the refresh) and is cut off at
    maxiter = 56 with every entry of its history above 2 tol."""
    lv = hierarchy(name)
    for L in lv:
        assert np.array_equal(L['A'], L['A'].T) and np.linalg.eigvalsh(L['A']).min() > 0. and (L['A'] != 0.).all()
        n = L['A'].shape[0]
        dense = L['A']-np.diag(np.diagonal(L['A']))-np.diag(np.diagonal(L['A'], 1), 1)-np.diag(np.diagonal(L['A'], -1), -1)
        assert (np.diagonal(L['A']) > 2.*np.abs(dense).sum(axis=1)).all()      # the diagonal dominates the dense part
    A, B, tol = lv[-1]['A'], rhs(name), TOL
    mo = oracle_mg(name)
    if name != 'weak':
        x, it, res = mo.solve(B[0], tol=1e-8*np.linalg.norm(B[0]), maxiter=60)
        assert it < 60 and res[-1] <= 1e-8*np.linalg.norm(B[0])
    counts = []
    for v in range(KMAX):
        x, its, hist = oracle_cg(name, v)
        hist = np.asarray(hist)
        if v == ZERO_COLUMN:
            assert its == 0 and hist[0] == 0. and not x.any()
            continue
        assert not ((hist > tol/2.) & (hist < 2.*tol)).any(), (name, v, hist/tol)
        counts.append(its)
        if name == 'weak':
            assert its == MAXITER[name] > 50 and len(hist) == its+1 and hist.min() > 2.*tol, (v, its, hist/tol)
            continue
        assert hist[-1] <= tol and its < MAXITER[name] and len(hist) == its+2
        assert np.linalg.norm(A@x-B[v]) <= 1e-8*np.linalg.norm(B[v])
    assert len(set(counts)) > 1 or name == 'weak', counts                      # columns stop at different iterations
    # from a guess, and cut off
    X0 = guesses(name)
    assert len(guess_columns(name)) == 3
    for v in guess_columns(name):
        x, its, hist = oracle_cg(name, v, x0=X0[v])
        hist = np.asarray(hist)
        assert (hist[-1] <= tol or name == 'weak') and not ((hist > tol/2.) & (hist < 2.*tol)).any(), (name, v, hist/tol)
        x, its, hist = oracle_cg(name, v, maxiter=2)
        assert its == 2 and hist[-1] > 2.*tol


# ---- device helpers -----------------------------------------------------------------------------------------------------------------------

class Native:
    """the hierarchy in HBM and its pnl_mg, created through pnl_mg_create directly"""

    def __init__(self, name, kind_top=None, h2_top=False, **cycle):
        import torch
        from pynucleus_amd import _lib
        import scipy.sparse as sp
        self.ctx = _context()
        self.lv = hierarchy(name)
        self.keep, descs = [], []
        kw = dict(cycle)
        for l, L in enumerate(self.lv):
            n = L['A'].shape[0]
            ld = n+1 if n > 1000 else n                          # 4095 -> 4096: the 16-byte path of pnl_gemv_block; odd ld: the scalar one
            store = torch.full((n, ld), float(POISON), dtype=torch.float64, device='cuda')
            store[:, :n] = _dev(L['A'])
            diag = _dev(np.diagonal(L['A']).copy())
            d = _lib.pnl_mg_level_desc()
            d.n, d.A_dev, d.ldA, d.diag_dev = n, store.data_ptr(), ld, diag.data_ptr()
            self.keep += [store, diag]
            top = l == len(self.lv)-1
            if top and kind_top is not None:
                d.kind = kind_top
            if l > 0:
                for key in ('R', 'P'):
                    M = sp.csr_matrix(L[key])
                    M.sort_indices()
                    ip, ix, da = _dev(M.indptr.astype(np.int32)), _dev(M.indices.astype(np.int32)), _dev(M.data.astype(np.float64))
                    self.keep += [ip, ix, da]
                    setattr(d, key+'_indptr_dev', ip.data_ptr()); setattr(d, key+'_indices_dev', ix.data_ptr()); setattr(d, key+'_data_dev', da.data_ptr())
            if top and h2_top:
                d.kind = 1
                d.near_indptr_dev, d.near_indices_dev, d.near_data_dev = ip.data_ptr(), ix.data_ptr(), da.data_ptr()     # never dereferenced here
            descs.append(d)
        self.Atop, self.ldA, self.n = store, ld, n                  # the finest operator
        self.cinv = _dev(np.linalg.inv(self.lv[0]['A']))
        self.ctx.synchronize()
        self.mg = self.ctx.mg_create(descs, self.cinv.data_ptr(), kw.get('omega', 2./3.), kw.get('presmoothingSteps', 1), kw.get('postsmoothingSteps', 1))

    def close(self):
        self.ctx.mg_destroy(self.mg)
        self.ctx.close()

    def _run(self, call, B, X0, fill):
        """B, X in poisoned allocations with ld = n + PAD; checks the padding and the guards of X and that B is unchanged"""
        k, n = B.shape
        ld = n+PAD
        bs, bp = _dev_block(B, ld, 1)
        xs, xp = _dev_block(np.full((k, n), fill) if X0 is None else X0, ld, 0)
        out = call(k, bp, ld, xp, ld)
        self.ctx.synchronize()
        got = xs.cpu().numpy()
        X = got[:k*ld].reshape(k, ld)[:, :n].copy()
        assert np.array_equal(got, block_image(X, ld, 0)), 'padding column or guard element of X overwritten'
        assert np.array_equal(bs.cpu().numpy(), block_image(B, ld, 1)), 'B was written'
        assert not np.isnan(X).any()
        return X, out

    def cycle(self, B, X0=None):
        # from zero: X is not read, whatever it holds
        return self._run(lambda k, bp, ldb, xp, ldx: self.ctx.mg_cycle_block(self.mg, k, bp, ldb, xp, ldx, X0 is None), B, X0, 123.)[0]

    def cycle_single(self, b, x0=None):
        import torch
        bd = _dev(b)
        xd = torch.zeros_like(bd) if x0 is None else _dev(x0)
        self.ctx.mg_cycle(self.mg, bd.data_ptr(), xd.data_ptr(), x0 is None)
        self.ctx.synchronize()
        return xd.cpu().numpy()

    def cg(self, B, X0=None, tol=TOL, maxiter=200, given_A=False):
        Aptr, ldA = (self.Atop.data_ptr(), self.ldA) if given_A else (None, 0)
        X, (its, res) = self._run(lambda k, bp, ldb, xp, ldx: self.ctx.mg_cg_block(self.mg, Aptr, ldA, k, bp, ldb, xp, ldx, tol, maxiter, X0 is None),
                                  B, X0, 0.)
        return X, its, res


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ('X', 'iterations', 'residual')):
        assert np.array_equal(np.asarray(g), np.asarray(w)), '{}: {} differs: {!r} != {!r}'.format(what, name, g, w)


def _cycle_oracle(name, B, X0=None, **cycle):
    mo = oracle_mg(name, **cycle)
    out = np.zeros_like(B) if X0 is None else X0.copy()
    for v in range(B.shape[0]):
        mo.solveOnLevel(len(mo.levels)-1, B[v], out[v], X0 is None)
    return out


# ---- (2) the cycle against numpy ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', ('two', 'deep', 'big'))
def test_cycle_block_against_numpy(name):
    """(2) every column of pnl_mg_cycle_block, from zero and from a guess, for 1 .. 33 columns, agrees with SO.Multigrid.solveOnLevel to
    1e-12 of the largest entry of the result ('big': the larger of that and four times the error of pnl_mg_cycle on the same data;
    measured on an MI355X: pnl_mg_cycle 7.1e-15 from zero / 1.6e-14 from a guess, the block 8.7e-15 / 3.9e-14, so 1e-12 is the bound there
    too).  'deep' runs
    with its finest level as kind 2 and with two sweeps on either side as well; the padding is untouched, no NaN anywhere."""
    B, X0 = rhs(name), guesses(name)
    for cycle in ({},)+(({'presmoothingSteps': 2, 'postsmoothingSteps': 2}, {'presmoothingSteps': 0, 'postsmoothingSteps': 1}) if name == 'deep' else ()):
        N = Native(name, kind_top=2 if name == 'deep' else None, **cycle)
        for guess in (None, X0):
            want = _cycle_oracle(name, B, guess, **cycle)
            scale = np.abs(want).max(axis=1)
            scale[scale == 0.] = 1.
            bound = 1e-12
            if name == 'big':
                single = max(np.abs(N.cycle_single(B[v], None if guess is None else guess[v])-want[v]).max()/scale[v] for v in range(KMAX))
                bound = max(1e-12, 4.*single)
                print('MGB_CYCLE_ERR {} {}: pnl_mg_cycle {:.3e} -> bound {:.3e}'.format(name, 'zero' if guess is None else 'guess', single, bound))
            for k in NVECS:
                X = N.cycle(B[:k], None if guess is None else guess[:k])
                err = (np.abs(X-want[:k]).max(axis=1)/scale[:k]).max()
                print('MGB_CYCLE_ERR {} {} nvec={}: block {:.3e}'.format(name, 'zero' if guess is None else 'guess', k, err))
                assert err <= bound, (name, cycle, k, err, bound)
                assert k <= ZERO_COLUMN or guess is not None or not X[ZERO_COLUMN].any()
        N.close()


# ---- (3) column independence --------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', ('two', 'deep', 'big'))
def test_columns_are_independent_bit_for_bit(name):
    """(3) every column of pnl_mg_cycle_block and of pnl_mg_cg_block (X, iterations, residual) has the bits of its solo call with one
    column: in blocks of 1 .. 33 columns, in a permuted block and in a repeated call.  The zero column is frozen with 0 iterations
    and residual 0 and stays zero."""
    B, X0, tol = rhs(name), guesses(name), TOL
    N = Native(name, kind_top=2 if name == 'deep' else None)
    perm = np.random.default_rng(3).permutation(KMAX)
    # the cycle, from zero and from a guess
    for guess in (None, X0):
        g = lambda sel: None if guess is None else guess[sel]
        solo = np.stack([N.cycle(B[v:v+1], g(slice(v, v+1)))[0] for v in range(KMAX)])
        for k in NVECS:
            assert np.array_equal(N.cycle(B[:k], g(slice(0, k))), solo[:k]), (name, 'cycle', k)
        assert np.array_equal(N.cycle(B[perm], g(perm)), solo[perm]), (name, 'cycle permuted')
        assert np.array_equal(N.cycle(B, g(slice(None))), solo), (name, 'cycle repeated')
    # the CG
    solo = [N.cg(B[v:v+1], tol=tol) for v in range(KMAX)]
    sX, si, sr = np.stack([s[0][0] for s in solo]), np.array([s[1][0] for s in solo]), np.array([s[2][0] for s in solo])
    for k in NVECS:
        _assert_same(N.cg(B[:k], tol=tol), (sX[:k], si[:k], sr[:k]), '{} nrhs={}'.format(name, k))
    _assert_same(N.cg(B[perm], tol=tol), (sX[perm], si[perm], sr[perm]), name+' permuted')
    _assert_same(N.cg(B, tol=tol), (sX, si, sr), name+' repeated')
    _assert_same(N.cg(B, tol=tol, given_A=True), (sX, si, sr), name+' with the finest operator given')
    assert si[ZERO_COLUMN] == 0 and sr[ZERO_COLUMN] == 0. and not sX[ZERO_COLUMN].any()
    assert len(set(si.tolist())) > 2, si                                  # columns froze at different times
    gX, gi, gr = N.cg(B[:17], X0[:17], tol=tol)
    for v in (0, 5, 16):
        _assert_same(N.cg(B[v:v+1], X0[v:v+1], tol=tol), (gX[v:v+1], gi[v:v+1], gr[v:v+1]), '{} from a guess, solo {}'.format(name, v))
    N.close()


# ---- (4) the CG against numpy ---------------------------------------------------------------------------------------------------------------

def _assert_cg_matches(name, B, X, its, res, cols, x0=None, maxiter=None):
    A = hierarchy(name)[-1]['A']
    for j, v in enumerate(cols):
        xo, ito, ho = oracle_cg(name, v, x0=None if x0 is None else x0[j], maxiter=maxiter)
        print('MGB_CG {} column {}: iterations {} (numpy {}), conv {:.3e} (numpy {:.3e}), |x - x_numpy| / |x| {:.2e}'.format(
            name, v, its[j], ito, res[j], ho[-1], np.abs(X[j]-xo).max()/max(np.abs(xo).max(), 1e-300)))
        assert its[j] == ito, (name, v, its[j], ito)
        assert np.isclose(res[j], ho[-1], rtol=1e-5, atol=1e-13), (name, v, res[j], ho[-1])
        assert np.abs(X[j]-xo).max() <= 1e-9*np.abs(xo).max(), (name, v)
        if maxiter is None and name != 'weak':
            assert np.linalg.norm(A@X[j]-B[j]) <= 1e-8*np.linalg.norm(B[j]), (name, v)


@gpu
@pytest.mark.parametrize('name', ('two', 'deep', 'big', 'weak'))
def test_cg_block_against_numpy(name):
    """(4) pnl_mg_cg_block against SO.cg(A, b, B=mo.precondition) column by column: equal iteration counts (test (1) shows that they
    cannot flip), conv to rtol 1e-5, solutions to 1e-9 of the largest entry, |A x - b| <= 1e-8 |b|; from a non-zero guess; maxiter = 0
    leaves X untouched and reports the initial conv; maxiter = 2 cuts every non-zero column off with iterations == 2.  'weak' needs
    more than 50 iterations: the residual is recomputed in pass 50, and maxiter = 56 cuts the run off behind it."""
    B, X0, tol = rhs(name), guesses(name), TOL
    N = Native(name)
    cols = list(range(KMAX)) if name != 'weak' else [0, 1, 2, 3, 4]
    X, its, res = N.cg(B[cols], tol=tol, maxiter=MAXITER[name])
    _assert_cg_matches(name, B[cols], X, its, res, cols)
    assert its[ZERO_COLUMN] == 0 and res[ZERO_COLUMN] == 0. and not X[ZERO_COLUMN].any()
    if name == 'weak':
        assert all(its[v] == 56 for v in range(len(cols)) if v != ZERO_COLUMN), its
    g = guess_columns(name)
    X, its, res = N.cg(B[g], X0[g], tol=tol, maxiter=MAXITER[name])
    _assert_cg_matches(name, B[g], X, its, res, g, x0=X0[g])
    # maxiter = 0: X untouched, the initial conv
    Xz, iz, rz = N.cg(B[g], X0[g], tol=tol, maxiter=0)
    assert np.array_equal(Xz, X0[g]) and not iz.any()
    for j, v in enumerate(g):
        assert np.isclose(rz[j], oracle_cg(name, v, x0=X0[v])[2][0], rtol=1e-5, atol=1e-13)
    # maxiter = 2 cuts every non-zero column off
    c = [0, 1, 2, 3]
    X, its, res = N.cg(B[c], tol=tol, maxiter=2)
    _assert_cg_matches(name, B[c], X, its, res, c, maxiter=2)
    assert [int(i) for i in its] == [2, 2, 0, 2] and (res[[0, 1, 3]] > tol).all() and res[2] == 0.
    N.close()


# ---- (5) the steps ----------------------------------------------------------------------------------------------------------------------------

def _state(t):
    return t.cpu().numpy().reshape(-1, ST).copy()


@gpu
@pytest.mark.parametrize('n', (1, 255, 256, 257, 65537))
def test_external_steps_on_integer_blocks(n):
    """(5) pnl_cgb_residual (every column, then the active ones), _start, _step and _beta once each on integer-valued blocks, Z a power-of-
    two multiple of integers and the state crafted so that alpha is a power of two: every vector is exact and compared bit for bit, the
    dots with int64 sums.  nvec = 16 and 3, with padding.  Column 1 is inactive in the masked calls: its inputs hold NaN (it is not
    read) and nothing of it is written."""
    import torch
    ctx = _context()
    rng = np.random.default_rng(9400+n)
    for nv, pad in ((16, 3), (3, 0)):
        ld = n+pad
        ints = lambda: rng.integers(-16, 17, size=(nv, n)).astype(np.float64)
        blk = lambda core: _dev_block(core, ld, 1)
        img = lambda store: store.cpu().numpy()
        nan_col = lambda M: np.where(np.arange(nv)[:, None] == 1, np.nan, M)
        same = lambda a, b: np.array_equal(a, b, equal_nan=True)
        Bh, AXh = ints(), ints()
        # residual, every column (no state): R = B - AX and R = B
        (bs, bp), (axs, axp), (rs, rp) = blk(Bh), blk(AXh), blk(np.full((nv, n), 7.))
        ctx.cgb_residual(n, nv, bp, ld, axp, ld, rp, ld, 0)
        ctx.synchronize()
        assert same(img(rs), block_image(Bh-AXh, ld, 1))
        ctx.cgb_residual(n, nv, bp, ld, 0, 0, rp, ld, 0)
        ctx.synchronize()
        assert same(img(rs), block_image(Bh, ld, 1)) and same(img(bs), block_image(Bh, ld, 1))
        # start: column 1 has a zero residual (frozen), column 0 a negative r . z (conv takes the absolute value)
        R0 = ints()
        R0[1] = 0.
        e = rng.integers(-2, 3, size=nv)
        Z0 = ints()*2.**e[:, None]
        Z0[0] = -R0[0]*2.**e[0]
        b0 = (R0*Z0).sum(axis=1)
        assert np.array_equal(b0, ((R0*4).astype(np.int64)*(Z0*4).astype(np.int64)).sum(axis=1)/16.) and (b0[0] < 0. or not R0[0].any())
        conv0 = np.sqrt(np.abs(b0))
        tol = float(np.sort(conv0)[1 if nv > 2 else 0]) if n > 1 else 0.5     # freezes the column with the smallest residual besides column 1
        (rs, rp), (zs, zp), (ps, pp) = blk(R0), blk(Z0), blk(np.full((nv, n), 7.))
        state = torch.full((nv*ST,), 77., dtype=torch.float64, device='cuda')
        ctx.cgb_start(n, nv, rp, ld, zp, ld, pp, ld, tol, state.data_ptr())
        ctx.synchronize()
        st = _state(state)
        assert same(img(ps), block_image(Z0, ld, 1)) and same(img(rs), block_image(R0, ld, 1)) and same(img(zs), block_image(Z0, ld, 1))
        assert np.array_equal(st[:, ST_BETA_OLD], b0) and np.array_equal(st[:, ST_BETA], b0) and np.array_equal(st[:, ST_CONV], conv0)
        assert np.array_equal(st[:, ST_ACTIVE], ((conv0 > tol) & (b0 != 0.)).astype(np.float64)) and st[1, ST_ACTIVE] == 0.
        assert not st[:, ST_PAP].any() and not st[:, ST_ACTIVE+1:].any()
        # step: alpha = betaOld / p.Ap = 2^f; column 1 inactive and full of NaN
        Ph = ints()
        Ph[Ph == 0.] = 1.
        APh = Ph*rng.integers(1, 4, size=(nv, n))
        Xh, R1 = ints(), ints()
        pap = (Ph*APh).sum(axis=1)
        f = rng.integers(-2, 3, size=nv)
        act = np.ones(nv)
        act[1] = 0.
        on = act[:, None] != 0.
        st[:, ST_BETA_OLD], st[:, ST_ACTIVE] = pap*2.**f, act
        state.copy_(torch.from_numpy(st.reshape(-1)))
        (ps, pp), (aps, app), (xs, xp), (rs, rp) = blk(nan_col(Ph)), blk(nan_col(APh)), blk(Xh), blk(R1)
        ctx.cgb_step(n, nv, pp, ld, app, ld, xp, ld, rp, ld, state.data_ptr())
        ctx.synchronize()
        X2 = np.where(on, Xh+2.**f[:, None]*Ph, Xh)
        R2 = np.where(on, R1-2.**f[:, None]*APh, R1)
        st2 = _state(state)
        assert same(img(xs), block_image(X2, ld, 1)) and same(img(rs), block_image(R2, ld, 1))
        assert same(img(ps), block_image(nan_col(Ph), ld, 1)) and same(img(aps), block_image(nan_col(APh), ld, 1))
        assert np.array_equal(st2[on[:, 0], ST_PAP], pap[on[:, 0]]) and np.array_equal(st2[1], st[1])
        assert np.array_equal(np.delete(st2, ST_PAP, axis=1), np.delete(st, ST_PAP, axis=1))
        # residual, the active columns: column 1 keeps its R, its B and AX are NaN
        (bs, bp), (axs, axp) = blk(nan_col(Bh)), blk(nan_col(AXh))
        ctx.cgb_residual(n, nv, bp, ld, axp, ld, rp, ld, state.data_ptr())
        ctx.synchronize()
        R3 = np.where(on, Bh-AXh, R2)
        assert same(img(rs), block_image(R3, ld, 1)) and np.array_equal(_state(state), st2)
        # beta: the active columns; the Z of column 1 is NaN
        Z3 = ints()*2.**e[:, None]
        (zs, zp) = blk(nan_col(Z3))
        ctx.cgb_beta(n, nv, rp, ld, zp, ld, state.data_ptr())
        ctx.synchronize()
        b3 = (R3*Z3).sum(axis=1)
        st3 = _state(state)
        assert np.array_equal(st3[on[:, 0], ST_BETA], b3[on[:, 0]]) and np.array_equal(st3[on[:, 0], ST_CONV], np.sqrt(np.abs(b3[on[:, 0]])))
        assert np.array_equal(st3[1], st2[1]) and np.array_equal(st3[:, [ST_BETA_OLD, ST_PAP, ST_ACTIVE]], st2[:, [ST_BETA_OLD, ST_PAP, ST_ACTIVE]])
        assert same(img(rs), block_image(R3, ld, 1)) and same(img(zs), block_image(nan_col(Z3), ld, 1))
        assert not np.isnan(st3).any()
    ctx.close()


# ---- (6) validation ---------------------------------------------------------------------------------------------------------------------------

@gpu
def test_validation():
    """(6) every invalid argument of the header returns PNL_ERR_INVALID and leaves a sentinel X untouched; a hierarchy with an H2 finest
    level is refused by both calls; so are the bad arguments of the four steps"""
    import torch
    N = Native('two')
    ctx, n, k = N.ctx, N.n, 3
    t = lambda *shape, fill=1.: torch.full(shape, fill, dtype=torch.float64, device='cuda')
    B, X = t(k, n), t(k, n, fill=77.)
    its, res = (C.c_int*k)(), (C.c_double*k)()
    p = lambda v: C.c_void_p(v) if v else None
    good = dict(mg=N.mg, A=None, ldA=0, nrhs=k, B=B.data_ptr(), ldb=n, X=X.data_ptr(), ldx=n, tol=1e-8, maxiter=10)

    def cg(**kw):
        a = dict(good, **kw)
        rc = ctx.L.pnl_mg_cg_block(a['mg'], p(a['A']), a['ldA'], a['nrhs'], p(a['B']), a['ldb'], p(a['X']), a['ldx'], a['tol'], a['maxiter'], 0, its, res)
        ctx.synchronize()
        return rc

    def cycle(**kw):
        a = dict(good, **kw)
        rc = ctx.L.pnl_mg_cycle_block(a['mg'], a['nrhs'], p(a['B']), a['ldb'], p(a['X']), a['ldx'], 0)
        ctx.synchronize()
        return rc
    common = (dict(mg=None), dict(B=None), dict(X=None), dict(nrhs=0), dict(nrhs=-2), dict(ldb=n-1), dict(ldx=n-1), dict(B=X.data_ptr()))
    for kw in common:
        assert cycle(**kw) == PNL_ERR_INVALID, kw
        assert bool((X == 77.).all()), kw
    for kw in common+(dict(maxiter=-1), dict(A=N.Atop.data_ptr(), ldA=n-1)):
        assert cg(**kw) == PNL_ERR_INVALID, kw
        assert bool((X == 77.).all()), kw
    H = Native('two', h2_top=True)
    for f in (cg, cycle):
        assert f(mg=H.mg) == PNL_ERR_INVALID and bool((X == 77.).all())
    assert 'H2' in H.ctx.L.pnl_error_string(H.ctx.h).decode()
    H.close()
    assert cycle() == PNL_OK and not bool((X == 77.).any())
    X.fill_(1.)
    assert cg() == PNL_OK and bool(torch.isfinite(X).all())
    # the steps
    V = [t(17, n, fill=77.) for _ in range(5)]
    state = t(17*ST, fill=77.)
    P_ = [v.data_ptr() for v in V]
    L, h, sp = ctx.L, ctx.h, p(state.data_ptr())
    steps = {
        'residual': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_residual(h, nn, nv, p(a), ld, p(P_[1]), n, p(P_[2]), n, s),
        'start': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_start(h, nn, nv, p(a), ld, p(P_[1]), n, p(P_[2]), n, 1e-8, s),
        'step': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_step(h, nn, nv, p(a), ld, p(P_[1]), n, p(P_[2]), n, p(P_[3]), n, s),
        'beta': lambda nv=3, ld=n, a=P_[0], s=sp, nn=n: L.pnl_cgb_beta(h, nn, nv, p(a), ld, p(P_[1]), n, s),
    }
    for name, f in steps.items():
        for kw in (dict(nv=17), dict(nv=0), dict(ld=n-1), dict(a=None), dict(nn=0))+((dict(s=None),) if name != 'residual' else ()):
            assert f(**kw) == PNL_ERR_INVALID, (name, kw)
        ctx.synchronize()
        assert all(bool((v == 77.).all()) for v in V) and bool((state == 77.).all()), name
    assert L.pnl_cgb_beta(None, n, 3, p(P_[0]), n, p(P_[1]), n, sp) == PNL_ERR_INVALID
    assert steps['start']() == PNL_OK
    N.close()


# ---- (7) the Python layer -----------------------------------------------------------------------------------------------------------------------

class OnlyMatvecMulti:
    """a dense operator of which only matvec_multi is visible: cg_multi must run its loop over the steps"""

    def __init__(self, op):
        self._op = op
        self.ctx, self.num_rows, self.num_columns, self.shape, self.device = op.ctx, op.num_rows, op.num_columns, op.shape, op.A.device

    def matvec_multi(self, X):
        return self._op.matvec_multi(X)


@gpu
@pytest.mark.parametrize('domain,noRef,s', (('interval', 6, 0.25), ('disc', 3, 0.75)))
def test_python_layer_on_assembled_operators(domain, noRef, s):
    """(7) five right-hand sides on assembled P1 hierarchies: mg.cycle(B) and mg.cg(B) agree row by row with the 1-D calls (values: those
    use the half-read product) to the tolerances of (2) and (4); cg_multi with the multigrid or its asPreconditioner() gives the bits
    of mg.cg(B) on the dense finest operator and runs the stepped loop for an operator that shows matvec_multi only; numpy in gives
    numpy out, torch in torch out; a plain callable, a Chebyshev multigrid and an H2-level multigrid raise NotImplementedError"""
    import torch
    from pynucleus_amd import getFractionalKernel, solvers
    from pynucleus_amd.multigrid import fractionalHierarchy, multigrid
    dim = 1 if domain == 'interval' else 2
    H = fractionalHierarchy(domain, noRef, getFractionalKernel(dim, s), {'target_order': 2.-s} if dim == 1 else {})
    mg = multigrid(H)
    A = H.finest['A']
    n = A.num_rows
    rng = np.random.default_rng(11)
    B = rng.standard_normal((5, n))*np.array([1., 1e-3, 0., 10., 1.])[:, None]
    B[0] = np.asarray(H.finest['DoFMap'].assembleRHS(1.0))
    X0 = rng.standard_normal((5, n))
    Ah = A.toarray()
    # the cycle
    Z = mg.cycle(B)
    Zg = mg.cycle(B, X0)
    assert isinstance(Z, np.ndarray) and Z.shape == (5, n) and not Z[2].any()
    for v in range(5):
        z1, zg1 = mg.cycle(B[v]), mg.cycle(B[v], X0[v])
        assert np.abs(Z[v]-z1).max() <= 1e-12*max(np.abs(z1).max(), 1e-300) and np.abs(Zg[v]-zg1).max() <= 1e-12*np.abs(zg1).max()
    Zt = mg.cycle(torch.from_numpy(B).cuda())
    assert isinstance(Zt, torch.Tensor) and Zt.is_cuda and np.array_equal(Zt.cpu().numpy(), Z)
    # the CG
    X, its, res = mg.cg(B, tol=1e-10)
    assert isinstance(X, np.ndarray) and X.shape == (5, n) and its.shape == res.shape == (5,) and its[2] == 0 and res[2] == 0. and not X[2].any()
    for v in (0, 1, 3, 4):
        x1, it1, res1 = mg.cg(B[v], tol=1e-10)
        print('MGB_PY {} column {}: iterations {} (1-D {}), conv {:.3e} (1-D {:.3e})'.format(domain, v, its[v], it1, res[v], res1[-1]))
        assert res[v] <= 1e-10 and np.abs(X[v]-x1).max() <= 1e-9*np.abs(x1).max()
        assert np.linalg.norm(Ah@X[v]-B[v]) <= 1e-8*np.linalg.norm(B[v])
        # equal counts unless the 1-D history passes within a factor 2 of tol, where the two products may stop one pass apart
        near = ((np.asarray(res1) > 0.5e-10) & (np.asarray(res1) < 2e-10)).any()
        assert its[v] == it1 or (near and abs(int(its[v])-it1) <= 1), (v, its[v], it1, res1)
        if not near:
            assert np.isclose(res[v], res1[-1], rtol=1e-5, atol=1e-13)
    Xt, it_t, rt = mg.cg(torch.from_numpy(B).cuda(), tol=1e-10)
    assert isinstance(Xt, torch.Tensor) and Xt.is_cuda
    _assert_same((Xt.cpu().numpy(), it_t, rt), (X, its, res), 'torch in / out')
    Xg, ig, rg = mg.cg(B, X0, tol=1e-10)
    assert (rg <= 1e-10).all() and np.abs(Xg[[0, 1, 3, 4]]-X[[0, 1, 3, 4]]).max() <= 1e-8*np.abs(X).max()
    # cg_multi
    _assert_same(solvers.cg_multi(A, B, tol=1e-10, maxiter=100, preconditioner=mg), (X, its, res), 'cg_multi with the multigrid')
    _assert_same(solvers.cg_multi(A, B, tol=1e-10, maxiter=100, preconditioner=mg.asPreconditioner()), (X, its, res), 'cg_multi with asPreconditioner()')
    _assert_same(solvers.cg(A, B, tol=1e-10, maxiter=100, preconditioner=mg), (X, its, res), 'cg with a 2-D b')
    _assert_same(solvers.cg_multi(A, B, X0, tol=1e-10, maxiter=100, preconditioner=mg), (Xg, ig, rg), 'cg_multi from a guess')
    W = OnlyMatvecMulti(A)
    for pre in (mg, mg.asPreconditioner()):
        Xs, is_, rs = solvers.cg_multi(W, B, tol=1e-10, maxiter=100, preconditioner=pre)
        assert isinstance(Xs, np.ndarray) and np.array_equal(is_, its) and np.allclose(rs, res, rtol=1e-5, atol=1e-13)
        assert np.abs(Xs-X).max() <= 1e-9*np.abs(X).max()
    Xs2, is2, rs2 = mg.cg(B, tol=1e-10, A=W)
    _assert_same((Xs2, is2, rs2), (Xs, is_, rs), 'mg.cg with an operator that is not dense')
    Xst = solvers.cg_multi(W, torch.from_numpy(B).cuda(), tol=1e-10, maxiter=100, preconditioner=mg)[0]
    assert isinstance(Xst, torch.Tensor) and np.array_equal(Xst.cpu().numpy(), Xs)
    # what is not built says so
    with pytest.raises(NotImplementedError):
        solvers.cg_multi(A, B, preconditioner=lambda r: r)
    cheb = multigrid(H, smoother=('chebyshev', {'degree': 2}))
    generic = multigrid(H, native=False)
    for bad in (cheb, generic):
        with pytest.raises(NotImplementedError):
            bad.cycle(B)
        with pytest.raises(NotImplementedError):
            bad.cg(B)
        with pytest.raises(NotImplementedError):
            solvers.cg_multi(A, B, preconditioner=bad)
        with pytest.raises(NotImplementedError):
            solvers.cg_multi(A, B, preconditioner=bad.asPreconditioner())
        assert bad.cycle(B[0]).shape == (n,)                       # a 1-D b takes the code it took


@gpu
def test_stepped_loop_on_a_csr_operator_with_a_hand_made_hierarchy():
    """(7) cg_multi on the CSR form of a sparse operator with a two-level hierarchy made by hand from its dense copy: the stepped loop
    over pnl_cgb_residual / _start / _step / _beta / _direction with the block cycle as preconditioner, against SO.cg column by
    column; every row has the bits of its solo solve"""
    import torch
    import scipy.sparse as sp
    from pynucleus_amd import solvers
    from pynucleus_amd.multigrid import multigrid
    from pynucleus_amd.linear_operators import Dense_LinearOperator
    from test_cg_block import _csr_operator
    nc = 31
    n = 2*nc+1
    h = 1./(n+1)
    x = h*np.arange(1, n+1)
    # a banded (5 entries per row) symmetric positive definite operator and its Galerkin coarse operator
    Af = (2.*np.eye(n)-np.eye(n, k=1)-np.eye(n, k=-1))/h+h*(np.eye(n)+0.25*np.eye(n, k=2)+0.25*np.eye(n, k=-2))*np.cos(x)[:, None]*np.cos(x)[None, :]
    Af = 0.5*(Af+Af.T)
    P = prolongation(nc)
    Ac = P.T@Af@P
    lv = [{'A': Ac}, {'A': Af, 'P': P, 'R': P.T.copy()}]
    cctx = _context_with_dofs(n)
    cop = _csr_operator(cctx, Af)
    levels = [{'A': Dense_LinearOperator(_dev(Ac), cctx, symmetric=True)},
              {'A': Dense_LinearOperator(_dev(Af), cctx, symmetric=True), 'P': sp.csr_matrix(P), 'R': sp.csr_matrix(P.T)}]
    mg = multigrid(levels)
    mo = SO.Multigrid(lv)
    rng = np.random.default_rng(21)
    B = rng.standard_normal((5, n))
    B[2] = 0.
    X, its, res = solvers.cg_multi(cop, B, tol=1e-10, maxiter=100, preconditioner=mg)
    for v in range(5):
        xo, ito, ho = SO.cg(Af, B[v], tol=1e-10, maxiter=100, B=mo.precondition)
        ho = np.asarray(ho)
        print('MGB_CSR column {}: iterations {} (numpy {}), conv {:.3e} (numpy {:.3e})'.format(v, its[v], ito, res[v], ho[-1]))
        near = ((ho > 0.5e-10) & (ho < 2e-10)).any()
        assert its[v] == ito or (near and abs(int(its[v])-ito) <= 1), (v, its[v], ito, ho)
        if its[v] == ito:
            assert np.isclose(res[v], ho[-1], rtol=1e-5, atol=1e-13) and np.abs(X[v]-xo).max() <= 1e-9*max(np.abs(xo).max(), 1e-300)
        assert np.linalg.norm(Af@X[v]-B[v]) <= 1e-8*max(np.linalg.norm(B[v]), 1e-300)
    assert its[2] == 0 and res[2] == 0. and not X[2].any()
    for v in (0, 2, 4):
        _assert_same(solvers.cg_multi(cop, B[v:v+1], tol=1e-10, maxiter=100, preconditioner=mg), (X[v:v+1], its[v:v+1], res[v:v+1]), 'solo {}'.format(v))
    Xt = solvers.cg_multi(cop, torch.from_numpy(B).cuda(), tol=1e-10, maxiter=100, preconditioner=mg.asPreconditioner())[0]
    assert isinstance(Xt, torch.Tensor) and np.array_equal(Xt.cpu().numpy(), X)
    del mg
    cctx.close()
