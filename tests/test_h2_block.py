"""The atomic-free H2 far field for blocks of vectors (csrc/pnl_h2_block.hip: k_h2b_up_leaves, k_h2b_nodes<0, 1, 2>, k_h2b_down_leaves)
through the C ABI, stage by stage, and H2Matrix.farField = 'ordered' on top of it.

Contracts as include/pnl_hip.h states them: pnl_h2_upward_block / _interact_block / _downward_block are the single-vector phases on
coefficient blocks [nnodes][M][16] (vector index fastest, slots v >= nvec zero, cupB and cdownB overwritten, cdownB modified in place by
the downward pass, Y added to at the DoFs of the plan's leaves only, X read there only, the padding ld > N untouched);
pnl_h2_matvec_block chains them on the context's own blocks for any nvec in groups of 16.  No float atomics: the bits of Y[v] depend on
the plan, K, V, T, X[v] and the old Y[v] only.

The trees, the data and the references are those of test_h2_kernels.py (imported), with a block form of the references here.

(E) exact.  Integer data whose chain on absolute values stays below 2^53 for EVERY vector of the block
    (test_exact_blocks_stay_below_2_53, no GPU), so fp64 is exact in any summation order and the device must return the bits of the
    int64 reference: cupB, cdownB after the interactions and after the downward pass, Y, for nvec = 1, 2, 15, 16 in the phase calls
    and 1, 5, 16, 17, 33 in pnl_h2_matvec_block, ld = N and N + 3.  Every array sits between 2^30 guards, cupB / cdownB arrive holding
    2^30, Y arrives holding integers, the padding holds 2^30 and must survive, X must come back unchanged.
(R) rounding.  ROUNDING_CASES of test_h2_kernels.py with 5 vectors against the longdouble / mpmath reference, with that file's tolerance
    verbatim: (sum of the stage products + c) u (abs-chain + |y0|) per component.  It counts one rounding per product and per addition
    and the merges as additions, so it covers a fixed-order fused sum.  The device output never enters the tolerance.
(B) bits.  One vector alone, as vector 0 of 5, 7 of 16 and 16 of 17 among unrelated vectors, each setting called twice: identical bits.
    pnl_h2_matvec_block equals the three block phases chained on caller arrays.
(O) operator.  getH2 on disc(3) with {'farField': 'ordered'}: matvec_multi(X)[v] == matvec(X[v]) bit for bit (5 and 17 vectors), dotMV,
    two CG runs with identical residual lists and solutions, agreement with 'atomic' within 2 x (R) for the far part + the gamma bound
    of test_apply_kernels.py for the CSR near part (both formed from farFieldData(), the plan's transfer matrices and Anear on absolute
    values), and 'atomic' giving back today's product.

Measured on an MI355X, largest error / tolerance per case of (R) (the bound is 1):
  2-1-single-0 0.0098, 2-2-balanced-0 0.0098, 2-7-unbalanced-1 < 0.0001, 2-9-gap-0 < 0.0001, 2-16-unbalanced-0 < 0.0001,
  2-11-balanced-1 < 0.0001, 1-3-unbalanced-0 0.0119, 1-16-balanced-1 0.0020, 1-16-single-0 0.0103, 2-8-gap-1 0.0001: the bound is
  dominated by the chain on absolute values, as for the single-vector kernels.  (O) ordered against atomic: < 0.0001.
"""
import ctypes as C

import numpy as np
import pytest

from test_h2_kernels import (synthetic_tree, exact_data, rounding_data, ref_upward, ref_interact, ref_downward, ref_matvec, exact_bound,
                             _install, _guarded, _back, _p1_builder, stage_products, hp_array, num_dofs, _case_id, ROUNDING_CASES,
                             POISON, LIMIT, U, PNL_OK, PNL_ERR_INVALID, PNL_ERR_STATE)

gpu = pytest.mark.gpu

NV = 16
BLOCK_ORDERS = [(2, 1), (1, 3), (2, 2), (1, 16), (2, 7), (2, 9), (2, 16)]     # M = 1, 3, 4, 16, 49, 81, 256
BLOCK_KINDS = ('single', 'balanced', 'unbalanced', 'gap')
EXACT_BLOCK_CASES = [(dim, m, kind, partial, 'mixed') for dim, m in BLOCK_ORDERS for kind in BLOCK_KINDS for partial in (0, 1)]
EXACT_BLOCK_CASES += [(2, 7, 'unbalanced', 0, 'empty')]
PHASE_NVEC = (1, 2, 15, 16)
MATVEC_NVEC = (1, 5, 16, 17, 33)
NVMAX = max(MATVEC_NVEC)
BITS_CASES = [(2, 7, 'unbalanced', 1), (2, 16, 'unbalanced', 0), (1, 3, 'unbalanced', 0)]
assert all(c in ROUNDING_CASES for c in BITS_CASES)


# ---- block references -----------------------------------------------------------------------------------------------------------

def exact_block(t, m, nvec=NVMAX):
    """(V, T, K, X[nvec][N], Y0[nvec][N]): exact_data of the case; vector 0 is its x and y0, the others integer vectors of their own"""
    V, T, K, x, y0 = exact_data(t, m)
    rng = np.random.default_rng([77, m, t['dim'], BLOCK_KINDS.index(t['kind']), t['partial']])
    X = rng.integers(-3, 4, size=(nvec, t['N']), dtype=np.int64)
    X[X == 0] = 1
    Y0 = rng.integers(-1024, 1025, size=(nvec, t['N']), dtype=np.int64)
    X[0], Y0[0] = x, y0
    return V, T, K, X, Y0


def _levels(t, deepest_first):
    out = [[int(c) for c in np.nonzero(t['level'] == l)[0]] for l in range(1, t['nlevels'])]
    return out[::-1] if deepest_first else out


def block_upward(t, V, T, X):
    """cupB[nnodes][M][nvec] for the rows of X, all vectors at once"""
    cup = np.zeros((len(t['parent']), T.shape[1], X.shape[0]), dtype=np.result_type(V[0], T, X))
    for (node, dofs), v in zip(t['leaves'], V):
        cup[node] = v.T@X[:, dofs].T
    for nodes in _levels(t, True):
        for c in nodes:
            cup[t['parent'][c]] += T[c]@cup[c]
    return cup


def block_interact(t, K, cup):
    cdown = np.zeros_like(cup)
    for p, (n1, n2) in enumerate(t['far']):
        cdown[n1] += K[p]@cup[n2]
    return cdown


def block_downward(t, V, T, cdown, Y0):
    cdown = cdown.copy()
    Y = Y0.astype(cdown.dtype) if cdown.dtype != object else Y0.copy()
    for nodes in _levels(t, False):
        for c in nodes:
            cdown[c] += T[c].T@cdown[t['parent'][c]]
    for (node, dofs), v in zip(t['leaves'], V):
        Y[:, dofs] += (v@cdown[node]).T
    return cdown, Y


def block_matvec(t, V, T, K, X, Y0):
    cup = block_upward(t, V, T, X)
    cd0 = block_interact(t, K, cup)
    cd1, Y = block_downward(t, V, T, cd0, Y0)
    return cup, cd0, cd1, Y


def pad16(B, nvec):
    """[nnodes][M][nvec] -> the device layout [nnodes][M][16] with zero slots v >= nvec"""
    out = np.zeros(B.shape[:2]+(NV,), dtype=np.float64)
    out[:, :, :nvec] = B[:, :, :nvec]
    return out


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', EXACT_BLOCK_CASES, ids=_case_id)
def test_exact_blocks_stay_below_2_53(case):
    """the condition of (E) for every vector of the block: the chain on absolute values in exact integers (its float64 run shows that
    int64 did not wrap), per vector through exact_bound for the first vectors and through the block chain for all of them"""
    dim, m, kind, partial, far_kind = case
    t = synthetic_tree(kind, dim, partial, far_kind)
    V, T, K, X, Y0 = exact_block(t, m)
    assert np.abs(X).min() >= 1 and X.shape == (NVMAX, t['N'])
    av, at, ak, ax, ay = [np.abs(v) for v in V], np.abs(T), np.abs(K), np.abs(X), np.abs(Y0)
    outs = block_matvec(t, av, at, ak, ax, ay)
    fl = block_matvec(t, [v.astype(np.float64) for v in av], at.astype(np.float64), ak.astype(np.float64), ax.astype(np.float64),
                      ay.astype(np.float64))
    assert max(float(o.max()) for o in fl) < 2.**62
    b = max(int(o.max()) for o in outs)
    assert b+POISON < LIMIT, (b, np.log2(float(b)))
    for v in (0, 1, NVMAX-1):
        bv = exact_bound(t, V, T, K, X[v], Y0[v])
        assert bv <= b and bv+POISON < LIMIT


@pytest.mark.parametrize('case', [(2, 2, 'unbalanced', 0), (1, 3, 'gap', 1), (2, 7, 'unbalanced', 1), (1, 1, 'single', 0), (2, 3, 'balanced', 1)],
                         ids=_case_id)
def test_block_reference_equals_per_vector_references(case):
    dim, m, kind, partial = case
    t = synthetic_tree(kind, dim, partial)
    V, T, K, X, Y0 = exact_block(t, m, 17)
    cup, cd0, cd1, Y = block_matvec(t, V, T, K, X, Y0)
    assert cup.shape == (len(t['parent']), m**dim, 17)
    for v in range(17):
        r = ref_matvec(t, V, T, K, X[v], Y0[v])
        assert np.array_equal(cup[:, :, v], r[0]) and np.array_equal(cd0[:, :, v], r[1])
        assert np.array_equal(cd1[:, :, v], r[2]) and np.array_equal(Y[v], r[3])
    assert np.array_equal(cup[:, :, 3], ref_upward(t, V, T, X[3]))
    assert np.array_equal(cd0[:, :, 3], ref_interact(t, K, cup[:, :, 3]))
    assert np.array_equal(block_downward(t, V, T, cd0, Y0)[1][3], ref_downward(t, V, T, cd0[:, :, 3], Y0[3])[1])
    p = pad16(cup, 5)
    assert p.shape[2] == 16 and not p[:, :, 5:].any() and np.array_equal(p[:, :, :5], cup[:, :, :5])


# ---- device plumbing ------------------------------------------------------------------------------------------------------------

def _ptr(v):
    return C.c_void_p(v.data_ptr())


def _rows(A, ld):
    """host [nvec][ld] holding A in the first N columns and 2^30 in the padding"""
    A = np.asarray(A, dtype=np.float64)
    out = np.full((A.shape[0], ld), float(POISON))
    out[:, :A.shape[1]] = A
    return out


def _assert_exact(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError('{}: {} of {} entries differ, first at {}: got {!r}, expected {!r}'.format(
            what, len(bad), ref.size, bad[:6].tolist(), [got[tuple(b)] for b in bad[:4]], [ref[tuple(b)] for b in bad[:4]]))


def _block_phases(ctx, t, M, X, Y0, ldx, ldy):
    """(cupB, cdownB after the interactions, cdownB after the downward pass, Y [nvec][ldy]) of the three block phases; cupB and cdownB
    arrive poisoned; X (with its padding) must come back unchanged"""
    nn, nvec = len(t['parent']), X.shape[0]
    L, h = ctx.L, ctx.h
    xh = _rows(X, ldx)
    xs, xv = _guarded(xh)
    us, uv = _guarded(np.full(nn*M*NV, POISON))
    ds, dv = _guarded(np.full(nn*M*NV, POISON))
    ys, yv = _guarded(_rows(Y0, ldy))
    ctx.check(L.pnl_h2_upward_block(h, nvec, _ptr(xv), ldx, _ptr(uv)))
    cup = _back(ctx, us, (nn, M, NV), 'cupB')
    ctx.check(L.pnl_h2_interact_block(h, _ptr(uv), _ptr(dv)))
    cd0 = _back(ctx, ds, (nn, M, NV), 'cdownB')
    assert np.array_equal(_back(ctx, us, (nn, M, NV), 'cupB'), cup), 'pnl_h2_interact_block changed cupB'
    ctx.check(L.pnl_h2_downward_block(h, nvec, _ptr(dv), _ptr(yv), ldy))
    cd1 = _back(ctx, ds, (nn, M, NV), 'cdownB')
    Y = _back(ctx, ys, (nvec, ldy), 'Y')
    assert np.array_equal(_back(ctx, xs, xh.shape, 'X'), xh), 'X was written'
    return cup, cd0, cd1, Y


def _block_matvec(ctx, X, Y0, ldx, ldy):
    xh = _rows(X, ldx)
    xs, xv = _guarded(xh)
    ys, yv = _guarded(_rows(Y0, ldy))
    ctx.check(ctx.L.pnl_h2_matvec_block(ctx.h, X.shape[0], _ptr(xv), ldx, _ptr(yv), ldy))
    Y = _back(ctx, ys, (X.shape[0], ldy), 'Y')
    assert np.array_equal(_back(ctx, xs, xh.shape, 'X'), xh), 'X was written'
    return Y


def _unlisted(t):
    return np.setdiff1d(np.arange(t['N']), np.concatenate([d for _, d in t['leaves']]))


# ---- (E) ------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('case', EXACT_BLOCK_CASES, ids=_case_id)
def test_block_phases_exact(case):
    """(E): every entry of cupB, of cdownB after pnl_h2_interact_block and after pnl_h2_downward_block, and of Y, bit for bit; the
    slots v >= nvec are zero; with partial_leaves X holds 2^30 at the DoFs of no listed leaf and Y keeps its bits there; the padding
    of Y keeps its 2^30"""
    dim, m, kind, partial, far_kind = case
    M = m**dim
    t = synthetic_tree(kind, dim, partial, far_kind)
    V, T, K, X, Y0 = exact_block(t, m)
    ctx = _p1_builder(dim).context()
    _install(ctx, t, m, V, T, K)
    N = t['N']
    unl = _unlisted(t)
    assert (len(unl) > 0) == bool(partial)
    ref = block_matvec(t, V, T, K, X, Y0)
    Xdev = X.copy()
    Xdev[:, unl] = POISON
    name = _case_id(case)
    for i, nvec in enumerate(PHASE_NVEC):
        ldx, ldy = (N, N+3) if i % 2 else (N+3, N)
        cup, cd0, cd1, Y = _block_phases(ctx, t, M, Xdev[:nvec], Y0[:nvec], ldx, ldy)
        tag = '{} nvec={} ldx={} ldy={}: '.format(name, nvec, ldx, ldy)
        _assert_exact(cup, pad16(ref[0], nvec), tag+'pnl_h2_upward_block cupB[node][alpha][v]')
        _assert_exact(cd0, pad16(ref[1], nvec), tag+'pnl_h2_interact_block cdownB[node][alpha][v]')
        _assert_exact(cd1, pad16(ref[2], nvec), tag+'pnl_h2_downward_block cdownB[node][alpha][v]')
        _assert_exact(Y[:, :N], ref[3][:nvec], tag+'pnl_h2_downward_block Y')
        assert np.all(Y[:, N:] == POISON), tag+'padding of Y'
        assert np.array_equal(Y[:, unl], Y0[:nvec][:, unl].astype(np.float64))
    for i, nvec in enumerate(MATVEC_NVEC):
        ldx, ldy = (N+3, N+3) if i % 2 else (N, N)
        Y = _block_matvec(ctx, Xdev[:nvec], Y0[:nvec], ldx, ldy)
        tag = '{} nvec={} ldx={} ldy={}: '.format(name, nvec, ldx, ldy)
        _assert_exact(Y[:, :N], ref[3][:nvec], tag+'pnl_h2_matvec_block Y')
        assert np.all(Y[:, N:] == POISON), tag+'padding of Y'


# ---- (R) ------------------------------------------------------------------------------------------------------------------------

def rounding_block(t, m, nvec):
    V, T, K, x, y0 = rounding_data(t, m)
    rng = np.random.default_rng([78, m, t['dim'], BLOCK_KINDS.index(t['kind']), t['partial']])
    r = lambda shape: rng.standard_normal(shape)*10.**rng.uniform(-3., 3., size=shape)
    X, Y0 = r((nvec, t['N'])), r((nvec, t['N']))
    X[0], Y0[0] = x, y0
    return V, T, K, X, Y0


@gpu
@pytest.mark.parametrize('case', ROUNDING_CASES, ids=_case_id)
def test_block_rounding(case):
    """(R): Y of the three block phases and of pnl_h2_matvec_block, 5 vectors, per component within
    (sum of the stage products + c) u (abs-chain + |y0|), the tolerance of test_h2_kernels.py"""
    dim, m, kind, partial = case
    M = m**dim
    t = synthetic_tree(kind, dim, partial)
    V, T, K, X, Y0 = rounding_block(t, m, 5)
    ctx = _p1_builder(dim).context()
    _install(ctx, t, m, V, T, K)
    hv, hT, hK, hX, hY = [hp_array(v) for v in V], hp_array(T), hp_array(K), hp_array(X), hp_array(Y0)
    ref = block_matvec(t, hv, hT, hK, hX, hY)[3]
    mag = block_matvec(t, [abs(v) for v in hv], abs(hT), abs(hK), abs(hX), abs(hY))[3]
    n, c = stage_products(t, m)
    N = t['N']
    unl = _unlisted(t)
    Xdev = X.copy()
    Xdev[:, unl] = POISON
    Yp = _block_phases(ctx, t, M, Xdev, Y0, N, N+3)[3][:, :N]
    Ym = _block_matvec(ctx, Xdev, Y0, N+3, N)[:, :N]
    worst = 0.
    for what, got in (('phases', Yp), ('pnl_h2_matvec_block', Ym)):
        g = hp_array(got)
        for v in range(5):
            for i in range(N):
                err, tol = abs(g[v, i]-ref[v, i]), (n+c)*U*mag[v, i]
                assert err <= tol, '{} {} vector {} component {}: got {!r}, reference {!r}, error {:.3e} > tol {:.3e}'.format(
                    _case_id(case), what, v, i, got[v, i], float(ref[v, i]), float(err), float(tol))
                worst = max(worst, float(err/tol)) if tol else worst
    assert np.array_equal(Yp[:, unl], Y0[:, unl])
    assert np.array_equal(Yp, Ym), 'pnl_h2_matvec_block and the chained phases differ'
    print('(R) block {}: n = {}, c = {}, largest error / tolerance {:.4f}'.format(_case_id(case), n, c, worst))


# ---- (B) ------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('case', BITS_CASES, ids=_case_id)
def test_bits_do_not_depend_on_the_block(case):
    """(B): the result of one vector alone, as vector 0 of 5, 7 of 16 and 16 of 17 among unrelated vectors, each setting called twice;
    pnl_h2_matvec_block against the three block phases chained on caller arrays"""
    dim, m, kind, partial = case
    M = m**dim
    t = synthetic_tree(kind, dim, partial)
    V, T, K, X, Y0 = rounding_block(t, m, 18)
    ctx = _p1_builder(dim).context()
    _install(ctx, t, m, V, T, K)
    N = t['N']
    X[:, _unlisted(t)] = 0.
    x, y0 = X[0].copy(), Y0[0].copy()
    base = None
    for pos, nvec in ((0, 1), (0, 5), (7, 16), (16, 17)):
        Xs, Ys = X[1:nvec+1].copy(), Y0[1:nvec+1].copy()
        Xs[pos], Ys[pos] = x, y0
        first = _block_matvec(ctx, Xs, Ys, N, N)
        second = _block_matvec(ctx, Xs, Ys, N+3, N+3)[:, :N]
        assert np.array_equal(first, second), 'vector {} of {}: a second call gives other bits'.format(pos, nvec)
        if base is None:
            base = first[0].copy()
            assert np.any(base != y0)
        assert np.array_equal(first[pos], base), 'vector {} of {}: other bits than alone'.format(pos, nvec)
    Yp = _block_phases(ctx, t, M, X[:5], Y0[:5], N, N)[3]
    assert np.array_equal(Yp, _block_matvec(ctx, X[:5], Y0[:5], N, N))
    assert np.array_equal(Yp[0], base)


# ---- error paths ----------------------------------------------------------------------------------------------------------------

@gpu
def test_block_error_paths():
    """PNL_ERR_STATE before pnl_h2_setup; PNL_ERR_INVALID for null pointers, nvec < 1, nvec > 16 in the phase calls, ldx < N, ldy < N and
    X_dev == Y_dev: each returns its code and leaves Y (and the coefficient blocks) untouched"""
    import torch
    dim, m = 2, 3
    M = m**dim
    b = _p1_builder(dim, fresh=True)
    ctx = b.context()
    L, h = ctx.L, ctx.h
    N = num_dofs(dim)
    t = synthetic_tree('unbalanced', dim, 0)
    nn = len(t['parent'])
    Xd = torch.ones((17, N), dtype=torch.float64, device='cuda')
    Yd = torch.full((17, N), 5., dtype=torch.float64, device='cuda')
    Ud = torch.full((nn*M*NV,), 7., dtype=torch.float64, device='cuda')
    Dd = torch.full((nn*M*NV,), 9., dtype=torch.float64, device='cuda')
    x, y, u, d = _ptr(Xd), _ptr(Yd), _ptr(Ud), _ptr(Dd)

    def untouched(why):
        ctx.synchronize()
        assert bool((Yd == 5.).all()) and bool((Ud == 7.).all()) and bool((Dd == 9.).all()) and bool((Xd == 1.).all()), why
    for name, rc in (('matvec_block', L.pnl_h2_matvec_block(h, 2, x, N, y, N)), ('upward_block', L.pnl_h2_upward_block(h, 2, x, N, u)),
                     ('interact_block', L.pnl_h2_interact_block(h, u, d)), ('downward_block', L.pnl_h2_downward_block(h, 2, d, y, N))):
        assert rc == PNL_ERR_STATE, (name, rc)
        untouched(name+' before pnl_h2_setup')
    V, T, K, _, _ = exact_data(t, m)
    _install(ctx, t, m, V, T, K)
    bad = {
        'matvec_block null X': lambda: L.pnl_h2_matvec_block(h, 2, None, N, y, N),
        'matvec_block null Y': lambda: L.pnl_h2_matvec_block(h, 2, x, N, None, N),
        'matvec_block nvec = 0': lambda: L.pnl_h2_matvec_block(h, 0, x, N, y, N),
        'matvec_block nvec = -1': lambda: L.pnl_h2_matvec_block(h, -1, x, N, y, N),
        'matvec_block ldx < N': lambda: L.pnl_h2_matvec_block(h, 2, x, N-1, y, N),
        'matvec_block ldy < N': lambda: L.pnl_h2_matvec_block(h, 2, x, N, y, N-1),
        'matvec_block X == Y': lambda: L.pnl_h2_matvec_block(h, 2, y, N, y, N),
        'upward_block null X': lambda: L.pnl_h2_upward_block(h, 2, None, N, u),
        'upward_block null cupB': lambda: L.pnl_h2_upward_block(h, 2, x, N, None),
        'upward_block nvec = 0': lambda: L.pnl_h2_upward_block(h, 0, x, N, u),
        'upward_block nvec = 17': lambda: L.pnl_h2_upward_block(h, 17, x, N, u),
        'upward_block ldx < N': lambda: L.pnl_h2_upward_block(h, 2, x, N-1, u),
        'interact_block null cupB': lambda: L.pnl_h2_interact_block(h, None, d),
        'interact_block null cdownB': lambda: L.pnl_h2_interact_block(h, u, None),
        'downward_block null cdownB': lambda: L.pnl_h2_downward_block(h, 2, None, y, N),
        'downward_block null Y': lambda: L.pnl_h2_downward_block(h, 2, d, None, N),
        'downward_block nvec = 0': lambda: L.pnl_h2_downward_block(h, 0, d, y, N),
        'downward_block nvec = 17': lambda: L.pnl_h2_downward_block(h, 17, d, y, N),
        'downward_block ldy < N': lambda: L.pnl_h2_downward_block(h, 2, d, y, N-1),
    }
    for why, call in bad.items():
        rc = call()
        assert rc == PNL_ERR_INVALID, (why, rc)
        untouched(why)
    assert L.pnl_h2_matvec_block(h, 17, x, N, y, N) == PNL_OK
    ctx.synchronize()
    assert not bool((Yd == 5.).all())
    ctx._h2_owner = None


# ---- (O) ------------------------------------------------------------------------------------------------------------------------

def _plan_tree(pl, dim):
    """the plan of an H2Matrix as the dict the references of test_h2_kernels.py take"""
    leaves = [(int(n), pl.leaf_dofs[pl.leaf_dof_off[l]:pl.leaf_dof_off[l+1]]) for l, n in enumerate(pl.leaf_node)]
    return dict(parent=pl.parent, level=pl.level, nlevels=pl.nlevels, leaves=leaves, far=pl.far, dim=dim, N=None)


@gpu
def test_ordered_far_field_operator():
    import torch
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel, solvers
    from pynucleus_amd.builder import nonlocalBuilder
    from test_apply_kernels import gamma_tol
    dm = P1_DoFMap(disc(3), PHYSICAL)
    kernel = getFractionalKernel(2, 0.75)
    params = {'target_order': 0.5, 'eta': 3., 'minClusterSize': 12}
    H0 = nonlocalBuilder(dm, kernel, dict(params), zeroExterior=True).getH2()
    assert H0.farField == 'atomic', 'getH2() without the parameter'
    H = nonlocalBuilder(dm, kernel, dict(params, farField='ordered'), zeroExterior=True).getH2()
    assert H.farField == 'ordered'
    with pytest.raises(ValueError):
        H.farField = 'sorted'
    n = H.num_rows
    rng = np.random.default_rng(7801)
    for k in (5, 17):
        X = rng.standard_normal((k, n))
        Y = H.matvec_multi(X)
        assert Y.shape == (k, n)
        for v in range(k):
            assert np.array_equal(Y[v], H.matvec(X[v])), (k, v)
        assert np.array_equal(H.matvec_multi(X), Y), 'a repeated product gives other bits'
        assert np.array_equal(H.dotMV(np.ascontiguousarray(X.T)), Y.T)
        assert np.array_equal(H*np.ascontiguousarray(X.T), Y.T)
    Xt = torch.from_numpy(X).cuda()
    assert np.array_equal(H.matvec_multi(Xt).cpu().numpy(), Y) and np.array_equal(H.matvec(Xt[3]).cpu().numpy(), Y[3])
    # CG twice: the same residual lists and the same solution, bit for bit
    bvec = rng.standard_normal(n)
    runs = [solvers.cg(H, bvec, tol=1e-8, maxiter=200) for _ in range(2)]
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2] and len(runs[0][2]) > 3
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][2][-1] <= 1e-8
    # against the 'atomic' product of the same operator
    pl = H.plan
    t = _plan_tree(pl, 2)
    Kf, Vf = H.farFieldData()
    x = X[0]
    aT, aK, aV, ax = hp_array(np.abs(pl.transfer)), hp_array(np.abs(Kf)), [hp_array(np.abs(v)) for v in Vf], hp_array(np.abs(x))
    An = H.Anear.toarray()
    magnear = np.abs(An)@np.abs(x)
    rowlen = np.diff(H.Anear.indptr)
    magfar = ref_matvec(t, aV, aT, aK, ax, hp_array(magnear))[3]          # abs-chain + |y0|, y0 = the near-field part
    ns, c = stage_products(t, pl.m)
    y_ord = H.matvec(x)
    H.farField = 'atomic'
    y_atm = H.matvec(x)
    worst = 0.
    for i in range(n):
        tol = 2.*(ns+c)*U*float(magfar[i])+gamma_tol(int(rowlen[i]), float(magnear[i]))
        err = abs(float(y_ord[i])-float(y_atm[i]))
        assert err <= tol, (i, y_ord[i], y_atm[i], err, tol)
        worst = max(worst, err/tol)
    assert np.any(y_ord != y_atm) or worst == 0.
    # 'atomic' again is today's path: matvec_multi is the loop of matvec, bit for bit as test_block_products.py asserts it for getH2()
    Ya = H.matvec_multi(X[:3])
    for v in range(3):
        assert np.array_equal(Ya[v], H.matvec(X[v])), v
    assert np.array_equal(Ya[0], y_atm)
    H.farField = 'ordered'
    assert np.array_equal(H.matvec(x), y_ord), 'back in ordered mode: the bits of before'
    print('(O) ordered against atomic: largest difference / tolerance {:.4f}'.format(worst))
