"""The H2 far-field kernels (k_h2_up_leaves, k_h2_up_level, k_h2_far, k_h2_down_level, k_h2_down_leaves; k_h2_kernel_interp,
k_h2_leaf_values; the host pnl_h2_transfer_matrices) through the C ABI, kernel by kernel and value by value.

Contracts as the code and include/pnl_hip.h state them ("Contracts of the H2 far-field kernels"):
  pnl_h2_setup      validates the tree (one root, level = parent's level + 1, leaf DoFs sorted and disjoint, all DoFs covered unless
                    partial_leaves, 1 <= m <= 16, far indices in range) BEFORE it touches the installed operator: a rejected plan
                    leaves the previous operator in place.  Then K = -2 gamma at the Chebyshev tensor grids, V = int phi L.
  pnl_h2_upward     cup[nnodes][M] is OVERWRITTEN: 0, then cup[leaf] = V^T x[dofs of the leaf] for the plan's leaves, then level by
                    level from the deepest cup[parent] += T_child cup[child].  x is read at the DoFs of the plan's leaves only.
  pnl_h2_interact   cdown[nnodes][M] is OVERWRITTEN: 0, then cdown[n1] += K_p cup[n2] for every ordered pair p = (n1, n2).
  pnl_h2_downward   cdown is MODIFIED IN PLACE: level by level from the root cdown[child] += T_child^T cdown[parent]; then
                    y[dofs of the leaf] += V cdown[leaf] for the plan's leaves.  y is ADDED to, at the DoFs of the plan's leaves only.
  pnl_h2_matvec     the three phases on the context's own cup / cdown: y += far field.
  pnl_h2_sizes      (nnodes, M).      pnl_h2_get / _set    K[nfar][M][M] (which = 0), V of the plan's leaves one after the other (1).

Three kinds of check.

(E) exact.  Synthetic trees (single node; balanced; unbalanced with leaves at depths 1 .. 5 and nodes with 1, 2 and 5 children, node
    numbers shuffled; a tree with an interior node that has neither children nor DoFs), leaves of 0, 1, 63, 64, 65, 300 and more
    interleaved DoFs, integer V, T, K, x, y.  T and K are not symmetric, (n1, n2) and (n2, n1) carry unrelated blocks.  For
    M > 4 the transfer blocks are sums of two signed permutation matrices (every row and column is used, the growth per level
    is 2): the chain x -> V -> T^depth -> K -> T^depth -> V then stays below 2^53, which exact_bound() proves per case in exact
    integers on the absolute values (every partial sum of every stage is bounded by the same stage on absolute values).
    test_exact_cases_stay_below_2_53 asserts it for every parametrised case: fp64 is then exact in any order, fused or not,
    atomics included, and the assertion on the device is bit equality -- against a level-by-level int64 reference and against
    the dense N x N operator F = sum_pairs W_n1 K W_n2^T.  cup, cdown, y are views with 2^30 guards on both sides; cup and
    cdown arrive holding 2^30 (the zero fill is observed), y arrives holding integers (the contract is y +=).
(R) rounding.  The same trees with standard_normal * 10^uniform(-3, 3) data (14 factors of at most ~1e4: no overflow), reference
    in np.longdouble (mpmath where longdouble is a double).  A sum of products with one rounding per operation has
    |err| <= gamma_n |terms| (Higham 3.1) and gamma_j + gamma_k + gamma_j gamma_k <= gamma_(j+k) (Lemma 3.3), so the chain has
        tol_i = (nd_max + M depth + M + M depth + M + c) u (abs-chain_i + |y0_i|),
    nd_max the largest leaf, depth the deepest leaf.  c counts the additions that are not products of a stage: the atomics that
    merge the children of a node (sum over the levels of the largest number of children) and the pairs of one n1 (largest number),
    the `+=` of every downward level and of y (depth + 1), and 4 for gamma_n = n u / (1 - n u) against n u and the error of the
    reference, as in test_apply_kernels.py.  No other tolerance is used.
(C) set-up kernels on real plans (getH2 on disc / interval), value by value against mpmath at 40 digits.
    K[p][i][j] = -2 gamma(|xi_i - eta_j|^2) at the exact Chebyshev nodes, coordinate 0 fastest.  Relative tolerance per entry
        1e-14 (what tests/test_device_math.py asserts for kern_eval<0>: exp(e ln d2), pnl_exp_ranged)
        + own(d2)  the conditioning to the rounding of the kernel's own argument that the same file allows: |y| u for exp(y),
                   y = e d2 (Gaussian), 2 |y| u, y = e sqrt(d2) (exponential), 0 for the power
        + cond * delta(d2), cond = |exponent| (power), |e d2| (Gaussian), |e sqrt(d2)| / 2 (exponential),
    delta(d2) = 2 sum_d |xi_d - eta_d| CN u (S1_d + S2_d) / d2 + 4 u the relative error of d2 from the device's nodes: a node
    (b - a) / 2 (cos(theta) + 1) + a carries a few u of its box scale S = max(|a|, |b|) + (b - a) (the rounding of theta times
    theta sin(theta) <= 1.82, cos to an ulp, three more roundings); CN = 4 is that "few".  Entries whose d2 lies within delta of
    the horizon are not judged (0 or the value).
    V[dof][alpha] = sum_cells sum_q vol w_q phi(x_q) L_alpha(x_q) with the uploaded rule as exact doubles and exact nodes.
    Tolerance per value, accumulated from the reference's own terms t = vol w phi L:
        CV u sum_points |t| (n_ops + sum_d sum_(k != l) (S_d / |x_d - x_k| + S_d / |x_l - x_k|)),   CV = 4,
    n_ops = 4 (m - 1) dim + dim + 3 + number of terms of the sum; S / |x - x_k| is the relative error of a difference whose two
    operands carry an absolute error of u S (first order); CV covers the device cos, the rounding of theta and FMA contraction.
    The device output never enters the tolerance.
    pnl_h2_transfer_matrices and the numpy h2.transferMatrix against L^parent_I(xi^child_J) with the same kind of bound (no GPU).
    Subsampling: all entries of a block of <= 64, else a seeded choice of 64 plus every box-corner node (K) / every leaf's first
    and last DoF (V).

Measured on an MI355X, largest error / tolerance per case (the bound is 1):
  K   2D (disc(3), m = 3 or 4): s = 1/4 0.058, 1/2 0.057, 3/4 0.063, 0.4 0.058, Gaussian 0.139, piecewise-constant order 0.059; m = 9 0.078.
      1D (interval(6), m = 5 or 6): s = 1/4 0.068, 1/2 0.039, 3/4 0.048, 0.4 0.062, Gaussian 0.073, exponential 0.060, finite horizon
      (1204 pairs, m = 8) 0.168, piecewise-constant order 0.081; m = 16: 0.078 (s = 3/4), 0.073 (s = 0.4).
      (The exponential kernel exists in 1D only.)
  V   2D P0 0.093, P1 0.030, P2 0.068, P1 at m = 9 0.016; 1D P0 0.089, P1 0.051, P2 0.073, P3 0.080, P1 at m = 16 0.030: the product
      form of the Lagrange factors meets the bound at m = 16 with a wide margin, the barycentric formula is not needed.
  T   (host) at most 0.213 (1D, m = 16).        (R)  at most 0.0077: the bound is dominated by the chain on absolute values.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

gpu = pytest.mark.gpu

U = 2.**-53
LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
POISON = 2**30
GUARD = 64
LIMIT = 2**53
PNL_OK, PNL_ERR_INVALID, PNL_ERR_STATE = 0, -1, -4
SPECIAL_LEAVES = (0, 1, 63, 64, 65, 300)
CN, CV = 4., 4.

# (dim, m): M = 1, 4, 49, 64, 81, 121, 256 in 2D, 1, 3, 16 in 1D
ORDERS = [(2, 1), (2, 2), (2, 7), (2, 8), (2, 9), (2, 11), (2, 16), (1, 1), (1, 3), (1, 16)]
KINDS = ('single', 'balanced', 'unbalanced', 'gap')
EXACT_CASES = [(dim, m, kind, partial, 'mixed') for dim, m in ORDERS for kind in KINDS for partial in (0, 1)]
EXACT_CASES += [(2, 9, 'balanced', 0, 'empty'), (1, 16, 'unbalanced', 1, 'empty'), (2, 2, 'single', 0, 'empty')]
ROUNDING_CASES = [(2, 1, 'single', 0), (2, 2, 'balanced', 0), (2, 7, 'unbalanced', 1), (2, 9, 'gap', 0), (2, 16, 'unbalanced', 0),
                  (2, 11, 'balanced', 1), (1, 3, 'unbalanced', 0), (1, 16, 'balanced', 1), (1, 16, 'single', 0), (2, 8, 'gap', 1)]


def _case_id(c):
    return '-'.join(str(v) for v in c)


# ---- synthetic trees (plain numpy; tested below without a GPU) -----------------------------------------------------------------

_SHAPES = {
    # parent of every node, leaves in the order that takes SPECIAL_LEAVES
    'single': ([-1], [0]),
    'balanced': ([-1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6], [7, 8, 9, 10, 11, 12, 13, 14]),
    # leaves at depths 1 (1), 2 (3, 4, 7), 3 (8), 4 (14, 15), 5 (11, 12); children: 0: 2, 2: 5, 5: 2, 9: 1, 10: 2, 6: 1, 13: 2
    'unbalanced': ([-1, 0, 0, 2, 2, 2, 2, 2, 5, 5, 9, 10, 10, 6, 13, 13], [11, 3, 14, 1, 8, 12, 4, 7, 15]),
    # node 5 (level 2) has no children and is no leaf: nothing below that branch
    'gap': ([-1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 6, 6], [7, 8, 9, 10, 11, 12]),
}


def num_dofs(dim):
    """N of the P1 space the contexts of this file are built on: disc(4) and interval(10)"""
    return {1: 1023, 2: 721}[dim]


def synthetic_tree(kind, dim, partial, far_kind='mixed', seed=0):
    """dict(parent, level, nlevels, box[nnodes][dim][2], leaves = [(node, sorted dofs)] as the plan lists them, all_leaves, far[nfar][2],
    N).  partial: the plan lists only some of the leaves (and, for the single node, only some of the DoFs)."""
    N = num_dofs(dim)
    rng = np.random.default_rng([seed, dim, partial, KINDS.index(kind)])
    parent, leaf_nodes = _SHAPES[kind]
    parent, leaf_nodes = np.array(parent), np.array(leaf_nodes)
    nn = len(parent)
    if kind == 'unbalanced':
        # the node numbers carry no order: the root is not node 0, parents may follow their children
        perm = rng.permutation(nn)
        newp = np.full(nn, -1)
        for k in range(nn):
            newp[perm[k]] = perm[parent[k]] if parent[k] >= 0 else -1
        parent, leaf_nodes = newp, perm[leaf_nodes]
        assert parent[0] != -1 or nn == 1
    level = np.zeros(nn, dtype=np.int64)
    for k in range(nn):
        p, l = parent[k], 0
        while p >= 0:
            p, l = parent[p], l+1
        level[k] = l
    sizes = list(SPECIAL_LEAVES[:max(len(leaf_nodes)-(1 if kind == 'gap' else 2), 0)])
    rest = N-sum(sizes)
    nrest = len(leaf_nodes)-len(sizes)
    sizes += [rest//nrest+(1 if i < rest % nrest else 0) for i in range(nrest)]
    assert sum(sizes) == N and len(sizes) == len(leaf_nodes)
    order = rng.permutation(N)                 # interleaved DoF sets
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    all_leaves = [(int(leaf_nodes[i]), np.sort(order[cuts[i]:cuts[i+1]]).astype(np.int32)) for i in range(len(leaf_nodes))]
    leaves = list(all_leaves)
    if partial:
        if len(leaves) == 1:
            leaves = [(leaves[0][0], leaves[0][1][rng.random(N) < 0.5])]
        else:
            leaves = [lf for i, lf in enumerate(leaves) if i not in (1, len(leaves)-1)]     # drops the 1-DoF leaf and a large one
    leaves = [leaves[i] for i in rng.permutation(len(leaves))]
    a = rng.uniform(-1., 1., size=(nn, dim))
    box = np.stack([a, a+rng.uniform(0.1, 1., size=(nn, dim))], axis=2)
    far = []
    if far_kind == 'mixed':
        if nn == 1:
            far = [(0, 0)]
        else:
            root = int(np.nonzero(parent < 0)[0][0])
            lv = [n for n, _ in all_leaves]
            inner = [k for k in range(nn) if k not in lv and k != root]
            hub = lv[2]
            far += [(hub, n2) for n2 in (lv+inner)[:8]]                       # many pairs of one n1, its self pair among them
            far += [(n, n) for n in (lv[0], inner[0], root)]                  # self pairs
            far += [(root, lv[1]), (lv[3], root), (inner[0], lv[-1]), (lv[-1], inner[-1])]       # across levels
            far += [(lv[0], lv[4]), (lv[4], lv[0]), (inner[0], inner[-1]), (inner[-1], inner[0])]      # both orientations
            far += [(hub, lv[3]), (hub, lv[3])]                               # the same pair twice, two blocks
            far += [(int(rng.integers(nn)), int(rng.integers(nn))) for _ in range(6)]
            far = [far[i] for i in rng.permutation(len(far))]
    return dict(parent=parent.astype(np.int32), level=level.astype(np.int32), nlevels=int(level.max())+1, box=box, leaves=leaves,
                all_leaves=all_leaves, far=np.array(far, dtype=np.int32).reshape(-1, 2), N=N, kind=kind, dim=dim, partial=partial)


def signed_permutations(rng, M):
    """P1 D1 + P2 D2, D diagonal +-1, P2 = P1 shifted by 1 .. M - 1 rows (no collision): exactly two entries per row and column"""
    T = np.zeros((M, M), dtype=np.int64)
    perm = rng.permutation(M)
    T[np.arange(M), perm] = rng.choice([-1, 1], size=M)
    T[np.arange(M), np.roll(perm, int(rng.integers(1, M)))] = rng.choice([-1, 1], size=M)
    return T


def exact_data(t, m, seed=1):
    """integer V (per listed leaf), T[nnodes], K[nfar], x, y0"""
    M = m**t['dim']
    rng = np.random.default_rng([seed, m, t['dim'], KINDS.index(t['kind']), t['partial']])
    nn = len(t['parent'])
    V = [rng.integers(-2, 3, size=(len(d), M), dtype=np.int64) for _, d in t['leaves']]
    if M <= 4:
        T = rng.integers(-3, 4, size=(nn, M, M), dtype=np.int64)
    else:
        T = np.stack([signed_permutations(rng, M) for _ in range(nn)])
    K = rng.integers(-4, 5, size=(len(t['far']), M, M), dtype=np.int64)
    x = rng.integers(-3, 4, size=t['N'], dtype=np.int64)
    x[x == 0] = 1
    y0 = rng.integers(-1024, 1025, size=t['N'], dtype=np.int64)
    return V, T, K, x, y0


def rounding_data(t, m, seed=2):
    M = m**t['dim']
    rng = np.random.default_rng([seed, m, t['dim'], KINDS.index(t['kind']), t['partial']])

    def r(shape):
        return rng.standard_normal(shape)*10.**rng.uniform(-3., 3., size=shape)
    nn = len(t['parent'])
    return [r((len(d), M)) for _, d in t['leaves']], r((nn, M, M)), r((len(t['far']), M, M)), r(t['N']), r(t['N'])


# ---- expected values: level by level, and through the dense operator ------------------------------------------------------------

def _by_level(t, deepest_first):
    lv = t['level']
    out = [[int(c) for c in np.nonzero(lv == l)[0]] for l in range(1, t['nlevels'])]
    return out[::-1] if deepest_first else out


def ref_upward(t, V, T, x):
    """cup[nnodes][M]: 0; cup[leaf] = V^T x[dofs]; deepest level first: cup[parent] += T_child cup[child]"""
    M = T.shape[1]
    cup = np.zeros((len(t['parent']), M), dtype=np.result_type(V[0], T, x))
    for (node, dofs), v in zip(t['leaves'], V):
        cup[node] = v.T@x[dofs]
    for nodes in _by_level(t, True):
        for c in nodes:
            cup[t['parent'][c]] += T[c]@cup[c]
    return cup


def ref_interact(t, K, cup):
    cdown = np.zeros_like(cup)
    for p, (n1, n2) in enumerate(t['far']):
        cdown[n1] += K[p]@cup[n2]
    return cdown


def ref_downward(t, V, T, cdown, y0):
    """(cdown after the pass, y): from the root cdown[child] += T_child^T cdown[parent]; y[dofs] += V cdown[leaf]"""
    cdown = cdown.copy()
    y = y0.astype(cdown.dtype) if cdown.dtype != object else y0.copy()
    for nodes in _by_level(t, False):
        for c in nodes:
            cdown[c] += T[c].T@cdown[t['parent'][c]]
    for (node, dofs), v in zip(t['leaves'], V):
        y[dofs] += v@cdown[node]
    return cdown, y


def ref_matvec(t, V, T, K, x, y0):
    cup = ref_upward(t, V, T, x)
    cd0 = ref_interact(t, K, cup)
    cd1, y = ref_downward(t, V, T, cd0, y0)
    return cup, cd0, cd1, y


def dense_operator(t, V, T, K, dtype=np.float64):
    """F = sum_pairs W_n1 K W_n2^T, W_leaf[dofs] = V_leaf, W_parent = sum_children W_child T_child^T (N x M each)"""
    nn, M, N = len(t['parent']), T.shape[1], t['N']
    W = np.zeros((nn, N, M), dtype=dtype)
    for (node, dofs), v in zip(t['leaves'], V):
        W[node][dofs] = v
    for nodes in _by_level(t, True):
        for c in nodes:
            W[t['parent'][c]] += W[c]@T[c].T.astype(dtype)
    F = np.zeros((N, N), dtype=dtype)
    for p, (n1, n2) in enumerate(t['far']):
        F += W[n1]@(K[p].astype(dtype)@W[n2].T)
    return F


def exact_bound(t, V, T, K, x, y0):
    """largest value any partial sum of any stage can reach: the chain on absolute values, in exact integers.  The float64 run of the
    same chain (which cannot wrap) shows that the int64 one did not."""
    av, at, ak, ax, ay = [np.abs(v) for v in V], np.abs(T), np.abs(K), np.abs(x), np.abs(y0)
    outs = ref_matvec(t, av, at, ak, ax, ay)
    fl = ref_matvec(t, [v.astype(np.float64) for v in av], at.astype(np.float64), ak.astype(np.float64), ax.astype(np.float64),
                    ay.astype(np.float64))
    assert max(float(o.max()) for o in fl) < 2.**62
    return max(int(o.max()) for o in outs)


def stage_products(t, m):
    """(sum of the products per stage, c) of (R)"""
    M = m**t['dim']
    depth = max(int(t['level'][n]) for n, _ in t['leaves'])
    nd = max(len(d) for _, d in t['leaves'])
    kids = np.zeros(len(t['parent']), dtype=int)
    for c, p in enumerate(t['parent']):
        if p >= 0:
            kids[p] += 1
    merges = sum(int(kids[t['level'] == l].max()) for l in range(t['nlevels']-1))
    pairs = int(np.bincount(t['far'][:, 0]).max()) if len(t['far']) else 0
    return nd+M*depth+M+M*depth+M, merges+pairs+depth+1+4


def hp_array(a):
    a = np.asarray(a)
    if LD_OK:
        return a.astype(LD)
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [mpmath.mpf(float(v)) for v in a.ravel()]
    return out


# ---- CPU-only: the references themselves ---------------------------------------------------------------------------------------

def test_trees_are_what_they_claim():
    for dim in (1, 2):
        for kind in KINDS:
            for partial in (0, 1):
                t = synthetic_tree(kind, dim, partial)
                parent, level = t['parent'], t['level']
                assert (parent < 0).sum() == 1
                assert all(level[k] == level[parent[k]]+1 for k in range(len(parent)) if parent[k] >= 0)
                alld = np.concatenate([d for _, d in t['all_leaves']])
                assert sorted(alld.tolist()) == list(range(t['N']))
                for _, d in t['leaves']:
                    assert np.all(np.diff(d) > 0)
                    assert len(d) < 3 or len(d) == t['N'] or d[-1]-d[0] > len(d), 'DoF sets are interleaved, not ranges'
                assert np.all(t['box'][:, :, 1]-t['box'][:, :, 0] >= 0.1)
                listed = sum(len(d) for _, d in t['leaves'])
                assert (listed < t['N']) == bool(partial)
                sizes = sorted(len(d) for _, d in t['leaves'])
                kids = np.bincount(parent[parent >= 0], minlength=len(parent))
                if kind == 'unbalanced':
                    assert {1, 2, 5} <= set(kids.tolist())
                    assert {1, 2, 3, 4, 5} == {int(level[n]) for n, _ in t['all_leaves']}
                    assert parent[0] >= 0
                    assert set(sizes) >= ({0, 63, 64, 65, 300} if partial else set(SPECIAL_LEAVES))
                if kind == 'balanced' and not partial:
                    assert set(sizes) >= set(SPECIAL_LEAVES)
                if kind == 'gap':
                    lv = {n for n, _ in t['all_leaves']}
                    dead = [k for k in range(len(parent)) if kids[k] == 0 and k not in lv]
                    assert len(dead) == 1 and level[dead[0]] == 2
                if kind != 'single':
                    far = [tuple(p) for p in t['far'].tolist()]
                    assert max(np.bincount(t['far'][:, 0])) >= 8
                    assert any(a == b for a, b in far) and any((b, a) in far for a, b in far if a != b)
                    assert any(level[a] != level[b] for a, b in far)
                else:
                    assert t['far'].tolist() == [[0, 0]]
    assert synthetic_tree('balanced', 2, 0, 'empty')['far'].shape == (0, 2)


def test_level_reference_equals_dense_operator_and_loops():
    """the two expected-value helpers agree with each other and with plain loops over Python integers; the data are not symmetric,
    so a transposed T or K, or a swapped pair, changes the result"""
    for dim, m, kind, partial in ((2, 2, 'unbalanced', 0), (1, 3, 'gap', 1), (2, 3, 'balanced', 1), (1, 1, 'single', 0), (2, 7, 'unbalanced', 1)):
        t = synthetic_tree(kind, dim, partial)
        V, T, K, x, y0 = exact_data(t, m)
        M = m**dim
        cup, cd0, cd1, y = ref_matvec(t, V, T, K, x, y0)
        F = dense_operator(t, V, T, K, np.int64)
        assert np.array_equal(y, y0+F@x)
        assert np.array_equal(dense_operator(t, V, T, K).astype(np.int64), F)
        # loops
        nn = len(t['parent'])
        cu = [[0]*M for _ in range(nn)]
        for (node, dofs), v in zip(t['leaves'], V):
            for a in range(M):
                cu[node][a] = sum(int(x[I])*int(v[k, a]) for k, I in enumerate(dofs))
        for l in range(t['nlevels']-1, 0, -1):
            for c in range(nn):
                if t['level'][c] == l:
                    for i in range(M):
                        cu[t['parent'][c]][i] += sum(int(T[c, i, j])*cu[c][j] for j in range(M))
        assert [[int(v) for v in row] for row in cup] == cu
        cd = [[0]*M for _ in range(nn)]
        for p, (n1, n2) in enumerate(t['far']):
            for i in range(M):
                cd[n1][i] += sum(int(K[p, i, j])*cu[n2][j] for j in range(M))
        assert [[int(v) for v in row] for row in cd0] == cd
        for l in range(1, t['nlevels']):
            for c in range(nn):
                if t['level'][c] == l:
                    for j in range(M):
                        cd[c][j] += sum(int(T[c, i, j])*cd[t['parent'][c]][i] for i in range(M))
        assert [[int(v) for v in row] for row in cd1] == cd
        yy = [int(v) for v in y0]
        for (node, dofs), v in zip(t['leaves'], V):
            for k, I in enumerate(dofs):
                yy[I] += sum(int(v[k, a])*cd[node][a] for a in range(M))
        assert [int(v) for v in y] == yy
        if len(t['far']) > 1 and M > 1:
            Tt = np.ascontiguousarray(np.swapaxes(T, 1, 2))
            Kt = np.ascontiguousarray(np.swapaxes(K, 1, 2))
            assert not np.array_equal(ref_matvec(t, V, Tt, K, x, y0)[0], cup)
            assert not np.array_equal(ref_matvec(t, V, T, Kt, x, y0)[1], cd0)
            assert not np.array_equal(F, F.T)
        if partial:
            unl = np.setdiff1d(np.arange(t['N']), np.concatenate([d for _, d in t['leaves']]))
            xp = x.copy(); xp[unl] = POISON
            assert np.array_equal(ref_matvec(t, V, T, K, xp, y0)[3], y) and np.array_equal(y[unl], y0[unl])
            assert not F[unl].any() and not F[:, unl].any()


@pytest.mark.parametrize('case', EXACT_CASES, ids=_case_id)
def test_exact_cases_stay_below_2_53(case):
    """the condition of (E), per case: the chain on absolute values, one-hot and random x alike (|x| >= 1 everywhere, so the random
    vector dominates every one-hot vector), stays below 2^53"""
    dim, m, kind, partial, far_kind = case
    t = synthetic_tree(kind, dim, partial, far_kind)
    V, T, K, x, y0 = exact_data(t, m)
    assert np.abs(x).min() >= 1
    b = exact_bound(t, V, T, K, x, y0)
    assert b+POISON < LIMIT, (b, np.log2(float(b)))
    if m**dim > 2 and len(t['parent']) > 1:
        assert any(not np.array_equal(Tk, Tk.T) for Tk in T)
        assert all(Tk.any(axis=0).all() and Tk.any(axis=1).all() for Tk in T) or m**dim <= 4
        assert m**dim <= 4 or all(((Tk != 0).sum(axis=0) == 2).all() and ((Tk != 0).sum(axis=1) == 2).all() for Tk in T)


def test_stage_products():
    t = synthetic_tree('unbalanced', 2, 0)
    n, c = stage_products(t, 7)
    nd = max(len(d) for _, d in t['leaves'])
    assert n == nd+49*5+49+49*5+49
    # children merged per level: 2, 5, 2, 1 (levels 0 .. 3 hold nodes with 2 / 5 / 2 and 1 / 1 and 2 children), 2 at level 4
    assert c == (2+5+2+2+2)+int(np.bincount(t['far'][:, 0]).max())+5+1+4
    t = synthetic_tree('single', 1, 0)
    assert stage_products(t, 3) == (t['N']+3+3, 0+1+0+1+4)


# ---- transfer matrices: pnl_h2_transfer_matrices (host) and h2.transferMatrix against mpmath ------------------------------------

def mp_nodes(a, b, m):
    """exact Chebyshev nodes of [a, b] (a, b doubles): (b - a) / 2 (cos((2 (m - j) - 1) pi / (2 m)) + 1) + a"""
    a, b = mpmath.mpf(float(a)), mpmath.mpf(float(b))
    return [(b-a)/2*(mpmath.cos(mpmath.mpf(2*(m-j)-1)/(2*m)*mpmath.pi)+1)+a for j in range(m)]


def box_scale(a, b):
    return max(abs(float(a)), abs(float(b)))+(float(b)-float(a))


def mp_lagrange_table(nodes, S, xs):
    """L[l][q] = l-th Lagrange polynomial on `nodes` at xs[q], and cond[l][q] = sum_(k != l) (S / |x - x_k| + S / |x_l - x_k|);
    a factor that vanishes exactly (x on a node) contributes nothing to cond: the value is then judged against the rest"""
    m = len(nodes)
    L = [[None]*len(xs) for _ in range(m)]
    cond = [[None]*len(xs) for _ in range(m)]
    for l in range(m):
        den = [nodes[l]-nodes[k] for k in range(m)]
        cden = sum(S/abs(den[k]) for k in range(m) if k != l)
        for q, x in enumerate(xs):
            v, c = mpmath.mpf(1), cden
            for k in range(m):
                if k != l:
                    d = x-nodes[k]
                    v *= d/den[k]
                    c += S/abs(d) if d != 0 else 0
            L[l][q], cond[l][q] = v, c
    return L, cond


TRANSFER_BOXES = {
    'nested': ([[-0.3, 0.9], [0.1, 0.75]], [[-0.1, 0.35], [0.3, 0.55]]),
    'equal': ([[-0.3, 0.9], [0.1, 0.75]], [[-0.3, 0.9], [0.1, 0.75]]),
    'corner': ([[-0.3, 0.9], [0.1, 0.75]], [[0.4, 0.9], [0.1, 0.3]]),
    'far from 0': ([[100.25, 100.75], [-7., -6.5]], [[100.5, 100.75], [-6.875, -6.75]]),
}


@pytest.mark.parametrize('m', (1, 2, 5, 9, 16))
@pytest.mark.parametrize('dim', (1, 2))
def test_transfer_matrices_against_mpmath(dim, m):
    """T[I][J] = L^parent_I(xi^child_J): the native host builder and the numpy one, every entry, within
    CV u |T| (4 (m - 1) dim + dim + sum_d sum_k (S / |x - x_k| + S / |x_l - x_k|)), S the parent's box scale (the child's nodes
    carry u of the child's scale, which is not larger for a nested box; the far-from-0 boxes have both alike); a child equal to
    its parent gives the identity and every column sums to 1 (the Lagrange polynomials are a partition of unity), to the bound"""
    from pynucleus_amd import _lib
    from pynucleus_amd.h2 import transferMatrix
    mpmath.mp.dps = 40
    M = m**dim
    names = list(TRANSFER_BOXES)
    box = np.zeros((1+len(names), dim, 2))
    parent = np.full(1+len(names), -1, dtype=np.int32)
    out = np.full((1+len(names), M, M), np.nan)
    # one plan per parent box would do; here every case is a two-node tree of its own, run one after the other
    worst = 0.
    for name in names:
        bp, bc = np.array(TRANSFER_BOXES[name][0][:dim]), np.array(TRANSFER_BOXES[name][1][:dim])
        bx = np.ascontiguousarray(np.stack([bp, bc]))
        par = np.array([-1, 0], dtype=np.int32)
        res = np.full((2, M, M), np.nan)
        rc = _lib.load().pnl_h2_transfer_matrices(2, dim, m, bx.ctypes.data, par.ctypes.data, res.ctypes.data)
        assert rc == PNL_OK
        assert not res[0].any(), 'the root has no transfer block'
        tabs = []
        for d in range(dim):
            S = max(box_scale(*bp[d]), box_scale(*bc[d]))
            tabs.append(mp_lagrange_table(mp_nodes(bp[d, 0], bp[d, 1], m), S, mp_nodes(bc[d, 0], bc[d, 1], m)))
        ref = np.empty((M, M), dtype=object)
        tol = np.empty((M, M))
        for i in range(M):
            for j in range(M):
                v, c = mpmath.mpf(1), 4*(m-1)*dim+dim
                for d in range(dim):
                    l, q = (i//m**d) % m, (j//m**d) % m
                    v *= tabs[d][0][l][q]
                    c += tabs[d][1][l][q]
                ref[i, j], tol[i, j] = v, float(CV*U*abs(v)*c)
        for what, got in (('pnl_h2_transfer_matrices', res[1]), ('h2.transferMatrix', transferMatrix(bp, bc, m))):
            for i in range(M):
                for j in range(M):
                    err = float(abs(mpmath.mpf(float(got[i, j]))-ref[i, j]))
                    # an entry that vanishes exactly (a child node on a parent node) is judged against the scale of its column
                    t = tol[i, j] if ref[i, j] != 0 else CV*U*(4*(m-1)*dim+dim)*m
                    assert err <= t, '{} {} dim={} m={} entry ({}, {}): got {!r}, reference {}, error {:.3e} > {:.3e}'.format(
                        what, name, dim, m, i, j, got[i, j], mpmath.nstr(ref[i, j], 20), err, t)
                    worst = max(worst, err/t) if t else worst
            coltol = tol.sum(axis=0)+U*M
            assert np.all(np.abs(got.sum(axis=0)-1.) <= coltol), (what, name, 'columns sum to 1')
            if name == 'equal':
                assert np.all(np.abs(got-np.eye(M)) <= np.maximum(tol, CV*U*(4*(m-1)*dim+dim)*m)), (what, 'identity')
    print('transfer matrices dim={} m={}: largest error / tolerance {:.3f}'.format(dim, m, worst))
    assert parent[0] == -1 and box.shape[0] == out.shape[0]


# ---- device plumbing ------------------------------------------------------------------------------------------------------------

_BUILDERS = {}


def _p1_builder(dim, fresh=False):
    """nonlocalBuilder on disc(4) / interval(10), P1, fractional kernel: its context() knows the mesh, the DoF map and N"""
    from pynucleus_amd import disc, interval, P1_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    if fresh or dim not in _BUILDERS:
        mesh = disc(4) if dim == 2 else interval(10)
        b = nonlocalBuilder(P1_DoFMap(mesh, PHYSICAL), getFractionalKernel(dim, 0.75 if dim == 2 else 0.25), {})
        assert b.dm.num_dofs == num_dofs(dim)
        if fresh:
            return b
        _BUILDERS[dim] = b
    return _BUILDERS[dim]


def test_num_dofs():
    from pynucleus_amd import disc, interval, P1_DoFMap, PHYSICAL
    assert P1_DoFMap(disc(4), PHYSICAL).num_dofs == num_dofs(2) and P1_DoFMap(interval(10), PHYSICAL).num_dofs == num_dofs(1)
    assert min(num_dofs(1), num_dofs(2)) >= sum(SPECIAL_LEAVES)+2


def _plan(t, m, T, keep, **override):
    """pnl_h2_plan of a synthetic tree: no cells (the leaf-value kernel has nothing to do), a one-point rule"""
    from pynucleus_amd._lib import pnl_h2_plan

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data
    v = dict(parent=t['parent'], level=t['level'], nlevels=t['nlevels'], far=t['far'], leaves=t['leaves'], m=m, partial=t['partial'])
    v.update(override)
    leaves = v['leaves']
    P = pnl_h2_plan()
    P.nnodes, P.nleaves, P.nfar = len(v['parent']), len(leaves), len(v['far'])
    P.m, P.nlevels, P.nq = v['m'], v['nlevels'], 1
    P.box = ptr(t['box'], np.float64)
    P.parent, P.level = ptr(v['parent'], np.int32), ptr(v['level'], np.int32)
    P.leaf_node = ptr([n for n, _ in leaves], np.int32)
    P.leaf_dof_off = ptr(np.concatenate([[0], np.cumsum([len(d) for _, d in leaves])]), np.int32)
    P.leaf_dofs = ptr(np.concatenate([d for _, d in leaves]+[np.zeros(0, dtype=np.int32)]), np.int32)
    P.leaf_cell_off = ptr(np.zeros(len(leaves)+1), np.int32)
    P.leaf_cells = ptr(np.zeros(1), np.int32)
    P.far = ptr(v['far'], np.int32)
    P.transfer = ptr(T, np.float64)
    P.qbary, P.qw, P.qphi = ptr(np.full(3, 1./3.), np.float64), ptr(np.ones(1), np.float64), ptr(np.full(8, 0.5), np.float64)
    P.far_class = None
    P.partial_leaves = int(v['partial'])
    return P


def _install(ctx, t, m, V, T, K):
    """pnl_h2_setup of the synthetic plan, then K and V through pnl_h2_set; pnl_h2_get returns the same bits"""
    keep = []
    P = _plan(t, m, T, keep)
    ctx.check(ctx.L.pnl_h2_setup(ctx.h, C.byref(P)))
    ctx._h2_owner = None
    Kf = np.ascontiguousarray(K, dtype=np.float64)
    Vf = np.ascontiguousarray(np.concatenate(list(V)+[np.zeros((0, T.shape[1]))]), dtype=np.float64)
    for which, a in ((0, Kf), (1, Vf)):
        if a.size:
            ctx.check(ctx.L.pnl_h2_set(ctx.h, which, a.ctypes.data))
    for which, a in ((0, Kf), (1, Vf)):
        back = np.full(a.size+2, float(POISON))
        ctx.check(ctx.L.pnl_h2_get(ctx.h, which, back[1:].ctypes.data))
        assert back[0] == POISON and back[-1] == POISON and np.array_equal(back[1:-1], a.ravel()), 'pnl_h2_get(which={})'.format(which)
    sz = np.full(4, -7, dtype=np.int32)
    ctx.check(ctx.L.pnl_h2_sizes(ctx.h, sz[1:].ctypes.data))
    assert sz.tolist() == [-7, len(t['parent']), T.shape[1], -7]


def _guarded(a):
    """(storage, view): the values on the device with GUARD elements of 2^30 before and after"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    host = np.full(a.size+2*GUARD, float(POISON))
    host[GUARD:GUARD+a.size] = a
    store = torch.from_numpy(host).cuda()
    return store, store[GUARD:GUARD+a.size]


def _back(ctx, store, shape, what):
    ctx.synchronize()
    h = store.cpu().numpy()
    assert np.all(h[:GUARD] == POISON) and np.all(h[-GUARD:] == POISON), 'write outside '+what
    return h[GUARD:-GUARD].reshape(shape).copy()


def _phases(ctx, t, M, x, y0):
    """(cup, cdown after interact, cdown after downward, y of the phases, y of pnl_h2_matvec); cup and cdown arrive poisoned"""
    nn = len(t['parent'])
    L, h = ctx.L, ctx.h
    xs, xv = _guarded(x)
    us, uv = _guarded(np.full(nn*M, POISON))
    ds, dv = _guarded(np.full(nn*M, POISON))
    ys, yv = _guarded(y0)
    ms, mv = _guarded(y0)
    p = lambda v: C.c_void_p(v.data_ptr())
    ctx.check(L.pnl_h2_upward(h, p(xv), p(uv)))
    cup = _back(ctx, us, (nn, M), 'cup')
    ctx.check(L.pnl_h2_interact(h, p(uv), p(dv)))
    cd0 = _back(ctx, ds, (nn, M), 'cdown')
    assert np.array_equal(_back(ctx, us, (nn, M), 'cup'), cup), 'pnl_h2_interact changed cup'
    ctx.check(L.pnl_h2_downward(h, p(dv), p(yv)))
    cd1 = _back(ctx, ds, (nn, M), 'cdown')
    y = _back(ctx, ys, (t['N'],), 'y')
    ctx.check(L.pnl_h2_matvec(h, p(xv), p(mv)))
    ym = _back(ctx, ms, (t['N'],), 'y')
    assert np.array_equal(_back(ctx, xs, (t['N'],), 'x'), np.asarray(x, dtype=np.float64)), 'x was written'
    return cup, cd0, cd1, y, ym


def _assert_exact(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError('{}: {} of {} entries differ, first at {}: got {!r}, expected {!r}'.format(
            what, len(bad), ref.size, bad[:6].tolist(), [got[tuple(b)] for b in bad[:4]], [ref[tuple(b)] for b in bad[:4]]))


def hot_dofs(t):
    """first and last DoF of every listed leaf; the 64th and 65th DoF of the leaves that have them"""
    out = set()
    for _, d in t['leaves']:
        if len(d):
            out |= {int(d[0]), int(d[-1])}
        if len(d) >= 65:
            out |= {int(d[63]), int(d[64])}
    return sorted(out)


# ---- (E) ------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('case', EXACT_CASES, ids=_case_id)
def test_phases_exact(case):
    """(E): every entry of cup, of cdown after pnl_h2_interact and after pnl_h2_downward, and of y, bit for bit, for a random integer
    x and for one-hot x (component i of y - y0 is then the entry (i, k) of the far-field operator); pnl_h2_matvec gives the bits of
    the three phases; with partial_leaves x holds 2^30 at the DoFs of no listed leaf and y keeps its bits there"""
    dim, m, kind, partial, far_kind = case
    M = m**dim
    t = synthetic_tree(kind, dim, partial, far_kind)
    V, T, K, x, y0 = exact_data(t, m)
    ctx = _p1_builder(dim).context()
    _install(ctx, t, m, V, T, K)
    F = dense_operator(t, V, T, K)
    listed = np.concatenate([d for _, d in t['leaves']])
    unlisted = np.setdiff1d(np.arange(t['N']), listed)
    assert (len(unlisted) > 0) == bool(partial)
    hots = hot_dofs(t)
    if kind == 'single' or M >= 121:
        hots = hots[:2]+hots[-2:]
    for k in [None]+hots:
        if k is None:
            xx, tag = x.copy(), 'random x'
        else:
            xx = np.zeros(t['N'], dtype=np.int64); xx[k] = 1
            tag = 'x=e_{} (y - y0 = column {} of the operator)'.format(k, k)
        ref = ref_matvec(t, V, T, K, xx, y0)
        assert np.array_equal(ref[3].astype(np.float64), y0+F@xx), 'the two references disagree'
        xdev = xx.copy()
        xdev[unlisted] = POISON
        cup, cd0, cd1, y, ym = _phases(ctx, t, M, xdev, y0)
        name = '{} {}: '.format(_case_id(case), tag)
        _assert_exact(cup, ref[0], name+'pnl_h2_upward cup[node][alpha]')
        _assert_exact(cd0, ref[1], name+'pnl_h2_interact cdown[node][alpha]')
        _assert_exact(cd1, ref[2], name+'pnl_h2_downward cdown[node][alpha]')
        _assert_exact(y, ref[3], name+'pnl_h2_downward y')
        _assert_exact(ym, y, name+'pnl_h2_matvec against the three phases')
        assert np.array_equal(y[unlisted], y0[unlisted].astype(np.float64))


@gpu
@pytest.mark.parametrize('dim', (1, 2))
def test_error_paths_and_rejected_plans(dim):
    """PNL_ERR_STATE from every phase entry point before pnl_h2_setup; PNL_ERR_INVALID for two roots, a level that is not its
    parent's + 1, unsorted leaf DoFs, a DoF in two leaves, an uncovered DoF without partial_leaves, m = 0, m = 17 and a far index
    out of range; after each rejected plan the operator installed before still applies, bit for bit"""
    import torch
    b = _p1_builder(dim, fresh=True)
    ctx = b.context()
    L, h = ctx.L, ctx.h
    N = num_dofs(dim)
    buf = torch.zeros(4*N+4096, dtype=torch.float64, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    host = np.zeros(16)
    sz = np.zeros(2, dtype=np.int32)
    for name, rc in (('upward', L.pnl_h2_upward(h, p, p)), ('interact', L.pnl_h2_interact(h, p, p)), ('downward', L.pnl_h2_downward(h, p, p)),
                     ('matvec', L.pnl_h2_matvec(h, p, p)), ('sizes', L.pnl_h2_sizes(h, sz.ctypes.data)),
                     ('get', L.pnl_h2_get(h, 0, host.ctypes.data)), ('set', L.pnl_h2_set(h, 1, host.ctypes.data))):
        assert rc == PNL_ERR_STATE, (name, rc)
    m = 3
    M = m**dim
    t = synthetic_tree('unbalanced', dim, 0)
    V, T, K, x, y0 = exact_data(t, m)
    _install(ctx, t, m, V, T, K)
    ref = ref_matvec(t, V, T, K, x, y0)

    def still_applies(why):
        cup, cd0, cd1, y, ym = _phases(ctx, t, M, x, y0)
        _assert_exact(cup, ref[0], why+': cup')
        _assert_exact(cd1, ref[2], why+': cdown')
        _assert_exact(y, ref[3], why+': y')
        _assert_exact(ym, ref[3], why+': pnl_h2_matvec')
        sz = np.zeros(2, dtype=np.int32)
        assert L.pnl_h2_sizes(h, sz.ctypes.data) == PNL_OK and sz.tolist() == [len(t['parent']), M]
    still_applies('before any rejected plan')
    # the rejected plans describe ANOTHER tree, with another m: whatever a rejected set-up leaves behind would show
    t2 = synthetic_tree('balanced', dim, 0)
    m2 = 2
    T2 = exact_data(t2, m2)[1]
    root = int(np.nonzero(t2['parent'] < 0)[0][0])
    bad = {}
    par = t2['parent'].copy(); par[3] = -1
    bad['two roots'] = dict(parent=par)
    lev = t2['level'].copy(); lev[9] = 2
    bad['a level that is not the parent\'s + 1'] = dict(level=lev)
    lv = [(n, d.copy()) for n, d in t2['leaves']]
    big = max(range(len(lv)), key=lambda i: len(lv[i][1]))
    sw = lv[big][1].copy(); sw[[5, 6]] = sw[[6, 5]]
    bad['unsorted leaf DoFs'] = dict(leaves=lv[:big]+[(lv[big][0], sw)]+lv[big+1:])
    other = [i for i in range(len(lv)) if i != big and len(lv[i][1]) > 10][0]
    sh = np.sort(np.concatenate([lv[other][1][1:], lv[big][1][:1]])).astype(np.int32)
    bad['a DoF in two leaves'] = dict(leaves=[(n, sh if i == other else d) for i, (n, d) in enumerate(lv)], partial=1)
    bad['an uncovered DoF'] = dict(leaves=[(n, d[1:] if i == big else d) for i, (n, d) in enumerate(lv)])
    bad['m = 0'] = dict(m=0)
    bad['m = 17'] = dict(m=17)
    far = t2['far'].copy(); far[4, 1] = len(t2['parent'])
    bad['a far index = nnodes'] = dict(far=far)
    far = t2['far'].copy(); far[0, 0] = -1
    bad['a far index = -1'] = dict(far=far)
    assert root >= 0
    for why, override in bad.items():
        keep = []
        # m = 17 would read 17^dim x 17^dim transfer blocks if it got that far: give it room
        mm = override.get('m', m2)
        Tbig = np.zeros((len(t2['parent']), max(mm, 1)**dim, max(mm, 1)**dim)) if 'm' in override else T2
        P = _plan(t2, mm, Tbig, keep, **{k: v for k, v in override.items() if k != 'm'})
        rc = L.pnl_h2_setup(h, C.byref(P))
        assert rc == PNL_ERR_INVALID, (why, rc)
        still_applies('after the plan with '+why+' was rejected')
    # the uncovered DoF is legal with partial_leaves, and the tree of the rejected plans is a valid one
    keep = []
    P = _plan(t2, m2, T2, keep, **dict(bad['an uncovered DoF'], partial=1))
    assert L.pnl_h2_setup(h, C.byref(P)) == PNL_OK
    assert L.pnl_h2_sizes(h, sz.ctypes.data) == PNL_OK and sz.tolist() == [len(t2['parent']), m2**dim]
    ctx._h2_owner = None


# ---- (R) ------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('case', ROUNDING_CASES, ids=_case_id)
def test_phases_rounding(case):
    """(R): y of the three phases and of pnl_h2_matvec per component within (sum of the stage products + c) u (abs-chain + |y0|)"""
    dim, m, kind, partial = case
    M = m**dim
    t = synthetic_tree(kind, dim, partial)
    V, T, K, x, y0 = rounding_data(t, m)
    ctx = _p1_builder(dim).context()
    _install(ctx, t, m, V, T, K)
    hv, hT, hK, hx, hy = [hp_array(v) for v in V], hp_array(T), hp_array(K), hp_array(x), hp_array(y0)
    ref = ref_matvec(t, hv, hT, hK, hx, hy)[3]
    mag = ref_matvec(t, [abs(v) for v in hv], abs(hT), abs(hK), abs(hx), abs(hy))[3]
    n, c = stage_products(t, m)
    unlisted = np.setdiff1d(np.arange(t['N']), np.concatenate([d for _, d in t['leaves']]))
    xdev = x.copy()
    xdev[unlisted] = POISON
    cup, cd0, cd1, y, ym = _phases(ctx, t, M, xdev, y0)
    worst = 0.
    for what, got in (('phases', y), ('pnl_h2_matvec', ym)):
        g = hp_array(got)
        for i in range(t['N']):
            err, tol = abs(g[i]-ref[i]), (n+c)*U*mag[i]
            assert err <= tol, '{} {} component {}: got {!r}, reference {!r}, error {:.3e} > tol {:.3e}'.format(
                _case_id(case), what, i, got[i], float(ref[i]), float(err), float(tol))
            worst = max(worst, float(err/tol)) if tol else worst
    assert np.array_equal(y[unlisted], y0[unlisted])
    print('(R) {}: n = {}, c = {}, largest error / tolerance {:.4f}'.format(_case_id(case), n, c, worst))


# ---- (C) set-up kernels ---------------------------------------------------------------------------------------------------------

def _c_builder(name, dim, element, m):
    """builder of a real problem: (builder, params)"""
    from pynucleus_amd import disc, interval, uniformSquare, PHYSICAL, NO_BOUNDARY, dofmapFactory, getKernel, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.fractionalOrders import leftRightFractionalOrder
    params = {'eta': 3., 'minClusterSize': 8 if dim == 2 else 4}
    if m is not None:
        params['interpolation_order'] = m
    zero = True
    if name == 'horizon':
        mesh = interval(9) if dim == 1 else uniformSquare(65)
        dm = dofmapFactory(element, mesh, NO_BOUNDARY)
        kernel, zero = getFractionalKernel(dim, 0.75, horizon=0.5 if dim == 1 else 0.25), False
    else:
        mesh = (disc(3) if element != 'P2' else disc(2)) if dim == 2 else interval(6 if element in ('P0', 'P1') else 5)
        if name == 'far_class':
            mesh = uniformSquare(2**4+1, None, -1., -1., 1., 1.) if dim == 2 else interval(7)
        dm = dofmapFactory(element, mesh, PHYSICAL)
        if name.startswith('s='):
            kernel = getFractionalKernel(dim, float(name[2:]))
        elif name == 'gaussian':
            kernel = getKernel(dim, kernel='gaussian', horizon=np.inf, variance=0.3)
        elif name == 'exponential':
            kernel = getKernel(dim, kernel='exponential', horizon=np.inf, exponentialRate=3.)
        else:
            kernel = getFractionalKernel(dim, leftRightFractionalOrder(0.25, 0.75, 0.3, 0.6))
    return nonlocalBuilder(dm, kernel, params, zeroExterior=zero)


def mp_gamma(p, d2):
    """(gamma(d2), own): the kernel of device_params p at d2 in mpmath; own = the relative conditioning to the rounding of the
    kernel's own argument that tests/test_device_math.py allows the device"""
    e, scale = mpmath.mpf(p['exponent']), mpmath.mpf(p['scale'])
    if not d2 <= mpmath.mpf(p['horizon2']):
        return mpmath.mpf(0), 0.
    if p['ktype'] == 0:
        return scale*d2**e, 0.
    if p['ktype'] == 3:
        return scale*mpmath.exp(e*d2), float(abs(e*d2))*U
    assert p['ktype'] == 4, p
    return scale*mpmath.exp(e*mpmath.sqrt(d2)), 2.*float(abs(e)*mpmath.sqrt(d2))*U


def kernel_cond(p, d2):
    """d ln gamma / d ln d2"""
    if p['ktype'] == 0:
        return abs(p['exponent'])
    if p['ktype'] == 3:
        return abs(p['exponent'])*float(d2)
    return 0.5*abs(p['exponent'])*float(mpmath.sqrt(d2))


def sample_entries(rng, M, m, dim, rows=None):
    """(i, j) entries of an M x M block: all of them for <= 64, else 64 seeded ones and every pair of box-corner nodes"""
    if M*M <= 64:
        return [(i, j) for i in range(M) for j in range(M)]
    corners = sorted({sum(c[d]*m**d for d in range(dim)) for c in np.ndindex(*(2,)*dim) for c in [[(m-1)*b for b in c]]})
    out = {(i, j) for i in corners for j in corners}
    flat = rng.choice(M*M, size=64, replace=False)
    out |= {(int(f)//M, int(f) % M) for f in flat}
    return sorted(out)


K_CASES = [('s=0.25', 2, None), ('s=0.5', 2, None), ('s=0.75', 2, None), ('s=0.4', 2, None), ('gaussian', 2, None),
           ('far_class', 2, None), ('s=0.75', 2, 9), ('s=0.25', 1, None), ('s=0.5', 1, None), ('s=0.75', 1, None), ('s=0.4', 1, None),
           ('gaussian', 1, None), ('exponential', 1, None), ('horizon', 1, None), ('far_class', 1, None), ('s=0.75', 1, 16), ('s=0.4', 1, 16)]


def test_sample_entries():
    rng = np.random.default_rng(0)
    assert len(sample_entries(rng, 4, 2, 2)) == 16 and len(sample_entries(rng, 8, 8, 1)) == 64
    s = sample_entries(rng, 81, 9, 2)
    assert 64 <= len(s) <= 64+16 and {(0, 0), (8, 72), (80, 80), (72, 8)} <= set(s)
    s = sample_entries(rng, 16, 16, 1)
    assert {(0, 0), (0, 15), (15, 0), (15, 15)} <= set(s) and len(s) >= 64


@gpu
@pytest.mark.parametrize('name,dim,m', K_CASES, ids=[_case_id(c) for c in K_CASES])
def test_kernel_interpolants_against_mpmath(name, dim, m):
    """k_h2_kernel_interp on the plan of getH2: K[p][i][j] = -2 gamma(|xi_i - eta_j|^2), tensor index with coordinate 0 fastest, per
    entry within (1e-14 + own(d2) + cond delta(d2)) |K| (module docstring)"""
    mpmath.mp.dps = 40
    b = _c_builder(name, dim, 'P1', m)
    h2 = b.getH2()
    pl = h2.plan
    assert pl.far.shape[0] > 0 and (m is None or pl.m == m) and (m is not None or pl.m <= 8)
    K, _ = h2.farFieldData()
    if name == 'far_class':
        assert pl.far_class is not None and len(set(pl.far_class.tolist())) > 1
        params = [c.kernel.device_params() for c in b.tables.classes]
    else:
        assert pl.far_class is None
        params = [b.kernel.device_params()]
    assert (name == 'horizon') == np.isfinite(params[0]['horizon2'])
    mm, M = pl.m, pl.M
    rng = np.random.default_rng(11)
    nodes, scale = {}, {}
    for n in set(pl.far.ravel().tolist()):
        nodes[n] = [mp_nodes(pl.box[n, d, 0], pl.box[n, d, 1], mm) for d in range(dim)]
        scale[n] = [box_scale(pl.box[n, d, 0], pl.box[n, d, 1]) for d in range(dim)]
    worst, judged, skipped = 0., 0, 0
    for p, (n1, n2) in enumerate(pl.far.tolist()):
        kp = params[int(pl.far_class[p])] if pl.far_class is not None else params[0]
        for i, j in sample_entries(rng, M, mm, dim):
            d2, dd = mpmath.mpf(0), mpmath.mpf(0)
            for d in range(dim):
                diff = nodes[n1][d][(i//mm**d) % mm]-nodes[n2][d][(j//mm**d) % mm]
                d2 += diff*diff
                dd += abs(diff)*CN*U*(scale[n1][d]+scale[n2][d])
            delta = float(2*dd/d2)+4*U
            if abs(d2-mpmath.mpf(kp['horizon2'])) <= delta*d2:
                skipped += 1
                continue
            g, own = mp_gamma(kp, d2)
            ref = -2*g
            got = float(K[p, i, j])
            if kp['ktype'] in (3, 4) and abs(ref) < 2e-300*kp['scale']:
                assert -2e-300*kp['scale']*(1.+1e-12) <= got <= 0.
                continue
            tol = (1e-14+own+kernel_cond(kp, d2)*delta)*float(abs(ref))
            err = float(abs(mpmath.mpf(got)-ref))
            assert err <= tol, '{} dim={} m={} pair {} = ({}, {}) entry ({}, {}): got {!r}, reference {}, error {:.3e} > {:.3e}'.format(
                name, dim, mm, p, n1, n2, i, j, got, mpmath.nstr(ref, 20), err, tol)
            worst, judged = max(worst, err/tol) if tol else worst, judged+1
    assert judged >= min(64, M*M)*pl.far.shape[0]-skipped and skipped <= 0.01*judged
    print('K {} dim={} m={}: {} pairs, {} entries judged, {} at the horizon skipped, largest error / tolerance {:.3f}'.format(
        name, dim, mm, pl.far.shape[0], judged, skipped, worst))


V_CASES = [(2, 'P0', None), (2, 'P1', None), (2, 'P2', None), (2, 'P1', 9), (1, 'P0', None), (1, 'P1', None), (1, 'P2', None), (1, 'P3', None),
           (1, 'P1', 16)]


@gpu
@pytest.mark.parametrize('dim,element,m', V_CASES, ids=[_case_id(c) for c in V_CASES])
def test_leaf_values_against_mpmath(dim, element, m):
    """k_h2_leaf_values on the plan of getH2: V[dof][alpha] = sum_cells sum_q vol w_q phi_dof(x_q) L_alpha(x_q) with the uploaded rule
    (qbary, qw, qphi, cell volumes, vertices) as exact doubles; tolerance accumulated from the reference's terms (module docstring)"""
    mpmath.mp.dps = 40
    b = _c_builder('s=0.25' if element == 'P0' else 's=0.75', dim, element, m)      # P0 needs s < 1/2
    h2 = b.getH2()
    pl, dm = h2.plan, b.dm
    mesh = dm.mesh
    assert m is None or pl.m == m
    _, V = h2.farFieldData()
    mm, M, nq, dpe = pl.m, pl.M, pl.qw.shape[0], dm.dofs_per_element
    rng = np.random.default_rng(12)
    mpf = lambda v: mpmath.mpf(float(v))
    worst, judged = 0., 0
    assert sorted(np.concatenate([pl.leaf_dofs[pl.leaf_dof_off[l]:pl.leaf_dof_off[l+1]] for l in range(len(pl.leaf_node))]).tolist()) == \
        list(range(dm.num_dofs))
    for lf, node in enumerate(pl.leaf_node.tolist()):
        dofs = pl.leaf_dofs[pl.leaf_dof_off[lf]:pl.leaf_dof_off[lf+1]]
        cells = pl.leaf_cells[pl.leaf_cell_off[lf]:pl.leaf_cell_off[lf+1]]
        nd = len(dofs)
        if nd*M <= 64:
            want = [(k, a) for k in range(nd) for a in range(M)]
        else:
            flat = rng.choice(nd*M, size=64, replace=False)
            corner = sorted({0, mm-1, M-mm, M-1})
            want = sorted({(int(f)//M, int(f) % M) for f in flat} | {(k, a) for k in (0, nd-1) for a in corner})
        pos = {int(I): k for k, I in enumerate(dofs)}
        wanted_rows = {k for k, _ in want}
        S = [box_scale(pl.box[node, d, 0], pl.box[node, d, 1]) for d in range(dim)]
        nds = [mp_nodes(pl.box[node, d, 0], pl.box[node, d, 1], mm) for d in range(dim)]
        ref = {w: mpmath.mpf(0) for w in want}
        bound = {w: mpmath.mpf(0) for w in want}
        mag = {w: mpmath.mpf(0) for w in want}
        nterms = {w: 0 for w in want}
        for c in cells.tolist():
            loc = [(k, pos[int(dm.dofs[c, k])]) for k in range(dpe) if int(dm.dofs[c, k]) in pos and pos[int(dm.dofs[c, k])] in wanted_rows]
            if not loc:
                continue
            verts = mesh.vertices[mesh.cells[c]]
            vol = mpf(mesh.volVector[c])
            xs = [[sum(mpf(pl.qbary[j, v])*mpf(verts[v, d]) for v in range(dim+1)) for j in range(nq)] for d in range(dim)]
            tabs = [mp_lagrange_table(nds[d], S[d], xs[d]) for d in range(dim)]
            for kk, row in loc:
                for (r, a) in want:
                    if r != row:
                        continue
                    for j in range(nq):
                        Lv, cnd = mpmath.mpf(1), 0
                        for d in range(dim):
                            l = (a//mm**d) % mm
                            Lv *= tabs[d][0][l][j]
                            cnd += tabs[d][1][l][j]
                        term = vol*mpf(pl.qw[j])*mpf(pl.qphi[j, kk])*Lv
                        ref[(r, a)] += term
                        mag[(r, a)] += abs(term)
                        bound[(r, a)] += abs(term)*(4*(mm-1)*dim+dim+3+cnd)
                        nterms[(r, a)] += 1
        for (r, a) in want:
            tol = float(CV*U*(bound[(r, a)]+nterms[(r, a)]*mag[(r, a)]))
            got = float(V[lf][r, a])
            err = float(abs(mpmath.mpf(got)-ref[(r, a)]))
            assert err <= tol, '{} dim={} m={} leaf {} (node {}) dof {} alpha {}: got {!r}, reference {}, error {:.3e} > {:.3e}'.format(
                element, dim, mm, lf, node, int(dofs[r]), a, got, mpmath.nstr(ref[(r, a)], 20), err, tol)
            if tol:
                worst, judged = max(worst, err/tol), judged+1
    print('V {} dim={} m={}: {} leaves, {} values judged, largest error / tolerance {:.4f}'.format(
        element, dim, mm, len(pl.leaf_node), judged, worst))
    assert judged > 0
