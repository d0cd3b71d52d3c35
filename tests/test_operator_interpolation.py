"""Operators interpolated in the fractional order: the node selection (pynucleus_amd/operatorInterpolation.py), the Lagrange weights and the
operator classes (linear_operators.py), the ranged kernel (kernels.py), the two device calls pnl_lincomb / pnl_gemv_multi
(csrc/pnl_interp.hip) through the C ABI on SYNTHETIC blocks in the manner of tests/test_cholesky.py, and the assembled operators end to end.

tests/golden/cheby_intervals.json holds numbers only: for six argument tuples, the arguments and what the reference's
getChebyIntervalsAndNodes (nl/PyNucleus_nl/operatorInterpolation.py:123-265, variableOrder=True) returned, every float as its shortest
round-trip decimal.  It was produced once by loading the reference's module (pure Python / numpy) with a two-line stand-in for its import of
the INDEX / REAL dtype names and dumping intervals and nodes with json.dump; the package's restatement must reproduce it bit for bit.

Kernel constants (csrc/pnl_interp.hip): one wave per row, IP_ROWS = 4 rows per workgroup; a lane takes IP_PAIR = 2 columns per load, a wave
IP_WAVE = 128; a sweep of the wave loads G(m) = 8, 4, 2, 1 such groups for m = 1, 2-3, 4-7, 8-21 blocks, i.e. IP_WAVE G(m) columns.

(E) exact.  A_k integer in [-3, 3], c_k integer in [-4, 4], x and b integer in [-8, 8], alpha in {1, -1, 2}, beta in {0, 1, -1}: every partial
    sum in any order is an integer of magnitude <= |alpha| sum|c_k| 3 * 8 ncols + 8 < 2^53 (exact_bound, asserted per case in int64), so both
    calls must return the int64 result BIT FOR BIT.  Padding columns of B and the elements around B and y hold 2^30 and must still hold it.
(R) rounding.  u = 2^-53, gamma_j = j u / (1 - j u):  |B - sum c_k A_k| <= gamma_m sum|c_k||A_k| entrywise (m products, m - 1 additions with
    FMA) and |y - y*|_i <= gamma_{m+ncols+3} (|alpha| sum_k|c_k||A_k||x| + |beta||b|)_i, both sides in np.longdouble (mpmath on seeded rows where
    longdouble has fewer than 63 mantissa bits).  No other tolerance.
"""
import ctypes as C
import itertools
import json
import os
import numpy as np
import pytest

gpu = pytest.mark.gpu

IP_ROWS, IP_PAIR, IP_WAVE = 4, 2, 128                     # csrc/pnl_interp.hip
GROUP = {1: 8, 2: 4, 3: 4, 5: 2, 21: 1}                   # ip_group(m) for the m of this file
MS = (1, 2, 3, 5, 21)
SWEEPS = sorted({IP_WAVE*g for g in GROUP.values()})      # columns per wave sweep: 128, 256, 512, 1024
DIMS = sorted({1, 2, 3, IP_ROWS-1, IP_ROWS, IP_ROWS+1, IP_PAIR-1, IP_PAIR, IP_PAIR+1, 2049}
              | {s+d for s in SWEEPS for d in (-1, 0, 1)})
assert all(v+d in DIMS for v in (IP_ROWS, IP_PAIR, *SWEEPS) for d in (-1, 0, 1)) and max(DIMS) <= 2049
assert {1, 2, 3, 21} <= set(MS) and {GROUP[m] for m in MS} == {1, 2, 4, 8}
# every column count on a few rows, every row count on a few columns, rectangular blocks both ways round, squares across a sweep
SHAPES = ([(IP_ROWS+1, n) for n in DIMS]+[(n, 3) for n in DIMS]+[(n, IP_WAVE+1) for n in DIMS if n <= 513]
          + [(2049, 5), (5, 2049), (513, 129), (129, 513), (257, 257), (130, 1025)])
LD_PADS = (0, 1, 6)
ALPHAS, BETAS = (1., -1., 2.), (0., 1., -1.)
POISON = 2**30
U = 2.**-53
LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUPLES = [(0.2, 0.8, 2, 0.025, 20, 1, -1), (0.05, 0.95, 2, 1e-6, 20, 1, -1), (0.05, 0.95, 2, 1e-6, 20, 1, 0.3),
          (0.3, 0.7, 0.1, 1e-3, 20, 3, -1), (0.01, 0.99, 5, 1e-10, 12, 1, -1), (0.4, 0.41, 2.83, 0.05, 20, 1, -1)]
COUNTS = [(9, 27), (14, 140), (15, 147), (4, 20), (11, 143), (1, 2)]


def gamma(k):
    return k*U/(1.-k*U)


# ---- 1. interval selection ----------------------------------------------------------------------------------------------------------

def _select(t):
    from pynucleus_amd import getChebyIntervalsAndNodes
    s_left, s_right, delta, eta, M_max, M_min, xi = t
    return getChebyIntervalsAndNodes(s_left, s_right, delta, 0.5, eta, M_max=M_max, M_min=M_min, variableOrder=True, fixedXi=xi)


def test_selection_reproduces_the_reference_bit_for_bit():
    with open(os.path.join(ROOT, 'tests', 'golden', 'cheby_intervals.json')) as f:
        cases = json.load(f)['cases']
    assert len(cases) == len(TUPLES)
    for t, c, (ni, nn) in zip(TUPLES, cases, COUNTS):
        assert t == (c['s_left'], c['s_right'], c['delta'], c['eta'], c['M_max'], c['M_min'], c['fixedXi']) and c['r'] == 0.5
        intervals, nodes = _select(t)
        assert (len(intervals), sum(len(n) for n in nodes)) == (ni, nn)
        assert [[float(a), float(b)] for a, b in intervals] == c['intervals']
        assert [[float(v) for v in n] for n in nodes] == c['nodes']


@pytest.mark.parametrize('t', TUPLES)
def test_selection_properties(t):
    import mpmath
    s_left, s_right, delta, eta, M_max, M_min, xi = t
    intervals, nodes = _select(t)
    assert intervals[0][0] == s_left and intervals[-1][1] == s_right
    assert all(intervals[k][1] == intervals[k+1][0] for k in range(len(intervals)-1))
    for (a, b), n in zip(intervals, nodes):
        assert a < b and M_min+1 <= len(n) <= M_max+1
        assert np.all(np.diff(n) > 0) and a < n[0] and n[-1] < b
        # the Chebyshev formula in 40 digits on the float64 interval ends.  The float64 evaluation c + hw cos(theta), c = (a + b)/2,
        # hw = (b - a)/2, rounds c (<= u |c|), the result (<= u |v|) and hw cos(theta): theta = q pi with three roundings and |theta| <= pi
        # (<= 3 pi u), cos itself (<= 2 u), hw and the product (<= u each), together <= 14 u hw.  "1 ulp" of the node itself cannot hold
        # for any evaluation that forms the centre first (u |c| alone exceeds it for nodes near a small a); where c, hw and v are of
        # one magnitude this bound is about one ulp.
        with mpmath.workdps(40):
            fa, fb = mpmath.mpf(float(a)), mpmath.mpf(float(b))
            exact = [(fa+fb)/2+(fb-fa)/2*mpmath.cos((2*j-1)*mpmath.pi/(2*len(n))) for j in range(len(n), 0, -1)]
            assert all(abs(mpmath.mpf(float(v))-e) <= U*((a+b)/2+v+14*(b-a)/2) for v, e in zip(n, exact))


def test_fixed_order_branches_are_not_implemented():
    from pynucleus_amd import getChebyIntervalsAndNodes
    with pytest.raises(NotImplementedError):
        getChebyIntervalsAndNodes(0.2, 0.8, 2., 0.5, 0.025)
    with pytest.raises(NotImplementedError):
        getChebyIntervalsAndNodes(0.2, 0.8, 2., 0.5, 0.025, doSplitM=True)


def test_admissible_set():
    from pynucleus_amd import admissibleSet
    S = admissibleSet([0.2, 0.8])
    assert S.numParams == 1 and S.ranges.shape == (1, 2)
    assert S.isAdmissible(0.2) and S.isAdmissible(0.8) and S.isAdmissible(np.array([0.5])) and not S.isAdmissible(0.81)
    assert S.getLowerBounds().tolist() == [0.2] and S.getUpperBounds().tolist() == [0.8]


# ---- 2. weights -----------------------------------------------------------------------------------------------------------------------

def _mp_weights(nodes, val, derivative):
    """the Lagrange basis on nodes, differentiated symbolically (product rule on the linear factors), at val in 60 digits"""
    import mpmath
    with mpmath.workdps(60):
        x = [mpmath.mpf(float(v)) for v in nodes]
        t = mpmath.mpf(float(val))
        n = len(x)
        out = []
        for j in range(n):
            others = [i for i in range(n) if i != j]
            den = mpmath.fprod([x[j]-x[i] for i in others])
            if derivative == 0:
                num = mpmath.fprod([t-x[i] for i in others])
            elif derivative == 1:
                num = mpmath.fsum([mpmath.fprod([t-x[i] for i in others if i != a]) for a in others])
            else:
                num = mpmath.fsum([mpmath.fprod([t-x[i] for i in others if i not in (a, b)]) for a in others for b in others if a != b])
            out.append(num/den)
        return out


WEIGHT_CASES = [(n, ab) for n in (2, 5, 11, 21) for ab in ((0.2, 0.8), (0.70, 0.72), (0.05, 0.95))]


@pytest.mark.parametrize('n,ab', WEIGHT_CASES)
def test_weights_against_mpmath(n, ab):
    import mpmath
    from pynucleus_amd.linear_operators import interpolationOperator
    from pynucleus_amd.operatorInterpolation import chebyshevNodes
    a, b = ab
    nodes = chebyshevNodes(n, a, b)
    op = interpolationOperator([None]*n, nodes, a, b, shape=(1, 1))
    for val in (a, b, 0.5*(a+b), a+0.123*(b-a), nodes[n//2], a+0.9*(b-a)):
        for derivative in (0, 1, 2):
            op.set(val, derivative)
            assert op.val == val and op.derivative == derivative and op.numInterpolationNodes == n
            w = op.coeffs
            ref = _mp_weights(nodes, val, derivative)
            scale = max(abs(v) for v in ref)
            tol = 1e-14*scale if scale > 0 else 1e-14              # second derivative with two nodes: exactly 0, absolute bound
            err = max(abs(mpmath.mpf(float(wi))-ri) for wi, ri in zip(w, ref))
            assert err <= tol, (n, ab, val, derivative, float(err), float(tol))
            total = mpmath.fsum([mpmath.mpf(float(wi)) for wi in w])
            assert abs(total-(1 if derivative == 0 else 0)) <= tol, (n, ab, val, derivative, float(total))
    for j in range(n):
        op.set(nodes[j])
        assert np.array_equal(op.coeffs, np.eye(n)[j]), (n, ab, j)                 # exactly one-hot at a node
    with pytest.raises(AssertionError):
        op.set(b+1e-9)
    with pytest.raises(AssertionError):
        op.set(a-1e-9)
    with pytest.raises(NotImplementedError):
        op.set(0.5*(a+b), derivative=3)


# ---- 3. kernel and API plumbing -----------------------------------------------------------------------------------------------------

def test_ranged_kernel():
    from pynucleus_amd import getFractionalKernel, admissibleSet, RangedFractionalKernel, ball2_retriangulation
    from pynucleus_amd.kernels import FractionalKernel, fullSpace
    k = getFractionalKernel(1, admissibleSet([0.2, 0.8]))
    assert isinstance(k, RangedFractionalKernel) and repr(k).startswith('ranged ') and isinstance(k.interaction, fullSpace)
    assert k.sValue == 0.2 and k.admissibleOrders.isAdmissible(0.5) and (k.errorBound, k.M_min, k.M_max, k.xi) == (-1., 1, 20, 0.)
    f, g = k.getFrozenKernel(0.3), getFractionalKernel(1, 0.3)
    assert type(f) is FractionalKernel
    assert (f.sValue, f.scalingValue, f.singularityValue) == (g.sValue, g.scalingValue, g.singularityValue)
    k.setOrder(0.3)
    assert (k.sValue, k.scalingValue, k.singularityValue) == (g.sValue, g.scalingValue, g.singularityValue)
    with pytest.raises(AssertionError):
        k.getFrozenKernel(0.9)
    kh = getFractionalKernel(2, admissibleSet([0.3, 0.7]), horizon=0.5)
    assert isinstance(kh.interaction, ball2_retriangulation) and isinstance(kh.getFrozenKernel(0.4).interaction, ball2_retriangulation)
    gh = getFractionalKernel(2, 0.4, horizon=0.5)
    assert kh.getFrozenKernel(0.4).scalingValue == gh.scalingValue
    with pytest.raises(NotImplementedError):
        getFractionalKernel(1, admissibleSet([0.2, 0.8]), tempered=0.1)
    with pytest.raises(NotImplementedError):
        RangedFractionalKernel(1, admissibleSet([0.2, 0.8]), None, tempered=0.1)


class _HostOp:
    """a numpy-backed stand-in operator"""

    def __init__(self, M):
        self.M = np.asarray(M, dtype=np.float64)
        self.shape = self.M.shape

    def matvec(self, x, y=None):
        return self.M@np.asarray(x)

    def toarray(self):
        return self.M

    @property
    def diagonal(self):
        return np.diag(self.M).copy()


def test_multi_interval_operator_on_host_operators():
    from pynucleus_amd.linear_operators import multiIntervalInterpolationOperator, lagrangeWeights
    from pynucleus_amd.operatorInterpolation import chebyshevNodes
    rng = np.random.default_rng(5)
    intervals = [(0.2, 0.4), (0.4, 0.5), (0.5, 0.8)]
    nodes = [chebyshevNodes(n, a, b) for n, (a, b) in zip((3, 2, 4), intervals)]
    mats = [[rng.standard_normal((5, 5)) for _ in n] for n in nodes]
    calls = [[0]*len(n) for n in nodes]

    def delayed(i, k):
        def make():
            calls[i][k] += 1
            return _HostOp(mats[i][k])
        return make
    A = multiIntervalInterpolationOperator(intervals, nodes, [[delayed(i, k) for k in range(len(n))] for i, n in enumerate(nodes)], shape=(5, 5))
    assert (A.left, A.right, A.numInterpolationNodes) == (0.2, 0.8, 9) and np.isnan(A.get()) and A.shape == (5, 5)
    assert '3 intervals and 9 interpolation nodes' in repr(A)
    x = rng.standard_normal(5)
    with pytest.raises(AssertionError):
        A.matvec(x)                                        # applying before set
    with pytest.raises(AssertionError):
        A.toarray()
    assert calls == [[0, 0, 0], [0, 0], [0, 0, 0, 0]]
    A.set(0.4)                                             # a shared end point: the first interval that contains it
    assert A.selected == 0 and A.get() == 0.4 and A.getSelectedOp() is A.ops[0]
    assert calls == [[1, 1, 1], [0, 0], [0, 0, 0, 0]]
    A.set(0.5)
    assert A.selected == 1 and calls == [[1, 1, 1], [1, 1], [0, 0, 0, 0]]
    for val, derivative in ((0.45, 0), (0.3, 1), (0.3, 2), (0.25, 0)):
        A.set(val, derivative)
        i = 0 if val < 0.4 else 1
        w = lagrangeWeights(nodes[i], val, derivative)
        ref = sum(wk*M for wk, M in zip(w, mats[i]))
        assert np.allclose(A.toarray(), ref, rtol=0, atol=1e-13*np.abs(ref).max())
        assert np.allclose(A.matvec(x), ref@x, rtol=0, atol=1e-13*np.abs(ref).max()*np.abs(x).sum())
        assert np.allclose(A*x, A.dot(x)) and np.allclose(A.diagonal, np.diag(ref), rtol=0, atol=1e-13*np.abs(ref).max())
        with pytest.raises(NotImplementedError):
            A.materialize()                                # host operators are not dense device blocks
    assert calls == [[1, 1, 1], [1, 1], [0, 0, 0, 0]]      # each built exactly once, the third interval never
    with pytest.raises(AssertionError):
        A.set(0.81)
    A.assure_constructed()
    assert calls == [[1, 1, 1], [1, 1], [1, 1, 1, 1]]


# ---- 4. ABI ---------------------------------------------------------------------------------------------------------------------------

def test_abi_of_the_two_calls():
    from pynucleus_amd import _lib
    L = _lib.load()
    assert len(L.pnl_lincomb.argtypes) == 9 and len(L.pnl_gemv_multi.argtypes) == 12
    assert L.pnl_lincomb.restype is C.c_int and L.pnl_gemv_multi.restype is C.c_int and _lib.PNL_INTERP_MAX_OPS == 21
    assert hasattr(C.CDLL(_lib.LIB_PATH), 'pnl_lincomb') and hasattr(C.CDLL(_lib.LIB_PATH), 'pnl_gemv_multi')
    assert hasattr(_lib.Context, 'lincomb') and hasattr(_lib.Context, 'gemv_multi')
    txt = open(os.path.join(ROOT, 'include', 'pnl_hip.h')).read()
    for name, nargs in (('pnl_lincomb', 9), ('pnl_gemv_multi', 12)):
        decl = txt[txt.index('int '+name+'('):]
        assert decl[:decl.index(';')].count(',')+1 == nargs, name


# ---- host helpers of the device tests (tested here without a GPU) -------------------------------------------------------------------

def exact_inputs(rng, m, nrows, ncols):
    A = rng.integers(-3, 4, size=(m, nrows, ncols), dtype=np.int64)
    c = rng.integers(-4, 5, size=m, dtype=np.int64)
    if m == 1:
        c[0] = -3
    else:
        c[rng.permutation(m)[:2]] = (0, -2)               # at least one zero and one negative
    x = rng.integers(-8, 9, size=ncols, dtype=np.int64)
    b = rng.integers(-8, 9, size=nrows, dtype=np.int64)
    return A, c, x, b


def exact_bound(c, ncols, alpha, beta):
    """an upper bound, in exact integers, of every partial sum of both calls"""
    return int(abs(alpha))*int(np.abs(c).sum())*3*8*ncols+int(abs(beta))*8


def exact_results(A, c, x, b, alpha, beta):
    B = np.tensordot(c, A, axes=1)
    return B, int(alpha)*(B@x)+int(beta)*b


def test_exact_helpers():
    rng = np.random.default_rng(0)
    for m in MS:
        A, c, x, b = exact_inputs(rng, m, 7, 2049)
        assert np.abs(A).max() <= 3 and np.abs(c).max() <= 4 and (c < 0).any() and (m == 1 or (c == 0).any())
        assert exact_bound(c, 2049, 2., -1.) <= 21*4*3*8*2049*2+8 < 2**53
        B, y = exact_results(A, c, x, b, 2., -1.)
        assert np.array_equal(B, sum(int(ck)*Ak for ck, Ak in zip(c, A))) and np.array_equal(y, 2*(B@x)-b)
        assert max(np.abs(B).max(), np.abs(y).max()) <= exact_bound(c, 2049, 2., -1.)
    combos = [(LD_PADS[i % 3], LD_PADS[(i//3) % 3]) for i in range(len(SHAPES))]
    assert set(combos) == set(itertools.product(LD_PADS, LD_PADS))
    assert sum(r > 8*c for r, c in SHAPES) >= 2 and sum(c > 8*r for r, c in SHAPES) >= 2


def _ld_weights():
    from pynucleus_amd.linear_operators import lagrangeWeights
    from pynucleus_amd.operatorInterpolation import chebyshevNodes
    w = lagrangeWeights(chebyshevNodes(21, 0.05, 0.95), 0.05+0.123*0.9, 0)
    assert np.sum(w[:-1]*w[1:] < 0) == 19                 # they alternate in sign, except the two around the point of evaluation
    return w


def lincomb_violations(B, A, c, rows):
    """entries of the rows with |B - sum c_k A_k| > gamma_m sum|c_k||A_k|, and the largest ratio"""
    m = len(c)
    if LD_OK:
        ref = np.tensordot(c.astype(LD), A[:, rows].astype(LD), axes=1)
        bound = LD(gamma(m))*np.tensordot(np.abs(c).astype(LD), np.abs(A[:, rows]).astype(LD), axes=1)
        err = np.abs(B[rows].astype(LD)-ref)
        bad = np.argwhere(err > bound)
        return [(int(rows[i]), int(j)) for i, j in bad[:8]], float((err/np.where(bound > 0, bound, 1)).max())
    import mpmath
    bad, worst = [], 0.
    for i in rows:
        for j in range(A.shape[2]):
            ref = mpmath.fsum([mpmath.mpf(float(ck))*mpmath.mpf(float(A[k, i, j])) for k, ck in enumerate(c)])
            bound = gamma(m)*mpmath.fsum([abs(mpmath.mpf(float(ck))*mpmath.mpf(float(A[k, i, j]))) for k, ck in enumerate(c)])
            err = abs(mpmath.mpf(float(B[i, j]))-ref)
            worst = max(worst, float(err/bound) if bound > 0 else float(err))
            if err > bound:
                bad.append((int(i), j))
    return bad[:8], worst


def gemv_violations(y, A, c, x, alpha, beta, b, rows):
    """rows with |y - y*| > gamma_{m+ncols+3} (|alpha| sum_k|c_k||A_k||x| + |beta||b|), and the largest ratio"""
    m, ncols = len(c), A.shape[2]
    g = gamma(m+ncols+3)
    if LD_OK:
        S = np.tensordot(c.astype(LD), A[:, rows].astype(LD), axes=1)
        Sa = np.tensordot(np.abs(c).astype(LD), np.abs(A[:, rows]).astype(LD), axes=1)
        ref = LD(alpha)*(S@x.astype(LD))+LD(beta)*b[rows].astype(LD)
        bound = LD(g)*(LD(abs(alpha))*(Sa@np.abs(x).astype(LD))+LD(abs(beta))*np.abs(b[rows]).astype(LD))
        err = np.abs(y[rows].astype(LD)-ref)
        return [int(rows[i]) for i in np.nonzero(err > bound)[0][:8]], float((err/np.where(bound > 0, bound, 1)).max())
    import mpmath
    f = lambda v: mpmath.mpf(float(v))  # noqa: E731
    bad, worst = [], 0.
    for i in rows:
        S = [mpmath.fsum([f(ck)*f(A[k, i, j]) for k, ck in enumerate(c)]) for j in range(ncols)]
        Sa = [mpmath.fsum([abs(f(ck)*f(A[k, i, j])) for k, ck in enumerate(c)]) for j in range(ncols)]
        ref = f(alpha)*mpmath.fdot(S, [f(v) for v in x])+f(beta)*f(b[i])
        bound = g*(abs(f(alpha))*mpmath.fdot(Sa, [abs(f(v)) for v in x])+abs(f(beta)*f(b[i])))
        err = abs(f(y[i])-ref)
        worst = max(worst, float(err/bound) if bound > 0 else float(err))
        if err > bound:
            bad.append(int(i))
    return bad[:8], worst


def _rows_to_check(nrows):
    return np.arange(nrows) if LD_OK else np.unique(np.r_[0, nrows-1, np.random.default_rng(1).choice(nrows, size=min(nrows, 6), replace=False)])


def test_rounding_helpers_catch_one_ulp():
    """the checkers accept the correctly rounded results and flag an entry that is off by a few ulp of the bound"""
    rng = np.random.default_rng(3)
    c = _ld_weights()
    A = rng.standard_normal((21, 6, 40))*10.**rng.uniform(-3, 3, size=(1, 6, 1))
    x, b = rng.standard_normal(40), rng.standard_normal(6)
    rows = _rows_to_check(6)
    B = np.tensordot(c.astype(LD), A.astype(LD), axes=1).astype(np.float64)
    y = (2*(np.tensordot(c.astype(LD), A.astype(LD), axes=1)@x.astype(LD))-b.astype(LD)).astype(np.float64)
    assert lincomb_violations(B, A, c, rows)[0] == [] and gemv_violations(y, A, c, x, 2., -1., b, rows)[0] == []
    i = int(rows[-1])
    B2, y2 = B.copy(), y.copy()
    B2[i, 7] += 40*gamma(21)*np.abs(c)@np.abs(A[:, i, 7])
    y2[i] += 3*gamma(21+40+3)*(2*(np.abs(c)@np.abs(A[:, i]))@np.abs(x)+abs(b[i]))
    assert lincomb_violations(B2, A, c, rows)[0] == [(i, 7)] and gemv_violations(y2, A, c, x, 2., -1., b, rows)[0] == [i]


# ---- device plumbing ----------------------------------------------------------------------------------------------------------------

def _context():
    import torch
    from pynucleus_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream(0).cuda_stream)
    return ctx


def _dev_block(host, ld, off):
    """(storage, view): the rows of host with leading dimension ld, `off` doubles into a poisoned allocation (off = 2: 16-byte aligned,
    off = 1: not); padding columns and the elements before / after hold 2^30"""
    import torch
    nrows, ncols = host.shape
    full = np.full((nrows, ld), float(POISON))
    full[:, :ncols] = host
    store = torch.full((off+nrows*ld+2,), float(POISON), dtype=torch.float64, device='cuda')
    assert store.data_ptr() % 16 == 0
    view = store[off:off+nrows*ld].view(nrows, ld)
    view.copy_(torch.from_numpy(full))
    return store, view


def _block_and_guards(store, nrows, ncols, ld, off, what):
    h = store.cpu().numpy()
    assert (h[:off] == POISON).all() and (h[off+nrows*ld:] == POISON).all(), what+': write outside the buffer'
    M = h[off:off+nrows*ld].reshape(nrows, ld)
    assert (M[:, ncols:] == POISON).all(), what+': write into the padding columns'
    return M[:, :ncols]


def _run_both(ctx, A, c, x, b, alpha, beta, padA, padB, off, alias):
    """pnl_lincomb and pnl_gemv_multi on host inputs (any dtype, converted to float64) -> (B, y) with the guards checked"""
    import torch
    m, nrows, ncols = A.shape
    ldA, ldB = ncols+padA, ncols+padB
    what = 'm={} {}x{} pads {},{} off {} alpha {} beta {}{}'.format(m, nrows, ncols, padA, padB, off, alpha, beta, ' b=y' if alias else '')
    blocks = [_dev_block(A[k].astype(np.float64), ldA, off) for k in range(m)]
    Bs, Bv = _dev_block(np.full((nrows, ncols), float(POISON)), ldB, off)
    xs, xv = _dev_block(x.astype(np.float64)[None, :], ncols, off)
    bs, bv = _dev_block(b.astype(np.float64)[None, :], nrows, off)
    ys, yv = (bs, bv) if alias else _dev_block(np.full((1, nrows), float(POISON)), nrows, off)
    torch.cuda.current_stream(0).synchronize()
    ptrs = [v.data_ptr() for _, v in blocks]
    ctx.lincomb(ptrs, ldA, nrows, ncols, c.astype(np.float64), Bv.data_ptr(), ldB)
    ctx.gemv_multi(ptrs, ldA, nrows, ncols, c.astype(np.float64), xv.data_ptr(), alpha, beta, bv.data_ptr() if beta != 0. or alias else None,
                   yv.data_ptr())
    ctx.synchronize()
    for k, (s, _) in enumerate(blocks):
        assert np.array_equal(_block_and_guards(s, nrows, ncols, ldA, off, what+' A_{}'.format(k)), A[k].astype(np.float64)), what+': A changed'
    assert np.array_equal(_block_and_guards(xs, 1, ncols, ncols, off, what+' x')[0], x.astype(np.float64))
    return (_block_and_guards(Bs, nrows, ncols, ldB, off, what+' B').copy(), _block_and_guards(ys, 1, nrows, nrows, off, what+' y')[0].copy(), what)


# ---- 5. exact -------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('m', MS)
def test_exact_integer_blocks(m):
    import torch
    ctx = _context()
    rng = np.random.default_rng(100+m)
    ab = itertools.cycle(itertools.product(ALPHAS, BETAS))
    cases = [(s, LD_PADS[i % 3], LD_PADS[(i//3) % 3], 2, False) for i, s in enumerate(SHAPES)]
    cases += [((129, 257), 0, 0, 1, False), ((5, 1025), 1, 6, 1, False), ((130, 129), 6, 0, 2, True), ((3, 2049), 0, 1, 1, True)]
    try:
        for (nrows, ncols), padA, padB, off, alias in cases:
            alpha, beta = next(ab)
            if alias and beta == 0.:
                beta = 1.
            A, c, x, b = exact_inputs(rng, m, nrows, ncols)
            assert exact_bound(c, ncols, alpha, beta) < 2**53
            Bref, yref = exact_results(A, c, x, b, alpha, beta)
            B, y, what = _run_both(ctx, A, c, x, b, alpha, beta, padA, padB, off, alias)
            assert np.array_equal(B, Bref.astype(np.float64)), (what, np.argwhere(B != Bref)[:4])
            assert np.array_equal(y, yref.astype(np.float64)), (what, np.nonzero(y != yref)[0][:4])
    finally:
        ctx.close()
        torch.cuda.empty_cache()


# ---- 6. rounding ------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('shape,off', [((67, 1029), 2), ((130, 257), 2), ((5, 2049), 1), ((258, 127), 2)])
def test_rounding_bounds(shape, off):
    import torch
    ctx = _context()
    rng = np.random.default_rng(shape[0])
    nrows, ncols = shape
    c = _ld_weights()
    A = rng.standard_normal((21, nrows, ncols))*10.**rng.uniform(-3, 3, size=(1, nrows, 1))
    x, b = rng.standard_normal(ncols), rng.standard_normal(nrows)*np.abs(A[0]).max(axis=1)
    rows = _rows_to_check(nrows)
    try:
        for alpha, beta in ((1., 0.), (-1., 1.), (2., -1.)):
            B, y, what = _run_both(ctx, A, c, x, b, alpha, beta, 1 if off == 1 else 0, 6, off, False)
            bad, worst = lincomb_violations(B, A, c, rows)
            print('{}: lincomb error / bound {:.3f}'.format(what, worst))
            assert not bad, (what, bad, worst)
            bad, worst = gemv_violations(y, A, c, x, alpha, beta, b, rows)
            print('{}: gemv_multi error / bound {:.3f}'.format(what, worst))
            assert not bad, (what, bad, worst)
    finally:
        ctx.close()
        torch.cuda.empty_cache()


# ---- 7. reproducibility -------------------------------------------------------------------------------------------------------------

@gpu
def test_reproducible_bits_and_zero_coefficients():
    import torch
    ctx = _context()
    rng = np.random.default_rng(7)
    nrows, ncols = 2049, 1025
    try:
        for m in (3, 21):
            A = rng.standard_normal((m, nrows if m == 3 else 130, ncols))
            c = rng.standard_normal(m)
            x, b = rng.standard_normal(ncols), rng.standard_normal(A.shape[1])
            B1, y1, what = _run_both(ctx, A, c, x, b, 2., -1., 1, 6, 2, False)
            B2, y2, _ = _run_both(ctx, A, c, x, b, 2., -1., 1, 6, 2, False)
            assert np.array_equal(B1, B2) and np.array_equal(y1, y2), what
        # zero coefficients drop out exactly: the middle block alone, whatever the alignment of its neighbours
        A = rng.standard_normal((3, 131, 1027))
        x, b = rng.standard_normal(1027), rng.standard_normal(131)
        e = np.array([0., 1., 0.])
        for off in (2, 1):
            B3, y3, what = _run_both(ctx, A, e, x, b, 1., 0., 0, 1, off, False)
            B1, y1, _ = _run_both(ctx, A[1:2], e[1:2], x, b, 1., 0., 0, 1, off, False)
            assert np.array_equal(B3, A[1]) and np.array_equal(B1, A[1]), what
            assert np.array_equal(y3, y1), what
    finally:
        ctx.close()
        torch.cuda.empty_cache()


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------

@gpu
def test_bad_arguments_are_rejected_on_the_host():
    import torch
    from pynucleus_amd import _lib
    ctx = _context()
    P = C.c_void_p
    n = 8
    A = [torch.full((n, n), float(k+1), dtype=torch.float64, device='cuda') for k in range(22)]
    B = torch.full((n, n), float(POISON), dtype=torch.float64, device='cuda')
    x = torch.ones(n, dtype=torch.float64, device='cuda')
    y = torch.full((n,), float(POISON), dtype=torch.float64, device='cuda')
    coeffs = np.ones(22)
    pc = coeffs.ctypes.data

    def arr(ptrs):
        return (P*len(ptrs))(*ptrs)
    ptrs = [a.data_ptr() for a in A]
    L, h = ctx.L, ctx.h
    INV = _lib.PNL_ERR_INVALID
    torch.cuda.current_stream(0).synchronize()
    try:
        for m, pp in ((0, ptrs[:1]), (22, ptrs), (3, [ptrs[0], None, ptrs[2]])):
            assert L.pnl_lincomb(h, m, arr(pp), n, n, n, pc, P(B.data_ptr()), n) == INV
            assert L.pnl_gemv_multi(h, m, arr(pp), n, n, n, pc, P(x.data_ptr()), 1., 0., None, P(y.data_ptr())) == INV
        assert L.pnl_lincomb(h, 3, arr(ptrs[:3]), n, n, n, pc, P(ptrs[1]), n) == INV                       # B is one of the A_k
        assert L.pnl_lincomb(h, 3, arr(ptrs[:3]), n, n, n, pc, None, n) == INV
        assert L.pnl_lincomb(h, 3, arr(ptrs[:3]), n-1, n, n, pc, P(B.data_ptr()), n) == INV                # ldA < ncols
        assert L.pnl_lincomb(h, 3, None, n, n, n, pc, P(B.data_ptr()), n) == INV
        assert L.pnl_gemv_multi(h, 3, arr(ptrs[:3]), n, n, n, None, P(x.data_ptr()), 1., 0., None, P(y.data_ptr())) == INV
        assert L.pnl_gemv_multi(h, 3, arr(ptrs[:3]), n, n, n, pc, P(x.data_ptr()), 1., 1., None, P(y.data_ptr())) == INV   # beta != 0 without b
        assert L.pnl_gemv_multi(h, 3, arr(ptrs[:3]), n, n, n, pc, P(x.data_ptr()), 1., 0., None, P(x.data_ptr())) == INV   # x is y
        with pytest.raises(AssertionError):
            ctx.lincomb(ptrs, n, n, n, coeffs, B.data_ptr(), n)
        ctx.synchronize()
        assert (B.cpu().numpy() == POISON).all() and (y.cpu().numpy() == POISON).all()
        # a following valid call succeeds
        assert L.pnl_lincomb(h, 3, arr(ptrs[:3]), n, n, n, pc, P(B.data_ptr()), n) == _lib.PNL_OK
        assert L.pnl_gemv_multi(h, 21, arr(ptrs[:21]), n, n, n, pc, P(x.data_ptr()), 1., 0., None, P(y.data_ptr())) == _lib.PNL_OK
        ctx.synchronize()
        assert (B.cpu().numpy() == 6.).all() and (y.cpu().numpy() == n*231.).all()
    finally:
        ctx.close()


# ---- 9. - 11. end to end ----------------------------------------------------------------------------------------------------------------

_CACHE = {}


def _problem(name):
    """(mesh, DoF map, ranged kernel, interpolated operator, eta) of the interval and the disc case, built once"""
    if name not in _CACHE:
        from pynucleus_amd import driverMesh, disc, P1_DoFMap, PHYSICAL, getFractionalKernel, admissibleSet
        if name == 'interval':
            mesh, dim, rng_s = driverMesh('interval', 4), 1, (0.2, 0.8)
        else:
            mesh, dim, rng_s = disc(2), 2, (0.3, 0.7)
        dm = P1_DoFMap(mesh, PHYSICAL)
        kernel = getFractionalKernel(dim, admissibleSet(rng_s))
        _CACHE[name] = (mesh, dm, kernel, dm.assembleNonlocal(kernel, 'dense'), 0.1*mesh.h**0.5)
    return _CACHE[name]


def _direct(name, s):
    """the directly assembled operator at s as a numpy array, assembled once per value"""
    key = (name, float(s))
    if key not in _CACHE:
        _, dm, kernel, _, _ = _problem(name)
        _CACHE[key] = dm.assembleNonlocal(kernel.getFrozenKernel(s), 'dense').toarray().copy()
    return _CACHE[key]


def _combination_violations(M, mats, w):
    """entries with |M - sum w_k A_k| > gamma_m sum|w_k||A_k| (longdouble), the reference sum and the bound"""
    ref = sum(LD(wk)*Ak.astype(LD) for wk, Ak in zip(w, mats))
    bound = LD(gamma(len(w)))*sum(abs(LD(wk))*np.abs(Ak).astype(LD) for wk, Ak in zip(w, mats))
    return np.argwhere(np.abs(M.astype(LD)-ref) > bound), ref, bound


def _check_interval(name, i, with_solvers):
    """checks (a) - (g) on interval i at s = left, left + 0.123 width, the middle node, right.  (e): the largest |lambda| of
    (A(s) - A_d) v = lambda A_d v against the directly assembled A_d is held to eta, the bound the node selection is designed for;
    measured on the device: at most 1.96e-3 on the interval mesh (eta = 0.025), 8.97e-4 on the disc (eta = 0.0581), 1e-15 at a node"""
    import scipy.linalg
    from pynucleus_amd import solvers
    from pynucleus_amd.linear_operators import lagrangeWeights, Dense_LinearOperator
    mesh, dm, kernel, A, eta = _problem(name)
    op = A.ops[i]
    nodes, (a, b) = op.nodes, (op.left, op.right)
    n = dm.num_dofs
    rng = np.random.default_rng(i)
    x = rng.standard_normal(n)
    # (a) is formed from the node operators' own blocks, each downloaded by its Dense_LinearOperator.  Separately assembled operators at
    # the same nodes are NOT the same bits: the work-list and touching-pair kernels of the assembly add with atomics, whose order differs
    # from run to run (tests/test_run_state.py: bounded by TOL_ORDER = 1e-13 max|A|), which is 500 times the rounding bound of (R); they
    # are held to that documented bound instead
    op.assure_constructed()
    mats = [o.toarray().copy() for o in op.ops]
    for s, Mk in zip(nodes, mats):
        assert np.abs(_direct(name, s)-Mk).max() <= 1e-13*np.abs(Mk).max(), (name, i, s, 'separately assembled node operator')
    for val in (a, a+0.123*(b-a), nodes[len(nodes)//2], b):
        A.set(val)
        if val == a and i > 0:
            assert A.selected == i-1                      # a shared end point belongs to the first interval that contains it
            op.set(val)
        else:
            assert A.selected == i and A.get() == val
        w = lagrangeWeights(nodes, val, 0)
        assert np.array_equal(op.coeffs, w)
        M = op.toarray()
        bad, ref, bound = _combination_violations(M, mats, w)
        assert bad.shape[0] == 0, (name, i, val, 'toarray', bad[:4])                                                       # (a)
        if val == nodes[len(nodes)//2]:
            assert np.array_equal(M, op.ops[len(nodes)//2].toarray()), (name, i, 'the middle node is not reproduced bit for bit')   # (b)
        y = op.matvec(x)
        g = LD(gamma(len(w)+n+3))
        ybound = g*(sum(abs(LD(wk))*np.abs(Ak).astype(LD) for wk, Ak in zip(w, mats))@np.abs(x).astype(LD))
        assert np.all(np.abs(y.astype(LD)-ref@x.astype(LD)) <= ybound), (name, i, val, 'matvec')                           # (c)
        assert np.all(np.abs(op.diagonal.astype(LD)-np.diag(ref)) <= np.diag(bound)), (name, i, val, 'diagonal')           # (d)
        Ad = _direct(name, val)
        Ad = 0.5*(Ad+Ad.T)
        lam = scipy.linalg.eigh(0.5*((M-Ad)+(M-Ad).T), Ad, eigvals_only=True)
        print('{} interval {} s = {:.4f}: max |lambda| = {:.3e} (eta = {:.3e})'.format(name, i, val, np.abs(lam).max(), eta))
        assert np.abs(lam).max() <= eta, (name, i, val, np.abs(lam).max(), eta)                                            # (e)
        if not with_solvers:
            continue
        for derivative in (1, 2):                                                                                            # (f)
            op.set(val, derivative)
            wd = lagrangeWeights(nodes, val, derivative)
            bad, _, _ = _combination_violations(op.toarray(), mats, wd)
            assert bad.shape[0] == 0, (name, i, val, derivative, bad[:4])
        op.set(val)
        rhs = rng.standard_normal(n)
        xref = np.linalg.solve(ref.astype(np.float64), rhs)                                                                 # (g)
        Am = op.materialize()
        assert isinstance(Am, Dense_LinearOperator) and Am.symmetric and Am.A.stride(0) % 8 == 0
        xd = Am.solve_direct(rhs)
        assert np.abs(xd-xref).max() <= 1e-10*np.abs(xref).max(), (name, i, val, 'solve_direct')
        tol = 1e-8
        xc, its, _ = solvers.cg(A if A.selected == i else op, rhs, tol=tol)
        r = rhs-ref.astype(np.float64)@xc
        assert np.sqrt(r@(r/np.diag(ref).astype(np.float64))) <= tol, (name, i, val, 'cg', its)


@gpu
@pytest.mark.parametrize('i', range(9))
def test_interval_end_to_end(i):
    mesh, dm, kernel, A, eta = _problem('interval')
    assert dm.num_dofs == 31 and abs(mesh.h-1/16) < 1e-15 and abs(mesh.diam-2.) < 1e-15 and abs(eta-0.025) < 1e-15
    assert len(A.ops) == 9 and all(op.numInterpolationNodes == 3 for op in A.ops) and A.numInterpolationNodes == 27
    fresh = not A.ops[i].constructed
    if fresh:
        before = [op.constructed for op in A.ops]
        A.set(0.5*(A.ops[i].left+A.ops[i].right))
        after = [op.constructed for op in A.ops]                                                                            # (h)
        assert after == [c or k == i for k, c in enumerate(before)] and not any(callable(o) and not hasattr(o, 'matvec') for o in A.ops[i].ops)
    _check_interval('interval', i, True)


@gpu
@pytest.mark.parametrize('i', range(5))
def test_disc_end_to_end(i):
    mesh, dm, kernel, A, eta = _problem('disc')
    assert dm.num_dofs == 37 and abs(eta-0.0581) < 5e-5 and abs(mesh.diam-2.83) < 5e-3
    assert len(A.ops) == 5 and all(op.numInterpolationNodes == 3 for op in A.ops)
    _check_interval('disc', i, False)


@gpu
def test_two_dofmaps_give_the_rectangular_block():
    from pynucleus_amd import driverMesh, P1_DoFMap, PHYSICAL, getFractionalKernel, admissibleSet
    from pynucleus_amd.linear_operators import lagrangeWeights
    mesh = driverMesh('interval', 4)
    dm = P1_DoFMap(mesh, PHYSICAL)
    dm2 = dm.getComplementDoFMap()
    kernel = getFractionalKernel(1, admissibleSet([0.2, 0.8]))
    A = dm.assembleNonlocal(kernel, 'dense', dm2=dm2)
    assert A.shape == (dm.num_dofs, dm2.num_dofs)
    val = 0.33
    A.set(val)
    op = A.getSelectedOp()
    assert op.ops[0].A.data_ptr() % 16 != 0 or dm.num_dofs % 2 == 0       # the block full.A[:n1, n1:]: a misaligned base for odd n1
    mats = [o.toarray().copy() for o in op.ops]           # the node operators' own blocks (see _check_interval)
    for s, Mk in zip(op.nodes, mats):
        sep = dm.assembleNonlocal(kernel.getFrozenKernel(s), 'dense', dm2=dm2).toarray()
        assert sep.shape == Mk.shape and np.abs(sep-Mk).max() <= 1e-13*np.abs(Mk).max()
    w = lagrangeWeights(op.nodes, val, 0)
    bad, ref, _ = _combination_violations(A.toarray(), mats, w)
    assert bad.shape[0] == 0 and ref.shape == A.shape, bad[:4]
    x = np.random.default_rng(2).standard_normal(dm2.num_dofs)
    ybound = LD(gamma(len(w)+dm2.num_dofs+3))*(sum(abs(LD(wk))*np.abs(Ak).astype(LD) for wk, Ak in zip(w, mats))@np.abs(x).astype(LD))
    assert np.all(np.abs(A.matvec(x).astype(LD)-ref@x.astype(LD)) <= ybound)


@gpu
@pytest.mark.parametrize('fmt,horizon', [('sparse', 0.5), ('H2', None)])
def test_generic_path(fmt, horizon):
    """operators that are not dense blocks: y = sum w_k op_k.matvec(x) of the same node operators, accumulated on the device"""
    from pynucleus_amd import driverMesh, P1_DoFMap, PHYSICAL, getFractionalKernel, admissibleSet
    from pynucleus_amd.linear_operators import lagrangeWeights, Dense_LinearOperator
    mesh = driverMesh('interval', 4)
    dm = P1_DoFMap(mesh, PHYSICAL)
    kernel = getFractionalKernel(1, admissibleSet([0.2, 0.8]), horizon=horizon)
    A = dm.assembleNonlocal(kernel, fmt)
    val = 0.47
    A.set(val)
    op = A.getSelectedOp()
    assert not any(isinstance(o, Dense_LinearOperator) for o in op.ops)
    w = lagrangeWeights(op.nodes, val, 0)
    g = LD(gamma(len(w)+1))
    x = np.random.default_rng(4).standard_normal(dm.num_dofs)
    # The products y_k = op_k.matvec(x) that A.matvec combines are recorded on the way: the SSS and H2 products add with atomics, so a
    # second call of op_k.matvec(x) does not give the same bits (the order of the additions differs from run to run, as in the
    # assembly: tests/test_run_state.py), and the rounding bound of the combination can only hold against the y_k it was given.
    # Separately computed products are held to the 1e-13 of that test instead.
    ys = []

    def recorded(method, into):
        def call(*args):
            out = method(*args)
            into.append(out.detach().cpu().numpy().copy() if hasattr(out, 'detach') else np.array(out, dtype=np.float64))
            return out
        return call
    for o in op.ops:
        o.matvec = recorded(o.matvec, ys)
    y = A.matvec(x)
    for o in op.ops:
        del o.matvec
    assert len(ys) == len(w)
    ref = sum(LD(wk)*yk.astype(LD) for wk, yk in zip(w, ys))
    assert np.all(np.abs(y.astype(LD)-ref) <= g*sum(abs(LD(wk))*np.abs(yk).astype(LD) for wk, yk in zip(w, ys))), fmt
    again = sum(wk*np.asarray(o.matvec(x)) for wk, o in zip(w, op.ops))
    assert np.abs(y-again).max() <= 1e-13*sum(abs(wk)*np.abs(yk).max() for wk, yk in zip(w, ys)), fmt
    with pytest.raises(NotImplementedError):
        A.materialize()
    mats = []                                             # likewise the arrays A.toarray combines (an H2 operator forms its own by products)
    for o in op.ops:
        o.toarray = recorded(o.toarray, mats)
    T = A.toarray()
    for o in op.ops:
        del o.toarray
    assert len(mats) == len(w) and T.shape == (dm.num_dofs, dm.num_dofs)
    refT = sum(LD(wk)*Mk.astype(LD) for wk, Mk in zip(w, mats))
    assert np.all(np.abs(T.astype(LD)-refT) <= g*sum(abs(LD(wk))*np.abs(Mk).astype(LD) for wk, Mk in zip(w, mats))), fmt


@gpu
def test_finite_horizon_dense_blocks_take_the_fused_path():
    from pynucleus_amd import driverMesh, P1_DoFMap, PHYSICAL, getFractionalKernel, admissibleSet
    from pynucleus_amd.linear_operators import lagrangeWeights, Dense_LinearOperator
    dm = P1_DoFMap(driverMesh('interval', 4), PHYSICAL)
    A = dm.assembleNonlocal(getFractionalKernel(1, admissibleSet([0.2, 0.8]), horizon=0.5), 'dense')
    val = 0.47
    A.set(val)
    op = A.getSelectedOp()
    assert all(type(o) is Dense_LinearOperator for o in op.ops)
    w = lagrangeWeights(op.nodes, val, 0)
    Am = A.materialize()
    assert _combination_violations(Am.toarray(), [o.toarray() for o in op.ops], w)[0].shape[0] == 0 and np.array_equal(Am.toarray(), A.toarray())
