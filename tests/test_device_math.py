"""The device functions behind every kernel value and quadrature order, evaluated by the production code through the test hook
pnl_selftest (csrc/pnl_selftest.hip), against mpmath at 40 digits: pnl_log, pnl_exp, pnl_exp_ranged, kern_eval on each of its
paths (rsq / quarter-power, LDS power tables, exp(e ln d2), integrable kernels and their Gauss-theorem twins, horizon test),
pw_scaling and the fp32 / fp64 quadrature-order decision.

The parity tests compare whole matrices with |A_gpu - A_oracle| <= 1e-11 max|A|, which does not see the far entries (1e-4 .. 1e-6 of
max|A| at the test sizes); the bounds here are per value."""
import math
import os
import re

import mpmath
import numpy as np
import pytest

gpu = pytest.mark.gpu
mp = mpmath.mp
mp.dps = 40

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MIN = 2.2250738585072014e-308


def _st(op, x, **kw):
    from pynucleus_amd import _lib
    return _lib.selftest(op, x, **kw)


def _ulps(x, k):
    """x and its k neighbours on both sides"""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


# ---- pnl_log / pnl_exp ---------------------------------------------------------------------------------------------------------

@gpu
def test_pnl_log():
    """absolute error <= 4e-16 max(1, |ln x|) over the normal range, the 64 table-cell edges m = 1/2 + j/128 (+- 1 ulp) of the
    reduction at several binary exponents, and x = 1 +- k ulp"""
    from pynucleus_amd import _lib
    xs = list(np.logspace(-307.6, 308.2, 6001))
    for k in (-1021, -300, -47, -1, 0, 1, 2, 47, 300, 1023):
        for j in range(64):
            xs += _ulps(math.ldexp(0.5+j/128., k), 1)
    xs += _ulps(1., 32)
    xs += [DBL_MIN, 1.7976931348623157e308]
    x = np.array(xs)
    got = _st(_lib.SELFTEST_LOG, x)
    ref = np.array([float(mpmath.log(mpmath.mpf(v))) for v in x])
    err = np.abs(got-ref)/np.maximum(1., np.abs(ref))
    assert err.max() <= 4e-16, (x[err.argmax()], err.max())


def _exp_inputs():
    ys = list(np.linspace(-708., 709., 20001))
    ys += list(np.logspace(-20, 2.8, 2000))+list(-np.logspace(-20, 2.8, 2000))
    ln2_64 = math.log(2.)/64.
    for n in list(range(-65370, 65470, 1009))+list(range(-130, 130)):
        for y in ((n+0.5)*ln2_64, (n-0.5)*ln2_64):
            ys += _ulps(y, 1)
    y = np.array(ys)
    return y[(y >= -708.) & (y <= 709.)]


def _exp_ref(y):
    return np.array([float(mpmath.exp(mpmath.mpf(v))) for v in y])


@gpu
@pytest.mark.parametrize('ranged', [False, True])
def test_pnl_exp_relative_error(ranged):
    """relative error <= 1e-15 on [-708, 709], including both sides of the reduction edges (n +- 1/2) ln 2 / 64"""
    from pynucleus_amd import _lib
    y = _exp_inputs()
    got = _st(_lib.SELFTEST_EXP_RANGED if ranged else _lib.SELFTEST_EXP, y)
    ref = _exp_ref(y)
    err = np.abs(got/ref-1.)
    assert err.max() <= 1e-15, (y[err.argmax()], err.max())


@gpu
def test_pnl_exp_ranged_underflow():
    """pnl_exp_ranged (the Gaussian and exponential kernels, y <= 0): below the normal range (y < ln 2.2e-308) the result satisfies
    0 <= result <= 2.3e-308 -- it is 0 below -708, also far below (-720, -1000, -1e4, -inf) and for NaN, where pnl_exp returned -6.6e303
    at y = -720 -- and on [-708, 709] it is pnl_exp"""
    from pynucleus_amd import _lib
    lo = np.concatenate([np.linspace(-760., -708., 5001), _ulps(-708., 2), _ulps(math.log(DBL_MIN), 2),
                         [-720., -1000., -1e4, -1e300, -np.inf, np.nan]])
    got = _st(_lib.SELFTEST_EXP_RANGED, lo)
    assert np.all(got >= 0.) and np.all(np.isfinite(got)), lo[~((got >= 0.) & np.isfinite(got))]
    assert np.all(got[~(lo >= math.log(DBL_MIN))] <= 2.3e-308)
    assert np.all(got[~(lo >= -708.)] == 0.)
    ok = lo >= -708.
    assert np.all(np.abs(got[ok]/_exp_ref(lo[ok])-1.) <= 1e-15)
    y = _exp_inputs()
    assert np.array_equal(_st(_lib.SELFTEST_EXP_RANGED, y), _st(_lib.SELFTEST_EXP, y))


def test_pnl_exp_callers_stay_in_its_domain():
    """pnl_exp has no range check (pnl_common.h): valid on [-708, 709] only.  Every call of it in the library is a fractional power
    exp(e ln d2) -- `...*pnl_log(d2))` or `...*L)` with L = pnl_log(d2) -- whose exponent e = -(s + d/2) lies in (-2, 0); for
    1e-150 < d2 < 1e150 that is inside the domain.  The integrable kernels call pnl_exp_ranged."""
    csrc = os.path.join(ROOT, 'pynucleus_amd', 'csrc')
    calls = []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(('.h', '.hip')) or fn == 'pnl_selftest.hip':
            continue
        src = open(os.path.join(csrc, fn)).read()
        for m in re.finditer(r'\bpnl_exp\((?!double)', src):
            line = src[m.start():src.index('\n', m.start())]
            if fn == 'pnl_common.h' and line.startswith('pnl_exp(y) : 0.'):
                continue                                    # pnl_exp_ranged: its own range check
            calls.append((fn, line))
            assert re.match(r'pnl_exp\([^;]*\*(pnl_log\(d2\)|L)\)', line), (fn, line)
            if line.endswith('*L)') or '*L)' in line:
                assert re.search(r'\bL = pnl_log\(d2\)', src), fn
    assert len(calls) >= 5, calls
    e_max, ln_max = 2., math.log(1e150)
    assert e_max*ln_max < 708.


# ---- kernel values ---------------------------------------------------------------------------------------------------------------

def _kernel(ktype, exponent, scale, horizon2=np.inf):
    from pynucleus_amd._lib import pnl_kernel
    return pnl_kernel(int(ktype), 0, float(exponent), float(scale), float(horizon2))


def _d2_sweep(lo, hi, n=3001):
    d2 = list(np.logspace(np.log10(lo), np.log10(hi), n))
    for k in range(int(math.floor(math.log2(lo))), int(math.ceil(math.log2(hi)))):
        for j in (0, 1, 37, 64, 127):
            d2 += _ulps(math.ldexp(1.+j/128., k), 1)
    d2 = np.array(d2)
    return d2[(d2 >= lo) & (d2 < hi)]


def _frac_ref(k, d2):
    e = mpmath.mpf(k.exponent)
    return np.array([float(k.scale*mpmath.mpf(v)**e) for v in d2])


def _rel(got, ref):
    return np.abs(got-ref)/np.abs(ref)


FAST = [(1, 0.25), (1, 0.5), (1, 0.75), (2, 0.25), (2, 0.5), (2, 0.75)]


@gpu
@pytest.mark.parametrize('dim,s', FAST)
def test_fractional_quarter_orders(dim, s):
    """s = 1/4, 1/2, 3/4 (qm = -4 exponent = 3 .. 7): what kern_dispatch picks, KT 1 with qm at run time, the compile-time KT 2 / 1x
    (rsq with Halley steps, the single-precision quarter-power seed) within 2e-15 relative over d2 in [1e-14, 1e3]; the same
    exponents through the LDS tables (4e-15, 2^-96 <= d2 < 2^31) and through exp(e ln d2) (1e-14 where |e ln d2| < 60)"""
    from pynucleus_amd import _lib, getFractionalKernel
    p = getFractionalKernel(dim, s).device_params()
    k = _kernel(0, p['exponent'], p['scale'])
    qm = int(round(-4*k.exponent))
    assert abs(qm+4*k.exponent) < 1e-13
    d2 = _d2_sweep(1e-14, 1e3)
    ref = _frac_ref(k, d2)
    paths = [_lib.SELFTEST_DISPATCH, _lib.SELFTEST_DISPATCH+1, 1]+([10+qm] if qm in (3, 4, 5, 7) else [])+([2] if qm == 6 else [])
    for path in paths:
        err = _rel(_st(_lib.SELFTEST_KERNEL, d2, path=path, dim=dim, param=k), ref)
        assert err.max() <= 2e-15, (path, d2[err.argmax()], err.max())
    dt = _d2_sweep(2.**-96, 2.**31)
    err = _rel(_st(_lib.SELFTEST_KERNEL, dt, path=3, dim=dim, param=k), _frac_ref(k, dt))
    assert err.max() <= 4e-15, ('tables', dt[err.argmax()], err.max())
    m = np.abs(k.exponent*np.log(d2)) < 60.
    err = _rel(_st(_lib.SELFTEST_KERNEL, d2[m], path=0, dim=dim, param=k), ref[m])
    assert err.max() <= 1e-14, ('exp/ln', d2[m][err.argmax()], err.max())


@gpu
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('s', [0.1, 0.3, 0.4, 0.6, 0.9, 0.99])
def test_fractional_general_orders(dim, s):
    """general s: the LDS power tables (what kern_dispatch picks without and with INSIDE, and KT 3 itself) within 4e-15 relative
    over 2^-96 <= d2 < 2^31, exp(e ln d2) within 1e-14 where |e ln d2| < 60 of d2 in [1e-14, 1e3]"""
    from pynucleus_amd import _lib, getFractionalKernel
    p = getFractionalKernel(dim, s).device_params()
    k = _kernel(0, p['exponent'], p['scale'])
    dt = _d2_sweep(2.**-96, 2.**31)
    ref = _frac_ref(k, dt)
    for path in (_lib.SELFTEST_DISPATCH, _lib.SELFTEST_DISPATCH+1, 3):
        err = _rel(_st(_lib.SELFTEST_KERNEL, dt, path=path, dim=dim, param=k), ref)
        assert err.max() <= 4e-15, (path, dt[err.argmax()], err.max())
    d2 = _d2_sweep(1e-14, 1e3)
    d2 = d2[np.abs(k.exponent*np.log(d2)) < 60.]
    err = _rel(_st(_lib.SELFTEST_KERNEL, d2, path=0, dim=dim, param=k), _frac_ref(k, d2))
    assert err.max() <= 1e-14, ('exp/ln', d2[err.argmax()], err.max())


@gpu
@pytest.mark.parametrize('ktype', [0, 1, 2])
def test_horizon_semantics(ktype):
    """finite horizon (nl_oracle.c kernel_eval): a value at d2 = horizon^2, 0 at the next double and for NaN, on the general path
    (with the power tables of a fractional kernel and without); INSIDE (kern_dispatch<0, true>): the constant kernel is its scale,
    the fractional one takes the tables without a horizon test"""
    from pynucleus_amd import _lib
    h2 = 0.3**2
    k = _kernel(ktype, -1.2 if ktype == 0 else 0., 0.7, h2)
    d2 = np.array([1e-6, 0.01, h2, np.nextafter(h2, np.inf), 0.5, np.nan, np.inf])
    if ktype == 0:
        ref = np.array([0.7*v**-1.2 for v in d2[:3]])
    elif ktype == 1:
        ref = np.full(3, 0.7)
    else:
        ref = 0.7/np.sqrt(d2[:3])
    for path in (_lib.SELFTEST_DISPATCH, 0):
        got = _st(_lib.SELFTEST_KERNEL, d2, path=path, dim=2, param=k)
        assert np.all(got[3:] == 0.), (path, got)
        assert np.all(_rel(got[:3], ref) <= 1e-14), (path, got, ref)
    got = _st(_lib.SELFTEST_KERNEL, d2[:3], path=_lib.SELFTEST_DISPATCH+1, dim=2, param=k)
    assert np.all(_rel(got, ref) <= 1e-14), got


def _integrable_ref(kt, e, scale, d2):
    e, scale, d2 = mpmath.mpf(e), mpmath.mpf(scale), mpmath.mpf(d2)
    r = mpmath.sqrt(d2)
    if kt == 3:
        return scale*mpmath.exp(e*d2)
    if kt == 4:
        return scale*mpmath.exp(e*r)
    if kt == 5:
        return scale*mpmath.sqrt(mpmath.pi/(-e))*mpmath.erfc(mpmath.sqrt(-e*d2))
    if kt == 6:
        return 2*scale*mpmath.exp(e*r)/(-e)
    if kt == 7:
        return scale*mpmath.exp(e*d2)/(-e*d2)
    return 2*scale*mpmath.exp(e*r)/(-e*r)


INTEGRABLE = [(dim, 'gaussian', v) for dim in (1, 2) for v in (1., 0.1, 0.01, 1e-3)]+[(dim, 'exponential', r) for dim in (1, 2) for r in (1., 30., 1e3)]


@gpu
@pytest.mark.parametrize('dim,name,par', INTEGRABLE)
def test_integrable_kernels(dim, name, par):
    """Gaussian / exponential kernels (ktypes 3, 4) and their Gauss-theorem twins (5, 6 in 1D; the folded 2D forms 7, 8) over d2 in
    [1e-12, 16]: where the exact value is >= 1e-300 scale the relative error is <= 1e-14 plus the conditioning of the formula to
    the rounding of its argument: |y| 2^-53 for exp(y) with y = e d2, 2 |y| 2^-53 with y = e sqrt(d2), 4 x^2 2^-53 for erfc(x) with
    x = sqrt(-e d2) (the oracle rounds the same way); below that 0 <= value <= 1e-300 scale (pnl_exp_ranged flushes exp(y) < 3.4e-308 to 0).  Before pnl_exp_ranged the far values of variance <= 0.01 (2D) / 1e-3 (1D) and rate 1e3
    came out as huge numbers of either sign."""
    from pynucleus_amd import _lib, getKernel
    if name == 'gaussian':
        p = getKernel(dim, kernel='gaussian', horizon=np.inf, variance=par).device_params()
        e, scale = p['exponent'], p['scale']
    else:
        p = getKernel(1, kernel='exponential', horizon=np.inf, exponentialRate=par).device_params()
        e, scale = -par, p['scale']      # normalised in 1D only: the 1D constant in 2D
    kt = 3 if name == 'gaussian' else 4
    d2 = _d2_sweep(1e-12, 16., 4001)
    for boundary in (False, True):
        k = _kernel(kt+2 if boundary else kt, e, scale)
        rkt = (kt+2 if dim == 1 else kt+4) if boundary else kt
        ref = np.array([float(_integrable_ref(rkt, e, scale, v)) for v in d2])
        y = e*d2 if kt == 3 else e*np.sqrt(d2)
        # the rounding of y (and of sqrt(d2), and of x = sqrt(-y) for erfc(x), d ln erfc / dx = -2 x) at 2^-53 relative each
        cond = (4. if rkt == 5 else (1. if kt == 3 else 2.))*np.abs(y)*2.**-53
        for path in (_lib.SELFTEST_DISPATCH, _lib.SELFTEST_DISPATCH+1):
            got = _st(_lib.SELFTEST_KERNEL, d2, path=path, dim=dim, boundary=boundary, param=k)
            big = ref >= 1e-300*scale
            err = _rel(got[big], ref[big])-cond[big]
            assert err.max() <= 1e-14, (rkt, path, d2[big][err.argmax()], err.max()+cond[big][err.argmax()])
            small = got[~big]
            fine = (small >= 0.) & (small <= 1e-300*scale*(1.+1e-12))
            assert np.all(fine), (rkt, path, small[~fine][:4])


# ---- pw_scaling ----------------------------------------------------------------------------------------------------------------

def _scaling_exact(dim, s):
    s = mpmath.mpf(s)
    return 2**(2*s)*s*mpmath.gamma(s+mpmath.mpf(dim)/2)/(mpmath.pi**(mpmath.mpf(dim)/2)*mpmath.gamma(1-s))/2


@gpu
@pytest.mark.parametrize('case', ['smoothedLeftRight_disc', 'innerOuter_disc', 'smoothedLeftRight_interval'])
def test_pw_scaling(case):
    """C(s) of the pointwise kernels by Clenshaw on the Chebyshev series of local_matrix._setup_pointwise, and by the Gamma functions
    without it, within 1e-13 relative of 2^(2s) s Gamma(s + d/2) / (pi^(d/2) Gamma(1 - s)) / 2 (boundary: / s) on 2001 orders in
    [smin, smax] of the order functions of the parity tests"""
    import ctypes as C
    from pynucleus_amd import _lib, disc, interval, PHYSICAL, P1_DoFMap, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.fractionalOrders import smoothedLeftRightFractionalOrder, smoothedInnerOuterFractionalOrder
    if case == 'smoothedLeftRight_disc':
        mesh, sF = disc(2), smoothedLeftRightFractionalOrder(0.25, 0.75, r=0.3)
    elif case == 'innerOuter_disc':
        mesh, sF = disc(2), smoothedInnerOuterFractionalOrder(0.3, 0.7, r=0.5, slope=200.)
    else:
        mesh, sF = interval(4), smoothedLeftRightFractionalOrder(0.25, 0.75, r=0.3)
    T = nonlocalBuilder(P1_DoFMap(mesh, PHYSICAL), getFractionalKernel(mesh.dim, sF), {}).tables
    assert T.pointwise and T.scaling_cheb is not None
    s = np.linspace(sF.min, sF.max, 2001)
    mid, half, c = T.scaling_cheb
    with_cheb = _lib.pnl_order_function(int(T.order_type), 1, (C.c_double*6)(*[float(x) for x in T.order_params]))
    with_cheb.scal_n, with_cheb.scal_mid, with_cheb.scal_half = len(c), mid, half
    for i, v in enumerate(c):
        with_cheb.scal_cheb[i] = float(v)
    gamma = _lib.pnl_order_function(int(T.order_type), 1, (C.c_double*6)(*[float(x) for x in T.order_params]))
    for boundary in (False, True):
        ref = np.array([float(_scaling_exact(mesh.dim, v)/(v if boundary else 1)) for v in s])
        for f in (with_cheb, gamma):
            got = _st(_lib.SELFTEST_SCALING, s, dim=mesh.dim, boundary=boundary, param=f)
            err = _rel(got, ref)
            assert err.max() <= 1e-13, (boundary, f.scal_n, s[err.argmax()], err.max())


# ---- quadrature order ----------------------------------------------------------------------------------------------------------

def _order_args(F, h1, h2, d2, H0):
    """the two ceil() arguments of the oracle's formula (oracle/tables.py Formula)"""
    d = np.sqrt(d2)
    l1, l2 = np.log(d/h1), np.log(d/h2)
    L1, L2 = np.abs(np.log(h1/H0)), np.abs(np.log(h2/H0))
    Lm = np.maximum(L1, L2)
    n1, n2 = (np.maximum(l1, 0.), np.maximum(l2, 0.)) if F.clip_num else (l1, l2)
    a1 = (F.c0+F.a*L2+F.b*Lm-F.e*n2)/(np.maximum(l1, 0.)+F.den0)
    a2 = (F.c0+F.a*L1+F.b*Lm-F.e*n1)/(np.maximum(l2, 0.)+F.den0)
    return a1, a2


def _formulas():
    from oracle.tables import Formula
    out = []
    for s in (0.25, 0.5, 0.75, 0.4):
        c2 = (0.5*0.5+0.5)*np.log(4000*0.7**2)
        out.append(('2d_s{}'.format(s), Formula(c2, s-1., 1., s, 0.4, False)))                 # constant order, 2D (FL2:622-642)
        out.append(('1d_s{}'.format(s), Formula((3.-s+2.)*np.log(200*0.35), 2.*s-1., 0., 2.*s, 0.8, False)))
        out.append(('2d_bnd_s{}'.format(s), Formula(c2, s-1., 1., s, 0.35, True)))            # boundary, clipped numerator
        out.append(('pw_s{}'.format(s), Formula(c2, s-1., 1., s, 0.4, True)))                 # pw_formula (den0 0.4), clipped
    return out


@gpu
@pytest.mark.parametrize('name,F', _formulas(), ids=lambda v: v if isinstance(v, str) else '')
def test_quad_order(name, F):
    """quad_order_fast == quad_order_exact on 1e5 random cell pairs and on pairs built so that a ceil() argument lies 1e-7 .. 1e-3 from
    an integer; quad_order_try is -1 or the exact order; quad_order_exact == the oracle's formula except within 1e-12 of a tie"""
    from pynucleus_amd import _lib
    f = _lib.pnl_order_formula(F.c0, F.a, F.b, F.e, F.den0, int(F.clip_num), 0)
    rng = np.random.default_rng(7)
    n = 100000
    H0 = 0.7
    h1 = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), n))
    h2 = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), n))
    d = np.maximum(h1, h2)*np.exp(rng.uniform(-1., 7., n))
    rows = [np.stack([h1, h2, d*d, np.full(n, H0)], axis=1)]
    # near ties: h1 = h2 = h, l = ln(d / h) > 0 solves (C - e l) / (l + den0) = m + delta
    h = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), 4000))
    L = np.abs(np.log(h/H0))
    Cn = F.c0+(F.a+F.b)*L
    m = rng.integers(2, 25, h.size)
    delta = np.exp(rng.uniform(np.log(1e-7), np.log(1e-3), h.size))*rng.choice([-1., 1.], h.size)
    t = m+delta
    l = (Cn-t*F.den0)/(t+F.e)
    ok = l > 0.
    dd = h[ok]*np.exp(l[ok])
    rows.append(np.stack([h[ok], h[ok], dd*dd, np.full(ok.sum(), H0)], axis=1))
    x = np.concatenate(rows)
    assert ok.sum() > 1000
    q = _st(_lib.SELFTEST_QORDER, x, param=f)
    exact, tr, fast = q[:, 0], q[:, 1], q[:, 2]
    bad = fast != exact
    assert not bad.any(), (name, x[bad][:4], exact[bad][:4], fast[bad][:4])
    assert np.all((tr == -1) | (tr == exact)), x[(tr != -1) & (tr != exact)][:4]
    a1, a2 = _order_args(F, x[:, 0], x[:, 1], x[:, 2], H0)
    ref = np.maximum(np.maximum(np.ceil(a1), 2.), np.maximum(np.ceil(a2), 2.))
    tie = (np.abs(a1-np.rint(a1)) < 1e-12) | (np.abs(a2-np.rint(a2)) < 1e-12)
    assert np.all((ref == exact) | tie), x[(ref != exact) & ~tie][:4]
    near = x.shape[0]-ok.sum()
    assert np.sum(tr[near:] == -1) > 0.1*ok.sum()       # the near ties do reach the fp64 fallback
