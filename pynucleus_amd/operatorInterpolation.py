"""Where to assemble so that an operator can be interpolated in the fractional order s.

Host mirror of the reference's nl/PyNucleus_nl/operatorInterpolation.py: ``admissibleSet`` (:12-93, the parts a single order
needs) and ``getChebyIntervalsAndNodes`` (:123-265, the ``variableOrder=True`` branch that DoFMap.assembleNonlocal uses,
fem/PyNucleus_fem/DoFMaps.pyx:852-855).  The range [s_left, s_right] is cut into intervals; on each, the operator is assembled at
M + 1 Chebyshev nodes and A(s) = sum_k w_k(s) A(s_k) with the Lagrange weights (linear_operators.interpolationOperator).

The rule, restated (line numbers of the reference file).  For the left end smin of an interval and a parameter xi:
    lift  = min(r + smin, 1/2)                               regularity lift of a right-hand side in H^r              (:130-132)
    s1    = smin,  s2 = min(1, smin + lift)                                                                          (:153-154)
    smax  = (s1 + s2)/2 - xi min(1 - smin, lift)             right end before clipping to s_right                    (:155)
    eps(t) = s1 + s2 - 2 t                                                                                           (:159)
    C     = 4 (1/e + delta^(eps(smin) + 1)) if delta > 1, else 4/e                                                   (:160-163)
    sigma = (smax - smin) / (2 eps(smax))                    contraction factor of the Chebyshev error               (:164)
    M     = ceil(ln(eta / C) / ln(sigma) - 1), clipped to [M_min, M_max]                                             (:167, 206-207)
The interval is (smin, min(smax, s_right)) and carries M + 1 nodes; the next one starts at its right end, until s_right is reached
or 1000 intervals exist (:195-214).  xi is ``fixedXi`` if that is positive (it must lie in (0.1, 0.5)), otherwise the first
minimiser of the total number of nodes over the interior points of linspace(0.1, 0.5, 300) (:227-240).  The nodes of [a, b] are the
Chebyshev points of the first kind in ascending order, (a + b)/2 + (b - a)/2 cos((2 j - 1) pi / (2 n)), j = n .. 1 (:216-221).
The arithmetic follows the reference operation by operation: tests/golden/cheby_intervals.json holds what the reference returns, and
the two agree bit for bit.
"""
import numpy as np

MAX_INTERVALS = 1000


class admissibleSet:
    """box of admissible parameters, one row (lower, upper) per parameter (operatorInterpolation.py:12-93); the ranged kernels use one"""

    def __init__(self, ranges):
        ranges = np.array(ranges, dtype=np.float64)
        if ranges.ndim == 1:
            ranges = ranges[np.newaxis, :]
        assert ranges.ndim == 2 and ranges.shape[1] == 2
        self.ranges = ranges

    @property
    def numParams(self):
        return self.ranges.shape[0]

    def getNumParams(self):
        return self.numParams

    def getLowerBounds(self):
        return self.ranges[:, 0].copy()

    def getUpperBounds(self):
        return self.ranges[:, 1].copy()

    def isAdmissible(self, z):
        z = np.atleast_1d(np.asarray(z, dtype=np.float64))
        assert z.shape[0] == self.numParams
        return bool(np.all((self.ranges[:, 0] <= z) & (z <= self.ranges[:, 1])))

    def __repr__(self):
        return '{}({})'.format(type(self).__name__, self.ranges)


def chebyshevNodes(n, a, b):
    """the n Chebyshev points of the first kind on [a, b], ascending"""
    j = np.arange(n, 0, -1)
    return 0.5*(a+b)+0.5*(b-a)*np.cos((2.0*j-1.0)/(2*n)*np.pi)


def getChebyIntervalsAndNodes(s_left, s_right, delta, r, eta, M_max=20, M_min=3, variableOrder=False, doSplitM=False, fixedXi=-1):
    """(intervals, nodes): intervals = [(left, right), ...] contiguous from s_left to s_right, nodes[k] = the ascending Chebyshev
    nodes of interval k.  delta: the horizon (or the diameter of the domain), r: regularity of the right-hand side, eta: the bound on
    the relative interpolation error of the operator."""
    assert delta > 0. and s_left > 0. and s_right < 1.
    if not variableOrder:
        raise NotImplementedError('getChebyIntervalsAndNodes: one interpolation order for all intervals (variableOrder=False{}); '
                                  'DoFMap.assembleNonlocal uses variableOrder=True'.format(', doSplitM' if doSplitM else ''))
    exp_m1 = np.exp(-1.)

    def right_end_and_order(smin, xi):
        lift = min(r+smin, 1/2)
        s1, s2 = smin, min(1, smin+lift)
        smax = (s1+s2)/2-xi*min(1-smin, lift)
        assert (s1+s2)/2-1/2 < smax < (s1+s2)/2
        C_delta = 4*(exp_m1+delta**((s1+s2-2*smin)+1)) if delta > 1 else 4*exp_m1
        sigma = (smax-smin)/2/(s1+s2-2*smax)
        assert 0. <= sigma < 1.
        return smax, int(np.ceil(np.log(eta/C_delta)/np.log(sigma)-1))

    def cut(xi):
        s, intervals, orders = s_left, [], []
        while s < s_right and len(intervals) < MAX_INTERVALS:
            s_new, M = right_end_and_order(s, xi)
            s_new = min(s_new, s_right)
            intervals.append((s, s_new))
            orders.append(min(max(M, M_min), M_max))
            s = s_new
        return intervals, orders

    if fixedXi <= 0:
        candidates = np.linspace(0.1, 0.5, 300)[1:-1]
    else:
        assert 0.1 < fixedXi < 0.5
        candidates = np.array([fixedXi])
    costs = np.array([sum(M+1 for M in cut(xi)[1]) for xi in candidates])
    intervals, orders = cut(candidates[costs.argmin()])                     # argmin: the first minimiser
    return intervals, [chebyshevNodes(M+1, a, b) for (a, b), M in zip(intervals, orders)]
