"""IMEX Runge-Kutta steppers (pynucleus_amd/timestepping.py, pnl_imex_sweep), the mass solve they end with (pnl_csr_cg_jacobi), the
tableaux and the Brusselator problem, against a numpy restatement written here from the scheme

    stage k:  U_k = u if row k of A^E is zero, else per component
              (m_c M + dt A^I[k,k] S) U_k = m_c M u_prev - dt sum_{j<k} (A^E[k,j] E_j + A^I[k,j] I_j) + dt sum_{j<=k} A^I[k,j] g_j
              E_k = -N(U_k), I_k = S U_k
    final:    m_c M u_new = m_c M u_prev - dt sum_k (b^E[k] E_k + b^I[k] I_k) + dt sum_k b^I[k] g_k

with numpy.linalg.solve, S = A.toarray() of the device operator, the dense mass matrix and the restated nonlinearity of
tests/test_reaction.py."""
import numpy as np
import pytest
from test_reaction import restated_nonlinearity, f_brusselator, f_cubic, dev, EPS

G = (3.+np.sqrt(3.))/6.
TABLEAUX = {      # c, A^E, A^I, b^E, b^I
    'euler_imex': ([0., 1.], [[0., 0.], [1., 0.]], [[0., 0.], [0., 1.]], [1., 0.], [0., 1.]),
    'ars3': ([0., G, 1.-G], [[0., 0., 0.], [G, 0., 0.], [G-1., 2.*(1.-G), 0.]], [[0., 0., 0.], [0., G, 0.], [0., 1.-2.*G, G]],
             [0., .5, .5], [0., .5, .5]),
    'koto': ([0., 1., .5, 1.], [[0., 0., 0., 0.], [1., 0., 0., 0.], [.5, 0., 0., 0.], [0., 0., 1., 0.]],
             [[0., 0., 0., 0.], [0., 1., 0., 0.], [0., -.5, 1., 0.], [0., -1., 1., 1.]], [0., 0., 1., 0.], [0., -1., 1., 1.]),
}
SCHEMES = ['euler_imex', 'ars3', 'koto']
ORDER = {'euler_imex': 1, 'koto': 2, 'ars3': 3}


def tab(name):
    return tuple(np.array(a, dtype=np.float64) for a in TABLEAUX[name])


# ---- the restatement -----------------------------------------------------------------------------------------------------
class Restated:
    """the scheme above on the host.  ``solves`` counts the linear solves, ``systems`` collects the matrices solved with"""

    def __init__(self, name, dm, f, S, M, massScales, dt):
        self.c, self.AE, self.AI, self.bE, self.bI = tab(name)
        self.s = self.c.shape[0]
        self.dm, self.f, self.S, self.M, self.ms, self.dt = dm, f, S, M, np.asarray(massScales, dtype=np.float64), dt
        self.solves = 0
        gam = [self.AI[k, k] for k in range(self.s) if np.abs(self.AE[k]).max() != 0.]
        assert min(gam) == max(gam)
        self.gamma = gam[0]
        self.picardNorms = []

    def implicit_system(self, c):
        return self.ms[c]*self.M+self.dt*self.gamma*self.S

    def N(self, U):
        return restated_nonlinearity(self.dm, self.f, U)[0]

    def sweep(self, u_prev, u, g=None):
        s, dt, AE, AI, bE, bI = self.s, self.dt, self.AE, self.AI, self.bE, self.bI
        nc = u.shape[0]
        U, E, I = [None]*s, [None]*s, [None]*s
        Mu = [self.ms[c]*(self.M@u_prev[c]) for c in range(nc)]
        for k in range(s):
            if np.abs(AE[k]).max() == 0.:
                U[k] = u.copy()
            else:
                U[k] = np.empty_like(u)
                for c in range(nc):
                    rhs = Mu[c].copy()
                    for j in range(k):
                        if AE[k, j] != 0.:
                            rhs -= dt*AE[k, j]*E[j][c]
                        if AI[k, j] != 0.:
                            rhs -= dt*AI[k, j]*I[j][c]
                    if g is not None:
                        for j in range(k+1):
                            rhs += dt*AI[k, j]*g[j][c]
                    U[k][c] = np.linalg.solve(self.ms[c]*self.M+dt*AI[k, k]*self.S, rhs)
                    self.solves += 1
            if np.abs(AE[:, k]).max() != 0. or bE[k] != 0.:
                E[k] = -self.N(U[k])
            if np.abs(AI[:, k]).max() != 0. or bI[k] != 0.:
                I[k] = U[k]@self.S.T
        unew = np.empty_like(u)
        for c in range(nc):
            rhs = Mu[c].copy()
            for k in range(s):
                if bE[k] != 0.:
                    rhs -= dt*bE[k]*E[k][c]
                if bI[k] != 0.:
                    rhs -= dt*bI[k]*I[k][c]
                if g is not None and bI[k] != 0.:
                    rhs += dt*bI[k]*g[k][c]
            unew[c] = np.linalg.solve(self.ms[c]*self.M, rhs)
            self.solves += 1
        return unew

    def step(self, u, g=None):
        return self.sweep(u, u, g)

    def picardStep(self, u, tol, g=None):
        u_prev, its, norms = u.copy(), 0, []
        while True:
            new = self.sweep(u_prev, u, g)
            its += 1
            norms.append(float(np.linalg.norm(new-u)))
            u = new
            if norms[-1] <= tol:
                break
            assert its < 100, norms
        self.picardNorms.append(norms)
        return u, its


# ---- CPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SCHEMES)
def test_tableaux(name):
    from pynucleus_amd.timestepping import tableau
    c, AE, AI, bE, bI = tableau(name)
    for got, want in zip((c, AE, AI, bE, bI), tab(name)):
        assert np.array_equal(got, want)
    assert np.abs(AE.sum(axis=1)-c).max() < 1e-15 and np.abs(AI.sum(axis=1)-c).max() < 1e-15
    assert abs(bE.sum()-1.) < 1e-15 and abs(bI.sum()-1.) < 1e-15
    assert np.array_equal(AE, np.tril(AE, -1)) and np.array_equal(AI, np.tril(AI))


def test_brusselator_problem_parameters():
    from pynucleus_amd.nonlocalProblems import brusselatorProblem
    from pynucleus_amd import P1_DoFMap, NO_BOUNDARY, PHYSICAL
    p = brusselatorProblem('disc', problem='spots')
    assert abs(p.Bcr-1.21) < 1e-15 and abs(p.Q-0.1) < 1e-16 and abs(p.A-0.5) < 1e-15 and abs(p.kcr-0.1**(4./3.)) < 1e-16
    assert abs(p.B-1.22) < 1e-15 and p.alpha == p.beta == 0.75 and p.eta == 0.2 and p.Dx == 1. and abs(p.Dy-25.) < 1e-13
    assert np.allclose(p.massScales, [1., 0.04], rtol=1e-15, atol=0.) and p.tag == NO_BOUNDARY and p.zeroExterior is False
    assert p.nonlinearity.params == (p.B, p.Q) and p.dim == 2
    d = brusselatorProblem('disc', bc='Dirichlet', noRef=1)
    assert d.tag == PHYSICAL and d.zeroExterior is True
    dm = P1_DoFMap(p.mesh.refine(), NO_BOUNDARY)
    u0 = p.initial(dm)
    x = dm.getDoFCoordinates()
    r2 = (x**2).sum(axis=1)
    want = np.where(r2 < 100., (100.-r2)**2/1e4, 0.)
    assert np.abs(u0[0]-0.2*want).max() < 1e-15 and np.abs(u0[1]-want/0.2).max() < 1e-14 and u0[0].max() == 0.2
    s1 = brusselatorProblem('disc', problem='stripes', seed=7)
    s2 = brusselatorProblem('disc', problem='stripes', seed=7)
    s3 = brusselatorProblem('disc', problem='stripes', seed=8)
    assert abs(s1.Bcr-6.25) < 1e-14 and abs(s1.Q-1.5) < 1e-15
    a, b, c = s1.initial(dm), s2.initial(dm), s3.initial(dm)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert (a[0] >= 0.).all() and (a[0] <= 0.2).all() and (a[1] <= 5.).all() and a[1].max() > 1.
    assert brusselatorProblem('interval', noRef=4).mesh.num_vertices == 3
    for bad in (dict(domain='twinDisc'), dict(bc='Robin'), dict(problem='waves')):
        with pytest.raises(NotImplementedError):
            brusselatorProblem(**bad)


def test_factory_rejects_unknown_names():
    from pynucleus_amd.timestepping import timestepperFactory
    with pytest.raises(NotImplementedError):
        timestepperFactory('rk4', None, None, 0.1)


# ---- GPU: set-up shared by the tests ---------------------------------------------------------------------------------------
NOREF = {'interval': 4, 'disc': 2}       # interval: 33 vertices on the finest level; disc: disc(2, radius=50)
_setups = {}


def setup(domain, bc):
    """(problem, hierarchy, dm, S, M, u0) of the Brusselator spots problem, built once"""
    key = (domain, bc)
    if key not in _setups:
        from pynucleus_amd.nonlocalProblems import brusselatorProblem
        p = brusselatorProblem(domain, bc, NOREF[domain], 'spots')
        h = p.hierarchy()
        L = h.finest
        dm = L['DoFMap']
        assert L['mesh'].num_vertices == (33 if domain == 'interval' else 61)
        S = np.array(L['A'].toarray())
        M = L['M'].toarray()
        _setups[key] = (p, h, dm, S, M, p.initial(dm))
    return _setups[key]


def chol_bound(R, n, u_ref):
    """64 n 2^-52 kappa (number of solves) max|u_ref| with kappa the largest condition number of the systems solved"""
    kappa = max(max(np.linalg.cond(R.implicit_system(c)), np.linalg.cond(R.ms[c]*R.M)) for c in range(R.ms.shape[0]))
    return 64.*n*2.**-52*kappa*R.solves*np.abs(u_ref).max()


# plain steps: dt = 0.05.  Picard steps: (dt, tolerance) per domain and scheme, chosen on the restatement (with the operator of the
# CPU oracle) so that no Picard norm lies within a factor 2 of the tolerance: the counts then do not hinge on rounding.  The tests
# assert that margin on the restatement with the device's S before they compare the counts.
DT = {'interval': 0.05, 'disc': 0.05}
PICARD = {('interval', 'euler_imex'): (0.01, 2e-4), ('interval', 'ars3'): (0.05, 3e-4), ('interval', 'koto'): (0.05, 3e-4),
          ('disc', 'euler_imex'): (0.02, 1e-4), ('disc', 'ars3'): (0.05, 1e-4), ('disc', 'koto'): (0.05, 3e-4)}


def picard_margin_ok(R, tol):
    return all(not (tol/2. <= x <= 2.*tol) for norms in R.picardNorms for x in norms)


@pytest.mark.gpu
@pytest.mark.parametrize('bc', ['Neumann', 'Dirichlet'])
@pytest.mark.parametrize('domain', ['interval', 'disc'])
def test_neumann_operator_annihilates_constants_and_S_is_symmetric(domain, bc):
    p, h, dm, S, M, u0 = setup(domain, bc)
    assert np.array_equal(S, S.T) or np.abs(S-S.T).max() <= 1e-13*np.abs(S).max()
    if bc == 'Neumann':
        rs = np.abs(S.sum(axis=1)).max()
        print(domain, 'row sums', rs, 'max|S|', np.abs(S).max())
        assert rs <= 1e-10*np.abs(S).max()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['step', 'picard'])
@pytest.mark.parametrize('name', SCHEMES)
@pytest.mark.parametrize('bc', ['Neumann', 'Dirichlet'])
@pytest.mark.parametrize('domain', ['interval', 'disc'])
def test_chol_steppers_against_restatement(domain, bc, name, mode):
    import torch
    from pynucleus_amd.timestepping import timestepperFactory
    p, h, dm, S, M, u0 = setup(domain, bc)
    dt, ptol = (DT[domain], None) if mode == 'step' else PICARD[domain, name]
    st = timestepperFactory(name, h, p.nonlinearity, dt, massScales=p.massScales, solver='chol', massTol=1e-13)
    R = Restated(name, dm, f_brusselator(p.B, p.Q), S, M, p.massScales, dt)
    u, ur, t = dev(u0), u0.copy(), 0.
    if mode == 'step':
        for _ in range(3):
            t = st.step(t, dt, u)
            ur = R.step(ur)
        assert abs(t-3*dt) < 1e-14
    else:
        counts, rcounts = [], []
        for _ in range(2):
            t, its = st.picardStep(t, dt, u, tol=ptol)
            ur, rits = R.picardStep(ur, ptol)
            counts.append(its)
            rcounts.append(rits)
        print(domain, bc, name, 'picard norms', R.picardNorms, 'device', st.picardNorms)
        assert picard_margin_ok(R, ptol), R.picardNorms
        assert counts == rcounts and min(counts) >= 3, (counts, rcounts)
    torch.cuda.synchronize()
    got = u.cpu().numpy()
    bound = chol_bound(R, dm.num_dofs, ur)
    err = np.abs(got-ur).max()
    print(domain, bc, name, mode, 'err', err, 'bound', bound, 'solves', R.solves, 'max|u|', np.abs(ur).max())
    assert np.isfinite(got).all() and err <= bound, (err, bound)
    assert np.abs(ur-u0).max() > 1e-3                                # the steps moved the solution


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['step', 'picard'])
@pytest.mark.parametrize('name', SCHEMES)
@pytest.mark.parametrize('bc', ['Neumann', 'Dirichlet'])
def test_cg_mg_steppers_against_restatement(bc, name, mode):
    """solver='cg-mg' on the interval at tol = 1e-10: the criterion sqrt(r.Br) <= tol bounds the error of a solve in the energy
    norm of T = m_c M + dt gamma S up to the spectral equivalence of the preconditioner and T^-1, hence
    10 tol / sqrt(lambda_min(T)) per solve (the smaller lambda_min of the two components); the mass solves run at 1e-13."""
    import torch
    from pynucleus_amd.timestepping import timestepperFactory
    p, h, dm, S, M, u0 = setup('interval', bc)
    tol = 1e-10
    dt, ptol = (DT['interval'], None) if mode == 'step' else PICARD['interval', name]
    st = timestepperFactory(name, h, p.nonlinearity, dt, massScales=p.massScales, solver='cg-mg', tol=tol, massTol=1e-13)
    R = Restated(name, dm, f_brusselator(p.B, p.Q), S, M, p.massScales, dt)
    u, ur, t = dev(u0), u0.copy(), 0.
    if mode == 'step':
        for _ in range(3):
            t = st.step(t, dt, u)
            ur = R.step(ur)
    else:
        counts, rcounts = [], []
        for _ in range(2):
            t, its = st.picardStep(t, dt, u, tol=ptol)
            ur, rits = R.picardStep(ur, ptol)
            counts.append(its)
            rcounts.append(rits)
        assert picard_margin_ok(R, ptol), R.picardNorms
        assert counts == rcounts, (counts, rcounts)
    torch.cuda.synchronize()
    got = u.cpu().numpy()
    lmin = min(np.linalg.eigvalsh(R.implicit_system(c))[0] for c in range(2))
    bound = 10.*tol/np.sqrt(lmin)*R.solves
    err = np.abs(got-ur).max()
    its = np.array(st.iterations)
    print(bc, name, mode, 'err', err, 'bound', bound, 'lambda_min', lmin, 'iterations max', its.max())
    assert err <= bound, (err, bound)
    assert its[:, :-1].max() > 0 and its[:, :-1].max() < st.maxiter and its[:, -1].max() < st.massMaxiter


@pytest.mark.gpu
@pytest.mark.parametrize('name', SCHEMES)
def test_forcing(name):
    """a constant random force block [s, ncomp, n] (the values of g at the stages)"""
    import torch
    from pynucleus_amd.timestepping import timestepperFactory
    p, h, dm, S, M, u0 = setup('interval', 'Dirichlet')
    dt = DT['interval']
    st = timestepperFactory(name, h, p.nonlinearity, dt, massScales=p.massScales, solver='chol', massTol=1e-13)
    R = Restated(name, dm, f_brusselator(p.B, p.Q), S, M, p.massScales, dt)
    g = np.random.default_rng(11).uniform(-1., 1., size=(st.s, 2, dm.num_dofs))
    u, ur, t = dev(u0), u0.copy(), 0.
    for _ in range(2):
        t = st.step(t, dt, u, force=g)
        ur = R.step(ur, g)
    torch.cuda.synchronize()
    err, bound = np.abs(u.cpu().numpy()-ur).max(), chol_bound(R, dm.num_dofs, ur)
    unforced = Restated(name, dm, f_brusselator(p.B, p.Q), S, M, p.massScales, dt)
    v = unforced.step(unforced.step(u0.copy()))
    assert np.abs(v-ur).max() > 1e-3                                 # the force matters
    assert err <= bound, (err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('bc', ['Neumann', 'Dirichlet'])
def test_euler_imex_reduces_to_implicit_euler(bc):
    """without the nonlinearity (cubic at u = 0 is 0, and stays 0) EulerIMEX.step is ImplicitEuler.step with solver='chol' on the same
    hierarchy: for force = None both leave u = 0 exactly; with the same load in both (g at t + dt) they take the same non-trivial
    steps, to the chol bound of the restatement"""
    import torch
    from pynucleus_amd.timestepping import EulerIMEX
    from pynucleus_amd.multigrid import ImplicitEuler
    from pynucleus_amd.reaction import cubic
    p, h, dm, S, M, u0 = setup('interval', bc)
    n, dt = dm.num_dofs, DT['interval']
    st = EulerIMEX(h, cubic(), dt, solver='chol', massTol=1e-13)
    ie = ImplicitEuler(h, dt, solver='chol')
    u, v = dev(np.zeros((1, n))), dev(np.zeros(n))
    st.step(0., dt, u)
    ie.step(0., v, np.zeros(n))
    assert not u.any() and not v.any()
    # one step from zero with a load: N(0) = 0 in the explicit stage, so the step is linear
    g = np.random.default_rng(3).uniform(-1., 1., size=n)
    st.step(0., dt, u, force=np.stack([np.zeros(n), g])[:, None, :])
    ie.step(0., v, g)
    torch.cuda.synchronize()
    R = Restated('euler_imex', dm, f_cubic, S, M, [1.], dt)
    ur = R.step(np.zeros((1, n)), np.stack([np.zeros(n), g])[:, None, :])
    a, b = u.cpu().numpy()[0], v.cpu().numpy()
    bound = chol_bound(R, n, ur)
    print(bc, 'euler vs implicit euler', np.abs(a-b).max(), 'vs restatement', np.abs(a-ur[0]).max(), 'bound', bound)
    assert np.abs(ur).max() > 1e-3
    assert np.abs(a-ur[0]).max() <= bound and np.abs(b-ur[0]).max() <= bound and np.abs(a-b).max() <= bound


@pytest.mark.gpu
def test_unsupported_configurations_raise():
    from pynucleus_amd.timestepping import ARS3, IMEX, tableau
    from pynucleus_amd.reaction import cubic
    p, h, dm, S, M, u0 = setup('interval', 'Dirichlet')
    with pytest.raises(NotImplementedError):
        ARS3(h, p.nonlinearity, 0.1, massScales=p.massScales, solver='lu')
    with pytest.raises(NotImplementedError):
        ARS3(h, p.nonlinearity, 0.1, massScales=p.massScales, solver='gmres')
    L = dict(h.finest)

    class NotDense:
        num_rows = num_columns = dm.num_dofs
    L['A'] = NotDense()
    with pytest.raises(NotImplementedError):
        ARS3(h.getLevelList()[:-1]+[L], p.nonlinearity, 0.1, massScales=p.massScales)
    A = h.finest['A']
    try:
        A.symmetric = False
        with pytest.raises(NotImplementedError):
            ARS3(h, p.nonlinearity, 0.1, massScales=p.massScales)
    finally:
        A.symmetric = True
    c, AE, AI, bE, bI = tableau('ars3')
    AI2 = AI.copy()
    AI2[2, 2] = 0.5
    with pytest.raises(NotImplementedError):
        IMEX(h, cubic(), 0.1, c, AE, AI2, bE, bI, solver='chol')


# ---- GPU: mass solve -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('element', ['P1', 'P2'])
@pytest.mark.parametrize('mesh', ['disc2', 'interval67'])
def test_csr_cg_jacobi_on_mass_matrices(mesh, element):
    """pnl_csr_cg_jacobi at tol = 1e-12 against numpy.linalg.solve on the dense matrix.  sqrt(r.D^-1 r) <= tol bounds the error in
    the M-norm up to the spectral equivalence of D and M (the factor 10), so |x - x_ref|_2 <= 10 tol / sqrt(lambda_min(M))."""
    import torch
    from test_reaction import dofmap
    from pynucleus_amd.multigrid import _DevCSR
    from pynucleus_amd.reaction import _default_context
    dm = dofmap(mesh, element, 'NO_BOUNDARY')
    Msp = dm.assembleMass()
    M = Msp.toarray()
    n, tol = dm.num_dofs, 1e-12
    ctx = _default_context(torch.device('cuda', 0))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    Md = _DevCSR(Msp, 'cuda:0')
    rng = np.random.default_rng(n)
    b, x0 = rng.uniform(-1., 1., n), rng.uniform(-1., 1., n)
    lmin = np.linalg.eigvalsh(M)[0]
    for scale, zero in ((1., True), (0.04, False)):
        x = dev(np.full(n, np.nan) if zero else x0)
        its, res = ctx.csr_cg_jacobi(n, Md.indptr.data_ptr(), Md.indices.data_ptr(), Md.data.data_ptr(), scale, dev(b).data_ptr(), x.data_ptr(),
                                     tol, 1000, x_is_zero=zero)
        ctx.synchronize()
        ref = np.linalg.solve(scale*M, b)
        err, bound = np.linalg.norm(x.cpu().numpy()-ref), 10.*tol/np.sqrt(scale*lmin)
        print(mesh, element, 'scale', scale, 'n', n, 'iterations', its, 'criterion', res, 'err', err, 'bound', bound)
        assert 0 < its < 1000 and res <= tol and err <= bound, (its, res, err, bound)
    # the iteration cap is honoured and reported
    x = dev(np.zeros(n))
    its, res = ctx.csr_cg_jacobi(n, Md.indptr.data_ptr(), Md.indices.data_ptr(), Md.data.data_ptr(), 1., dev(b).data_ptr(), x.data_ptr(), tol, 2)
    assert its == 2 and res > tol


# ---- GPU: order of convergence ---------------------------------------------------------------------------------------------
# on the restatement (operator of the CPU oracle) the ratios 16 -> 32 steps over T = 0.25 are 2.05, 3.68, 7.54
ORDER_T = 0.25
ORDER_STEPS = {'euler_imex': (16, 32), 'koto': (16, 32), 'ars3': (16, 32)}
_order_ref = {}


def order_reference(R0args, nfine):
    """the restatement with ARS3 at the fine step, run once and shared by the three schemes"""
    if nfine not in _order_ref:
        dm, f, S, M, ms, u0 = R0args
        R = Restated('ars3', dm, f, S, M, ms, ORDER_T/nfine)
        u = u0.copy()
        for _ in range(nfine):
            u = R.step(u)
        _order_ref[nfine] = u
    return _order_ref[nfine]


@pytest.mark.gpu
@pytest.mark.parametrize('name', SCHEMES)
def test_order_of_convergence(name):
    """interval, Dirichlet, solver='chol', plain steps to T: the error against ARS3 at dt / 64 (restatement) falls by 2^p per halving
    of dt, p = 1, 2, 3 for euler_imex, koto, ars3.  The step counts are those at which the RESTATEMENT's ratio lies within 20 % of
    2^p (asserted first); the device run must then show the same."""
    import torch
    from pynucleus_amd.timestepping import timestepperFactory
    p, h, dm, S, M, u0 = setup('interval', 'Dirichlet')
    f = f_brusselator(p.B, p.Q)
    n1, n2 = ORDER_STEPS[name]
    ref = order_reference((dm, f, S, M, p.massScales, u0), 64*max(n for pair in ORDER_STEPS.values() for n in pair))
    errs, rerrs = [], []
    for nsteps in (n1, n2):
        dt = ORDER_T/nsteps
        R = Restated(name, dm, f, S, M, p.massScales, dt)
        st = timestepperFactory(name, h, p.nonlinearity, dt, massScales=p.massScales, solver='chol', massTol=1e-13)
        u, ur, t = dev(u0), u0.copy(), 0.
        for _ in range(nsteps):
            t = st.step(t, dt, u)
            ur = R.step(ur)
        torch.cuda.synchronize()
        errs.append(np.linalg.norm(u.cpu().numpy()-ref))
        rerrs.append(np.linalg.norm(ur-ref))
    want = 2.**ORDER[name]
    print(name, 'restatement', rerrs, rerrs[0]/rerrs[1], 'device', errs, errs[0]/errs[1])
    assert abs(rerrs[0]/rerrs[1]-want) <= 0.2*want, rerrs
    assert abs(errs[0]/errs[1]-want) <= 0.2*want, errs
