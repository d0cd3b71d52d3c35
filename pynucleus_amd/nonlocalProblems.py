"""Problem definitions of the transient drivers.

``brusselatorProblem`` mirrors nl/PyNucleus_nl/nonlocalProblems.py:2450-2591: the fractional Brusselator

              dU/dt = -(-Laplace)^alpha U + (B - 1) U + Q^2 V + B/Q U^2 + 2 Q U V + U^2 V
        eta^2 dV/dt = -(-Laplace)^beta  V -      B  U - Q^2 V - B/Q U^2 - 2 Q U V - U^2 V

with alpha = beta, so that both species share one operator S and differ in their mass scales (1, eta^2).
"""
import numpy as np


class brusselatorProblem:
    """brusselatorProblem(domain='disc' | 'interval', bc='Neumann' | 'Dirichlet', noRef, problem='spots' | 'stripes', radius=50.,
    seed=0): parameters, kernel, nonlinearity, seed mesh and initial data.  The finest mesh is the seed mesh refined ``noRef``
    times (disc: the hexagon of the given radius; interval: (-radius, radius) in two cells, so that a Dirichlet space has a DoF
    on the coarsest level)."""

    def __init__(self, domain='disc', bc='Neumann', noRef=3, problem='spots', radius=50., seed=0):
        from .kernels import getFractionalKernel
        from .mesh import simpleInterval, uniform_disc, PHYSICAL, NO_BOUNDARY
        from .reaction import brusselator
        if domain not in ('disc', 'interval'):
            raise NotImplementedError('domain {!r}: disc and interval are built (twinDisc is not)'.format(domain))
        if bc not in ('Neumann', 'Dirichlet'):
            raise NotImplementedError('boundary condition {!r}'.format(bc))
        if problem == 'spots':
            x = 0.1
        elif problem == 'stripes':
            x = 1.5
        else:
            raise NotImplementedError('problem {!r}: spots and stripes'.format(problem))
        self.domain, self.bc, self.noRef, self.problem, self.radius, self.seed = domain, bc, int(noRef), problem, float(radius), seed
        self.alpha = self.beta = 0.75
        self.eta = 0.2
        s =self.alpha/self.beta
        self.Bcr = (1.+x)**2/(1.+(1.-s)*x)
        self.kcr = x**(1./self.alpha)
        self.B = self.Bcr+0.01
        self.Q = np.sqrt(s*x**(1.+1./s)/(1.+(1.-s)*x))
        self.A = self.Q/self.eta
        self.Dx = 1.
        self.Dy = 1./self.eta**2
        self.massScales = np.array([1., self.eta**2])
        self.dim = 2 if domain == 'disc' else 1
        self.kernel = self.kernelU = self.kernelV = getFractionalKernel(self.dim, self.alpha)
        self.nonlinearity = brusselator(self.B, self.Q)
        # zero flux: the regional operator on all vertices; Dirichlet: zero exterior values, boundary vertices carry no DoF
        self.tag = NO_BOUNDARY if bc == 'Neumann' else PHYSICAL
        self.zeroExterior = bc == 'Dirichlet'
        if domain == 'disc':
            self.mesh = uniform_disc(self.radius)
        else:
            self.mesh = simpleInterval(-self.radius, self.radius).refine()

    def initial_U(self, x):
        R = 10.
        r2 = float(np.dot(x, x))
        return (R**2-r2)**2/R**4*self.eta if r2 < R**2 else 0.

    def initial_V(self, x):
        R = 10.
        r2 = float(np.dot(x, x))
        return (R**2-r2)**2/R**4/self.eta if r2 < R**2 else 0.

    def initial(self, dm):
        """[2, num_dofs] initial data on a DoF map: the bump of radius 10 (spots) or seeded uniform random numbers (stripes), U
        times eta, V divided by eta"""
        if self.problem == 'spots':
            return np.stack([np.asarray(dm.interpolate(self.initial_U)), np.asarray(dm.interpolate(self.initial_V))])
        rng = np.random.default_rng(self.seed)
        return np.stack([rng.random(dm.num_dofs)*self.eta, rng.random(dm.num_dofs)/self.eta])

    def hierarchy(self, element='P1', device=None):
        """the fractionalHierarchy of the problem's operator with mass matrices"""
        from .multigrid import fractionalHierarchy
        return fractionalHierarchy(self.domain, self.noRef, self.kernel, element=element, buildMass=True, tag=self.tag, device=device,
                                   mesh=self.mesh, zeroExterior=self.zeroExterior)
