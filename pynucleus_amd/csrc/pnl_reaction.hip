// Pointwise nonlinearities against the test functions and the IMEX Runge-Kutta sweep of reaction-diffusion systems with a
// nonlocal operator (gfx950 only).
//
// Reference (Cython / Python, CPU):
//   fem/PyNucleus_fem/femCy.pyx:3087-3178                 assembleNonlinearity (cell loop, scatter-add into the vector)
//   fem/PyNucleus_fem/femCy.pyx:3025-3041                 brusselator (multi_function)
//   base/PyNucleus_base/timestepping.py:377-682           IMEX, EulerIMEX, ARS3, koto (_stepOfPicard)
//
// Assembly without float atomics (two passes, bitwise reproducible): pass 1 gives every cell to one lane, which gathers the
// cell's DoF values, evaluates f at the quadrature points and stores the nout x dofs_per_cell local contributions with plain,
// coalesced stores ([out][local][cell]); pass 2 gives every DoF to one lane, which adds the DoF's contributions in the fixed
// order of an inverted index (ascending cell number) and applies alpha / beta.  A vertex of these meshes lies in at most ~8 cells,
// so the lists are short and even.  The sweep composes the library's own products and solvers; everything stays in HBM.
#include "pnl_context.h"
#include "pnl_common.h"

#define PNL_FE_MAX_DPC 6
#define PNL_FE_MAX_NQ 7

struct pnl_fe_space {
    pnl_context *ctx = nullptr;
    int ncells = 0, dpc = 0, nq = 0, ndofs = 0;
    DevBuf dofs, vol, phiw, inv_ptr, inv_idx, work;     // phiw: phi[dpc][nq] followed by w[nq]; work: [PNL_FUN_MAX_OUT][dpc][ncells]
};

struct pnl_imex {
    pnl_context *ctx = nullptr;
    pnl_imex_desc d;
    double gamma = 0.;                  // the non-zero diagonal of A^I
    bool explicit_stage[PNL_IMEX_MAX_STAGES], need_E[PNL_IMEX_MAX_STAGES], need_I[PNL_IMEX_MAX_STAGES];
    DevBuf store;                       // U, E, I: [s][ncomp][n] each; Mu: [ncomp][n]; rhs: [n]
};

namespace {

constexpr int FUN_MAX_IO = 2;

struct FunParams { double p[4]; };

template <int FUN> struct FunTraits;
template <> struct FunTraits<PNL_FUN_BRUSSELATOR> { static constexpr int nin = 2, nout = 2, nparams = 2; };
template <> struct FunTraits<PNL_FUN_CUBIC> { static constexpr int nin = 1, nout = 1, nparams = 0; };

template <int FUN>
__device__ __forceinline__ void fun_eval(const FunParams &P, const double *u, double *f) {
    if constexpr (FUN == PNL_FUN_BRUSSELATOR) {
        const double B = P.p[0], Q = P.p[1], x = u[0], y = u[1];
        const double z = B*x+Q*Q*y+(B/Q)*x*x+2.*Q*x*y+x*x*y;
        f[0] = -x+z;
        f[1] = -z;
    } else {
        f[0] = u[0]*u[0]*u[0]-u[0];
    }
}

// pass 1: one lane per cell (grid stride).  work[(o * DPC + m) * ncells + c] = vol_c sum_q w_q f_o(u(c, q)) phi_m(xi_q)
template <int DPC, int FUN>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_nl_cells(int ncells, int nq, const int *__restrict__ dofs, const double *__restrict__ vol, const double *__restrict__ phiw, FunParams P,
           const double *__restrict__ U, long long ldU, double *__restrict__ work) {
    constexpr int NIN = FunTraits<FUN>::nin, NOUT = FunTraits<FUN>::nout;
    __shared__ double s_phi[PNL_FE_MAX_DPC*PNL_FE_MAX_NQ+PNL_FE_MAX_NQ];
    for (int t = threadIdx.x; t < DPC*nq+nq; t += PNL_NTHREADS) s_phi[t] = phiw[t];
    __syncthreads();
    const double *s_w = s_phi+DPC*nq;
    for (int c = blockIdx.x*PNL_NTHREADS+threadIdx.x; c < ncells; c += gridDim.x*PNL_NTHREADS) {
        double ul[NIN][DPC], acc[NOUT][DPC];
#pragma unroll
        for (int m = 0; m < DPC; m++) {
            const int I = dofs[(size_t)c*DPC+m];
#pragma unroll
            for (int j = 0; j < NIN; j++) ul[j][m] = I >= 0 ? U[j*ldU+I] : 0.;
#pragma unroll
            for (int o = 0; o < NOUT; o++) acc[o][m] = 0.;
        }
        for (int q = 0; q < nq; q++) {
            double uq[NIN], f[NOUT];
#pragma unroll
            for (int j = 0; j < NIN; j++) {
                double s = 0.;
#pragma unroll
                for (int m = 0; m < DPC; m++) s = __builtin_fma(ul[j][m], s_phi[m*nq+q], s);
                uq[j] = s;
            }
            fun_eval<FUN>(P, uq, f);
            const double w = s_w[q];
#pragma unroll
            for (int o = 0; o < NOUT; o++) {
                const double wf = w*f[o];
#pragma unroll
                for (int m = 0; m < DPC; m++) acc[o][m] = __builtin_fma(wf, s_phi[m*nq+q], acc[o][m]);
            }
        }
        const double v = vol[c];
#pragma unroll
        for (int o = 0; o < NOUT; o++)
#pragma unroll
            for (int m = 0; m < DPC; m++) work[(size_t)(o*DPC+m)*ncells+c] = v*acc[o][m];
    }
}

// pass 2: one lane per DoF.  R[o][I] = beta R[o][I] + alpha sum over the DoF's list, in list order
__global__ void __launch_bounds__(PNL_NTHREADS)
k_nl_dofs(int ndofs, int nout, long long ostride, const int *__restrict__ inv_ptr, const int *__restrict__ inv_idx,
          const double *__restrict__ work, double alpha, double beta, double *R, long long ldR) {
    const int I = blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (I >= ndofs) return;
    const int b = inv_ptr[I], e = inv_ptr[I+1];
    for (int o = 0; o < nout; o++) {
        const double *wo = work+o*ostride;
        double s = 0.;
        for (int t = b; t < e; t++) s += wo[inv_idx[t]];
        double *r = R+o*ldR+I;
        *r = beta != 0. ? __builtin_fma(alpha, s, beta*(*r)) : alpha*s;
    }
}

// out[i] = base[i] + sum_t coef[t] rows[t][i]: the right-hand side of a stage from the stored E_j, I_j, g_j in one pass
struct LinComb {
    int nterms;
    double coef[3*PNL_IMEX_MAX_STAGES];
    const double *rows[3*PNL_IMEX_MAX_STAGES];
};

__global__ void __launch_bounds__(PNL_NTHREADS)
k_imex_rhs(int n, const double *__restrict__ base, LinComb L, double *__restrict__ out) {
    const int i = blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (i >= n) return;
    double s = base[i];
    for (int t = 0; t < L.nterms; t++) s = __builtin_fma(L.coef[t], L.rows[t][i], s);
    out[i] = s;
}

inline unsigned nblocks(long long n) { return (unsigned)std::max<long long>(1, (n+PNL_NTHREADS-1)/PNL_NTHREADS); }

template <int DPC, int FUN>
void launch_cells(pnl_fe_space *sp, const FunParams &P, const double *U, long long ldU) {
    const unsigned grid = std::min(nblocks(sp->ncells), 2048u);
    hipLaunchKernelGGL((k_nl_cells<DPC, FUN>), dim3(grid), dim3(PNL_NTHREADS), 0, sp->ctx->stream, sp->ncells, sp->nq, (const int*)sp->dofs.p,
                       (const double*)sp->vol.p, (const double*)sp->phiw.p, P, U, ldU, (double*)sp->work.p);
}

template <int FUN>
int launch_fun(pnl_fe_space *sp, const FunParams &P, const double *U, long long ldU) {
    switch (sp->dpc) {
    case 2: launch_cells<2, FUN>(sp, P, U, ldU); break;
    case 3: launch_cells<3, FUN>(sp, P, U, ldU); break;
    case 6: launch_cells<6, FUN>(sp, P, U, ldU); break;
    default: return fail(sp->ctx, PNL_ERR_UNSUPPORTED, "pnl_assemble_nonlinearity: %d DoFs per cell (2, 3 and 6 are built)", sp->dpc);
    }
    return PNL_OK;
}

}  // namespace

extern "C" {

int pnl_fe_space_create(pnl_context *ctx, int ncells, int dofs_per_cell, int nq, int ndofs, const int32_t *dofs_host, const double *vol_host,
                        const double *phi_host, const double *w_host, pnl_fe_space **out) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!out || ncells <= 0 || ndofs <= 0 || !dofs_host || !vol_host || !phi_host || !w_host)
        return fail(ctx, PNL_ERR_INVALID, "pnl_fe_space_create: null pointer or empty space");
    if (dofs_per_cell != 2 && dofs_per_cell != 3 && dofs_per_cell != 6)
        return fail(ctx, PNL_ERR_UNSUPPORTED, "pnl_fe_space_create: %d DoFs per cell (2, 3 and 6 are built)", dofs_per_cell);
    if (nq < 1 || nq > PNL_FE_MAX_NQ) return fail(ctx, PNL_ERR_INVALID, "pnl_fe_space_create: 1 .. %d quadrature points", PNL_FE_MAX_NQ);
    if ((long long)ncells*dofs_per_cell*FUN_MAX_IO > 0x7fffffffLL) return fail(ctx, PNL_ERR_UNSUPPORTED, "pnl_fe_space_create: too many cells");
    const int dpc = dofs_per_cell;
    // inverted index DoF -> (cell, local index), ascending cell number; an entry is the workspace offset m * ncells + c
    std::vector<int> ptr(ndofs+1, 0);
    for (long long t = 0; t < (long long)ncells*dpc; t++) {
        const int I = dofs_host[t];
        if (I >= ndofs) return fail(ctx, PNL_ERR_INVALID, "pnl_fe_space_create: DoF %d of cell %lld is not below ndofs = %d", I, t/dpc, ndofs);
        if (I >= 0) ptr[I+1]++;
    }
    for (int I = 0; I < ndofs; I++) ptr[I+1] += ptr[I];
    std::vector<int> idx(std::max(ptr[ndofs], 1)), fill(ptr.begin(), ptr.end()-1);
    for (int c = 0; c < ncells; c++)
        for (int m = 0; m < dpc; m++) {
            const int I = dofs_host[(size_t)c*dpc+m];
            if (I >= 0) idx[fill[I]++] = m*ncells+c;
        }
    std::vector<double> phiw(phi_host, phi_host+dpc*nq);
    phiw.insert(phiw.end(), w_host, w_host+nq);
    pnl_fe_space *sp = new pnl_fe_space;
    sp->ctx = ctx; sp->ncells = ncells; sp->dpc = dpc; sp->nq = nq; sp->ndofs = ndofs;
    int rc;
    if ((rc = upload(ctx, sp->dofs, dofs_host, (size_t)ncells*dpc)) || (rc = upload(ctx, sp->vol, vol_host, (size_t)ncells)) ||
        (rc = upload(ctx, sp->phiw, phiw.data(), phiw.size())) || (rc = upload(ctx, sp->inv_ptr, ptr.data(), ptr.size())) ||
        (rc = upload(ctx, sp->inv_idx, idx.data(), idx.size())) ||
        (rc = ensure(ctx, sp->work, sizeof(double)*(size_t)FUN_MAX_IO*dpc*ncells))) {
        delete sp;
        return rc;
    }
    *out = sp;
    return PNL_OK;
}

int pnl_fe_space_destroy(pnl_fe_space *space) {
    if (!space) return PNL_ERR_INVALID;
    (void)hipStreamSynchronize(space->ctx->stream);
    delete space;
    return PNL_OK;
}

int pnl_assemble_nonlinearity(pnl_fe_space *space, int fun, const double *params_host, int nparams, int nin, const double *U_dev, int64_t ldU,
                              int nout, double alpha, double beta, double *R_dev, int64_t ldR) {
    if (!space) return PNL_ERR_INVALID;
    pnl_context *ctx = space->ctx;
    int want_in, want_out, want_p;
    switch (fun) {
    case PNL_FUN_BRUSSELATOR: want_in = 2; want_out = 2; want_p = 2; break;
    case PNL_FUN_CUBIC: want_in = 1; want_out = 1; want_p = 0; break;
    default: return fail(ctx, PNL_ERR_INVALID, "pnl_assemble_nonlinearity: unknown function %d", fun);
    }
    if (nin != want_in || nout != want_out)
        return fail(ctx, PNL_ERR_INVALID, "pnl_assemble_nonlinearity: function %d maps %d -> %d values, got nin = %d, nout = %d", fun, want_in,
                    want_out, nin, nout);
    if (nparams != want_p || (want_p > 0 && !params_host))
        return fail(ctx, PNL_ERR_INVALID, "pnl_assemble_nonlinearity: function %d takes %d parameters, got %d", fun, want_p, nparams);
    if (!U_dev || !R_dev || ldU < space->ndofs || ldR < space->ndofs)
        return fail(ctx, PNL_ERR_INVALID, "pnl_assemble_nonlinearity: null vector or a leading dimension below ndofs = %d", space->ndofs);
    FunParams P = {{0., 0., 0., 0.}};
    for (int i = 0; i < want_p; i++) P.p[i] = params_host[i];
    int rc = fun == PNL_FUN_BRUSSELATOR ? launch_fun<PNL_FUN_BRUSSELATOR>(space, P, U_dev, (long long)ldU)
                                        : launch_fun<PNL_FUN_CUBIC>(space, P, U_dev, (long long)ldU);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nl_dofs, dim3(nblocks(space->ndofs)), dim3(PNL_NTHREADS), 0, ctx->stream, space->ndofs, nout,
                       (long long)space->dpc*space->ncells, (const int*)space->inv_ptr.p, (const int*)space->inv_idx.p,
                       (const double*)space->work.p, alpha, beta, R_dev, (long long)ldR);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// ---- IMEX Runge-Kutta (timestepping.py:377-682) --------------------------------------------------------------------------------
int pnl_imex_create(pnl_context *ctx, const pnl_imex_desc *desc, pnl_imex **out) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!desc || !out) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: null descriptor");
    const pnl_imex_desc &d = *desc;
    if (d.s < 1 || d.s > PNL_IMEX_MAX_STAGES || d.ncomp < 1 || d.ncomp > PNL_IMEX_MAX_COMP || d.n <= 0 || !(d.dt > 0.))
        return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: 1 .. %d stages, 1 .. %d components, n > 0 and dt > 0 are needed", PNL_IMEX_MAX_STAGES,
                    PNL_IMEX_MAX_COMP);
    if (!d.S_dev || d.ldS < d.n || !d.M_indptr_dev || !d.M_indices_dev || !d.M_data_dev || !d.space)
        return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: the operator, the mass matrix and the space are needed");
    if (d.space->ctx != ctx || d.space->ndofs != d.n) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: the space belongs to another context or size");
    const int want = d.fun == PNL_FUN_BRUSSELATOR ? 2 : d.fun == PNL_FUN_CUBIC ? 1 : -1;
    if (want < 0) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: unknown function %d", d.fun);
    if (want != d.ncomp) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: function %d couples %d components, got %d", d.fun, want, d.ncomp);
    if (d.solver != PNL_IMEX_CG_MG && d.solver != PNL_IMEX_CHOL) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: unknown solver %d", d.solver);
    if (d.maxiter < 0 || d.mass_maxiter < 0) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: negative iteration cap");
    for (int c = 0; c < d.ncomp; c++) {
        if (!(d.mass_scale[c] > 0.)) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: mass scale of component %d is not positive", c);
        if (d.solver == PNL_IMEX_CG_MG ? !d.mg[c] : (!d.chol_dev[c] || d.ldchol[c] < d.n))
            return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: component %d has no solver (multigrid object or Cholesky factor)", c);
    }
    pnl_imex *im = new pnl_imex;
    im->ctx = ctx; im->d = d;
    const int s = d.s;
    for (int k = 0; k < s; k++) {
        bool rowE = false, colE = d.bE[k] != 0., colI = d.bI[k] != 0.;
        for (int j = 0; j < s; j++) {
            rowE = rowE || d.AE[k*s+j] != 0.;
            colE = colE || d.AE[j*s+k] != 0.;
            colI = colI || d.AI[j*s+k] != 0.;
            if (j > k && d.AI[k*s+j] != 0.) { delete im; return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: A^I is not lower triangular"); }
            if (j >= k && d.AE[k*s+j] != 0.) { delete im; return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: A^E is not strictly lower triangular"); }
        }
        im->explicit_stage[k] = !rowE; im->need_E[k] = colE; im->need_I[k] = colI;
        if (rowE) {
            const double g = d.AI[k*s+k];
            if (!(g > 0.) || (im->gamma != 0. && g != im->gamma)) {
                delete im;
                return fail(ctx, PNL_ERR_INVALID, "pnl_imex_create: the implicit stages need one positive diagonal entry of A^I (stage %d has %g)", k, g);
            }
            im->gamma = g;
        }
    }
    const size_t blk = (size_t)s*d.ncomp*d.n;
    int rc = ensure(ctx, im->store, sizeof(double)*(3*blk+(size_t)d.ncomp*d.n+d.n));
    if (rc) { delete im; return rc; }
    *out = im;
    return PNL_OK;
}

int pnl_imex_destroy(pnl_imex *imex) {
    if (!imex) return PNL_ERR_INVALID;
    (void)hipStreamSynchronize(imex->ctx->stream);
    delete imex;
    return PNL_OK;
}

// One sweep (u_prev, u) -> u_new (_stepOfPicard; E = -N(U), I = S U).  u_dev is read as the initial guess of every solve and receives
// u_new; u_prev_dev may be u_dev.  iters_out[(k * ncomp + c)]: iterations of the stage solves, iters_out[s * ncomp + c]: of the mass solves.
int pnl_imex_sweep(pnl_imex *imex, const double *u_prev_dev, double *u_dev, const double *force_dev, int32_t *iters_out) {
    if (!imex) return PNL_ERR_INVALID;
    pnl_context *ctx = imex->ctx;
    if (!u_prev_dev || !u_dev) return fail(ctx, PNL_ERR_INVALID, "pnl_imex_sweep: null vector");
    const pnl_imex_desc &d = imex->d;
    const int s = d.s, nc = d.ncomp, n = d.n;
    const size_t cn = (size_t)nc*n, blk = (size_t)s*cn;
    double *U = (double*)imex->store.p, *E = U+blk, *I = E+blk, *Mu = I+blk, *rhs = Mu+cn;
    const size_t vb = sizeof(double)*n;
    hipStream_t st = ctx->stream;
    int rc;
    if (iters_out) std::fill(iters_out, iters_out+(s+1)*nc, 0);
    for (int c = 0; c < nc; c++)
        if ((rc = pnl_csr_matvec(ctx, n, d.M_indptr_dev, d.M_indices_dev, d.M_data_dev, u_prev_dev+(size_t)c*n, d.mass_scale[c], 0., Mu+(size_t)c*n)))
            return rc;
    // rhs = Mu_c - dt sum_{j < nE} cE[j] E_j - dt sum_{j < nI} cI[j] I_j + dt sum_{j < ng} cI[j] g_j
    auto combine = [&](int c, const double *cE, int nE, const double *cI, int nI, int ng) -> int {
        LinComb L;
        L.nterms = 0;
        for (int j = 0; j < s; j++) {
            const size_t off = (size_t)j*cn+(size_t)c*n;
            if (j < nE && cE[j] != 0.) { L.coef[L.nterms] = -d.dt*cE[j]; L.rows[L.nterms++] = E+off; }
            if (j < nI && cI[j] != 0.) { L.coef[L.nterms] = -d.dt*cI[j]; L.rows[L.nterms++] = I+off; }
            if (j < ng && cI[j] != 0. && force_dev) { L.coef[L.nterms] = d.dt*cI[j]; L.rows[L.nterms++] = force_dev+off; }
        }
        hipLaunchKernelGGL(k_imex_rhs, dim3(nblocks(n)), dim3(PNL_NTHREADS), 0, st, n, (const double*)(Mu+(size_t)c*n), L, rhs);
        HIPCHK(ctx, hipGetLastError());
        return PNL_OK;
    };
    for (int k = 0; k < s; k++) {
        double *Uk = U+(size_t)k*cn;
        if (imex->explicit_stage[k]) {
            HIPCHK(ctx, hipMemcpyAsync(Uk, u_dev, sizeof(double)*cn, hipMemcpyDeviceToDevice, st));
        } else {
            for (int c = 0; c < nc; c++) {
                // the implicit term of stage k itself is on the left-hand side: E_j, I_j for j < k, g_j for j <= k
                if ((rc = combine(c, d.AE+k*s, k, d.AI+k*s, k, k+1))) return rc;
                double *Ukc = Uk+(size_t)c*n;
                if (d.solver == PNL_IMEX_CHOL) {
                    HIPCHK(ctx, hipMemcpyAsync(Ukc, rhs, vb, hipMemcpyDeviceToDevice, st));
                    if ((rc = pnl_potrs(ctx, d.chol_dev[c], d.ldchol[c], n, Ukc, n, 1))) return rc;
                } else {
                    HIPCHK(ctx, hipMemcpyAsync(Ukc, u_dev+(size_t)c*n, vb, hipMemcpyDeviceToDevice, st));
                    int its = 0;
                    if ((rc = pnl_mg_cg(d.mg[c], nullptr, 0, rhs, Ukc, d.tol, d.maxiter, 0, &its, nullptr, 0))) return rc;
                    if (iters_out) iters_out[k*nc+c] = its;
                }
            }
        }
        if (imex->need_E[k] &&
            (rc = pnl_assemble_nonlinearity(d.space, d.fun, d.params, d.nparams, nc, Uk, n, nc, -1., 0., E+(size_t)k*cn, n))) return rc;
        if (imex->need_I[k])
            for (int c = 0; c < nc; c++)
                if ((rc = pnl_gemv_axpby(ctx, d.S_dev, d.ldS, n, n, Uk+(size_t)c*n, 1., 0., nullptr, I+(size_t)k*cn+(size_t)c*n))) return rc;
    }
    for (int c = 0; c < nc; c++) {
        if ((rc = combine(c, d.bE, s, d.bI, s, s))) return rc;
        int its = 0;
        if ((rc = pnl_csr_cg_jacobi(ctx, n, d.M_indptr_dev, d.M_indices_dev, d.M_data_dev, d.mass_scale[c], rhs, u_dev+(size_t)c*n, d.mass_tol,
                                    d.mass_maxiter, 0, &its, nullptr))) return rc;
        if (iters_out) iters_out[s*nc+c] = its;
    }
    return PNL_OK;
}

}  // extern "C"
