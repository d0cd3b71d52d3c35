// Jacobi-preconditioned CG for a block of right-hand sides (gfx950 only): pnl_cg_jacobi_block for a dense symmetric positive definite
// block, and the steps of its loop (pnl_cgb_init / _update / _refresh / _direction) for operators whose product is made elsewhere.
//
// Reference: cg_solver.solve (base/PyNucleus_base/solvers.pyx:363-444) with the Jacobi preconditioner (:229-245), as pnl_cg_jacobi
// (pnl_solver.hip) restates it: update order x, r, (refresh), z = D^-1 r, beta, p; convergence on sqrt(r . D^-1 r) <= tol; the residual
// recomputed from b - A x when the counter reaches 50.
//
// Up to CGB_NV = 16 right-hand sides ("columns", stored one per row as in pnl_gemv_block) are solved together.  Every column runs its
// OWN recurrence -- its own alpha, beta and convergence; this is not O'Leary's block CG -- and the columns share the operator
// product: one pnl_gemv_block pass over the matrix per iteration.  A column that has converged is frozen: its x, r, z, p and its
// state are no longer written (the product still carries it along; its result is not used).
//
// Kernels, all over [nvec][n] blocks with ONE grid rule, cgb_blocks(n) = min(CGB_MAXBLK, ceil(n / 256)) workgroups of 256 threads,
// element i of every column in thread (i mod 256) of workgroup (i / 256) mod blocks:
//   k_kb_dot         partial sums of p . Ap per column and workgroup (pnl_krylov_block.h)                     -> part[0][wg][16]
//   k_cgb_update     every workgroup adds those partials (cgb_totals) to get alpha = betaOld / p.Ap, then x += alpha p,
//                    r -= alpha Ap, z = dinv r and the partial sums of r . z                                  -> part[1][wg][16]
//   k_cgb_residual   r = b - Ax, out = dinv r (out = p at the start, z in a refresh), partial sums of r . out  -> part[1][wg][16]
//   k_cgb_finish     one workgroup: adds the partials of part[1] and writes beta and conv (at the start: betaOld, conv, active)
//   k_cgb_direction  p = z + (beta / betaOld) p for the columns that go on
//   k_cgb_advance    one workgroup: betaOld = beta, or active = 0 where conv <= tol
// For a preconditioner that is applied between the calls (a multigrid cycle: pnl_mg_cg_block, pnl_mg_block.hip) the same kernels run
// split, without FUSED, on the same partial sums, grid rule and state (pnl_cgb_residual / _start / _step / _beta):
//   k_cgb_residual   r = b - Ax; no out, no sums
//   k_cgb_start      p = z and the partial sums of r . z (in the passes: k_kb_dot)                            -> part[1][wg][16]
//   k_cgb_update     up to r -= alpha Ap; no z, no sums
//   k_cgb_finish     with conv = sqrt(|r . z|), as pnl_mg_cg takes it
// The scalars stay on the device (state: PNL_CGB_STATE doubles per column); the driver reads the state back once per iteration.
//
// No floating-point atomics.  A dot product is summed in a fixed shape that depends on n only: per thread in ascending i (fma), the
// 64 lanes in the DPP tree of wave_sum, the four waves in ascending order, the workgroups in 16 interleaved runs in ascending order
// and those 16 in ascending order (cgb_block_sums and cgb_totals, pnl_krylov_block.h, shared with pnl_bicgstab_block.hip).  With a
// product whose bits are independent per vector (pnl_gemv_block, pnl_spmv_block on CSR, the ordered H2 far field) the bits of X[v], its iteration count and its residual therefore depend neither
// on nvec nor on the position v nor on the other columns, and two calls repeat bit for bit.  The redundant final adds cost
// 16 x blocks loads per workgroup, which the cap CGB_MAXBLK bounds at 4096.
#include "pnl_krylov_block.h"

namespace {

// slots of the per-column state (include/pnl_hip.h)
enum { ST_BETA_OLD = 0, ST_PAP = 1, ST_BETA = 2, ST_CONV = 3, ST_ACTIVE = 4 };
static_assert(ST_CONV == KB_ST_RES && ST_ACTIVE == KB_ST_ACTIVE, "the slots that the drivers read");

__device__ __forceinline__ unsigned cgb_active_mask(const double *__restrict__ state, int nv) { return kb_active_mask<PNL_CGB_STATE>(state, nv); }

// alpha = betaOld / p.Ap from the partials, x += alpha p, r -= alpha Ap; FUSED: z = dinv r (dinv == nullptr: the unit diagonal) and the
// partial sums of r . z as well
template <bool FUSED>
__global__ void __launch_bounds__(CGB_THREADS)
k_cgb_update(int n, int nv, const double *__restrict__ dinv, const double *__restrict__ P, long long ldp, const double *__restrict__ AP,
             long long ldap, double *__restrict__ X, long long ldx, double *__restrict__ R, long long ldr, double *__restrict__ Z, long long ldz,
             double *state, const double *__restrict__ part_pap, double *__restrict__ part_rz) {
    __shared__ double tot[CGB_NV], al[CGB_NV];
    const unsigned mask = cgb_active_mask(state, nv);
    cgb_totals(part_pap, (int)gridDim.x, tot);
    if (threadIdx.x < CGB_NV) {
        const int v = threadIdx.x;
        const bool on = (mask >> v) & 1;
        al[v] = on ? state[v*PNL_CGB_STATE+ST_BETA_OLD]/tot[v] : 0.;
        if (on && blockIdx.x == 0) state[v*PNL_CGB_STATE+ST_PAP] = tot[v];       // a slot that no workgroup of this launch reads
    }
    __syncthreads();
    double s[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = (FUSED && dinv) ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double alpha = al[v];
                X[v*ldx+i] = __builtin_fma(alpha, P[v*ldp+i], X[v*ldx+i]);
                const double ri = __builtin_fma(-alpha, AP[v*ldap+i], R[v*ldr+i]);
                R[v*ldr+i] = ri;
                if (FUSED) {
                    const double zi = dinv ? di*ri : ri;
                    Z[v*ldz+i] = zi;
                    s[v] = __builtin_fma(ri, zi, s[v]);
                }
            }
        }
    }
    if (FUSED) cgb_block_sums(s, mask, part_rz+(size_t)blockIdx.x*CGB_NV);
}

// r = b - Ax (AX == nullptr: r = b); FUSED: out = dinv r and the partial sums of r . out as well.  ALL: every column v < nv (a start:
// there is no state yet); else the active ones
template <bool ALL, bool FUSED>
__global__ void __launch_bounds__(CGB_THREADS)
k_cgb_residual(int n, int nv, const double *__restrict__ dinv, const double *__restrict__ B, long long ldb, const double *__restrict__ AX,
               long long ldax, double *__restrict__ R, long long ldr, double *__restrict__ Out, long long ldo, const double *__restrict__ state,
               double *__restrict__ part) {
    const unsigned mask = ALL ? (1u << nv)-1u : cgb_active_mask(state, nv);
    double s[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = (FUSED && dinv) ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double ri = AX ? B[v*ldb+i]-AX[v*ldax+i] : B[v*ldb+i];
                R[v*ldr+i] = ri;
                if (FUSED) {
                    const double oi = dinv ? di*ri : ri;
                    Out[v*ldo+i] = oi;
                    s[v] = __builtin_fma(ri, oi, s[v]);
                }
            }
        }
    }
    if (FUSED) cgb_block_sums(s, mask, part+(size_t)blockIdx.x*CGB_NV);
}

// one workgroup.  start: betaOld = beta = r . p, conv, active = conv > tol (a zero residual is never active: no 0 / 0 later);
// else, for the active columns, beta = r . z and conv
// abs_rz (the external-preconditioner steps): conv = sqrt(|r . z|), as pnl_mg_cg takes it
__global__ void __launch_bounds__(CGB_THREADS)
k_cgb_finish(int nb, int nv, const double *__restrict__ part, double tol, double *state, bool start, bool abs_rz) {
    __shared__ double tot[CGB_NV];
    cgb_totals(part, nb, tot);
    const int v = threadIdx.x;
    if (v >= nv) return;
    double *st = state+v*PNL_CGB_STATE;
    const double conv = sqrt(abs_rz ? fabs(tot[v]) : tot[v]);
    if (start) {
        st[ST_BETA_OLD] = tot[v]; st[ST_PAP] = 0.; st[ST_BETA] = tot[v]; st[ST_CONV] = conv;
        st[ST_ACTIVE] = (conv > tol && tot[v] != 0.) ? 1. : 0.;
        for (int k = ST_ACTIVE+1; k < PNL_CGB_STATE; k++) st[k] = 0.;
    } else if (st[ST_ACTIVE] != 0.) {
        st[ST_BETA] = tot[v]; st[ST_CONV] = conv;
    }
}

// p = z + (beta / betaOld) p for the active columns with conv > tol (the others are frozen by k_cgb_advance behind this launch)
__global__ void __launch_bounds__(CGB_THREADS)
k_cgb_direction(int n, int nv, const double *__restrict__ Z, long long ldz, double *__restrict__ P, long long ldp, double tol,
                const double *__restrict__ state) {
    __shared__ double tq[CGB_NV];
    unsigned mask = 0;
    for (int v = 0; v < nv; v++) {
        const double *st = state+v*PNL_CGB_STATE;
        if (st[ST_ACTIVE] != 0. && !(st[ST_CONV] <= tol)) mask |= 1u << v;
    }
    if (threadIdx.x < CGB_NV) {
        const double *st = state+threadIdx.x*PNL_CGB_STATE;
        tq[threadIdx.x] = ((mask >> threadIdx.x) & 1) ? st[ST_BETA]/st[ST_BETA_OLD] : 0.;
    }
    __syncthreads();
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int v = 0; v < CGB_NV; v++)
            if ((mask >> v) & 1) P[v*ldp+i] = __builtin_fma(tq[v], P[v*ldp+i], Z[v*ldz+i]);
    }
}

__global__ void k_cgb_advance(int nv, double tol, double *state) {
    const int v = threadIdx.x;
    if (v >= nv) return;
    double *st = state+v*PNL_CGB_STATE;
    if (st[ST_ACTIVE] == 0.) return;
    if (st[ST_CONV] <= tol) st[ST_ACTIVE] = 0.;
    else st[ST_BETA_OLD] = st[ST_BETA];
}

// the start for a preconditioner that is applied between the calls: p = z and the partial sums of r . z, every column v < nv
__global__ void __launch_bounds__(CGB_THREADS)
k_cgb_start(int n, int nv, const double *__restrict__ R, long long ldr, const double *__restrict__ Z, long long ldz, double *__restrict__ P,
            long long ldp, double *__restrict__ part) {
    const unsigned mask = (1u << nv)-1u;
    double s[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double zi = Z[v*ldz+i];
                P[v*ldp+i] = zi;
                s[v] = __builtin_fma(R[v*ldr+i], zi, s[v]);
            }
        }
    }
    cgb_block_sums(s, mask, part+(size_t)blockIdx.x*CGB_NV);
}

// the one-workgroup launch behind the partial sums of r . z (r . p at a start)
int cgb_finish(pnl_context *ctx, bool start, bool abs_rz, int n, int nv, const double *part, double tol, double *state) {
    KB_LAUNCH1(k_cgb_finish, ctx, cgb_blocks(n), nv, part, tol, state, start, abs_rz);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// p . Ap into part[0], then k_cgb_update<FUSED>: what pnl_cgb_update and pnl_cgb_step share
template <bool FUSED>
void cgb_update(pnl_context *ctx, int n, int nv, const double *dinv, const double *P, int64_t ldp, const double *AP, int64_t ldap, double *X,
                int64_t ldx, double *R, int64_t ldr, double *Z, int64_t ldz, double *state, double *part) {
    KB_LAUNCH((k_kb_dot<PNL_CGB_STATE, false>), ctx, n, nv, P, ldp, AP, ldap, state, part);
    KB_LAUNCH(k_cgb_update<FUSED>, ctx, n, nv, dinv, P, ldp, AP, ldap, X, ldx, R, ldr, Z, ldz, state, part, part+CGB_PART);
}

}  // namespace

extern "C" {

int pnl_cgb_init(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax,
                 double *R_dev, int64_t ldr, double *P_dev, int64_t ldp, double tol, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{B_dev, ldb, KB_READ}, {AX_dev, ldax, KB_APART | KB_OPTIONAL}, {R_dev, ldr, KB_WRITTEN}, {P_dev, ldp, KB_WRITTEN}}) ||
        !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_init: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH((k_cgb_residual<true, true>), ctx, n, nvec, dinv_dev, B_dev, ldb, AX_dev, ldax, R_dev, ldr, P_dev, ldp, state_dev, part+CGB_PART);
    HIPCHK(ctx, hipGetLastError());
    return cgb_finish(ctx, true, false, n, nvec, part+CGB_PART, tol, state_dev);
}

int pnl_cgb_update(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *P_dev, int64_t ldp, const double *AP_dev, int64_t ldap,
                   double *X_dev, int64_t ldx, double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{P_dev, ldp, KB_READ}, {AP_dev, ldap, KB_READ}, {X_dev, ldx, KB_WRITTEN}, {R_dev, ldr, KB_WRITTEN},
                              {Z_dev, ldz, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_update: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    cgb_update<true>(ctx, n, nvec, dinv_dev, P_dev, ldp, AP_dev, ldap, X_dev, ldx, R_dev, ldr, Z_dev, ldz, state_dev, part);
    HIPCHK(ctx, hipGetLastError());
    return cgb_finish(ctx, false, false, n, nvec, part+CGB_PART, 0., state_dev);
}

int pnl_cgb_refresh(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax,
                    double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{B_dev, ldb, KB_READ}, {AX_dev, ldax, KB_READ}, {R_dev, ldr, KB_WRITTEN}, {Z_dev, ldz, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_refresh: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH((k_cgb_residual<false, true>), ctx, n, nvec, dinv_dev, B_dev, ldb, AX_dev, ldax, R_dev, ldr, Z_dev, ldz, state_dev, part+CGB_PART);
    HIPCHK(ctx, hipGetLastError());
    return cgb_finish(ctx, false, false, n, nvec, part+CGB_PART, 0., state_dev);
}

int pnl_cgb_direction(pnl_context *ctx, int n, int nvec, const double *Z_dev, int64_t ldz, double *P_dev, int64_t ldp, double tol, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{Z_dev, ldz, KB_READ}, {P_dev, ldp, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_direction: bad arguments (n=%d nvec=%d)", n, nvec);
    KB_LAUNCH(k_cgb_direction, ctx, n, nvec, Z_dev, ldz, P_dev, ldp, tol, state_dev);
    hipLaunchKernelGGL(k_cgb_advance, dim3(1), dim3(64), 0, ctx->stream, nvec, tol, state_dev);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_cgb_residual(pnl_context *ctx, int n, int nvec, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax, double *R_dev,
                     int64_t ldr, const double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{B_dev, ldb, KB_READ}, {AX_dev, ldax, KB_READ | KB_OPTIONAL}, {R_dev, ldr, KB_WRITTEN}}))
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_residual: bad arguments (n=%d nvec=%d)", n, nvec);
    const auto k = state_dev ? k_cgb_residual<false, false> : k_cgb_residual<true, false>;        // no state yet: every column
    KB_LAUNCH(k, ctx, n, nvec, nullptr, B_dev, ldb, AX_dev, ldax, R_dev, ldr, nullptr, 0, state_dev, nullptr);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_cgb_start(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *Z_dev, int64_t ldz, double *P_dev, int64_t ldp,
                  double tol, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{R_dev, ldr, KB_READ}, {Z_dev, ldz, KB_READ}, {P_dev, ldp, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_start: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH(k_cgb_start, ctx, n, nvec, R_dev, ldr, Z_dev, ldz, P_dev, ldp, part+CGB_PART);
    HIPCHK(ctx, hipGetLastError());
    return cgb_finish(ctx, true, true, n, nvec, part+CGB_PART, tol, state_dev);
}

int pnl_cgb_step(pnl_context *ctx, int n, int nvec, const double *P_dev, int64_t ldp, const double *AP_dev, int64_t ldap, double *X_dev, int64_t ldx,
                 double *R_dev, int64_t ldr, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{P_dev, ldp, KB_READ}, {AP_dev, ldap, KB_READ}, {X_dev, ldx, KB_WRITTEN}, {R_dev, ldr, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_step: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    cgb_update<false>(ctx, n, nvec, nullptr, P_dev, ldp, AP_dev, ldap, X_dev, ldx, R_dev, ldr, nullptr, 0, state_dev, part);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_cgb_beta(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *Z_dev, int64_t ldz, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{R_dev, ldr, KB_READ}, {Z_dev, ldz, KB_READ}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cgb_beta: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH((k_kb_dot<PNL_CGB_STATE, false>), ctx, n, nvec, R_dev, ldr, Z_dev, ldz, state_dev, part+CGB_PART);
    HIPCHK(ctx, hipGetLastError());
    return cgb_finish(ctx, false, true, n, nvec, part+CGB_PART, 0., state_dev);
}

int pnl_cg_jacobi_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, int nrhs, const double *B_dev, int64_t ldb, double *X_dev,
                        int64_t ldx, double tol, int maxiter, int *iters, double *residuals) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!A_dev || !B_dev || !X_dev || n < 1 || nrhs < 1 || ldA < n || ldb < n || ldx < n || maxiter < 0 || B_dev == X_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_cg_jacobi_block: bad arguments (n=%d nrhs=%d ldA=%lld ldb=%lld ldx=%lld maxiter=%d)", n, nrhs,
                    (long long)ldA, (long long)ldb, (long long)ldx, maxiter);
    // work: dinv [n]; R, P, AP, Z [16][ld]; the state
    const int64_t ld = kb_ld(n);
    const int gmax = std::min(nrhs, CGB_NV);
    int rc;
    if ((rc = ensure(ctx, ctx->b_cgb_work, kb_work_bytes(ld, 4, gmax, ld, PNL_CGB_STATE)))) return rc;
    double *dinv = (double*)ctx->b_cgb_work.p;
    KbCarve work{dinv+ld, gmax*ld};
    double *R = work.next(), *P = work.next(), *AP = work.next(), *Z = work.next(), *state = work.p;
    if ((rc = pnl_inv_diagonal(ctx, A_dev, ldA, n, dinv))) return rc;
    for (int v0 = 0; v0 < nrhs; v0 += CGB_NV) {
        const int nv = std::min(CGB_NV, nrhs-v0);
        const double *B = B_dev+(int64_t)v0*ldb;
        double *X = X_dev+(int64_t)v0*ldx;
        KbColumns<PNL_CGB_STATE> cols{ctx, state, nv, iters ? iters+v0 : nullptr, residuals ? residuals+v0 : nullptr};
        auto product = [&](const double *V, int64_t ldv) { return pnl_gemv_block(ctx, A_dev, ldA, n, n, nv, V, ldv, 1., 0., nullptr, 0, AP, ld); };
        if ((rc = product(X, ldx))) return rc;
        if ((rc = pnl_cgb_init(ctx, n, nv, dinv, B, ldb, AP, ld, R, ld, P, ld, tol, state))) return rc;
        if ((rc = cols.read(-1))) return rc;
        int k = 0;
        for (int it = 0; it < maxiter && cols.nactive > 0; it++) {
            if ((rc = product(P, ld))) return rc;
            if ((rc = pnl_cgb_update(ctx, n, nv, dinv, P, ld, AP, ld, X, ldx, R, ld, Z, ld, state))) return rc;
            if (k == 50) {
                // recalculate the residual to limit rounding drift (solvers.pyx:412-415), for every active column of the group at once
                if ((rc = product(X, ldx))) return rc;
                if ((rc = pnl_cgb_refresh(ctx, n, nv, dinv, B, ldb, AP, ld, R, ld, Z, ld, state))) return rc;
                k = 0;
            }
            if ((rc = pnl_cgb_direction(ctx, n, nv, Z, ld, P, ld, tol, state))) return rc;
            if ((rc = cols.read(it))) return rc;
            k++;
        }
        cols.end(maxiter);
    }
    return PNL_OK;
}

}  // extern "C"
