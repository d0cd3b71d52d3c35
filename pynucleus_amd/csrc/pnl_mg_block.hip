// Multigrid for a block of right-hand sides (gfx950 only): the V cycle of pnl_solver.hip (solve_on_level) and the multigrid-
// preconditioned CG (pnl_mg_cg) for up to 16 columns per pass over the operators.
//
// Reference: multigrid.solveOnLevel (multilevelSolver/PyNucleus_multilevelSolver/multigrid_{SCALAR}.pxi:237-292), separableSmoother.eval
// with the Jacobi preconditioner (smoothers_{SCALAR}.pxi:88-108, 118-131), cg_solver.solve (base/PyNucleus_base/solvers.pyx:363-444)
// with multigridPreconditioner (multigrid_{SCALAR}.pxi:470-497), as pnl_solver.hip restates them for one vector.
//
// Columns are stored one per row as in pnl_gemv_block.  Everything in a cycle is HBM-bound on the finest operator: a cycle from a zero
// guess reads it twice (the residual behind the pre-smoothing sweep, the residual of the post-smoothing sweep; the first sweep's
// residual is the right-hand side), and a group of at most MGB_NV = 16 columns shares each of those passes.  Launches of one cycle on
// level l > 0, per group (pre = post = 1):
//   x_is_zero:  k_mgb_jacobi<SET>   X = invD B                         else: pnl_gemv_block  T = B - A X;  k_mgb_jacobi  X += invD T
//   pnl_gemv_block   T = B - A_l X                 (1 launch up to 2048 columns, else 2: the partial sums are added in a second one)
//   k_mgb_transfer   rhs_{l-1} = R T
//   the cycle on level l - 1 from a zero guess into sol_{l-1};  level 0: pnl_gemv_block  X = A_0^{-1} B
//   k_mgb_transfer   X += P sol_{l-1}
//   pnl_gemv_block   T = B - A_l X;   k_mgb_jacobi  X += invD T
// No host synchronisation inside a cycle and no floating-point atomics: k_mgb_jacobi and k_mgb_transfer give one thread one row and
// loop over the columns, so the bits of column v depend neither on the number of columns nor on v nor on the other columns, as those
// of pnl_gemv_block.  Levels of kind 0 and 2 are both read in full (no half-read of a symmetric level); a hierarchy whose finest
// level is an H2 operator (kind 1) is refused.
//
// pnl_mg_cg_block is the loop of pnl_mg_cg around pnl_gemv_block (A P), pnl_mg_cycle_block (Z = cycle(R) from a zero guess) and the
// external-preconditioner steps of pnl_cg_block.hip; the host reads the state of the group back once per iteration.
#include "pnl_krylov_block.h"
#include "pnl_mg.h"

namespace {

constexpr int MGB_NV = CGB_NV;              // columns per group = vectors per pass of pnl_gemv_block
constexpr int MGB_THREADS = 256;

inline unsigned mgb_blocks(int n) { return (unsigned)((n+MGB_THREADS-1)/MGB_THREADS); }

// damped Jacobi on a block: X[v][i] += invD[i] R[v][i]  (SET: X[v][i] = invD[i] R[v][i], the sweep from a zero guess; X is not read).
// One thread per i: invD[i] is loaded once for the nv columns, the loads and stores of every column are coalesced along i.
template <bool SET>
__global__ void __launch_bounds__(MGB_THREADS)
k_mgb_jacobi(int n, int nv, const double *__restrict__ invD, const double *__restrict__ R, long long ldr, double *__restrict__ X, long long ldx) {
    const int i = blockIdx.x*MGB_THREADS+threadIdx.x;
    if (i >= n) return;
    const double d = invD[i];
    double r[MGB_NV];
#pragma unroll
    for (int v = 0; v < MGB_NV; v++)
        if (v < nv) r[v] = R[v*ldr+i];                  // nv is uniform: all loads of the group in flight before the first use
#pragma unroll
    for (int v = 0; v < MGB_NV; v++)
        if (v < nv) X[v*ldx+i] = SET ? d*r[v] : __builtin_fma(d, r[v], X[v*ldx+i]);
}

// transfer operators on a block: Y[v][row] = alpha * sum_k data[k] X[v][indices[k]] + beta * Y[v][row] for a CSR matrix with a few
// entries per row (restriction, prolongation).  One thread per row: every (index, value) pair is loaded once for the nv columns, the
// sum runs in ascending k as in k_csr_axpby (pnl_solver.hip), loads of Y and stores are coalesced along row.
__global__ void __launch_bounds__(MGB_THREADS)
k_mgb_transfer(int nrows, int nv, const int *__restrict__ indptr, const int *__restrict__ indices, const double *__restrict__ data,
               const double *__restrict__ X, long long ldx, double alpha, double beta, double *Y, long long ldy) {
    const int row = blockIdx.x*MGB_THREADS+threadIdx.x;
    if (row >= nrows) return;
    double s[MGB_NV];
#pragma unroll
    for (int v = 0; v < MGB_NV; v++) s[v] = 0.;
    const int e = indptr[row+1];
    for (int k = indptr[row]; k < e; k++) {
        const int j = indices[k];
        const double a = data[k];
#pragma unroll
        for (int v = 0; v < MGB_NV; v++)
            if (v < nv) s[v] = __builtin_fma(a, X[v*ldx+j], s[v]);
    }
#pragma unroll
    for (int v = 0; v < MGB_NV; v++)
        if (v < nv) Y[v*ldy+row] = beta != 0. ? __builtin_fma(alpha, s[v], beta*Y[v*ldy+row]) : alpha*s[v];
}

// X[v][i] = S[v][i] (S == nullptr: 0) for i < n: the padding i >= n of a block with ld > n is not written
__global__ void __launch_bounds__(MGB_THREADS)
k_mgb_copy(int n, int nv, const double *__restrict__ S, long long lds, double *__restrict__ X, long long ldx) {
    const int i = blockIdx.x*MGB_THREADS+threadIdx.x;
    if (i >= n) return;
    for (int v = 0; v < nv; v++) X[v*ldx+i] = S ? S[v*lds+i] : 0.;
}

int jacobi(pnl_context *ctx, bool set, int n, int nv, const double *invD, const double *R, int64_t ldr, double *X, int64_t ldx) {
    if (set) hipLaunchKernelGGL((k_mgb_jacobi<true>), dim3(mgb_blocks(n)), dim3(MGB_THREADS), 0, ctx->stream, n, nv, invD, R, (long long)ldr, X, (long long)ldx);
    else hipLaunchKernelGGL((k_mgb_jacobi<false>), dim3(mgb_blocks(n)), dim3(MGB_THREADS), 0, ctx->stream, n, nv, invD, R, (long long)ldr, X, (long long)ldx);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int transfer(pnl_context *ctx, int nrows, int nv, const int *indptr, const int *indices, const double *data, const double *X, int64_t ldx,
             double alpha, double beta, double *Y, int64_t ldy) {
    hipLaunchKernelGGL(k_mgb_transfer, dim3(mgb_blocks(nrows)), dim3(MGB_THREADS), 0, ctx->stream, nrows, nv, indptr, indices, data, X, (long long)ldx,
                       alpha, beta, Y, (long long)ldy);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int copy(pnl_context *ctx, int n, int nv, const double *S, int64_t lds, double *X, int64_t ldx) {
    hipLaunchKernelGGL(k_mgb_copy, dim3(mgb_blocks(n)), dim3(MGB_THREADS), 0, ctx->stream, n, nv, S, (long long)lds, X, (long long)ldx);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// the level blocks, on the first block call
int ensure_blocks(pnl_mg *mg) {
    pnl_context *ctx = mg->ctx;
    const int nl = mg->nlevels;
    if ((int)mg->btemp.size() != nl) { mg->brhs.resize(nl); mg->bsol.resize(nl); mg->btemp.resize(nl); }
    for (int l = 0; l < nl; l++) {
        const size_t bytes = sizeof(double)*(size_t)MGB_NV*(size_t)kb_ld(mg->lv[l].n);
        int rc;
        if (l < nl-1 && ((rc = ensure(ctx, mg->brhs[l], bytes)) || (rc = ensure(ctx, mg->bsol[l], bytes)))) return rc;
        if (l > 0 && (rc = ensure(ctx, mg->btemp[l], bytes))) return rc;
    }
    return PNL_OK;
}

// T = B - A_l X, the operator read in full
int residual(pnl_mg *mg, int l, int nv, const double *B, int64_t ldb, const double *X, int64_t ldx, double *T, int64_t ldt) {
    const pnl_mg_level_desc &L = mg->lv[l];
    return pnl_gemv_block(mg->ctx, L.A_dev, L.ldA, L.n, L.n, nv, X, ldx, -1., 1., B, ldb, T, ldt);
}

// steps sweeps of X += (omega / D) (B - A X); simple: X counts as zero and is not read, the first residual is B
int smooth_block(pnl_mg *mg, int l, int nv, const double *B, int64_t ldb, double *X, int64_t ldx, int steps, bool simple) {
    pnl_context *ctx = mg->ctx;
    const int n = mg->lv[l].n;
    const int64_t ldt = kb_ld(n);
    double *T = (double*)mg->btemp[l].p;
    const double *invD = (const double*)mg->invD[l].p;
    int rc;
    for (int k = 0; k < steps; k++) {
        if (simple) {
            if ((rc = jacobi(ctx, true, n, nv, invD, B, ldb, X, ldx))) return rc;
            simple = false;
            continue;
        }
        if ((rc = residual(mg, l, nv, B, ldb, X, ldx, T, ldt))) return rc;
        if ((rc = jacobi(ctx, false, n, nv, invD, T, ldt, X, ldx))) return rc;
    }
    return PNL_OK;
}

// solve_on_level (pnl_solver.hip) for nv <= 16 columns; simple: X counts as zero whatever it holds
int solve_on_level_block(pnl_mg *mg, int l, int nv, const double *B, int64_t ldb, double *X, int64_t ldx, bool simple) {
    pnl_context *ctx = mg->ctx;
    const pnl_mg_level_desc &L = mg->lv[l];
    if (l == 0) return pnl_gemv_block(ctx, mg->coarse_inv, L.n, L.n, L.n, nv, B, ldb, 1., 0., nullptr, 0, X, ldx);     // X = A_0^{-1} B
    const pnl_mg_level_desc &C = mg->lv[l-1];
    const int64_t ldt = kb_ld(L.n), ldc = kb_ld(C.n);
    double *T = (double*)mg->btemp[l].p, *defect = (double*)mg->brhs[l-1].p, *solcg = (double*)mg->bsol[l-1].p;
    int rc;
    if ((rc = smooth_block(mg, l, nv, B, ldb, X, ldx, mg->pre, simple))) return rc;
    // residual, restricted to the coarser level
    if (simple && mg->pre == 0) {
        if ((rc = copy(ctx, L.n, nv, nullptr, 0, X, ldx))) return rc;                   // no sweep has written X: it is zero, the residual is B
        if ((rc = transfer(ctx, C.n, nv, L.R_indptr_dev, L.R_indices_dev, L.R_data_dev, B, ldb, 1., 0., defect, ldc))) return rc;
    } else {
        if ((rc = residual(mg, l, nv, B, ldb, X, ldx, T, ldt))) return rc;
        if ((rc = transfer(ctx, C.n, nv, L.R_indptr_dev, L.R_indices_dev, L.R_data_dev, T, ldt, 1., 0., defect, ldc))) return rc;
    }
    if ((rc = solve_on_level_block(mg, l-1, nv, defect, ldc, solcg, ldc, true))) return rc;
    // correction: X += P solcg
    if ((rc = transfer(ctx, L.n, nv, L.P_indptr_dev, L.P_indices_dev, L.P_data_dev, solcg, ldc, 1., 1., X, ldx))) return rc;
    return smooth_block(mg, l, nv, B, ldb, X, ldx, mg->post, false);
}

// the checks that pnl_mg_cycle_block and pnl_mg_cg_block share; 0 or the error
int check_block_call(pnl_mg *mg, const char *who, int nvec, const double *B, int64_t ldb, const double *X, int64_t ldx) {
    if (!mg) return PNL_ERR_INVALID;
    pnl_context *ctx = mg->ctx;
    const pnl_mg_level_desc &L = mg->lv[mg->nlevels-1];
    if (!B || !X || nvec < 1 || ldb < L.n || ldx < L.n || B == X)
        return fail(ctx, PNL_ERR_INVALID, "%s: bad arguments (n=%d nvec=%d ldb=%lld ldx=%lld)", who, L.n, nvec, (long long)ldb, (long long)ldx);
    if (L.kind == 1)
        return fail(ctx, PNL_ERR_INVALID, "%s: the finest level is an H2 operator (kind 1); the block cycle takes dense levels only", who);
    return PNL_OK;
}

}  // namespace

extern "C" {

int pnl_mg_cycle_block(pnl_mg *mg, int nvec, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx, int x_is_zero) {
    int rc;
    if ((rc = check_block_call(mg, "pnl_mg_cycle_block", nvec, B_dev, ldb, X_dev, ldx))) return rc;
    if ((rc = ensure_blocks(mg))) return rc;
    for (int v0 = 0; v0 < nvec; v0 += MGB_NV) {
        const int nv = std::min(MGB_NV, nvec-v0);
        if ((rc = solve_on_level_block(mg, mg->nlevels-1, nv, B_dev+(int64_t)v0*ldb, ldb, X_dev+(int64_t)v0*ldx, ldx, x_is_zero != 0))) return rc;
    }
    return PNL_OK;
}

int pnl_mg_cg_block(pnl_mg *mg, const double *A_dev, int64_t ldA, int nrhs, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx,
                    double tol, int maxiter, int x_is_zero, int *iters, double *residuals) {
    int rc;
    if ((rc = check_block_call(mg, "pnl_mg_cg_block", nrhs, B_dev, ldb, X_dev, ldx))) return rc;
    pnl_context *ctx = mg->ctx;
    const int top = mg->nlevels-1;
    const pnl_mg_level_desc &L = mg->lv[top];
    const int n = L.n;
    if (!A_dev) { A_dev = L.A_dev; ldA = L.ldA; }
    if (!A_dev || ldA < n || maxiter < 0)
        return fail(ctx, PNL_ERR_INVALID, "pnl_mg_cg_block: no operator, ldA < n or maxiter < 0 (n=%d ldA=%lld maxiter=%d)", n, (long long)ldA, maxiter);
    if ((rc = ensure_blocks(mg))) return rc;
    // work: R, P, AP, Z [16][ld]; the state
    const int64_t ld = kb_ld(n);
    if ((rc = ensure(ctx, mg->bcg, kb_work_bytes(0, 4, MGB_NV, ld, PNL_CGB_STATE)))) return rc;
    KbCarve work{(double*)mg->bcg.p, std::min(nrhs, MGB_NV)*ld};
    double *R = work.next(), *P = work.next(), *AP = work.next(), *Z = work.next(), *state = work.p;
    for (int v0 = 0; v0 < nrhs; v0 += MGB_NV) {
        const int nv = std::min(MGB_NV, nrhs-v0);
        const double *B = B_dev+(int64_t)v0*ldb;
        double *X = X_dev+(int64_t)v0*ldx;
        KbColumns<PNL_CGB_STATE> cols{ctx, state, nv, iters ? iters+v0 : nullptr, residuals ? residuals+v0 : nullptr};
        auto product = [&](const double *V, int64_t ldv) { return pnl_gemv_block(ctx, A_dev, ldA, n, n, nv, V, ldv, 1., 0., nullptr, 0, AP, ld); };
        // one V cycle from a zero guess for the whole group: its cost does not depend on the frozen columns, whose Z is not used
        auto precond = [&]() { return solve_on_level_block(mg, top, nv, R, ld, Z, ld, true); };
        if (!x_is_zero && (rc = product(X, ldx))) return rc;                        // else the caller's X holds zeros, as for pnl_mg_cg
        if ((rc = pnl_cgb_residual(ctx, n, nv, B, ldb, x_is_zero ? nullptr : AP, ld, R, ld, nullptr))) return rc;
        if ((rc = precond())) return rc;
        if ((rc = pnl_cgb_start(ctx, n, nv, R, ld, Z, ld, P, ld, tol, state))) return rc;
        if ((rc = cols.read(-1))) return rc;
        int k = 0;
        for (int it = 0; it < maxiter && cols.nactive > 0; it++) {
            if ((rc = product(P, ld))) return rc;
            if ((rc = pnl_cgb_step(ctx, n, nv, P, ld, AP, ld, X, ldx, R, ld, state))) return rc;
            if (k == 50) {
                // recalculate the residual to avoid rounding errors (solvers.pyx:412-415), for every active column of the group at once
                if ((rc = product(X, ldx))) return rc;
                if ((rc = pnl_cgb_residual(ctx, n, nv, B, ldb, AP, ld, R, ld, state))) return rc;
                k = 0;
            }
            if ((rc = precond())) return rc;
            if ((rc = pnl_cgb_beta(ctx, n, nv, R, ld, Z, ld, state))) return rc;
            if ((rc = pnl_cgb_direction(ctx, n, nv, Z, ld, P, ld, tol, state))) return rc;
            if ((rc = cols.read(it))) return rc;
            k++;
        }
        cols.end(maxiter);
    }
    return PNL_OK;
}

}  // extern "C"
