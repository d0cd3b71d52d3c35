// Right-preconditioned BiCGStab for a block of right-hand sides (gfx950 only): pnl_bicgstab_block for a dense, square, general block
// (nothing assumes symmetry), and the steps of its loop (pnl_bcgb_init / _start / _alpha / _omega / _direction) for operators whose
// product is made elsewhere and for a preconditioner that is applied between the calls.
//
// Reference: bicgstab_solver.solve (base/PyNucleus_base/solvers.pyx:716-787):
//   start:  R = B - A X;  P = R;  R0 = M^-1 R;  P2 = M^-1 P;  kappa = R . R0;  res = sqrt(|kappa|)
//   pass:   T  = A P2
//           alpha = kappa / (T . R0);   S = R - alpha T;   S2 = M^-1 S
//           T2 = A S2
//           omega = (T2 . S) / (T2 . T2);   X += alpha P2 + omega S2;   R = S - omega T2
//           res = sqrt(R . R);   kappaNew = R . R0
//           res < tol: converged in this pass
//           else beta = kappaNew / kappa * alpha / omega;  P = R + beta (P - omega T);  P2 = M^-1 P;  kappa = kappaNew
// Up to 16 right-hand sides ("columns", stored one per row as in pnl_gemv_block) are solved together.  Every column runs its OWN
// recurrence -- its own alpha, omega, beta, convergence and breakdown -- and the columns share the two operator products of a pass.
// A column that has converged or broken down is frozen: none of its blocks and nothing of its state is written again (the products
// still carry it along; their result is not used).
//
// SEVEN work blocks [nvec][ld]: R (S lives in R's storage between the alpha and the omega step), P, R0, P2, S2, T, T2; plus dinv [n]
// and the state.  T and T2 are both needed by the direction step, P2 and S2 both by the X update.
//
// Kernels, with the grid rule and the dot products of pnl_krylov_block.h (cgb_blocks(n) workgroups of 256 threads, a grid-stride loop, a
// thread owns the same elements in every column; no floating-point atomics):
//   k_bcgb_init      R = B - AX, P = R and, unless the preconditioner is external, R0 = P2 = dinv R with the partial sums of R . R0
//   k_kb_dot         partial sums of one dot product per column (R . R0 of an external start; T . R0 of the active columns: behind
//                    k_bcgb_begin and k_bcgb_finish these are the live ones)                                   -> part[0]
//   k_bcgb_begin     one workgroup: kappa, res = sqrt(|kappa|), active = kappa is finite and not 0; the rest of the state 0
//   k_bcgb_s         every workgroup adds the partials of T . R0 to get alpha; S = R - alpha T (in R's storage), S2 = dinv S: T, R and
//                    dinv are read once
//   k_bcgb_dot2      partial sums of T2 . S and T2 . T2 from one pass over T2 and S                            -> part[1], part[2]
//   k_bcgb_xr        every workgroup adds those partials to get omega; X += alpha P2 + omega S2, R = S - omega T2 and the partial sums
//                    of R . R and R . R0 in the same pass                                                      -> part[3], part[4]
//   k_bcgb_finish    one workgroup: res, kappaNew; converged (res < tol), broken down, or beta and kappa = kappaNew
//   k_bcgb_direction P = R + beta (P - omega T) and P2 = dinv P together, for the columns that go on
// A launch never reads a state slot that one of its workgroups writes: k_bcgb_s and k_bcgb_xr decide alike in every workgroup from the
// same totals, workgroup 0 records alpha, omega, the sums and (k_bcgb_s) the breakdown code, and the one-workgroup kernels behind them
// change active and kappa.  A column is LIVE while active != 0 and code == 0; k_bcgb_finish clears active of a column whose code
// k_bcgb_s has set.
//
// Breakdowns (the reference divides and produces NaN): T2 . T2 == 0 (S = 0, the lucky breakdown) gives omega := 0, so X += alpha P2,
// R = S, and the column converges by the normal test.  A column whose next scalar would be 0 / 0, x / 0 or not finite -- T . R0 == 0,
// omega == 0 or kappaNew == 0 when it has not converged, any sum that is not finite -- is frozen BEFORE anything that is not finite is
// written to one of its blocks, with the code PNL_BCGB_* in its state.
#include "pnl_krylov_block.h"

namespace {

// slots of the per-column state (include/pnl_hip.h)
enum { ST_KAPPA = 0, ST_ALPHA = 1, ST_OMEGA = 2, ST_RES = 3, ST_ACTIVE = 4, ST_KAPPA_NEW = 5, ST_CODE = 6, ST_TR0 = 7, ST_T2S = 8, ST_T2T2 = 9,
       ST_RR = 10, ST_BETA = 11 };
static_assert(PNL_BCGB_STATE == 12, "the slots above");
static_assert(ST_RES == KB_ST_RES && ST_ACTIVE == KB_ST_ACTIVE, "the slots that the drivers read");

// bit v: column v < nv is live
__device__ __forceinline__ unsigned bcgb_live_mask(const double *__restrict__ state, int nv) {
    unsigned m = 0;
    for (int v = 0; v < nv; v++)
        m |= (state[v*PNL_BCGB_STATE+ST_ACTIVE] != 0. && state[v*PNL_BCGB_STATE+ST_CODE] == 0.) ? 1u << v : 0u;
    return m;
}

// bit v: column v < nv is active (the launches in front of which a column with a code is no longer active)
__device__ __forceinline__ unsigned bcgb_active_mask(const double *__restrict__ state, int nv) { return kb_active_mask<PNL_BCGB_STATE>(state, nv); }

__device__ __forceinline__ bool bcgb_finite(double x) { return __builtin_isfinite(x); }

// alpha = kappa / (T . R0); the breakdown code, with alpha = 0, where that is no finite number
__device__ __forceinline__ int bcgb_alpha(double kappa, double tr0, double &alpha) {
    alpha = 0.;
    if (!bcgb_finite(tr0)) return PNL_BCGB_NONFINITE;
    if (tr0 == 0.) return PNL_BCGB_TR0;
    const double a = kappa/tr0;
    if (!bcgb_finite(a)) return PNL_BCGB_NONFINITE;
    alpha = a;
    return PNL_BCGB_OK;
}

// omega = (T2 . S) / (T2 . T2); 0 for T2 . T2 == 0 (the lucky breakdown); the code, with omega = 0, where a sum or omega is not finite
__device__ __forceinline__ int bcgb_omega(double t2s, double t2t2, double &omega) {
    omega = 0.;
    if (!bcgb_finite(t2s) || !bcgb_finite(t2t2)) return PNL_BCGB_NONFINITE;
    if (t2t2 == 0.) return PNL_BCGB_OK;
    const double o = t2s/t2t2;
    if (!bcgb_finite(o)) return PNL_BCGB_NONFINITE;
    omega = o;
    return PNL_BCGB_OK;
}

// R = B - AX (AX == nullptr: R = B), P = R for every column v < nv; !EXT: R0 = P2 = dinv R (dinv == nullptr: the unit diagonal) and the
// partial sums of R . R0
template <bool EXT>
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_init(int n, int nv, const double *__restrict__ dinv, const double *__restrict__ B, long long ldb, const double *__restrict__ AX,
            long long ldax, double *__restrict__ R, long long ldr, double *__restrict__ P, long long ldp, double *__restrict__ R0, long long ldr0,
            double *__restrict__ P2, long long ldp2, double *__restrict__ part) {
    const unsigned mask = (1u << nv)-1u;
    double s[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = (!EXT && dinv) ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double ri = AX ? B[v*ldb+i]-AX[v*ldax+i] : B[v*ldb+i];
                R[v*ldr+i] = ri;
                P[v*ldp+i] = ri;
                if (!EXT) {
                    const double oi = dinv ? di*ri : ri;
                    R0[v*ldr0+i] = oi;
                    P2[v*ldp2+i] = oi;
                    s[v] = __builtin_fma(ri, oi, s[v]);
                }
            }
        }
    }
    if (!EXT) cgb_block_sums(s, mask, part+(size_t)blockIdx.x*CGB_NV);
}

// one workgroup: the start state of every column v < nv from the partial sums of R . R0
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_begin(int nb, int nv, const double *__restrict__ part, double *state) {
    __shared__ double tot[CGB_NV];
    cgb_totals(part, nb, tot);
    const int v = threadIdx.x;
    if (v >= nv) return;
    double *st = state+v*PNL_BCGB_STATE;
    const double kappa = tot[v];
    for (int k = 0; k < PNL_BCGB_STATE; k++) st[k] = 0.;
    st[ST_KAPPA] = kappa;
    st[ST_RES] = sqrt(fabs(kappa));
    if (!bcgb_finite(kappa)) st[ST_CODE] = PNL_BCGB_NONFINITE;
    else if (kappa != 0.) st[ST_ACTIVE] = 1.;
}

// alpha from the partial sums of T . R0; S = R - alpha T in R's storage; !EXT: S2 = dinv S.  The active columns (none of them has a
// code in front of this launch); a column that breaks down here is not written, workgroup 0 records its code
template <bool EXT>
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_s(int n, int nv, const double *__restrict__ dinv, const double *__restrict__ T, long long ldt, double *__restrict__ RS, long long ldr,
         double *__restrict__ S2, long long lds2, double *state, const double *__restrict__ part_tr0) {
    __shared__ double tot[CGB_NV], al[CGB_NV];
    __shared__ unsigned okm;
    unsigned mask = bcgb_active_mask(state, nv);
    if (threadIdx.x == 0) okm = 0u;
    cgb_totals(part_tr0, (int)gridDim.x, tot);
    if (threadIdx.x < CGB_NV) {
        const int v = threadIdx.x;
        double alpha = 0.;
        if ((mask >> v) & 1) {
            const int code = bcgb_alpha(state[v*PNL_BCGB_STATE+ST_KAPPA], tot[v], alpha);
            if (code == PNL_BCGB_OK) atomicOr(&okm, 1u << v);
            if (blockIdx.x == 0) {                  // slots that no workgroup of this launch reads
                state[v*PNL_BCGB_STATE+ST_ALPHA] = alpha;
                state[v*PNL_BCGB_STATE+ST_TR0] = tot[v];
                if (code != PNL_BCGB_OK) state[v*PNL_BCGB_STATE+ST_CODE] = (double)code;
            }
        }
        al[v] = alpha;
    }
    __syncthreads();
    mask &= okm;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = (!EXT && dinv) ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double si = __builtin_fma(-al[v], T[v*ldt+i], RS[v*ldr+i]);
                RS[v*ldr+i] = si;
                if (!EXT) S2[v*lds2+i] = dinv ? di*si : si;
            }
        }
    }
}

// partial sums of T2 . S and T2 . T2 for the live columns, one pass over T2 and S
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_dot2(int n, int nv, const double *__restrict__ T2, long long ldt2, const double *__restrict__ S, long long lds,
            const double *__restrict__ state, double *__restrict__ part_t2s, double *__restrict__ part_t2t2) {
    const unsigned mask = bcgb_live_mask(state, nv);
    double s1[CGB_NV], s2[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s1[v] = s2[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double t = T2[v*ldt2+i];
                s1[v] = __builtin_fma(t, S[v*lds+i], s1[v]);
                s2[v] = __builtin_fma(t, t, s2[v]);
            }
        }
    }
    cgb_block_sums(s1, mask, part_t2s+(size_t)blockIdx.x*CGB_NV);
    __syncthreads();
    cgb_block_sums(s2, mask, part_t2t2+(size_t)blockIdx.x*CGB_NV);
}

// omega from the partial sums of T2 . S and T2 . T2; X += alpha P2 + omega S2; R = S - omega T2 (in place); partial sums of R . R and
// R . R0.  The live columns; a column whose omega is not finite is not written (k_bcgb_finish, which decides alike, records the code)
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_xr(int n, int nv, const double *__restrict__ P2, long long ldp2, const double *__restrict__ S2, long long lds2,
          const double *__restrict__ T2, long long ldt2, double *__restrict__ X, long long ldx, double *__restrict__ RS, long long ldr,
          const double *__restrict__ R0, long long ldr0, double *state, const double *__restrict__ part_t2s,
          const double *__restrict__ part_t2t2, double *__restrict__ part_rr, double *__restrict__ part_rr0) {
    __shared__ double tot1[CGB_NV], tot2[CGB_NV], al[CGB_NV], om[CGB_NV];
    __shared__ unsigned okm;
    unsigned mask = bcgb_live_mask(state, nv);
    if (threadIdx.x == 0) okm = 0u;
    cgb_totals(part_t2s, (int)gridDim.x, tot1);
    cgb_totals(part_t2t2, (int)gridDim.x, tot2);
    if (threadIdx.x < CGB_NV) {
        const int v = threadIdx.x;
        double omega = 0., alpha = 0.;
        if ((mask >> v) & 1) {
            alpha = state[v*PNL_BCGB_STATE+ST_ALPHA];
            if (bcgb_omega(tot1[v], tot2[v], omega) == PNL_BCGB_OK) atomicOr(&okm, 1u << v);
            if (blockIdx.x == 0) {                  // slots that no workgroup of this launch reads
                state[v*PNL_BCGB_STATE+ST_OMEGA] = omega;
                state[v*PNL_BCGB_STATE+ST_T2S] = tot1[v];
                state[v*PNL_BCGB_STATE+ST_T2T2] = tot2[v];
            }
        }
        al[v] = alpha;
        om[v] = omega;
    }
    __syncthreads();
    mask &= okm;
    double s1[CGB_NV], s2[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s1[v] = s2[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double omega = om[v];
                X[v*ldx+i] = __builtin_fma(omega, S2[v*lds2+i], __builtin_fma(al[v], P2[v*ldp2+i], X[v*ldx+i]));
                const double ri = __builtin_fma(-omega, T2[v*ldt2+i], RS[v*ldr+i]);
                RS[v*ldr+i] = ri;
                s1[v] = __builtin_fma(ri, ri, s1[v]);
                s2[v] = __builtin_fma(ri, R0[v*ldr0+i], s2[v]);
            }
        }
    }
    cgb_block_sums(s1, mask, part_rr+(size_t)blockIdx.x*CGB_NV);
    __syncthreads();
    cgb_block_sums(s2, mask, part_rr0+(size_t)blockIdx.x*CGB_NV);
}

// one workgroup, the active columns: a code set by k_bcgb_s or an omega that is not finite freezes the column with the residual it had;
// else res = sqrt(R . R), kappaNew = R . R0; res < tol: converged; else a breakdown, or beta and kappa = kappaNew
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_finish(int nb, int nv, const double *__restrict__ part_rr, const double *__restrict__ part_rr0, double tol, double *state) {
    __shared__ double tot1[CGB_NV], tot2[CGB_NV];
    cgb_totals(part_rr, nb, tot1);
    cgb_totals(part_rr0, nb, tot2);
    const int v = threadIdx.x;
    if (v >= nv) return;
    double *st = state+v*PNL_BCGB_STATE;
    if (st[ST_ACTIVE] == 0.) return;
    if (st[ST_CODE] != 0.) { st[ST_ACTIVE] = 0.; return; }
    double omega;
    int code = bcgb_omega(st[ST_T2S], st[ST_T2T2], omega);
    if (code == PNL_BCGB_OK) {
        const double rr = tot1[v], kn = tot2[v];
        st[ST_RR] = rr;
        st[ST_KAPPA_NEW] = kn;
        if (!bcgb_finite(rr)) code = PNL_BCGB_NONFINITE;
        else {
            const double res = sqrt(rr);
            st[ST_RES] = res;
            if (res < tol) { st[ST_ACTIVE] = 0.; return; }
            if (!bcgb_finite(kn)) code = PNL_BCGB_NONFINITE;
            else if (omega == 0.) code = PNL_BCGB_OMEGA;
            else if (kn == 0.) code = PNL_BCGB_KAPPA;
            else {
                const double beta = kn/st[ST_KAPPA]*st[ST_ALPHA]/omega;
                if (!bcgb_finite(beta)) code = PNL_BCGB_NONFINITE;
                else { st[ST_BETA] = beta; st[ST_KAPPA] = kn; }
            }
        }
    }
    if (code != PNL_BCGB_OK) { st[ST_CODE] = (double)code; st[ST_ACTIVE] = 0.; }
}

// P = R + beta (P - omega T); !EXT: P2 = dinv P.  The active columns (behind k_bcgb_finish these are the ones that go on)
template <bool EXT>
__global__ void __launch_bounds__(CGB_THREADS)
k_bcgb_direction(int n, int nv, const double *__restrict__ dinv, const double *__restrict__ R, long long ldr, const double *__restrict__ T,
                 long long ldt, double *__restrict__ P, long long ldp, double *__restrict__ P2, long long ldp2, const double *__restrict__ state) {
    __shared__ double be[CGB_NV], om[CGB_NV];
    const unsigned mask = bcgb_active_mask(state, nv);
    if (threadIdx.x < CGB_NV) {
        const bool on = (mask >> threadIdx.x) & 1;
        be[threadIdx.x] = on ? state[threadIdx.x*PNL_BCGB_STATE+ST_BETA] : 0.;
        om[threadIdx.x] = on ? state[threadIdx.x*PNL_BCGB_STATE+ST_OMEGA] : 0.;
    }
    __syncthreads();
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = (!EXT && dinv) ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double pi = __builtin_fma(be[v], __builtin_fma(-om[v], T[v*ldt+i], P[v*ldp+i]), R[v*ldr+i]);
                P[v*ldp+i] = pi;
                if (!EXT) P2[v*ldp2+i] = dinv ? di*pi : pi;
            }
        }
    }
}

// the partial sums (kb_part): part[0] T . R0 (R . R0 at the start), [1] T2 . S, [2] T2 . T2, [3] R . R, [4] R . R0
int bcgb_begin(pnl_context *ctx, int n, int nv, const double *part, double *state) {
    KB_LAUNCH1(k_bcgb_begin, ctx, cgb_blocks(n), nv, part, state);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// a block that a step writes unless the preconditioner is external; then the step does not look at it
KbBlock bcgb_own(int external, const void *p, int64_t ld) { return external ? KbBlock{nullptr, 0, KB_OPTIONAL} : KbBlock{p, ld, KB_WRITTEN}; }

}  // namespace

extern "C" {

int pnl_bcgb_init(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev,
                  int64_t ldax, double *R_dev, int64_t ldr, double *P_dev, int64_t ldp, double *R0_dev, int64_t ldr0, double *P2_dev, int64_t ldp2,
                  double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{B_dev, ldb, KB_READ}, {AX_dev, ldax, KB_READ | KB_OPTIONAL}, {R_dev, ldr, KB_WRITTEN}, {P_dev, ldp, KB_WRITTEN},
                              bcgb_own(external, R0_dev, ldr0), bcgb_own(external, P2_dev, ldp2)}, true) || (!external && !state_dev))
        return fail(ctx, PNL_ERR_INVALID, "pnl_bcgb_init: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH(external ? k_bcgb_init<true> : k_bcgb_init<false>, ctx, n, nvec, dinv_dev, B_dev, ldb, AX_dev, ldax, R_dev, ldr, P_dev, ldp, R0_dev,
              ldr0, P2_dev, ldp2, part);
    HIPCHK(ctx, hipGetLastError());
    return external ? PNL_OK : bcgb_begin(ctx, n, nvec, part, state_dev);
}

int pnl_bcgb_start(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *R0_dev, int64_t ldr0, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{R_dev, ldr, KB_READ}, {R0_dev, ldr0, KB_READ}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_bcgb_start: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH((k_kb_dot<PNL_BCGB_STATE, true>), ctx, n, nvec, R_dev, ldr, R0_dev, ldr0, state_dev, part);
    HIPCHK(ctx, hipGetLastError());
    return bcgb_begin(ctx, n, nvec, part, state_dev);
}

int pnl_bcgb_alpha(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *T_dev, int64_t ldt, const double *R0_dev,
                   int64_t ldr0, double *RS_dev, int64_t ldr, double *S2_dev, int64_t lds2, double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{T_dev, ldt, KB_READ}, {R0_dev, ldr0, KB_READ}, {RS_dev, ldr, KB_WRITTEN}, bcgb_own(external, S2_dev, lds2)}, true) ||
        !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_bcgb_alpha: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH((k_kb_dot<PNL_BCGB_STATE, false>), ctx, n, nvec, T_dev, ldt, R0_dev, ldr0, state_dev, part);
    KB_LAUNCH(external ? k_bcgb_s<true> : k_bcgb_s<false>, ctx, n, nvec, dinv_dev, T_dev, ldt, RS_dev, ldr, S2_dev, lds2, state_dev, part);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_bcgb_omega(pnl_context *ctx, int n, int nvec, const double *P2_dev, int64_t ldp2, const double *S2_dev, int64_t lds2, const double *T2_dev,
                   int64_t ldt2, const double *R0_dev, int64_t ldr0, double *X_dev, int64_t ldx, double *RS_dev, int64_t ldr, double tol,
                   double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    // what is written must stand alone; the blocks that are only read may coincide
    if (kb_bad_args(n, nvec, {{P2_dev, ldp2, KB_READ}, {S2_dev, lds2, KB_READ}, {T2_dev, ldt2, KB_READ}, {R0_dev, ldr0, KB_READ},
                              {X_dev, ldx, KB_WRITTEN}, {RS_dev, ldr, KB_WRITTEN}}) || !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_bcgb_omega: bad arguments (n=%d nvec=%d)", n, nvec);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    double *t2s = part+CGB_PART, *t2t2 = part+2*CGB_PART, *rr = part+3*CGB_PART, *rr0 = part+4*CGB_PART;
    KB_LAUNCH(k_bcgb_dot2, ctx, n, nvec, T2_dev, ldt2, RS_dev, ldr, state_dev, t2s, t2t2);
    KB_LAUNCH(k_bcgb_xr, ctx, n, nvec, P2_dev, ldp2, S2_dev, lds2, T2_dev, ldt2, X_dev, ldx, RS_dev, ldr, R0_dev, ldr0, state_dev, t2s, t2t2, rr, rr0);
    KB_LAUNCH1(k_bcgb_finish, ctx, cgb_blocks(n), nvec, rr, rr0, tol, state_dev);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_bcgb_direction(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *R_dev, int64_t ldr, const double *T_dev,
                       int64_t ldt, double *P_dev, int64_t ldp, double *P2_dev, int64_t ldp2, const double *state_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nvec, {{R_dev, ldr, KB_READ}, {T_dev, ldt, KB_READ}, {P_dev, ldp, KB_WRITTEN}, bcgb_own(external, P2_dev, ldp2)}, true) ||
        !state_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_bcgb_direction: bad arguments (n=%d nvec=%d)", n, nvec);
    KB_LAUNCH(external ? k_bcgb_direction<true> : k_bcgb_direction<false>, ctx, n, nvec, dinv_dev, R_dev, ldr, T_dev, ldt, P_dev, ldp, P2_dev,
              ldp2, state_dev);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_bicgstab_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, int nrhs, int jacobi, const double *B_dev, int64_t ldb,
                       double *X_dev, int64_t ldx, double tol, int maxiter, int *iters, double *residuals) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!A_dev || !B_dev || !X_dev || n < 1 || nrhs < 1 || ldA < n || ldb < n || ldx < n || maxiter < 0 || B_dev == X_dev ||
        (const void*)A_dev == (const void*)X_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_bicgstab_block: bad arguments (n=%d nrhs=%d ldA=%lld ldb=%lld ldx=%lld maxiter=%d)", n, nrhs,
                    (long long)ldA, (long long)ldb, (long long)ldx, maxiter);
    // work: dinv [n]; R, P, R0, P2, S2, T, T2 [16][ld]; the state
    const int64_t ld = kb_ld(n);
    const int gmax = std::min(nrhs, CGB_NV);
    int rc;
    if ((rc = ensure(ctx, ctx->b_bcgb_work, kb_work_bytes(ld, 7, gmax, ld, PNL_BCGB_STATE)))) return rc;
    double *dwork = (double*)ctx->b_bcgb_work.p;
    KbCarve work{dwork+ld, gmax*ld};
    double *R = work.next(), *P = work.next(), *R0 = work.next(), *P2 = work.next(), *S2 = work.next(), *T = work.next(), *T2 = work.next(),
           *state = work.p;
    if (jacobi && (rc = pnl_inv_diagonal(ctx, A_dev, ldA, n, dwork))) return rc;
    const double *dinv = jacobi ? dwork : nullptr;
    for (int v0 = 0; v0 < nrhs; v0 += CGB_NV) {
        const int nv = std::min(CGB_NV, nrhs-v0);
        const double *B = B_dev+(int64_t)v0*ldb;
        double *X = X_dev+(int64_t)v0*ldx;
        KbColumns<PNL_BCGB_STATE> cols{ctx, state, nv, iters ? iters+v0 : nullptr, residuals ? residuals+v0 : nullptr};
        auto product = [&](const double *V, int64_t ldv, double *W) {
            return pnl_gemv_block(ctx, A_dev, ldA, n, n, nv, V, ldv, 1., 0., nullptr, 0, W, ld);
        };
        if ((rc = product(X, ldx, T))) return rc;
        if ((rc = pnl_bcgb_init(ctx, n, nv, 0, dinv, B, ldb, T, ld, R, ld, P, ld, R0, ld, P2, ld, state))) return rc;
        if ((rc = cols.read(-1))) return rc;
        for (int it = 0; it < maxiter && cols.nactive > 0; it++) {
            if ((rc = product(P2, ld, T))) return rc;
            if ((rc = pnl_bcgb_alpha(ctx, n, nv, 0, dinv, T, ld, R0, ld, R, ld, S2, ld, state))) return rc;
            if ((rc = product(S2, ld, T2))) return rc;
            if ((rc = pnl_bcgb_omega(ctx, n, nv, P2, ld, S2, ld, T2, ld, R0, ld, X, ldx, R, ld, tol, state))) return rc;
            if ((rc = pnl_bcgb_direction(ctx, n, nv, 0, dinv, R, ld, T, ld, P, ld, P2, ld, state))) return rc;
            if ((rc = cols.read(it))) return rc;
        }
        cols.end(maxiter);
    }
    return PNL_OK;
}

}  // extern "C"
