// The vector side of a block eigensolver (gfx950 only): the three contractions that LOBPCG for the smallest eigenpairs of
// A x = lambda M x needs on blocks of vectors, next to the block products and preconditioners the library already has.  The loop itself
// (solvers.lobpcg) runs in Python: the small Rayleigh-Ritz problem, at most 48 x 48, is solved on the host as gmres keeps its Hessenberg
// problem there.
//
// Reference: PyNucleus has no eigensolver of its own; its drivers call scipy.sparse.linalg.lobpcg on a LinearOperator
// (A. Knyazev, SIAM J. Sci. Comput. 23 (2001): X <- C^T [X; W; P] with C from the Rayleigh-Ritz problem on the basis [X; W; P]).
//
// Blocks are row-major [k][ld], one vector per row as in pnl_gemv_block, with the grid rule of pnl_krylov_block.h: cgb_blocks(n)
// workgroups of 256 threads, element i in workgroup (i / 256) mod blocks.  No floating-point atomics; every sum has a shape that depends
// on n only.
//   k_eigb_gram      G = U V^T on v_mfma_f64_16x16x4_f64.  Up to 3 x 3 tile pairs of 16 rows of U (the A operand) and 16 rows of V (the B
//                    operand), the n direction is MFMA's k.  Wave w of a workgroup takes the elements [64 w, 64 w + 64) of each of the
//                    workgroup's chunks of 256, in four steps of 16: lane (m = l & 15, q = l >> 4) reads the contiguous run
//                    [4 q, 4 q + 4) of the step from row m of every group (two 16-byte loads where the address allows, four 8-byte
//                    loads otherwise: the same bits), and MFMA j of the step contracts element j of the four runs -- A and B agree on
//                    the slot, which is all the instruction needs.  Rows and elements that do not exist are zero operands.  One
//                    accumulator per tile pair runs through all the chunks; the four waves are added in ascending order through LDS
//                    and the workgroup writes its partial tiles to the context's scratch [workgroup][9][256] in the D layout
//                    (lane (m, q), register t: row q + 4 t, column m).  Every tile pair is computed on its own, the (a, b) and the
//                    (b, a) pair with the same products in the same order: U == V gives a bitwise symmetric G.
//   k_eigb_gram_sum  one workgroup per tile pair: thread (t, lane) adds its element over the workgroups in ascending order and stores
//                    it where the row and the column exist.
//   k_eigb_combine   Y = C S: a thread owns element i, holds the kout <= 16 results in registers and walks the kin rows of S in
//                    ascending order -- S is loaded once per call; C (<= 48 x 16) sits in LDS, read as broadcasts.
//   k_eigb_residual  R = AX - theta MX, W = dinv R and the partial sums of R . R and MX . MX in one pass over the columns of the mask;
//   k_eigb_sums      one workgroup: the totals (cgb_totals) -> sums[2 v], sums[2 v + 1]
#include "pnl_krylov_block.h"

namespace {

constexpr int EG_GROUPS = PNL_EIGB_MAXBASIS/CGB_NV;      // groups of 16 rows per side
constexpr int EG_PAIRS = EG_GROUPS*EG_GROUPS;
constexpr int EG_TILE = 256;                             // doubles of a 16 x 16 tile
static_assert(EG_GROUPS == 3 && PNL_EIGB_MAXBASIS == 3*CGB_NV, "three groups of 16 rows");

typedef double eg_d2 __attribute__((ext_vector_type(2)));
typedef double eg_d4 __attribute__((ext_vector_type(4)));

// x[0 .. 4) = row[i0 .. i0 + 4) where the row exists and the element is below n, 0 elsewhere
__device__ __forceinline__ void eg_load4(const double *__restrict__ row, bool have, long long i0, int n, double (&x)[4]) {
    x[0] = x[1] = x[2] = x[3] = 0.;
    if (!have || i0 >= n) return;
    const double *p = row+i0;
    if (i0+4 <= n) {
        if (((uintptr_t)p & 15) == 0) {
            const eg_d2 lo = *(const eg_d2*)p, hi = *(const eg_d2*)(p+2);
            x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
        } else {
            x[0] = p[0]; x[1] = p[1]; x[2] = p[2]; x[3] = p[3];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0+j < n) x[j] = p[j];
    }
}

__global__ void __launch_bounds__(CGB_THREADS)
k_eigb_gram(int n, int ku, const double *__restrict__ U, long long ldu, int kv, const double *__restrict__ V, long long ldv,
            double *__restrict__ part) {
    __shared__ double sw[CGB_THREADS/64-1][EG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = lane & 15, q = lane >> 4;
    const int gu = (ku+CGB_NV-1)/CGB_NV, gv = (kv+CGB_NV-1)/CGB_NV;
    const double *ur[EG_GROUPS], *vr[EG_GROUPS];
    bool uh[EG_GROUPS], vh[EG_GROUPS];
#pragma unroll
    for (int g = 0; g < EG_GROUPS; g++) {
        const int row = CGB_NV*g+m;
        uh[g] = row < ku;
        vh[g] = row < kv;
        ur[g] = U+(uh[g] ? row*ldu : 0);
        vr[g] = V+(vh[g] ? row*ldv : 0);
    }
    eg_d4 acc[EG_GROUPS][EG_GROUPS];
#pragma unroll
    for (int a = 0; a < EG_GROUPS; a++)
#pragma unroll
        for (int b = 0; b < EG_GROUPS; b++) acc[a][b] = eg_d4{0., 0., 0., 0.};
    for (long long c0 = (long long)blockIdx.x*CGB_THREADS; c0 < n; c0 += (long long)gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int sub = 0; sub < 4; sub++) {
            const long long s0 = c0+64*wv+16*sub;
            if (s0 >= n) break;                      // uniform over the wave, and a matter of n alone
            double ua[EG_GROUPS][4], va[EG_GROUPS][4];
#pragma unroll
            for (int g = 0; g < EG_GROUPS; g++) {
                if (g < gu) eg_load4(ur[g], uh[g], s0+4*q, n, ua[g]);
                if (g < gv) eg_load4(vr[g], vh[g], s0+4*q, n, va[g]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int a = 0; a < EG_GROUPS; a++)
#pragma unroll
                    for (int b = 0; b < EG_GROUPS; b++)
                        if (a < gu && b < gv) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[a][j], va[b][j], acc[a][b], 0, 0, 0);
        }
    }
    // lane (m, q) holds D[row q + 4 t][column m] in register t; the waves are added in ascending order
    double *out = part+(size_t)blockIdx.x*EG_PAIRS*EG_TILE;
#pragma unroll
    for (int a = 0; a < EG_GROUPS; a++)
#pragma unroll
        for (int b = 0; b < EG_GROUPS; b++) {
            if (a < gu && b < gv) {                  // uniform over the workgroup
                if (wv > 0) {
#pragma unroll
                    for (int t = 0; t < 4; t++) sw[wv-1][64*t+lane] = acc[a][b][t];
                }
                __syncthreads();
                if (wv == 0) {
#pragma unroll
                    for (int t = 0; t < 4; t++)
                        out[(a*EG_GROUPS+b)*EG_TILE+64*t+lane] = ((acc[a][b][t]+sw[0][64*t+lane])+sw[1][64*t+lane])+sw[2][64*t+lane];
                }
                __syncthreads();
            }
        }
}

// workgroup (a, b) of gu x gv: the tile pair's elements summed over the nb workgroups of k_eigb_gram in ascending order
__global__ void __launch_bounds__(CGB_THREADS)
k_eigb_gram_sum(int nb, int ku, int kv, const double *__restrict__ part, double *__restrict__ G, long long ldg) {
    const int gv = (kv+CGB_NV-1)/CGB_NV, a = blockIdx.x/gv, b = blockIdx.x%gv;
    const int tid = threadIdx.x, t = tid >> 6, lane = tid & 63, m = lane & 15, q = lane >> 4;
    const double *p = part+(size_t)(a*EG_GROUPS+b)*EG_TILE+tid;
    double s = p[0];
    for (int w = 1; w < nb; w++) s += p[(size_t)w*EG_PAIRS*EG_TILE];
    const int row = CGB_NV*a+q+4*t, col = CGB_NV*b+m;
    if (row < ku && col < kv) G[row*ldg+col] = s;
}

__global__ void __launch_bounds__(CGB_THREADS)
k_eigb_combine(int n, int kin, const double *__restrict__ S, long long lds, int kout, const double *__restrict__ C, long long ldc,
               double *__restrict__ Y, long long ldy) {
    __shared__ double sC[PNL_EIGB_MAXBASIS][CGB_NV];
    for (int idx = threadIdx.x; idx < PNL_EIGB_MAXBASIS*CGB_NV; idx += CGB_THREADS) {
        const int b = idx/CGB_NV, a = idx%CGB_NV;
        sC[b][a] = (a < kout && b < kin) ? C[a*ldc+b] : 0.;
    }
    __syncthreads();
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        double t[CGB_NV];
        const double s0 = S[i];
#pragma unroll
        for (int a = 0; a < CGB_NV; a++) t[a] = sC[0][a]*s0;
        for (int b = 1; b < kin; b++) {
            const double s = S[b*lds+i];
#pragma unroll
            for (int a = 0; a < CGB_NV; a++)
                if (a < kout) t[a] = __builtin_fma(sC[b][a], s, t[a]);
        }
#pragma unroll
        for (int a = 0; a < CGB_NV; a++)
            if (a < kout) Y[a*ldy+i] = t[a];
    }
}

__global__ void __launch_bounds__(CGB_THREADS)
k_eigb_residual(int n, unsigned mask, const double *__restrict__ AX, long long ldax, const double *__restrict__ MX, long long ldmx,
                const double *__restrict__ theta, const double *__restrict__ dinv, double *__restrict__ R, long long ldr,
                double *__restrict__ W, long long ldw, double *__restrict__ part_rr, double *__restrict__ part_mm) {
    double th[CGB_NV], s1[CGB_NV], s2[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) {
        th[v] = ((mask >> v) & 1) ? theta[v] : 0.;
        s1[v] = s2[v] = 0.;
    }
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
        const double di = dinv ? dinv[i] : 1.;
#pragma unroll
        for (int v = 0; v < CGB_NV; v++) {
            if ((mask >> v) & 1) {
                const double mx = MX[v*ldmx+i];
                const double ri = __builtin_fma(-th[v], mx, AX[v*ldax+i]);
                R[v*ldr+i] = ri;
                if (W) W[v*ldw+i] = dinv ? di*ri : ri;
                s1[v] = __builtin_fma(ri, ri, s1[v]);
                s2[v] = __builtin_fma(mx, mx, s2[v]);
            }
        }
    }
    cgb_block_sums(s1, mask, part_rr+(size_t)blockIdx.x*CGB_NV);
    __syncthreads();
    cgb_block_sums(s2, mask, part_mm+(size_t)blockIdx.x*CGB_NV);
}

__global__ void __launch_bounds__(CGB_THREADS)
k_eigb_sums(int nb, unsigned mask, const double *__restrict__ part_rr, const double *__restrict__ part_mm, double *__restrict__ sums) {
    __shared__ double tot1[CGB_NV], tot2[CGB_NV];
    cgb_totals(part_rr, nb, tot1);
    cgb_totals(part_mm, nb, tot2);
    const int v = threadIdx.x;
    if (v < CGB_NV && ((mask >> v) & 1)) {
        sums[2*v] = tot1[v];
        sums[2*v+1] = tot2[v];
    }
}

}  // namespace

extern "C" {

int pnl_eigb_gram(pnl_context *ctx, int n, int ku, const double *U_dev, int64_t ldu, int kv, const double *V_dev, int64_t ldv, double *G_dev,
                  int64_t ldg) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, 1, {{U_dev, ldu, KB_READ}, {V_dev, ldv, KB_READ}}) || ku < 1 || ku > PNL_EIGB_MAXBASIS || kv < 1 ||
        kv > PNL_EIGB_MAXBASIS || !G_dev || ldg < kv || (const void*)G_dev == (const void*)U_dev || (const void*)G_dev == (const void*)V_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_eigb_gram: bad arguments (n=%d ku=%d kv=%d ldu=%lld ldv=%lld ldg=%lld)", n, ku, kv,
                    (long long)ldu, (long long)ldv, (long long)ldg);
    if (int rc = ensure(ctx, ctx->b_eigb_part, sizeof(double)*CGB_MAXBLK*EG_PAIRS*EG_TILE)) return rc;
    double *part = (double*)ctx->b_eigb_part.p;
    const int gu = (ku+CGB_NV-1)/CGB_NV, gv = (kv+CGB_NV-1)/CGB_NV;
    KB_LAUNCH(k_eigb_gram, ctx, n, ku, U_dev, ldu, kv, V_dev, ldv, part);
    hipLaunchKernelGGL(k_eigb_gram_sum, dim3(gu*gv), dim3(CGB_THREADS), 0, ctx->stream, cgb_blocks(n), ku, kv, part, G_dev, ldg);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_eigb_combine(pnl_context *ctx, int n, int kin, const double *S_dev, int64_t lds, int kout, const double *C_dev, int64_t ldc,
                     double *Y_dev, int64_t ldy) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, kout, {{S_dev, lds, KB_READ}, {Y_dev, ldy, KB_WRITTEN}}) || kin < 1 || kin > PNL_EIGB_MAXBASIS || !C_dev || ldc < kin ||
        (const void*)C_dev == (const void*)Y_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_eigb_combine: bad arguments (n=%d kin=%d kout=%d lds=%lld ldc=%lld ldy=%lld)", n, kin, kout,
                    (long long)lds, (long long)ldc, (long long)ldy);
    KB_LAUNCH(k_eigb_combine, ctx, n, kin, S_dev, lds, kout, C_dev, ldc, Y_dev, ldy);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_eigb_residual(pnl_context *ctx, int n, int nv, unsigned mask, const double *AX_dev, int64_t ldax, const double *MX_dev, int64_t ldmx,
                      const double *theta_dev, const double *dinv_dev, double *R_dev, int64_t ldr, double *W_dev, int64_t ldw,
                      double *sums_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (kb_bad_args(n, nv, {{AX_dev, ldax, KB_READ}, {MX_dev, ldmx, KB_READ}, {R_dev, ldr, KB_WRITTEN}, {W_dev, ldw, KB_WRITTEN | KB_OPTIONAL}}) ||
        !theta_dev || !sums_dev || mask == 0u || (nv < 32 && (mask >> nv) != 0u))
        return fail(ctx, PNL_ERR_INVALID, "pnl_eigb_residual: bad arguments (n=%d nv=%d mask=0x%x)", n, nv, mask);
    double *part;
    if (int rc = kb_part(ctx, &part)) return rc;
    KB_LAUNCH(k_eigb_residual, ctx, n, mask, AX_dev, ldax, MX_dev, ldmx, theta_dev, dinv_dev, R_dev, ldr, W_dev, ldw, part, part+CGB_PART);
    KB_LAUNCH1(k_eigb_sums, ctx, cgb_blocks(n), mask, part, part+CGB_PART, sums_dev);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // extern "C"
