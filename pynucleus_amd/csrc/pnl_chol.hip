// Direct solver for the dense symmetric positive definite operators: blocked Cholesky factorisation A = L L^T in place on the lower
// triangle and the two triangular sweeps L y = b, L^T x = y (gfx950 only).
//
// Reference: lu_solver.setup / solve (base/PyNucleus_base/solvers.pyx:80-186: the operator to a dense array, LAPACK getrf, then
// getrs per right-hand side), the solver behind `--matrixFormat dense --solver lu`.  The operators of the symmetric kernels are
// positive definite, so the factor here is Cholesky; LU with pivoting for the non-symmetric orders is pnl_lu.hip.
//
// Storage: row-major A[n][ld], ld >= n, fp64, 64-bit offsets.  Only A[i][j] with j <= i < n is read or written, nothing above the
// diagonal and nothing in the padding columns.
//
// Factorisation, right-looking, two levels of blocking.  Columns go in panels of CH_NB = 64; CH_OB = 256 columns make a block:
//   k_chol_diag    one workgroup factors the NB x NB diagonal block in LDS (sqrt, /, a - l l as they stand: no fast-math);
//   k_chol_panel   the rows below it: X L11^T = A21 by substitution, one lane per row, the row in registers, L11 in LDS;
//   k_chol_update  A22 -= L21 L21^T on the lower block triangle in CH_T x CH_T tiles of v_mfma_f64_16x16x4_f64: after a panel for
//                  the remaining columns of its block only (K = NB), after a block for everything right of it (K = OB), so that
//                  the n^2 / 2 trailing entries are read and written once per 256 columns instead of once per 64.
// A pivot that is not > 0 (NaN included) is recorded, 1-based, with an atomic min in a device word; the kernels that follow run on
// whatever values are there (sqrt of a negative number is a NaN, not a fault) and the host reads the word once at the end.
//
// Solves: per block column of CH_NB a one-workgroup kernel for the diagonal block (a wave per right-hand side, a lane per row)
// and one sweep kernel: forward b[j1:n] -= L[j1:n, j0:j1] y[j0:j1] (16 lanes per row), backward y[0:j0] -= L[j0:j1, 0:j0]^T x[j0:j1]
// from column sums over the contiguous rows of the panel (a lane per column, as k_gemv_two_sided does for its transposed half).
// Each sweep reads the triangle once.
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int CH_NB = 64;          // panel width (columns per diagonal block / panel solve)
constexpr int CH_OB = 256;         // columns per block: the trailing matrix right of it is updated once, with K = CH_OB
constexpr int CH_T = 64;           // workgroup tile of the trailing update (4 waves x (16 rows x 64 columns))
constexpr int CH_KC = 32;          // columns of the panel staged in LDS per step of the update
constexpr int CH_LDS = CH_NB+1;    // row stride of the LDS blocks (odd: a column walks all banks)
constexpr int CH_KS = CH_KC+2;     // row stride of the staged panel: 16 rows x 2 k of an MFMA operand hit 32 different bank pairs
constexpr int CH_INFO_NONE = 0x7f7f7f7f;    // what hipMemset(0x7f) leaves in the info word

typedef double ch_v4d __attribute__((ext_vector_type(4)));

// ---- factorisation ----------------------------------------------------------------------------------------------------------------

// the w x w diagonal block at (j0, j0), w <= CH_NB: right-looking in LDS; reads and writes its lower triangle only
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_diag(double *__restrict__ A, long long ld, int j0, int w, int *__restrict__ info) {
    __shared__ double s[CH_NB][CH_LDS];
    const int tid = threadIdx.x, j = tid & 63, iq = tid >> 6;
    double *__restrict__ D = A+(long long)j0*ld+j0;
    for (int i = iq; i < w; i += 4)
        if (j <= i) s[i][j] = D[(long long)i*ld+j];
    __syncthreads();
    for (int k = 0; k < w; k++) {
        if (tid == 0) {
            const double d = s[k][k];
            if (!(d > 0.)) atomicMin(info, j0+k+1);
            s[k][k] = sqrt(d);
        }
        __syncthreads();
        if (tid > k && tid < w) s[tid][k] = s[tid][k]/s[k][k];
        __syncthreads();
        if (j > k)
            for (int i = iq+((k+1) & ~3); i < w; i += 4)
                if (i >= j) s[i][j] -= s[i][k]*s[j][k];
        __syncthreads();
    }
    for (int i = iq; i < w; i += 4)
        if (j <= i) D[(long long)i*ld+j] = s[i][j];
}

// rows [j0 + w, n) of the panel: x_ik = (a_ik - sum_{m < k} x_im l_km) / l_kk.  One wave per workgroup, a lane per row; the rows come
// in and leave through LDS so that global memory sees contiguous 512-byte pieces.  w < CH_NB: the block is padded with the identity.
// The lower triangle of L11 is packed in LDS (entry (m, k) at m (m + 1) / 2 + k; every read is a broadcast).
// pnl_potrf never gets here with w < CH_NB (only the last panel of the matrix can be narrower, and it has no rows below it); the
// padding keeps the kernel right for any caller.
__global__ void __launch_bounds__(64)
k_chol_panel(double *__restrict__ A, long long ld, int n, int j0, int w) {
    __shared__ double sl[CH_NB*(CH_NB+1)/2], sx[64][CH_LDS];
    const int lane = threadIdx.x;
    const int r0 = j0+w+blockIdx.x*64, nr = min(64, n-r0);
    const double *__restrict__ D = A+(long long)j0*ld+j0;
    for (int i = 0; i < CH_NB; i++)
        if (lane <= i) sl[i*(i+1)/2+lane] = i < w ? D[(long long)i*ld+lane] : (i == lane ? 1. : 0.);
    double *__restrict__ X = A+(long long)r0*ld+j0;
    for (int i = 0; i < nr; i++)
        sx[i][lane] = lane < w ? X[(long long)i*ld+lane] : 0.;
    __syncthreads();
    double x[CH_NB];
    const int row = lane < nr ? lane : 0;
#pragma unroll
    for (int k = 0; k < CH_NB; k++) x[k] = sx[row][k];
#pragma unroll
    for (int k = 0; k < CH_NB; k++) {
        x[k] = x[k]/sl[k*(k+1)/2+k];
#pragma unroll
        for (int m = k+1; m < CH_NB; m++) x[m] -= x[k]*sl[m*(m+1)/2+k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CH_NB; k++) sx[lane][k] = x[k];
    __syncthreads();
    for (int i = 0; i < nr; i++)
        if (lane < w) X[(long long)i*ld+lane] = sx[i][lane];
}

// A[i][j] -= sum_{k0 <= k < k0 + K} A[i][k] A[j][k]  for lo <= j <= i < n, j < chi  (k0 + K <= lo: the panel lies left of the tiles).
// Grid: the CH_T x CH_T tiles (ti, tj), tj <= ti, of the rows / columns from lo on; tri: the whole lower block triangle row by row,
// else ti = blockIdx.x / ntj, tj = blockIdx.x % ntj (the columns end at chi).  Wave w of a tile owns the rows 16 w .. 16 w + 15 and
// four 16 x 16 accumulators; the operand of lane l is P[l & 15][k + (l >> 4)] for both A (rows of the tile) and B (rows of the panel
// that are the tile's columns), the results are D[(l >> 4) + 4 v][l & 15], v = 0 .. 3.
// pnl_potrf calls it with K = CH_NB or CH_OB only, both multiples of CH_KC: the zero fill beyond K (`kin`) is for other callers.
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_update(double *__restrict__ A, long long ld, int n, int lo, int chi, int k0, int K, int ntj, int tri) {
    __shared__ double sr[CH_T][CH_KS], sc[CH_T][CH_KS];
    int ti, tj;
    if (tri) {
        const long long t = blockIdx.x;
        ti = (int)((sqrt(8.*(double)t+1.)-1.)*0.5);
        while ((long long)ti*(ti+1)/2 > t) ti--;
        while ((long long)(ti+1)*(ti+2)/2 <= t) ti++;
        tj = (int)(t-(long long)ti*(ti+1)/2);
    } else {
        ti = blockIdx.x/ntj; tj = blockIdx.x-ti*ntj;
        if (tj > ti) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = lo+ti*CH_T, c0 = lo+tj*CH_T;
    ch_v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = (ch_v4d){0., 0., 0., 0.};
    const int kk = tid & (CH_KC-1), rq = tid >> 5;             // staging: 8 rows x 32 columns per pass
    const int m = lane & 15, kq = lane >> 4;
    for (int kc = 0; kc < K; kc += CH_KC) {
        __syncthreads();
        const bool kin = kc+kk < K;
#pragma unroll
        for (int p = 0; p < CH_T/8; p++) {
            const int i = rq+8*p;
            sr[i][kk] = (kin && r0+i < n) ? A[(long long)(r0+i)*ld+k0+kc+kk] : 0.;
            sc[i][kk] = (kin && c0+i < n) ? A[(long long)(c0+i)*ld+k0+kc+kk] : 0.;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CH_KC; k += 4) {
            const double a = sr[16*wv+m][k+kq];
#pragma unroll
            for (int t = 0; t < 4; t++)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sc[16*t+m][k+kq], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int jc = c0+16*t+m;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int ir = r0+16*wv+kq+4*v;
            if (ir < n && jc < chi && jc <= ir) A[(long long)ir*ld+jc] -= acc[t][v];
        }
    }
}

// ---- triangular solves ----------------------------------------------------------------------------------------------------------

// the w x w diagonal block at (j0, j0) against B[r][j0 .. j0 + w) of every right-hand side r: wave q takes r = q, q + 4, ...; lane i
// holds component i.  !TRANS: L y = b, column by column (y_k = b_k / l_kk, then b_i -= l_ik y_k below it); TRANS: L^T x = y from the
// last column up (x_k = y_k / l_kk, then y_i -= l_ki x_k above it).
template <bool TRANS>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_trsv_diag(const double *__restrict__ L, long long ld, int j0, int w, double *__restrict__ B, long long ldb, int nrhs) {
    __shared__ double s[CH_NB][CH_LDS];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const double *__restrict__ D = L+(long long)j0*ld+j0;
    for (int i = q; i < CH_NB; i += 4)
        s[i][lane] = (i < w && lane <= i) ? D[(long long)i*ld+lane] : (i == lane ? 1. : 0.);
    __syncthreads();
    for (int r = q; r < nrhs; r += 4) {
        double *__restrict__ b = B+(long long)r*ldb+j0;
        double v = lane < w ? b[lane] : 0.;
        if (!TRANS) {
            for (int k = 0; k < w; k++) {
                const double xk = __shfl(v, k)/s[k][k];
                if (lane == k) v = xk;
                else if (lane > k) v -= s[lane][k]*xk;
            }
        } else {
            for (int k = w-1; k >= 0; k--) {
                const double xk = __shfl(v, k)/s[k][k];
                if (lane == k) v = xk;
                else if (lane < k) v -= s[k][lane]*xk;
            }
        }
        if (lane < w) b[lane] = v;
    }
}

// forward: B[r][i] -= sum_{k < w} L[i][j0 + k] B[r][j0 + k] for the rows i in [j0 + w, n): 16 lanes per row (lane c of them takes the
// columns c, c + 16, c + 32, c + 48), 16 rows per pass, 64 rows per workgroup; the right-hand sides in groups of four
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_fwd_sweep(const double *__restrict__ L, long long ld, int n, int j0, int w, double *__restrict__ B, long long ldb, int nrhs) {
    const int tid = threadIdx.x, c = tid & 15, rr = tid >> 4;
    const int base = j0+w+blockIdx.x*64;
    for (int g = 0; g < nrhs; g += 4) {
        double y[4][4];
#pragma unroll
        for (int h = 0; h < 4; h++)
#pragma unroll
            for (int u = 0; u < 4; u++)
                y[h][u] = (g+h < nrhs && c+16*u < w) ? B[(long long)(g+h)*ldb+j0+c+16*u] : 0.;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int i = base+16*p+rr;
            double l[4];
#pragma unroll
            for (int u = 0; u < 4; u++) l[u] = (i < n && c+16*u < w) ? L[(long long)i*ld+j0+c+16*u] : 0.;
#pragma unroll
            for (int h = 0; h < 4; h++) {
                double sum = 0.;
#pragma unroll
                for (int u = 0; u < 4; u++) sum = __builtin_fma(l[u], y[h][u], sum);
                sum += __shfl_xor(sum, 8);
                sum += __shfl_xor(sum, 4);
                sum += __shfl_xor(sum, 2);
                sum += __shfl_xor(sum, 1);
                if (c == 0 && i < n && g+h < nrhs) B[(long long)(g+h)*ldb+i] -= sum;
            }
        }
    }
}

// backward: B[r][c] -= sum_{j0 <= i < j0 + w} L[i][c] B[r][i] for the columns c in [0, j0): a lane per column, 64 columns per workgroup,
// wave q sums the rows j0 + q, j0 + q + 4, ... of the panel (each row a contiguous 512-byte read), the four parts meet in LDS
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_bwd_sweep(const double *__restrict__ L, long long ld, int j0, int w, double *__restrict__ B, long long ldb, int nrhs) {
    __shared__ double part[4][4][64];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int c = blockIdx.x*64+lane;
    for (int g = 0; g < nrhs; g += 4) {
        double acc[4] = {0., 0., 0., 0.};
        if (c < j0)
            for (int i = q; i < w; i += 4) {
                const double l = L[(long long)(j0+i)*ld+c];
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (g+h < nrhs) acc[h] = __builtin_fma(l, B[(long long)(g+h)*ldb+j0+i], acc[h]);
            }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 4; h++) part[q][h][lane] = acc[h];
        __syncthreads();
        if (q < 4 && g+q < nrhs && c < j0)
            B[(long long)(g+q)*ldb+c] -= (part[0][q][lane]+part[1][q][lane])+(part[2][q][lane]+part[3][q][lane]);
    }
}

}  // namespace

extern "C" {

int pnl_potrf(pnl_context *ctx, double *A, int64_t ldA, int n, int *info) {
    if (!ctx) return PNL_ERR_INVALID;
    if (n < 0 || ldA < n || !info || (n > 0 && !A)) return fail(ctx, PNL_ERR_INVALID, "pnl_potrf: n < 0, ldA < n or a null pointer");
    *info = 0;
    if (n == 0) return PNL_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->b_cholinfo, sizeof(int)))) return rc;
    int *dinfo = (int*)ctx->b_cholinfo.p;
    HIPCHK(ctx, hipMemsetAsync(dinfo, 0x7f, sizeof(int), ctx->stream));
    const long long ld = ldA;
    for (int J0 = 0; J0 < n; J0 += CH_OB) {
        const int J1 = std::min(J0+CH_OB, n);
        for (int j0 = J0; j0 < J1; j0 += CH_NB) {
            const int j1 = std::min(j0+CH_NB, J1), w = j1-j0;
            hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, j0, w, dinfo);
            if (j1 < n)
                hipLaunchKernelGGL(k_chol_panel, dim3((n-j1+63)/64), dim3(64), 0, ctx->stream, A, ld, n, j0, w);
            if (j1 < J1) {
                // the rest of this block's columns, all rows below
                const int ntj = (J1-j1+CH_T-1)/CH_T, nti = (n-j1+CH_T-1)/CH_T;
                hipLaunchKernelGGL(k_chol_update, dim3((unsigned)(nti*ntj)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, n, j1, J1, j0, w, ntj, 0);
            }
        }
        if (J1 < n) {
            const long long nt = (n-J1+CH_T-1)/CH_T;
            hipLaunchKernelGGL(k_chol_update, dim3((unsigned)(nt*(nt+1)/2)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, n, J1, n, J0, J1-J0,
                               (int)nt, 1);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    int h = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h, dinfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *info = h == CH_INFO_NONE ? 0 : h;
    return PNL_OK;
}

int pnl_potrs(pnl_context *ctx, const double *L, int64_t ldL, int n, double *B, int64_t ldb, int nrhs) {
    if (!ctx) return PNL_ERR_INVALID;
    if (n < 0 || nrhs < 0 || ldL < n || ldb < n || (n > 0 && nrhs > 0 && (!L || !B)))
        return fail(ctx, PNL_ERR_INVALID, "pnl_potrs: n < 0, nrhs < 0, ldL < n, ldb < n or a null pointer");
    if (n == 0 || nrhs == 0) return PNL_OK;
    const long long ld = ldL, lb = ldb;
    const int nblk = (n+CH_NB-1)/CH_NB;
    for (int b = 0; b < nblk; b++) {
        const int j0 = b*CH_NB, j1 = std::min(j0+CH_NB, n);
        hipLaunchKernelGGL((k_chol_trsv_diag<false>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
        if (j1 < n)
            hipLaunchKernelGGL(k_chol_fwd_sweep, dim3((n-j1+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, n, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    for (int b = nblk-1; b >= 0; b--) {
        const int j0 = b*CH_NB, j1 = std::min(j0+CH_NB, n);
        hipLaunchKernelGGL((k_chol_trsv_diag<true>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
        if (j0 > 0)
            hipLaunchKernelGGL(k_chol_bwd_sweep, dim3((j0+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // extern "C"
