// Direct solvers for the dense operators (gfx950 only): blocked Cholesky A = L L^T for the symmetric positive definite ones
// (pnl_potrf / pnl_potrs), blocked LU with partial pivoting P A = L U for the others (pnl_getrf / pnl_getrs), and their triangular
// solves.  One unit for both: they share the sweep, the diagonal-block solve and the MFMA trailing update.
//
// Reference: lu_solver.setup / solve (base/PyNucleus_base/solvers.pyx:80-186: the operator to a dense array, LAPACK getrf, then
// getrs per right-hand side), the solver behind `--matrixFormat dense --solver lu`.  The operators of the symmetric kernels are
// positive definite, so their factor is Cholesky; the orders evaluated per quadrature point (constantNonSymFractionalOrder,
// smoothedLeftRightFractionalOrder, ...) need the pivoted LU.
//
// Storage: row-major A[n][ld], ld >= n, fp64, 64-bit offsets; nothing in the padding columns [n, ld) is read or written.
//   Cholesky  only A[i][j] with j <= i < n is read or written: L in the lower triangle, nothing above the diagonal is touched;
//   LU        the strict lower triangle receives L (unit diagonal, not stored), the upper triangle with the diagonal U; piv[k]
//             (0-based, k <= piv[k] < n) is LAPACK's swap sequence: at step k the rows k and piv[k] of the whole matrix were exchanged.
//
// Factorisation, right-looking, two levels of blocking.  Columns go in panels of NB = 64; OB = 256 columns make a block.  A panel is
// factored, then the rest of its block's columns is updated with K = NB; once the block is factored, everything right of it is
// updated with K = OB, so that the trailing matrix is read and written once per 256 columns instead of once per 64.
//   k_chol_diag     one workgroup factors the NB x NB diagonal block in LDS (sqrt, /, a - l l as they stand: no fast-math);
//   k_chol_panel    the rows below it: X L11^T = A21 by substitution, one lane per row, the row in registers, L11 in LDS;
//   k_lu_step       one launch per column k of a panel (and one before the first column), RB = 64 rows of the panel per workgroup,
//                   a wave per row and a lane per panel column, so that a row's piece of the panel is one contiguous 512-byte access.
//                   The launch of column k moves the pivot row (found by the launch before it) to row k, writes l_ik = a_ik / pivot
//                   and a_ij -= l_ik u_kj for the later columns j of the panel, and looks for the pivot of column k + 1 on the way:
//                   every workgroup leaves its (largest |a|, lowest row) pair in a scratch array and takes a ticket with an ordinary
//                   atomicAdd; the workgroup that draws the last ticket combines the pairs (the order (|a| descending, row ascending)
//                   is total, so the result does not depend on who comes last), and copies the pivot row and row k + 1 of the panel
//                   into a scratch buffer for the next launch.  No workgroup ever waits for another one: stream order between the
//                   launches is the only synchronisation across workgroups;
//   k_lu_swap       a panel's NB row interchanges, in order, on a range of columns outside the panel: a lane per column;
//   k_lu_u12        U12 = L11^-1 A12 for a range of columns right of the panel: unit-lower substitution, a lane per column, the
//                   column in registers, L11 in LDS (broadcast reads);
//   k_direct_update in T x T tiles of v_mfma_f64_16x16x4_f64: <true> A22 -= L21 L21^T on the lower block triangle (pnl_potrf),
//                   <false> C -= L21 U12 on a rectangle (pnl_getrf).
// LU after a panel: swap, U12 and update run on the block's own columns only (swap also on the columns left of it).  The columns
// right of the block are touched once the block is factored: all its interchanges, then per panel U12 and the update of the rest of
// the block's rows (K = NB), then everything below and right of the block (K = OB).  (The rows below the block lack the block's
// updates in those columns until then: an interchange across the block's lower edge must not fall between two of them.)
// A Cholesky pivot that is not > 0, or an LU pivot p without |p| > 0 (NaN included), is recorded, 1-based, with an atomic min in a
// device word; the kernels that follow run on whatever values are there (sqrt of a negative number and 0 / 0 are NaNs, not faults)
// and the host reads the word once at the end.
//
// Solves: per block column of NB a one-workgroup kernel for the diagonal block, k_direct_trsv_diag (a wave per right-hand side, a lane
// per row), and one sweep kernel over the rows that are left.  pnl_getrs first undoes the swap sequence per component into a scratch
// copy (k_lu_gather: lane i walks the swaps i, i - 1, ..., 0 backwards, a later swap k > i cannot touch it).
//   k_direct_sweep    b[rows] -= M[rows, j0:j1] x[j0:j1], 16 lanes per row: the rows below for L of either factorisation, the rows
//                     above for U (the rows of U right of the diagonal are contiguous, so that sweep has the same shape);
//   k_chol_bwd_sweep  y[0:j0] -= L[j0:j1, 0:j0]^T x[j0:j1] from column sums over the contiguous rows of the panel (a lane per column,
//                     as k_gemv_two_sided does for its transposed half).
// Each sweep reads its triangle once; the sums of one right-hand side do not depend on nrhs.
#include <climits>
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int NB = 64;             // panel width (columns per diagonal block / panel)
constexpr int OB = 256;            // columns per block: what lies right of it is updated once, with K = OB
constexpr int T = 64;              // workgroup tile of the trailing update (4 waves x (16 rows x 64 columns))
constexpr int KC = 32;             // k staged in LDS per step of the update
constexpr int RB = 64;             // rows of a panel per workgroup of k_lu_step
constexpr int LDS = NB+1;          // row stride of the NB x NB blocks in LDS (odd: a column walks all banks)
constexpr int KS = KC+2;           // row stride of staged rows [T][KC]: 16 rows x 2 k of an MFMA operand hit 32 different bank pairs
constexpr int US = T+16;           // row stride of the staged rows of U12 [KC][T]: 2 k x 16 columns of an MFMA operand do the same
constexpr int INFO_NONE = 0x7f7f7f7f;       // what hipMemset(0x7f) leaves in the info word
// scratch of pnl_getrf (pnl_context::b_luwork): words [info, ticket, pivot row, -], then the pivot row and row k of the panel, then
// the partial maxima
constexpr int W_INFO = 0, W_TICKET = 1, W_PIVROW = 2;
constexpr size_t OFF_ROWS = 16, OFF_PART = OFF_ROWS+2*NB*sizeof(double);

typedef double v4d __attribute__((ext_vector_type(4)));

// (|a|, row): larger |a| wins, among equal ones the lower row; a NaN never wins
__device__ __forceinline__ void lu_better(double &bv, int &bi, double v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// ---- factorisation ----------------------------------------------------------------------------------------------------------------

// the w x w diagonal block at (j0, j0), w <= NB: right-looking in LDS; reads and writes its lower triangle only
__global__ void __launch_bounds__(PNL_NTHREADS)
k_chol_diag(double *__restrict__ A, long long ld, int j0, int w, int *__restrict__ info) {
    __shared__ double s[NB][LDS];
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
// in and leave through LDS so that global memory sees contiguous 512-byte pieces.  w < NB: the block is padded with the identity.
// The lower triangle of L11 is packed in LDS (entry (m, k) at m (m + 1) / 2 + k; every read is a broadcast).
// pnl_potrf never gets here with w < NB (only the last panel of the matrix can be narrower, and it has no rows below it); the
// padding keeps the kernel right for any caller.
__global__ void __launch_bounds__(64)
k_chol_panel(double *__restrict__ A, long long ld, int n, int j0, int w) {
    __shared__ double sl[NB*(NB+1)/2], sx[64][LDS];
    const int lane = threadIdx.x;
    const int r0 = j0+w+blockIdx.x*64, nr = min(64, n-r0);
    const double *__restrict__ D = A+(long long)j0*ld+j0;
    for (int i = 0; i < NB; i++)
        if (lane <= i) sl[i*(i+1)/2+lane] = i < w ? D[(long long)i*ld+lane] : (i == lane ? 1. : 0.);
    double *__restrict__ X = A+(long long)r0*ld+j0;
    for (int i = 0; i < nr; i++)
        sx[i][lane] = lane < w ? X[(long long)i*ld+lane] : 0.;
    __syncthreads();
    double x[NB];
    const int row = lane < nr ? lane : 0;
#pragma unroll
    for (int k = 0; k < NB; k++) x[k] = sx[row][k];
#pragma unroll
    for (int k = 0; k < NB; k++) {
        x[k] = x[k]/sl[k*(k+1)/2+k];
#pragma unroll
        for (int m = k+1; m < NB; m++) x[m] -= x[k]*sl[m*(m+1)/2+k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NB; k++) sx[lane][k] = x[k];
    __syncthreads();
    for (int i = 0; i < nr; i++)
        if (lane < w) X[(long long)i*ld+lane] = sx[i][lane];
}

// Column k of the panel [j0, j0 + w) (see the header); k = -1: only the search in column 0.  words[W_PIVROW], prow (the pivot
// row's w panel entries) and krow (those of row j0 + k) were left by the launch before this one.
__global__ void __launch_bounds__(PNL_NTHREADS)
k_lu_step(double *A, long long ld, int n, int j0, int w, int k, int *piv, int *words, double *prow, double *krow, double *pval, int *pidx) {
    __shared__ double s_val[PNL_NTHREADS];
    __shared__ int s_idx[PNL_NTHREADS];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int kr = j0+k, kc = k+1;
    int p = kr;
    double pv = 0., pl = 0.;
    if (k >= 0) {
        p = words[W_PIVROW];
        pl = lane < w ? prow[lane] : 0.;
        pv = prow[k];
        if (blockIdx.x == 0 && tid == 0) {
            piv[kr] = p;
            if (!(fabs(pv) > 0.)) atomicMin(&words[W_INFO], kr+1);
        }
    }
    double bestv = -1.;
    int besti = INT_MAX;
    const int base = j0+blockIdx.x*RB;
    for (int i = q; i < RB; i += 4) {
        const int r = base+i;
        if (r >= n || r < kr) continue;
        double *row = A+(long long)r*ld+j0;
        double v = 0.;
        if (k >= 0) {
            if (r == kr) {                                 // the pivot row arrives: a row of U (and of L11 left of column k)
                if (lane < w && p != kr) row[lane] = pl;
                continue;
            }
            const bool sw = r == p;                        // the row that was at j0 + k arrives here
            if (lane < w && (sw || lane >= k)) v = sw ? krow[lane] : row[lane];
            const double l = __shfl(v, k)/pv;
            if (lane == k) v = l;
            else if (lane > k) v -= l*pl;
            if (lane < w && (sw || lane >= k)) row[lane] = v;
        } else if (lane == 0) v = row[0];
        if (lane == kc) lu_better(bestv, besti, fabs(v), r);
    }
    if (kc >= w) return;
    // this workgroup's candidate, then the ticket
    __threadfence();
    if (lane == kc) { s_val[q] = bestv; s_idx[q] = besti; }
    __syncthreads();
    if (tid == 0) {
        bestv = s_val[0]; besti = s_idx[0];
        for (int t = 1; t < 4; t++) lu_better(bestv, besti, s_val[t], s_idx[t]);
        pval[blockIdx.x] = bestv;
        pidx[blockIdx.x] = besti;
        __threadfence();
        s_last = atomicAdd(&words[W_TICKET], 1) == (int)gridDim.x-1;
    }
    __syncthreads();
    if (!s_last) return;
    // the last one: every other workgroup of this launch has finished its rows and left its pair
    __threadfence();
    bestv = -1.; besti = INT_MAX;
    for (int t = tid; t < (int)gridDim.x; t += PNL_NTHREADS) lu_better(bestv, besti, pval[t], pidx[t]);
    __syncthreads();
    s_val[tid] = bestv; s_idx[tid] = besti;
    __syncthreads();
    for (int s = PNL_NTHREADS/2; s > 0; s >>= 1) {
        if (tid < s) {
            bestv = s_val[tid]; besti = s_idx[tid];
            lu_better(bestv, besti, s_val[tid+s], s_idx[tid+s]);
            s_val[tid] = bestv; s_idx[tid] = besti;
        }
        __syncthreads();
    }
    const int nr = j0+kc;
    const int pn = s_idx[0] == INT_MAX ? nr : s_idx[0];    // only NaNs in the column: no interchange
    if (tid == 0) { words[W_PIVROW] = pn; words[W_TICKET] = 0; }
    if (tid < w) prow[tid] = A[(long long)pn*ld+j0+tid];
    else if (tid >= 64 && tid-64 < w) krow[tid-64] = A[(long long)nr*ld+j0+tid-64];
}

// the interchanges k = j0 .. j0 + w - 1 in order on the columns [clo, chi) outside the panel: a lane per column
__global__ void __launch_bounds__(PNL_NTHREADS)
k_lu_swap(double *__restrict__ A, long long ld, int clo, int chi, int j0, int w, const int *__restrict__ piv) {
    const int c = clo+blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (c >= chi || (c >= j0 && c < j0+w)) return;
    for (int k = 0; k < w; k++) {
        const int r = j0+k, p = piv[r];
        if (p != r) {
            const double a = A[(long long)r*ld+c], b = A[(long long)p*ld+c];
            A[(long long)r*ld+c] = b;
            A[(long long)p*ld+c] = a;
        }
    }
}

// U12 = L11^-1 A12: the rows [j0, j0 + w) of the columns [clo, chi), clo >= j0 + w.  A lane per column, the column in registers; L11 transposed in
// LDS (st[k][m] = l_mk, every read a broadcast).  w < NB: the block is padded with the identity (pnl_getrf never gets here with
// w < NB: only the last panel of the matrix can be narrower, and it has no columns right of it).
__global__ void __launch_bounds__(PNL_NTHREADS)
k_lu_u12(double *__restrict__ A, long long ld, int clo, int chi, int j0, int w) {
    __shared__ double st[NB][NB];
    const int tid = threadIdx.x;
    const double *__restrict__ D = A+(long long)j0*ld+j0;
    for (int t = tid; t < NB*NB; t += PNL_NTHREADS) {
        const int m = t >> 6, kk = t & 63;
        st[kk][m] = (m < w && kk < m) ? D[(long long)m*ld+kk] : 0.;
    }
    __syncthreads();
    const int c = clo+blockIdx.x*PNL_NTHREADS+tid;
    if (c >= chi) return;
    double *__restrict__ X = A+(long long)j0*ld+c;
    double x[NB];
    // rows i >= w: row w - 1 again (memory that is there; the zero columns of the padded L11 keep it out of the rows < w)
    const double *xp = X;
#pragma unroll
    for (int i = 0; i < NB; i++) {
        x[i] = *xp;
        xp += i+1 < w ? ld : 0;
    }
    // the row of L11^T is read at an offset the compiler cannot see through and that waits for x[k]: otherwise it hoists the LDS reads
    // of the whole triangle to the top (nothing orders them) and spills a thousand registers
#pragma unroll
    for (int k = 0; k < NB-1; k++) {
        int off = k*NB;
        asm volatile("" : "+v"(off), "+v"(x[k]));
#pragma unroll
        for (int m = k+1; m < NB; m++) x[m] -= (&st[0][0])[off+m]*x[k];
    }
#pragma unroll
    for (int i = 1; i < NB; i++) {
        X += ld;
        if (i < w) *X = x[i];
    }
}

// A[i][j] -= sum_{k0 <= k < k0 + K} A[i][k] B[k][j]  for rlo <= i < rhi, clo <= j < chi, in T x T tiles (k0 + K <= rlo, clo).
//   SYM   B[k][j] = A[j][k], rows of the panel left of the tiles, and only j <= i is written (rlo == clo): the tiles (ti, tj) with
//         tj <= ti; tri: the grid is the whole lower block triangle row by row, else ti = blockIdx.x / ntj, tj = blockIdx.x % ntj
//         (the columns end at chi) and the tiles above the diagonal leave at once;
//   !SYM  B[k][j] = A[k][j], the rows of U12 above the rectangle; ti = blockIdx.x / ntj, tj = blockIdx.x % ntj.
// Wave w of a tile owns the rows 16 w .. 16 w + 15 and four 16 x 16 accumulators; the A operand of lane l is the staged
// A[r0 + (l & 15)][k + (l >> 4)], the B operand B[k + (l >> 4)][c0 + (l & 15)], the results are D[(l >> 4) + 4 v][l & 15], v = 0 .. 3.
// The callers pass K = NB or OB only, both multiples of KC: the zero fill beyond K (`kin`) is for other callers.
template <bool SYM>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_direct_update(double *__restrict__ A, long long ld, int rlo, int rhi, int clo, int chi, int k0, int K, int ntj, int tri) {
    __shared__ double sr[T][KS], sb[SYM ? T*KS : KC*US];
    const auto b_at = [](int k, int j) { return SYM ? j*KS+k : k*US+j; };          // where B[k][c0 + j] of the staged piece lies in sb
    int ti, tj;
    if (SYM && tri) {
        const long long t = blockIdx.x;
        ti = (int)((sqrt(8.*(double)t+1.)-1.)*0.5);
        while ((long long)ti*(ti+1)/2 > t) ti--;
        while ((long long)(ti+1)*(ti+2)/2 <= t) ti++;
        tj = (int)(t-(long long)ti*(ti+1)/2);
    } else {
        ti = blockIdx.x/ntj; tj = blockIdx.x-ti*ntj;
        if (SYM && tj > ti) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = rlo+ti*T, c0 = clo+tj*T;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = (v4d){0., 0., 0., 0.};
    const int kk = tid & (KC-1), rq = tid >> 5;                // staging of rows [T][KC]: 8 rows x 32 k per pass
    const int m = lane & 15, kq = lane >> 4;                   // staging of U12: 4 k x 64 columns per pass (k = wv + 4 p, column = lane)
    for (int kc = 0; kc < K; kc += KC) {
        __syncthreads();
        const bool kin = kc+kk < K;
#pragma unroll
        for (int p = 0; p < T/8; p++) {
            const int i = rq+8*p;
            sr[i][kk] = (kin && r0+i < rhi) ? A[(long long)(r0+i)*ld+k0+kc+kk] : 0.;
            if (SYM) sb[b_at(kk, i)] = (kin && c0+i < rhi) ? A[(long long)(c0+i)*ld+k0+kc+kk] : 0.;
        }
        if (!SYM) {
#pragma unroll
            for (int p = 0; p < KC/4; p++) {
                const int ku = wv+4*p;
                sb[b_at(ku, lane)] = (kc+ku < K && c0+lane < chi) ? A[(long long)(k0+kc+ku)*ld+c0+lane] : 0.;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KC; k += 4) {
            const double a = sr[16*wv+m][k+kq];
#pragma unroll
            for (int t = 0; t < 4; t++)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sb[b_at(k+kq, 16*t+m)], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int jc = c0+16*t+m;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int ir = r0+16*wv+kq+4*v;
            if (ir < rhi && jc < chi && (!SYM || jc <= ir)) A[(long long)ir*ld+jc] -= acc[t][v];
        }
    }
}

// ---- triangular solves ----------------------------------------------------------------------------------------------------------

// T[r][i] = B[r][perm(i)], perm(i) = where component i of P b comes from: the swaps i, i - 1, ..., 0 undone in that order (a swap k > i
// exchanges two positions >= k > i).  An entry of piv outside [k, n) is taken as no interchange.
__global__ void __launch_bounds__(PNL_NTHREADS)
k_lu_gather(const int *__restrict__ piv, int n, const double *__restrict__ B, long long ldb, int nrhs, double *__restrict__ T) {
    const int i = blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (i >= n) return;
    int pos = i;
    for (int k = i; k >= 0; k--) {
        const int p = piv[k];
        if (p <= k || p >= n) continue;
        if (pos == k) pos = p;
        else if (pos == p) pos = k;
    }
    for (int r = 0; r < nrhs; r++) T[(long long)r*n+i] = B[(long long)r*ldb+pos];
}

__global__ void __launch_bounds__(PNL_NTHREADS)
k_lu_put(const double *__restrict__ T, int n, double *__restrict__ B, long long ldb, int nrhs) {
    const int i = blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (i >= n) return;
    for (int r = 0; r < nrhs; r++) B[(long long)r*ldb+i] = T[(long long)r*n+i];
}

// The w x w triangular block S at (j0, j0) of M against B[r][j0 .. j0 + w) of every right-hand side r: wave q takes r = q, q + 4, ...;
// lane i holds component i.  !UPPER: S x = b column by column from the first (x_k = b_k / s_kk, then b_i -= s_ik x_k below it); UPPER:
// from the last column up (b_i -= s_ik x_k above it).  UNIT: the diagonal is 1 and not stored (no division, nothing to assign).
// TRANS: S is the transpose of the stored block; it goes into LDS transposed (the odd stride keeps the 64 stores of a row apart),
// so that the recurrence reads s[lane][k] in every case.
//   <false, false, false>  L y = b, Cholesky      <false, true, false>  L y = b, LU
//   <true, false, true>    L^T x = y, Cholesky    <true, false, false>  U x = y, LU
template <bool UPPER, bool UNIT, bool TRANS>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_direct_trsv_diag(const double *__restrict__ M, long long ld, int j0, int w, double *__restrict__ B, long long ldb, int nrhs) {
    __shared__ double s[NB][LDS];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const double *__restrict__ D = M+(long long)j0*ld+j0;
    for (int i = q; i < NB; i += 4) {
        // row i of the stored block: its upper or lower part; the rest of s is the identity
        const bool in = i < w && lane < w && (UPPER != TRANS ? lane >= i : UNIT ? lane < i : lane <= i);
        (TRANS ? s[lane][i] : s[i][lane]) = in ? D[(long long)i*ld+lane] : (i == lane ? 1. : 0.);
    }
    __syncthreads();
    for (int r = q; r < nrhs; r += 4) {
        double *__restrict__ b = B+(long long)r*ldb+j0;
        double v = lane < w ? b[lane] : 0.;
        for (int t = 0; t < w; t++) {
            const int k = UPPER ? w-1-t : t;
            const double xk = UNIT ? __shfl(v, k) : __shfl(v, k)/s[k][k];
            if (!UNIT && lane == k) v = xk;
            else if (UPPER ? lane < k : lane > k) v -= s[lane][k]*xk;
        }
        if (lane < w) b[lane] = v;
    }
}

// B[r][i] -= sum_{k < w} M[i][j0 + k] B[r][j0 + k] for the rows i in [rbeg, rend): 16 lanes per row (lane c of them takes the columns
// c, c + 16, c + 32, c + 48), 16 rows per pass, 64 rows per workgroup; the right-hand sides in groups of four
__global__ void __launch_bounds__(PNL_NTHREADS)
k_direct_sweep(const double *__restrict__ M, long long ld, int rbeg, int rend, int j0, int w, double *__restrict__ B, long long ldb, int nrhs) {
    const int tid = threadIdx.x, c = tid & 15, rr = tid >> 4;
    const int base = rbeg+blockIdx.x*64;
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
            for (int u = 0; u < 4; u++) l[u] = (i < rend && c+16*u < w) ? M[(long long)i*ld+j0+c+16*u] : 0.;
#pragma unroll
            for (int h = 0; h < 4; h++) {
                double sum = 0.;
#pragma unroll
                for (int u = 0; u < 4; u++) sum = __builtin_fma(l[u], y[h][u], sum);
                sum += __shfl_xor(sum, 8);
                sum += __shfl_xor(sum, 4);
                sum += __shfl_xor(sum, 2);
                sum += __shfl_xor(sum, 1);
                if (c == 0 && i < rend && g+h < nrhs) B[(long long)(g+h)*ldb+i] -= sum;
            }
        }
    }
}

// Cholesky backward: B[r][c] -= sum_{j0 <= i < j0 + w} L[i][c] B[r][i] for the columns c in [0, j0): a lane per column, 64 columns per
// workgroup, wave q sums the rows j0 + q, j0 + q + 4, ... of the panel (each row a contiguous 512-byte read), the four parts meet in
// LDS.  Not k_direct_sweep on L^T: this one sums down the columns of the panel wave by wave, then (p0 + p1) + (p2 + p3); the other
// order of summation would give other bits (and strided reads).
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

// ---- host -------------------------------------------------------------------------------------------------------------------------

// the device word that takes the first bad pivot (atomic min of 1-based columns): armed before the factorisation, read once after it
int info_arm(pnl_context *ctx, int *dinfo) {
    HIPCHK(ctx, hipMemsetAsync(dinfo, 0x7f, sizeof(int), ctx->stream));
    return PNL_OK;
}

int info_read(pnl_context *ctx, const int *dinfo, int *info) {
    int h = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h, dinfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *info = h == INFO_NONE ? 0 : h;
    return PNL_OK;
}

void launch_swap(pnl_context *ctx, double *A, long long ld, int clo, int chi, int j0, int w, const int *piv) {
    if (chi > clo)
        hipLaunchKernelGGL(k_lu_swap, dim3((unsigned)((chi-clo+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, clo, chi, j0, w, piv);
}

void launch_u12(pnl_context *ctx, double *A, long long ld, int clo, int chi, int j0, int w) {
    if (chi > clo)
        hipLaunchKernelGGL(k_lu_u12, dim3((unsigned)((chi-clo+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, clo, chi, j0, w);
}

void launch_lu_update(pnl_context *ctx, double *A, long long ld, int rlo, int rhi, int clo, int chi, int k0, int K) {
    const long long nti = (rhi-rlo+T-1)/T, ntj = (chi-clo+T-1)/T;
    if (nti <= 0 || ntj <= 0) return;
    hipLaunchKernelGGL((k_direct_update<false>), dim3((unsigned)(nti*ntj)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, rlo, rhi, clo, chi, k0, K,
                       (int)ntj, 0);
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
    if ((rc = info_arm(ctx, dinfo))) return rc;
    const long long ld = ldA;
    for (int J0 = 0; J0 < n; J0 += OB) {
        const int J1 = std::min(J0+OB, n);
        for (int j0 = J0; j0 < J1; j0 += NB) {
            const int j1 = std::min(j0+NB, J1), w = j1-j0;
            hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, j0, w, dinfo);
            if (j1 < n)
                hipLaunchKernelGGL(k_chol_panel, dim3((n-j1+63)/64), dim3(64), 0, ctx->stream, A, ld, n, j0, w);
            if (j1 < J1) {
                // the rest of this block's columns, all rows below
                const int ntj = (J1-j1+T-1)/T, nti = (n-j1+T-1)/T;
                hipLaunchKernelGGL((k_direct_update<true>), dim3((unsigned)(nti*ntj)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, j1, n, j1, J1,
                                   j0, w, ntj, 0);
            }
        }
        if (J1 < n) {
            const long long nt = (n-J1+T-1)/T;
            hipLaunchKernelGGL((k_direct_update<true>), dim3((unsigned)(nt*(nt+1)/2)), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, J1, n, J1, n,
                               J0, J1-J0, (int)nt, 1);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return info_read(ctx, dinfo, info);
}

int pnl_potrs(pnl_context *ctx, const double *L, int64_t ldL, int n, double *B, int64_t ldb, int nrhs) {
    if (!ctx) return PNL_ERR_INVALID;
    if (n < 0 || nrhs < 0 || ldL < n || ldb < n || (n > 0 && nrhs > 0 && (!L || !B)))
        return fail(ctx, PNL_ERR_INVALID, "pnl_potrs: n < 0, nrhs < 0, ldL < n, ldb < n or a null pointer");
    if (n == 0 || nrhs == 0) return PNL_OK;
    const long long ld = ldL, lb = ldb;
    const int nblk = (n+NB-1)/NB;
    for (int b = 0; b < nblk; b++) {
        const int j0 = b*NB, j1 = std::min(j0+NB, n);
        hipLaunchKernelGGL((k_direct_trsv_diag<false, false, false>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
        if (j1 < n)
            hipLaunchKernelGGL(k_direct_sweep, dim3((n-j1+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j1, n, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    for (int b = nblk-1; b >= 0; b--) {
        const int j0 = b*NB, j1 = std::min(j0+NB, n);
        hipLaunchKernelGGL((k_direct_trsv_diag<true, false, true>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
        if (j0 > 0)
            hipLaunchKernelGGL(k_chol_bwd_sweep, dim3((j0+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, L, ld, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_getrf(pnl_context *ctx, double *A, int64_t ldA, int n, int32_t *piv, int *info) {
    if (!ctx) return PNL_ERR_INVALID;
    if (n < 0 || ldA < n || !info || (n > 0 && (!A || !piv))) return fail(ctx, PNL_ERR_INVALID, "pnl_getrf: n < 0, ldA < n or a null pointer");
    *info = 0;
    if (n == 0) return PNL_OK;
    int rc;
    const int maxwg = (n+RB-1)/RB;
    if ((rc = ensure(ctx, ctx->b_luwork, OFF_PART+(size_t)maxwg*(sizeof(double)+sizeof(int))))) return rc;
    char *wk = (char*)ctx->b_luwork.p;
    int *words = (int*)wk;
    double *prow = (double*)(wk+OFF_ROWS), *krow = prow+NB, *pval = (double*)(wk+OFF_PART);
    int *pidx = (int*)(pval+maxwg);
    HIPCHK(ctx, hipMemsetAsync(words, 0, 4*sizeof(int), ctx->stream));
    if ((rc = info_arm(ctx, words+W_INFO))) return rc;
    const long long ld = ldA;
    for (int J0 = 0; J0 < n; J0 += OB) {
        const int J1 = std::min(J0+OB, n);
        for (int j0 = J0; j0 < J1; j0 += NB) {
            const int j1 = std::min(j0+NB, J1), w = j1-j0;
            const unsigned nwg = (unsigned)((n-j0+RB-1)/RB);
            for (int k = -1; k < w; k++)
                hipLaunchKernelGGL(k_lu_step, dim3(nwg), dim3(PNL_NTHREADS), 0, ctx->stream, A, ld, n, j0, w, k, piv, words, prow, krow, pval, pidx);
            // inside the block and left of it; the columns right of the block wait until the block is factored (their rows below the
            // block are updated once per block only, so a row may not cross the block's lower edge between two of their updates)
            launch_swap(ctx, A, ld, 0, J1, j0, w, piv);
            launch_u12(ctx, A, ld, j1, J1, j0, w);
            launch_lu_update(ctx, A, ld, j1, n, j1, J1, j0, w);                // the rest of this block's columns, all rows below
            HIPCHK(ctx, hipGetLastError());
        }
        if (J1 < n) {
            // right of the block: all its interchanges first, then U12 panel by panel with the rest of the block's rows updated in
            // between, then everything below
            for (int j0 = J0; j0 < J1; j0 += NB) launch_swap(ctx, A, ld, J1, n, j0, std::min(j0+NB, J1)-j0, piv);
            for (int j0 = J0; j0 < J1; j0 += NB) {
                const int j1 = std::min(j0+NB, J1);
                launch_u12(ctx, A, ld, J1, n, j0, j1-j0);
                launch_lu_update(ctx, A, ld, j1, J1, J1, n, j0, j1-j0);
            }
            launch_lu_update(ctx, A, ld, J1, n, J1, n, J0, J1-J0);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return info_read(ctx, words+W_INFO, info);
}

int pnl_getrs(pnl_context *ctx, const double *LU, int64_t ldLU, int n, const int32_t *piv, double *B, int64_t ldb, int nrhs) {
    if (!ctx) return PNL_ERR_INVALID;
    if (n < 0 || nrhs < 0 || ldLU < n || ldb < n || (n > 0 && nrhs > 0 && (!LU || !B || !piv)))
        return fail(ctx, PNL_ERR_INVALID, "pnl_getrs: n < 0, nrhs < 0, ldLU < n, ldb < n or a null pointer");
    if (n == 0 || nrhs == 0) return PNL_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->b_lutmp, (size_t)n*(size_t)nrhs*sizeof(double)))) return rc;
    double *T = (double*)ctx->b_lutmp.p;
    const long long ld = ldLU, lb = ldb;
    const unsigned ng = (unsigned)((n+PNL_NTHREADS-1)/PNL_NTHREADS);
    hipLaunchKernelGGL(k_lu_gather, dim3(ng), dim3(PNL_NTHREADS), 0, ctx->stream, piv, n, B, lb, nrhs, T);
    hipLaunchKernelGGL(k_lu_put, dim3(ng), dim3(PNL_NTHREADS), 0, ctx->stream, T, n, B, lb, nrhs);
    const int nblk = (n+NB-1)/NB;
    for (int b = 0; b < nblk; b++) {
        const int j0 = b*NB, j1 = std::min(j0+NB, n);
        hipLaunchKernelGGL((k_direct_trsv_diag<false, true, false>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, LU, ld, j0, j1-j0, B, lb, nrhs);
        if (j1 < n)
            hipLaunchKernelGGL(k_direct_sweep, dim3((n-j1+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, LU, ld, j1, n, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    for (int b = nblk-1; b >= 0; b--) {
        const int j0 = b*NB, j1 = std::min(j0+NB, n);
        hipLaunchKernelGGL((k_direct_trsv_diag<true, false, false>), dim3(1), dim3(PNL_NTHREADS), 0, ctx->stream, LU, ld, j0, j1-j0, B, lb, nrhs);
        if (j0 > 0)
            hipLaunchKernelGGL(k_direct_sweep, dim3((j0+63)/64), dim3(PNL_NTHREADS), 0, ctx->stream, LU, ld, 0, j0, j0, j1-j0, B, lb, nrhs);
    }
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // extern "C"
