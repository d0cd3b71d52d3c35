// Products with a block of vectors, one pass over the matrix for up to 16 of them (gfx950 only): pnl_gemv_block for a dense
// row-major block, pnl_spmv_block for the CSR / SSS pattern resident in the context.
//
// Reference: LinearOperator.matvec_multi / dotMV / A * X with a 2-D X (base/PyNucleus_base/LinearOperator_{SCALAR}.pxi:23-26, 64-76,
// 120-121), which loop over the vectors or call dgemm.  A product is bound by HBM, so k vectors should cost one sweep of the
// matrix and not k.  Vectors are stored one per row (the layout of pnl_potrs / pnl_getrs): vector v is X[v ldx .. v ldx + ncols).
//
// pnl_gemv_block.  The vectors are taken in groups of GB_NV = 16: one launch (and one pass over A) per group.  The contraction is
// v_mfma_f64_16x16x4_f64 with 16 rows of A as the A operand and the 16 vectors as the B operand; vectors that do not exist are
// zero operands whose results are not stored.
//   workgroup   GB_RB = 128 rows (8 waves x 16 rows) x GB_CW = 2048 columns; grid = (row blocks, column chunks);
//   sub-chunk   GB_KC = 64 columns: a lane holds its 8 pieces of 16 bytes of A in registers, the workgroup the 16 x 64 piece of X in
//               LDS (8 KB, shared by the 128 rows: X is re-read from L2 once per 128 rows, 1/8 of the bytes of A), and every wave
//               runs 16 MFMAs on them.  Both are double-buffered: the loads of the next sub-chunk (A into a second set of
//               registers, X into registers and from there into the other LDS buffer) are issued before the MFMAs of this one,
//               so 128 bytes of A per lane are in flight while the matrix pipe works, with one barrier per sub-chunk;
//   operands    the k index of an MFMA is free as long as A and B agree: lane (m = l & 15, q = l >> 4) loads for j = 0 .. 7 the
//               columns c + 8 j + 2 q, + 1 of row r0 + m in one 16-byte load, so that the four q lanes of a row read 64 contiguous
//               bytes per load and a 128-byte line is finished by two loads (plain loads: with non-temporal ones the second half
//               of a line missed the vector cache, 5.1 instead of 5.8 TB/s at n = 48,769).  MFMA (j, h) contracts the four columns
//               c + 8 j + 2 q + h, q = 0 .. 3.  The piece of X lies in LDS in that operand order, [j][v][q] pairs (h = 0, 1): lane
//               (v, q) reads pair j 64 + 4 v + q, a permutation of 64 contiguous 16-byte slots (no bank conflict);
//   edges       rows beyond nrows read row nrows - 1 (rows of the A operand do not mix; their results are not stored); columns
//               beyond the chunk or the matrix are zero in both operands and are not loaded.  16-byte loads where the base and
//               ldA allow them, 8-byte loads otherwise and in the last sub-chunk of a chunk: the same arithmetic, the same bits;
//   sums        h = 0 and h = 1 go to two accumulators that meet as acc0 + acc1 at the end of the chunk.  One chunk (ncols <= GB_CW):
//               the workgroup writes y = alpha s + beta b itself.  More: it writes s to the context's scratch [chunk][16][nrows],
//               and k_gb_reduce adds the chunks in ascending order, then alpha and beta.  No atomics: the shape of every sum
//               depends on (nrows, ncols, ldA, alignment) only, so the bits of Y[v] are the same on every call and do not depend
//               on nvec, on v or on the other vectors.
// The symmetric half-read (pnl_gemv with symmetric_half = 2) needs column sums across workgroups, which k_gemv_two_sided forms with
// atomics: not done here, a symmetric operator goes through the full read.
//
// pnl_spmv_block.  One wave per row as k_spmv; every (index, value) pair is loaded once per group of at most 16 vectors.  The gather
// X[v][J] would touch nvec different lines in the vector-major layout, so the group is transposed once into a context scratch of
// n x NV interleaved doubles (NV = the group's size rounded up to 1, 2, 4, 8 or 16; missing vectors are zero): the gather of an entry
// is then one piece of 8 NV contiguous bytes.  Per vector: fma in ascending entry order per lane, the lanes in the fixed DPP tree of
// wave_sum, so CSR is free of atomics and its bits do not depend on nvec or on the position.  SSS adds the mirrored entries with
// atomic_add_f64 as k_spmv does (Y is zeroed by the call): its contract is the value, not the bits.
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int GB_NV = 16;                  // vectors per group = columns of the MFMA's B operand
constexpr int GB_THREADS = 512;            // 8 waves
constexpr int GB_RB = 16*(GB_THREADS/64);  // rows per workgroup
constexpr int GB_KC = 64;                  // columns per sub-chunk (staged piece of X: GB_NV x GB_KC doubles)
constexpr int GB_CW = 2048;                // columns per workgroup; more columns are split over workgroups
constexpr int GB_J = GB_KC/8;              // 16-byte loads per lane and sub-chunk
constexpr int GB_XS = GB_NV*GB_KC/GB_THREADS;   // values of X per thread and sub-chunk
static_assert(GB_CW % GB_KC == 0 && GB_THREADS == 128*(GB_J/GB_XS), "staging: 8 columns x 16 vectors x GB_J / GB_XS values of j per pass");

typedef double gb_d2 __attribute__((ext_vector_type(2)));
typedef double gb_d4 __attribute__((ext_vector_type(4)));

// the lane's pieces of row arow for the sub-chunk at column c: columns c + 8 j + 2 q, + 1; zero beyond cend
template <bool AL>
__device__ __forceinline__ void gb_load_a(const double *__restrict__ arow, int c, int cend, int q, gb_d2 (&a)[GB_J]) {
    if (AL && c+GB_KC <= cend) {
#pragma unroll
        for (int j = 0; j < GB_J; j++) a[j] = *(const gb_d2*)(arow+c+8*j+2*q);
    } else {
#pragma unroll
        for (int j = 0; j < GB_J; j++) {
            const int col = c+8*j+2*q;
            a[j].x = col < cend ? arow[col] : 0.;
            a[j].y = col+1 < cend ? arow[col+1] : 0.;
        }
    }
}

// the thread's values of the piece of X at column c: vector sv (xrow; none if !have), columns c + 8 (jb + (GB_J / GB_XS) i) + cl
__device__ __forceinline__ void gb_load_x(const double *__restrict__ xrow, bool have, int c, int cend, int jb, int cl, double (&xs)[GB_XS]) {
#pragma unroll
    for (int i = 0; i < GB_XS; i++) {
        const int col = c+8*(jb+(GB_J/GB_XS)*i)+cl;
        xs[i] = (have && col < cend) ? xrow[col] : 0.;
    }
}

// AL: A_dev is 16-byte aligned and ldA is even
template <bool AL>
__global__ void __launch_bounds__(GB_THREADS)
k_gemv_block(const double *__restrict__ A, long long ldA, int nrows, int ncols, int nv, const double *__restrict__ X, long long ldx, double alpha,
             double beta, const double *B, long long ldb, double *Y, long long ldy, double *__restrict__ part) {
    __shared__ gb_d2 sx[2][GB_J*64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x*GB_RB+16*wv;
    const int c0 = blockIdx.y*GB_CW, cend = min(ncols, c0+GB_CW);
    const double *__restrict__ arow = A+(long long)min(r0+m, nrows-1)*ldA;
    // staging: thread -> (column c + 8 j + cl, vector sv), j = jb + (GB_J / GB_XS) i
    const int cl = tid & 7, sv = (tid >> 3) & 15, jb = tid >> 7;
    const double *__restrict__ xrow = X+(long long)min(sv, nv-1)*ldx;
    gb_d4 acc0 = (gb_d4){0., 0., 0., 0.}, acc1 = (gb_d4){0., 0., 0., 0.};
    gb_d2 an[GB_J];
    double xn[GB_XS];
    gb_load_a<AL>(arow, c0, cend, q, an);
    gb_load_x(xrow, sv < nv, c0, cend, jb, cl, xn);
    int buf = 0;
    for (int c = c0; c < cend; c += GB_KC, buf ^= 1) {
        gb_d2 a[GB_J];
#pragma unroll
        for (int j = 0; j < GB_J; j++) a[j] = an[j];
#pragma unroll
        for (int i = 0; i < GB_XS; i++) ((double*)sx[buf])[128*(jb+(GB_J/GB_XS)*i)+8*sv+cl] = xn[i];
        // one barrier per sub-chunk: whoever writes sx[buf ^ 1] next has passed this barrier, which every wave reaches only after its
        // reads of sx[buf ^ 1] in the sub-chunk before
        __syncthreads();
        // the next sub-chunk is in flight while this one is contracted
        if (c+GB_KC < cend) {
            gb_load_a<AL>(arow, c+GB_KC, cend, q, an);
            gb_load_x(xrow, sv < nv, c+GB_KC, cend, jb, cl, xn);
        }
#pragma unroll
        for (int j = 0; j < GB_J; j++) {
            const gb_d2 b = sx[buf][64*j+4*m+q];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j].x, b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j].y, b.y, acc1, 0, 0, 0);
        }
    }
    // lane (m, q) holds D[row q + 4 t][vector m], t = 0 .. 3
    if (m >= nv) return;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int r = r0+q+4*t;
        if (r >= nrows) continue;
        const double s = acc0[t]+acc1[t];
        if (part) part[((size_t)blockIdx.y*GB_NV+m)*(size_t)nrows+r] = s;
        else Y[m*ldy+r] = beta != 0. ? __builtin_fma(alpha, s, beta*B[m*ldb+r]) : alpha*s;
    }
}

// Y[v][r] = alpha (part[0][v][r] + part[1][v][r] + ... in ascending chunk order) + beta B[v][r]
__global__ void __launch_bounds__(PNL_NTHREADS)
k_gb_reduce(const double *__restrict__ part, int nchunks, int nrows, double alpha, double beta, const double *B, long long ldb, double *Y,
            long long ldy) {
    const int r = blockIdx.x*PNL_NTHREADS+threadIdx.x, v = blockIdx.y;
    if (r >= nrows) return;
    double s = part[(size_t)v*nrows+r];
    for (int k = 1; k < nchunks; k++) s += part[((size_t)k*GB_NV+v)*(size_t)nrows+r];
    Y[v*ldy+r] = beta != 0. ? __builtin_fma(alpha, s, beta*B[v*ldb+r]) : alpha*s;
}

// ---- CSR / SSS ------------------------------------------------------------------------------------------------------------------

// Xt[i][v] = X[v][i] for v < nv, 0 for nv <= v < NV
template <int NV>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_sb_pack(int n, int nv, const double *__restrict__ X, long long ldx, double *__restrict__ Xt) {
    const long long idx = (long long)blockIdx.x*PNL_NTHREADS+threadIdx.x;
    if (idx >= (long long)n*NV) return;
    const int i = (int)(idx/NV), v = (int)(idx-(long long)i*NV);
    Xt[idx] = v < nv ? X[v*ldx+i] : 0.;
}

template <int NV>
__device__ __forceinline__ void sb_gather(const double *__restrict__ Xt, int J, double (&x)[NV]) {
    const double *p = Xt+(size_t)J*NV;
    if constexpr (NV == 1) x[0] = p[0];
    else {
#pragma unroll
        for (int v = 0; v < NV; v += 2) {
            const gb_d2 t = *(const gb_d2*)(p+v);
            x[v] = t.x; x[v+1] = t.y;
        }
    }
}

// one wave per row.  !SSS: Y[v][row] = sum_t data[t] X[v][indices[t]];  SSS: Y (zeroed) += the row, its mirror image and the diagonal
template <int NV, bool SSS>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_spmv_block(const int *__restrict__ indptr, const int *__restrict__ indices, const double *__restrict__ data, const double *__restrict__ diag,
             int n, int nv, const double *__restrict__ Xt, double *Y, long long ldy) {
    const int lane = threadIdx.x & 63;
    const int row = (int)(((long long)blockIdx.x*PNL_NTHREADS+threadIdx.x) >> 6);
    if (row >= n) return;
    const int b = indptr[row], e = indptr[row+1];
    double s[NV], xr[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) s[v] = 0.;
    if (SSS) sb_gather<NV>(Xt, row, xr);
    int t = b+lane;
    if (!SSS) {
        // two (index, value, gather) chains per lane in flight; the sums stay in entry order
        for (; t+64 < e; t += 128) {
            const int J0 = indices[t], J1 = indices[t+64];
            const double a0 = data[t], a1 = data[t+64];
            double x0[NV], x1[NV];
            sb_gather<NV>(Xt, J0, x0);
            sb_gather<NV>(Xt, J1, x1);
#pragma unroll
            for (int v = 0; v < NV; v++) s[v] = __builtin_fma(a1, x1[v], __builtin_fma(a0, x0[v], s[v]));
        }
    }
    for (; t < e; t += 64) {
        const int J = indices[t];
        const double a = data[t];
        double x[NV];
        sb_gather<NV>(Xt, J, x);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            s[v] = __builtin_fma(a, x[v], s[v]);
            if (SSS && v < nv) atomic_add_f64(&Y[v*ldy+J], a*xr[v]);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
        if (v < nv) {                            // uniform over the wave
            const double tot = wave_sum(s[v]);
            if (lane == 0) {
                if (SSS) atomic_add_f64(&Y[v*ldy+row], __builtin_fma(diag[row], xr[v], tot));
                else Y[v*ldy+row] = tot;
            }
        }
    }
}

template <int NV>
int spmv_group(pnl_context *ctx, const double *data, const double *diag, int nv, const double *X, long long ldx, double *Y, long long ldy) {
    const int n = ctx->N;
    double *Xt = (double*)ctx->b_blk_xt.p;
    const long long tot = (long long)n*NV;
    hipLaunchKernelGGL((k_sb_pack<NV>), dim3((unsigned)((tot+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0, ctx->stream, n, nv, X, ldx, Xt);
    HIPCHK(ctx, hipGetLastError());
    const int *indptr = (const int*)ctx->b_sp_indptr.p, *indices = (const int*)ctx->b_sp_indices.p;
    const dim3 grid((n+PNL_NTHREADS/64-1)/(PNL_NTHREADS/64));
    if (diag) {
        HIPCHK(ctx, hipMemset2DAsync(Y, sizeof(double)*(size_t)ldy, 0, sizeof(double)*(size_t)n, (size_t)nv, ctx->stream));
        hipLaunchKernelGGL((k_spmv_block<NV, true>), grid, dim3(PNL_NTHREADS), 0, ctx->stream, indptr, indices, data, diag, n, nv, Xt, Y, ldy);
    } else
        hipLaunchKernelGGL((k_spmv_block<NV, false>), grid, dim3(PNL_NTHREADS), 0, ctx->stream, indptr, indices, data, diag, n, nv, Xt, Y, ldy);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // namespace

extern "C" {

int pnl_gemv_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int nrows, int ncols, int nvec, const double *X_dev, int64_t ldx,
                   double alpha, double beta, const double *B_dev, int64_t ldb, double *Y_dev, int64_t ldy) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!A_dev || !X_dev || !Y_dev || X_dev == Y_dev) return fail(ctx, PNL_ERR_INVALID, "pnl_gemv_block: null or overlapping arguments");
    if (nvec < 1 || nrows < 1 || ncols < 1 || ldA < ncols || ldx < ncols || ldy < nrows)
        return fail(ctx, PNL_ERR_INVALID, "pnl_gemv_block: bad sizes (nrows=%d ncols=%d nvec=%d ldA=%lld ldx=%lld ldy=%lld)", nrows, ncols, nvec,
                    (long long)ldA, (long long)ldx, (long long)ldy);
    if (beta != 0. && (!B_dev || ldb < nrows)) return fail(ctx, PNL_ERR_INVALID, "pnl_gemv_block: beta != 0 needs B with ldb >= nrows");
    const int nchunks = (ncols+GB_CW-1)/GB_CW;
    double *part = nullptr;
    if (nchunks > 1) {
        if (int rc = ensure(ctx, ctx->b_blk_part, sizeof(double)*(size_t)nchunks*GB_NV*(size_t)nrows)) return rc;
        part = (double*)ctx->b_blk_part.p;
    }
    const bool al = ((((uintptr_t)A_dev) & 15) == 0) && (ldA & 1) == 0;
    const dim3 grid((nrows+GB_RB-1)/GB_RB, nchunks);
    for (int v0 = 0; v0 < nvec; v0 += GB_NV) {
        const int nv = std::min(GB_NV, nvec-v0);
        const double *X = X_dev+(long long)v0*ldx, *B = beta != 0. ? B_dev+(long long)v0*ldb : nullptr;
        double *Y = Y_dev+(long long)v0*ldy;
        if (al)
            hipLaunchKernelGGL((k_gemv_block<true>), grid, dim3(GB_THREADS), 0, ctx->stream, A_dev, (long long)ldA, nrows, ncols, nv, X, (long long)ldx,
                               alpha, beta, B, (long long)ldb, Y, (long long)ldy, part);
        else
            hipLaunchKernelGGL((k_gemv_block<false>), grid, dim3(GB_THREADS), 0, ctx->stream, A_dev, (long long)ldA, nrows, ncols, nv, X, (long long)ldx,
                               alpha, beta, B, (long long)ldb, Y, (long long)ldy, part);
        HIPCHK(ctx, hipGetLastError());
        if (part) {
            hipLaunchKernelGGL(k_gb_reduce, dim3((nrows+PNL_NTHREADS-1)/PNL_NTHREADS, nv), dim3(PNL_NTHREADS), 0, ctx->stream, (const double*)part, nchunks,
                               nrows, alpha, beta, B, (long long)ldb, Y, (long long)ldy);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    return PNL_OK;
}

int pnl_spmv_block(pnl_context *ctx, const double *data_dev, const double *diag_dev, int nvec, const double *X_dev, int64_t ldx, double *Y_dev,
                   int64_t ldy) {
    if (!ctx || !X_dev || !Y_dev) return PNL_ERR_INVALID;
    if (ctx->sp_nnz < 0) return fail(ctx, PNL_ERR_STATE, "upload the sparsity pattern first");
    if (!data_dev && ctx->sp_nnz > 0) return fail(ctx, PNL_ERR_INVALID, "null matrix data");
    const int n = ctx->N;
    if (nvec < 1 || ldx < n || ldy < n || X_dev == Y_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_spmv_block: bad arguments (nvec=%d ldx=%lld ldy=%lld n=%d)", nvec, (long long)ldx, (long long)ldy, n);
    int nvmax = 1;
    while (nvmax < std::min(nvec, GB_NV)) nvmax *= 2;
    if (int rc = ensure(ctx, ctx->b_blk_xt, sizeof(double)*(size_t)n*nvmax)) return rc;
    for (int v0 = 0; v0 < nvec; v0 += GB_NV) {
        const int nv = std::min(GB_NV, nvec-v0);
        const double *X = X_dev+(long long)v0*ldx;
        double *Y = Y_dev+(long long)v0*ldy;
        int rc;
        if (nv == 1) rc = spmv_group<1>(ctx, data_dev, diag_dev, nv, X, (long long)ldx, Y, (long long)ldy);
        else if (nv == 2) rc = spmv_group<2>(ctx, data_dev, diag_dev, nv, X, (long long)ldx, Y, (long long)ldy);
        else if (nv <= 4) rc = spmv_group<4>(ctx, data_dev, diag_dev, nv, X, (long long)ldx, Y, (long long)ldy);
        else if (nv <= 8) rc = spmv_group<8>(ctx, data_dev, diag_dev, nv, X, (long long)ldx, Y, (long long)ldy);
        else rc = spmv_group<16>(ctx, data_dev, diag_dev, nv, X, (long long)ldx, Y, (long long)ldy);
        if (rc) return rc;
    }
    return PNL_OK;
}

}  // extern "C"
