// Linear combinations of m <= 21 dense blocks with host-side coefficients (gfx950 only): the device half of the operators
// interpolated in the fractional order (pynucleus_amd/linear_operators.py interpolationOperator).
//
// Reference: interpolationOperator / sumMultiplyOperator (base/PyNucleus_base/linear_operators.pyx:1261-1391): A(s) = sum_k w_k(s) A(s_k)
// over the operators assembled at the Chebyshev nodes of one interval; there the product is a loop of m matvecs and m axpys.  Here
//   pnl_gemv_multi   y = alpha (sum_k c_k A_k) x + beta b   without forming the sum:  m 8 n ld bytes per product,
//   pnl_lincomb      B = sum_k c_k A_k                       formed once:              (m + 1) 8 n ld bytes,
// both bound by HBM (m + 1 FMAs per 8 m bytes), both one stream over the m blocks.
//
// One wave per row, IP_ROWS = 4 rows per workgroup (the shape of k_gemv, pnl_solver.hip).  The columns of a row are taken in pairs:
// pair p = columns (2p, 2p + 1) belongs to lane p mod 64, which walks its pairs in ascending order.  Per sweep a lane loads the
// G(m) pairs p, p + 64, ... of ALL m blocks (16-byte non-temporal loads where the block is aligned), so m G(m) loads are in flight
// before the first FMA: G = 8, 4, 2, 1 for m = 1, 2-3, 4-7, 8-21, i.e. 128 to 336 bytes per lane and at most 42 data registers.  The
// pointers and coefficients are kernel arguments (a struct of 21 pointers and 21 doubles, read into SGPRs): no upload, no allocation per call.
//
// Arithmetic, the same on every path: the combined entry is t = c_0 a_0, t = fma(c_k, a_k, t) in ascending k; the product adds
// fma(t, x[col], acc) into the lane's accumulator of even or of odd columns in ascending column order, the two meet as acc0 + acc1,
// the lanes in the fixed DPP tree of wave_sum.  No atomics, nothing depends on the grid, on m's group size or on the alignment, so the
// result is bitwise reproducible and zero coefficients drop out exactly (c = (0, 1, 0) gives the bits of m = 1 on the middle block).
// Reading only the upper triangle of symmetric blocks would need column sums across workgroups, i.e. atomics (pnl_gemv2.hip): not done
// here; materialise the sum once and use pnl_gemv with symmetric_half = 2 for repeated products.
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int IP_ROWS = PNL_NTHREADS/64;           // rows per workgroup (one wave each)
constexpr int IP_PAIR = 2;                         // columns per lane and load
constexpr int IP_WAVE = 64*IP_PAIR;                // columns per wave and load

struct InterpArgs {
    const double *A[PNL_INTERP_MAX_OPS];
    double c[PNL_INTERP_MAX_OPS];
};

__host__ __device__ constexpr int ip_group(int m) { return m >= 8 ? 1 : (m >= 4 ? 2 : (m >= 2 ? 4 : 8)); }

typedef double ip_d2 __attribute__((ext_vector_type(2)));
template <bool AL>
__device__ __forceinline__ ip_d2 ip_load(const double *p) {
    if (AL) return __builtin_nontemporal_load((const ip_d2*)p);
    ip_d2 v;
    v.x = p[0]; v.y = p[1];
    return v;
}

// the combined entries of G pairs of one row: v[g] = sum_k c_k A_k[row][2 (p + 64 g) .. + 1], every load issued before the first FMA
template <int M, int G, bool AL>
__device__ __forceinline__ void ip_combine(const InterpArgs &P, long long off, ip_d2 (&t)[G]) {
    ip_d2 v[M][G];
#pragma unroll
    for (int k = 0; k < M; k++)
#pragma unroll
        for (int g = 0; g < G; g++) v[k][g] = ip_load<AL>(P.A[k]+off+IP_WAVE*g);
#pragma unroll
    for (int g = 0; g < G; g++) {
        t[g].x = P.c[0]*v[0][g].x;
        t[g].y = P.c[0]*v[0][g].y;
#pragma unroll
        for (int k = 1; k < M; k++) {
            t[g].x = __builtin_fma(P.c[k], v[k][g].x, t[g].x);
            t[g].y = __builtin_fma(P.c[k], v[k][g].y, t[g].y);
        }
    }
}

// the last column of a row with an odd number of columns
template <int M>
__device__ __forceinline__ double ip_combine_one(const InterpArgs &P, long long off) {
    double v[M];
#pragma unroll
    for (int k = 0; k < M; k++) v[k] = P.A[k][off];
    double t = P.c[0]*v[0];
#pragma unroll
    for (int k = 1; k < M; k++) t = __builtin_fma(P.c[k], v[k], t);
    return t;
}

template <int M, bool AL>
__device__ __forceinline__ double ip_row_dot(const InterpArgs &P, long long row_off, int ncols, const double *__restrict__ x, bool xal, int lane) {
    constexpr int G = ip_group(M);
    const int npairs = ncols >> 1;                    // complete pairs; an odd last column is taken alone
    double acc0 = 0., acc1 = 0.;
    int p = lane;
    for (; p+64*(G-1) < npairs; p += 64*G) {
        ip_d2 t[G];
        ip_combine<M, G, AL>(P, row_off+2*p, t);
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int j = 2*(p+64*g);
            ip_d2 xv;
            if (xal) xv = *(const ip_d2*)(x+j);
            else { xv.x = x[j]; xv.y = x[j+1]; }
            acc0 = __builtin_fma(t[g].x, xv.x, acc0);
            acc1 = __builtin_fma(t[g].y, xv.y, acc1);
        }
    }
    for (; p < npairs; p += 64) {
        ip_d2 t[1];
        ip_combine<M, 1, AL>(P, row_off+2*p, t);
        acc0 = __builtin_fma(t[0].x, x[2*p], acc0);
        acc1 = __builtin_fma(t[0].y, x[2*p+1], acc1);
    }
    if ((ncols & 1) && lane == (npairs & 63)) acc0 = __builtin_fma(ip_combine_one<M>(P, row_off+ncols-1), x[ncols-1], acc0);
    return wave_sum(acc0+acc1);
}

// y[row] = alpha * sum_j (sum_k c_k A_k[row][j]) x[j] + beta * b[row]   (b may be y)
template <int M>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_gemv_multi(const InterpArgs P, long long ldA, int nrows, int ncols, const double *__restrict__ x, double alpha, double beta, const double *b,
             double *y, int aligned) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x*IP_ROWS+(threadIdx.x >> 6);
    if (row >= nrows) return;
    const bool xal = (((uintptr_t)x) & 15) == 0;
    const long long off = (long long)row*ldA;
    const double s = aligned ? ip_row_dot<M, true>(P, off, ncols, x, xal, lane) : ip_row_dot<M, false>(P, off, ncols, x, xal, lane);
    if (lane == 0) y[row] = beta != 0. ? __builtin_fma(alpha, s, beta*b[row]) : alpha*s;
}

template <int M, bool AL, bool BAL>
__device__ __forceinline__ void ip_row_store(const InterpArgs &P, long long row_off, int ncols, double *__restrict__ brow, int lane) {
    constexpr int G = ip_group(M);
    const int npairs = ncols >> 1;
    int p = lane;
    for (; p+64*(G-1) < npairs; p += 64*G) {
        ip_d2 t[G];
        ip_combine<M, G, AL>(P, row_off+2*p, t);
#pragma unroll
        for (int g = 0; g < G; g++) {
            double *dst = brow+2*(p+64*g);
            if (BAL) __builtin_nontemporal_store(t[g], (ip_d2*)dst);
            else { dst[0] = t[g].x; dst[1] = t[g].y; }
        }
    }
    for (; p < npairs; p += 64) {
        ip_d2 t[1];
        ip_combine<M, 1, AL>(P, row_off+2*p, t);
        double *dst = brow+2*p;
        if (BAL) __builtin_nontemporal_store(t[0], (ip_d2*)dst);
        else { dst[0] = t[0].x; dst[1] = t[0].y; }
    }
    if ((ncols & 1) && lane == (npairs & 63)) brow[ncols-1] = ip_combine_one<M>(P, row_off+ncols-1);
}

// B[row][j] = sum_k c_k A_k[row][j], j < ncols (the padding columns of B are not touched)
template <int M>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_lincomb(const InterpArgs P, long long ldA, int nrows, int ncols, double *__restrict__ B, long long ldB, int aligned, int baligned) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x*IP_ROWS+(threadIdx.x >> 6);
    if (row >= nrows) return;
    const long long off = (long long)row*ldA;
    double *brow = B+(long long)row*ldB;
    if (aligned) {
        if (baligned) ip_row_store<M, true, true>(P, off, ncols, brow, lane);
        else ip_row_store<M, true, false>(P, off, ncols, brow, lane);
    } else {
        if (baligned) ip_row_store<M, false, true>(P, off, ncols, brow, lane);
        else ip_row_store<M, false, false>(P, off, ncols, brow, lane);
    }
}

template <int M>
void launch_gemv_multi(pnl_context *ctx, const InterpArgs &P, long long ldA, int nrows, int ncols, const double *x, double alpha, double beta,
                       const double *b, double *y, int aligned) {
    hipLaunchKernelGGL((k_gemv_multi<M>), dim3((nrows+IP_ROWS-1)/IP_ROWS), dim3(PNL_NTHREADS), 0, ctx->stream, P, ldA, nrows, ncols, x, alpha, beta,
                       b, y, aligned);
}

template <int M>
void launch_lincomb(pnl_context *ctx, const InterpArgs &P, long long ldA, int nrows, int ncols, double *B, long long ldB, int aligned,
                    int baligned) {
    hipLaunchKernelGGL((k_lincomb<M>), dim3((nrows+IP_ROWS-1)/IP_ROWS), dim3(PNL_NTHREADS), 0, ctx->stream, P, ldA, nrows, ncols, B, ldB, aligned,
                       baligned);
}

// the kernel of m blocks: one instantiation per m (the loads of all m blocks are unrolled into registers)
#define IP_CASE(M, CALL) case M: CALL<M>
#define IP_DISPATCH(m, CALL, ...)                                                                                            \
    switch (m) {                                                                                                             \
        IP_CASE(1, CALL)(__VA_ARGS__); break;   IP_CASE(2, CALL)(__VA_ARGS__); break;   IP_CASE(3, CALL)(__VA_ARGS__); break;   \
        IP_CASE(4, CALL)(__VA_ARGS__); break;   IP_CASE(5, CALL)(__VA_ARGS__); break;   IP_CASE(6, CALL)(__VA_ARGS__); break;   \
        IP_CASE(7, CALL)(__VA_ARGS__); break;   IP_CASE(8, CALL)(__VA_ARGS__); break;   IP_CASE(9, CALL)(__VA_ARGS__); break;   \
        IP_CASE(10, CALL)(__VA_ARGS__); break;  IP_CASE(11, CALL)(__VA_ARGS__); break;  IP_CASE(12, CALL)(__VA_ARGS__); break;  \
        IP_CASE(13, CALL)(__VA_ARGS__); break;  IP_CASE(14, CALL)(__VA_ARGS__); break;  IP_CASE(15, CALL)(__VA_ARGS__); break;  \
        IP_CASE(16, CALL)(__VA_ARGS__); break;  IP_CASE(17, CALL)(__VA_ARGS__); break;  IP_CASE(18, CALL)(__VA_ARGS__); break;  \
        IP_CASE(19, CALL)(__VA_ARGS__); break;  IP_CASE(20, CALL)(__VA_ARGS__); break;  IP_CASE(21, CALL)(__VA_ARGS__); break;  \
    }
static_assert(PNL_INTERP_MAX_OPS == 21, "IP_DISPATCH lists the cases 1 .. 21");

// the arguments both calls share: checked on the host before any launch; fills P and says whether every block may be read in 16-byte words
int ip_args(pnl_context *ctx, const char *who, int m, const double *const *A_dev, int64_t ldA, int nrows, int ncols, const double *coeffs,
            InterpArgs &P, int &aligned) {
    if (!ctx) return PNL_ERR_INVALID;
    if (m < 1 || m > PNL_INTERP_MAX_OPS) return fail(ctx, PNL_ERR_INVALID, "%s: m = %d operators (1 .. %d)", who, m, PNL_INTERP_MAX_OPS);
    if (!A_dev || !coeffs || nrows <= 0 || ncols <= 0 || ldA < ncols) return fail(ctx, PNL_ERR_INVALID, "%s: bad arguments", who);
    aligned = (ldA & 1) == 0;
    for (int k = 0; k < PNL_INTERP_MAX_OPS; k++) {
        P.A[k] = k < m ? A_dev[k] : nullptr;
        P.c[k] = k < m ? coeffs[k] : 0.;
        if (k < m && !A_dev[k]) return fail(ctx, PNL_ERR_INVALID, "%s: operator %d is a null pointer", who, k);
        if (k < m && (((uintptr_t)A_dev[k]) & 15)) aligned = 0;
    }
    return PNL_OK;
}

}  // namespace

int pnl_gemv_multi(pnl_context *ctx, int m, const double *const *A_dev, int64_t ldA, int nrows, int ncols, const double *coeffs_host,
                   const double *x_dev, double alpha, double beta, const double *b_dev, double *y_dev) {
    InterpArgs P;
    int aligned = 0;
    if (int rc = ip_args(ctx, "pnl_gemv_multi", m, A_dev, ldA, nrows, ncols, coeffs_host, P, aligned)) return rc;
    if (!x_dev || !y_dev || x_dev == y_dev || (beta != 0. && !b_dev)) return fail(ctx, PNL_ERR_INVALID, "pnl_gemv_multi: bad arguments");
    IP_DISPATCH(m, launch_gemv_multi, ctx, P, (long long)ldA, nrows, ncols, x_dev, alpha, beta, b_dev, y_dev, aligned);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_lincomb(pnl_context *ctx, int m, const double *const *A_dev, int64_t ldA, int nrows, int ncols, const double *coeffs_host,
                double *B_dev, int64_t ldB) {
    InterpArgs P;
    int aligned = 0;
    if (int rc = ip_args(ctx, "pnl_lincomb", m, A_dev, ldA, nrows, ncols, coeffs_host, P, aligned)) return rc;
    if (!B_dev || ldB < ncols) return fail(ctx, PNL_ERR_INVALID, "pnl_lincomb: bad arguments");
    for (int k = 0; k < m; k++)
        if (A_dev[k] == B_dev) return fail(ctx, PNL_ERR_INVALID, "pnl_lincomb: B is operator %d", k);
    const int baligned = (ldB & 1) == 0 && (((uintptr_t)B_dev) & 15) == 0;
    IP_DISPATCH(m, launch_lincomb, ctx, P, (long long)ldA, nrows, ncols, B_dev, (long long)ldB, aligned, baligned);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}
