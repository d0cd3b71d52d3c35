// Test hook pnl_selftest (include/pnl_hip.h): the device functions behind every kernel value and quadrature order -- pnl_log,
// pnl_exp, kern_eval on each of its paths, pw_scaling, quad_order_* -- evaluated one thread per input by the production code
// itself, with the DevKernel / PwDev / DevFormula built by the production host helpers (to_dev, to_dev_bkn, pow_table_values,
// pw_set_function).  tests/test_device_math.py compares them with mpmath.
#include "pnl_context.h"
// pnl_kernels.h defines its non-template kernels without `inline`: this translation unit keeps its copies in an unnamed namespace
namespace {
#include "pnl_pointwise.h"
}

namespace {

constexpr int ST_THREADS = 256;

template <int KT, bool BND>
__device__ __forceinline__ double st_value(const DevKernel &k, double d2, const double *ltab) {
    return kern_scale<KT>(k)*kern_eval<KT, BND>(k, d2, ltab);
}

// PATH < 0: kern_dispatch<-1 - PATH, INSIDE>, otherwise KT = PATH; the power tables (if any) in LDS as the tile kernels keep them
template <int PATH, bool INSIDE, bool BND>
__global__ void __launch_bounds__(ST_THREADS) k_st_kernel(DevKernel k, const double *__restrict__ tab, int n,
                                                          const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double s_pow[PNL_POW_TAB_DOUBLES];
    pnl_pow_tab_fill(s_pow, tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const double *ltab = tab ? s_pow : nullptr;
    const int i = blockIdx.x*blockDim.x+threadIdx.x;
    if (i >= n) return;
    const double d2 = in[i];
    if constexpr (PATH < 0) {
        kern_dispatch<-1-PATH, INSIDE>(k, ltab, [&](auto tag) { out[i] = st_value<decltype(tag)::value, BND>(k, d2, ltab); });
    } else {
        out[i] = st_value<PATH, BND>(k, d2, ltab);
    }
}

__global__ void __launch_bounds__(ST_THREADS) k_st_elementary(int op, int n, const double *__restrict__ in, double *__restrict__ out) {
    const int i = blockIdx.x*blockDim.x+threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    out[i] = op == PNL_SELFTEST_LOG ? pnl_log(x) : (op == PNL_SELFTEST_EXP ? pnl_exp(x) : pnl_exp_ranged(x));
}

template <int DIM>
__global__ void __launch_bounds__(ST_THREADS) k_st_scaling(PwDev W, int boundary, int n, const double *__restrict__ in,
                                                           double *__restrict__ out) {
    const int i = blockIdx.x*blockDim.x+threadIdx.x;
    if (i < n) out[i] = pw_scaling<DIM>(W, in[i], boundary != 0);
}

// in[7 i ..] = h1, h2, d2, ln h1, ln h2, |ln(h1/H0)|, |ln(h2/H0)| (the cell data of DevProblem::clog, computed on the host); the
// fp32 copies are made here as the tile kernels make them when they stage a tile
__global__ void __launch_bounds__(ST_THREADS) k_st_qorder(DevFormula F, int n, const double *__restrict__ in, double *__restrict__ out) {
    const int i = blockIdx.x*blockDim.x+threadIdx.x;
    if (i >= n) return;
    const double *a = in+7*(size_t)i;
    const double h1 = a[0], h2 = a[1], d2 = a[2], Ld1 = a[5], Ld2 = a[6];
    const float lh1 = (float)a[3], lh2 = (float)a[4], L1 = (float)Ld1, L2 = (float)Ld2;
    out[3*(size_t)i+0] = quad_order_exact(F, h1, h2, Ld1, Ld2, sqrt(d2));
    out[3*(size_t)i+1] = quad_order_try(F, lh1, lh2, L1, L2, d2);
    out[3*(size_t)i+2] = quad_order_fast(F, h1, h2, lh1, lh2, L1, L2, Ld1, Ld2, d2);
}

struct StBuf {
    void *p = nullptr;
    ~StBuf() { if (p) (void)hipFree(p); }
};

#define ST_CHK(call) do { if ((call) != hipSuccess) return PNL_ERR_HIP; } while (0)

template <int PATH, bool INSIDE>
void st_launch_kernel(bool bnd, int grid, const DevKernel &k, const double *tab, int n, const double *in, double *out) {
    if (bnd) k_st_kernel<PATH, INSIDE, true><<<grid, ST_THREADS>>>(k, tab, n, in, out);
    else k_st_kernel<PATH, INSIDE, false><<<grid, ST_THREADS>>>(k, tab, n, in, out);
}

}  // namespace

int pnl_selftest(int op, int path, int dim, int boundary, const void *param, int n, const double *in, double *out) {
    if (n < 0 || (n > 0 && (!in || !out)) || op < PNL_SELFTEST_LOG || op > PNL_SELFTEST_SETTLED_LAYOUT) return PNL_ERR_INVALID;
    if (op == PNL_SELFTEST_SETTLED_LAYOUT) {
        // the pairs of the threads of the mixed-tile kernel (pnl_device.h), on the host
        for (int i = 0; i < n; i++) {
            const int v = (int)in[i], tid = v >> 3, k = v & 7;
            if (v < 0 || tid >= 512) return PNL_ERR_INVALID;
            const int j = tid%64, r = tile_sweep_row(tid, k, 64, 512);
            out[3*(size_t)i] = r*64+j; out[3*(size_t)i+1] = tile_diag_cell(r, j, 64); out[3*(size_t)i+2] = j;
        }
        return PNL_OK;
    }
    if (op >= PNL_SELFTEST_KERNEL && !param) return PNL_ERR_INVALID;
    if (op >= PNL_SELFTEST_KERNEL && dim != 1 && dim != 2) return PNL_ERR_INVALID;
    if (n == 0) return PNL_OK;
    const int wout = op == PNL_SELFTEST_QORDER ? 3 : 1;
    std::vector<double> hin;
    if (op != PNL_SELFTEST_QORDER) hin.assign(in, in+n);
    else {
        // cell data as finalize stages it (ln h, |ln(h / H0)| per cell, pnl_setup.hip)
        hin.assign((size_t)7*n, 0.);
        for (int i = 0; i < n; i++) {
            const double h1 = in[4*i], h2 = in[4*i+1], d2 = in[4*i+2], H0 = in[4*i+3];
            double *a = &hin[7*(size_t)i];
            a[0] = h1; a[1] = h2; a[2] = d2;
            a[3] = std::log(h1); a[4] = std::log(h2);
            a[5] = std::fabs(std::log(h1/H0)); a[6] = std::fabs(std::log(h2/H0));
        }
    }
    StBuf din, dout, dtab;
    ST_CHK(hipMalloc(&din.p, sizeof(double)*hin.size()));
    ST_CHK(hipMalloc(&dout.p, sizeof(double)*(size_t)n*wout));
    ST_CHK(hipMemcpy(din.p, hin.data(), sizeof(double)*hin.size(), hipMemcpyHostToDevice));
    const int grid = (n+ST_THREADS-1)/ST_THREADS;
    const double *pin = (const double*)din.p;
    double *pout = (double*)dout.p;
    if (op <= PNL_SELFTEST_EXP_RANGED) {
        k_st_elementary<<<grid, ST_THREADS>>>(op, n, pin, pout);
    } else if (op == PNL_SELFTEST_KERNEL) {
        const pnl_kernel &kh = *(const pnl_kernel*)param;
        const bool bnd = boundary != 0;
        const DevKernel k = bnd ? to_dev_bkn(kh, dim) : to_dev(kh, dim);
        // power tables: those refresh_tables gives the interior kernel (the boundary tiles evaluate without), for the KT == 3 path
        // also those of a fast exponent (a launch over several order classes)
        std::vector<double> tab;
        const bool want = path == 3 ? pow_table_values(k, true, tab)
                                    : ((path == PNL_SELFTEST_DISPATCH || path == PNL_SELFTEST_DISPATCH+1) && !bnd && pow_table_values(k, false, tab));
        if (path == 3 && !want) return PNL_ERR_INVALID;
        if (want) {
            ST_CHK(hipMalloc(&dtab.p, sizeof(double)*tab.size()));
            ST_CHK(hipMemcpy(dtab.p, tab.data(), sizeof(double)*tab.size(), hipMemcpyHostToDevice));
        }
        const double *ptab = (const double*)dtab.p;
        const bool fast = k.fast != 0;
        switch (path) {
        case PNL_SELFTEST_DISPATCH:
            if (fast) st_launch_kernel<-2, false>(bnd, grid, k, ptab, n, pin, pout);
            else st_launch_kernel<-1, false>(bnd, grid, k, ptab, n, pin, pout);
            break;
        case PNL_SELFTEST_DISPATCH+1:
            if (fast) st_launch_kernel<-2, true>(bnd, grid, k, ptab, n, pin, pout);
            else st_launch_kernel<-1, true>(bnd, grid, k, ptab, n, pin, pout);
            break;
        case 0: st_launch_kernel<0, false>(bnd, grid, k, nullptr, n, pin, pout); break;
        case 3: st_launch_kernel<3, false>(bnd, grid, k, ptab, n, pin, pout); break;
        case 1: case 2: case 13: case 14: case 15: case 17:
            if (!fast || (path == 2 && k.qm != 6) || (path >= 10 && k.qm != path-10)) return PNL_ERR_INVALID;
            if (path == 1) st_launch_kernel<1, false>(bnd, grid, k, nullptr, n, pin, pout);
            else if (path == 2) st_launch_kernel<2, false>(bnd, grid, k, nullptr, n, pin, pout);
            else if (path == 13) st_launch_kernel<13, false>(bnd, grid, k, nullptr, n, pin, pout);
            else if (path == 14) st_launch_kernel<14, false>(bnd, grid, k, nullptr, n, pin, pout);
            else if (path == 15) st_launch_kernel<15, false>(bnd, grid, k, nullptr, n, pin, pout);
            else st_launch_kernel<17, false>(bnd, grid, k, nullptr, n, pin, pout);
            break;
        default: return PNL_ERR_INVALID;
        }
    } else if (op == PNL_SELFTEST_SCALING) {
        PwDev W;
        if (!pw_set_function(W, *(const pnl_order_function*)param)) return PNL_ERR_INVALID;
        if (dim == 1) k_st_scaling<1><<<grid, ST_THREADS>>>(W, boundary, n, pin, pout);
        else k_st_scaling<2><<<grid, ST_THREADS>>>(W, boundary, n, pin, pout);
    } else {
        k_st_qorder<<<grid, ST_THREADS>>>(to_dev(*(const pnl_order_formula*)param), n, pin, pout);
    }
    ST_CHK(hipGetLastError());
    ST_CHK(hipDeviceSynchronize());
    ST_CHK(hipMemcpy(out, dout.p, sizeof(double)*(size_t)n*wout, hipMemcpyDeviceToHost));
    return PNL_OK;
}
