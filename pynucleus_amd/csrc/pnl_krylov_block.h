// What the block Krylov solvers share (pnl_cg_block.hip, pnl_mg_block.hip, pnl_bicgstab_block.hip): the grid rule, the fixed-shape dot
// products, the dot kernel, the argument check of the step entry points, the partial-sums scratch, the work-buffer layout and the host's
// record of the columns of a group.
//
// Kernels over [nvec][n] blocks run cgb_blocks(n) = min(CGB_MAXBLK, ceil(n / 256)) workgroups of 256 threads, element i of every column
// in thread (i mod 256) of workgroup (i / 256) mod blocks.  A dot product is summed in a shape that depends on n only: per thread in
// ascending i (fma), the 64 lanes in the DPP tree of wave_sum, the four waves in ascending order (cgb_block_sums), the workgroups in 16
// interleaved runs in ascending order and those 16 in ascending order (cgb_totals).  No floating-point atomics.
// Both helpers keep their LDS in a function-local array: a kernel that calls one of them twice puts a barrier between the calls.
//
// The per-column states of the solvers differ in width and meaning (PNL_CGB_STATE, PNL_BCGB_STATE doubles), but both keep the residual
// in slot KB_ST_RES and the active flag in slot KB_ST_ACTIVE: that is all the drivers read.
#pragma once
#include <initializer_list>
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int CGB_NV = PNL_CGB_MAXVEC;     // columns per group = vectors per pass of the block products
constexpr int CGB_THREADS = 256;
constexpr int CGB_MAXBLK = 256;            // workgroups per launch at most (one per CU)
constexpr int CGB_PART = CGB_MAXBLK*CGB_NV;
static_assert(CGB_NV == 16 && CGB_THREADS == 16*CGB_NV, "cgb_totals: 16 runs of partial sums x 16 columns");
constexpr int KB_ST_RES = 3, KB_ST_ACTIVE = 4;

inline int cgb_blocks(int n) { return std::min(CGB_MAXBLK, (n+CGB_THREADS-1)/CGB_THREADS); }
// a launch by the grid rule on the context's stream of a kernel whose first argument is n; KB_LAUNCH1: one workgroup, any arguments
#define KB_LAUNCH(kernel, ctx, n, ...) hipLaunchKernelGGL(kernel, dim3(cgb_blocks(n)), dim3(CGB_THREADS), 0, (ctx)->stream, n, __VA_ARGS__)
#define KB_LAUNCH1(kernel, ctx, ...) hipLaunchKernelGGL(kernel, dim3(1), dim3(CGB_THREADS), 0, (ctx)->stream, __VA_ARGS__)

// the workgroup's sums of the thread values s[v] for the columns of mask (0 for the others) -> row[0 .. 16)
__device__ __forceinline__ void cgb_block_sums(const double (&s)[CGB_NV], unsigned mask, double *__restrict__ row) {
    __shared__ double sw[CGB_THREADS/64][CGB_NV];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) {
        if ((mask >> v) & 1) {                     // uniform over the workgroup
            const double t = wave_sum(s[v]);
            if (lane == 0) sw[wv][v] = t;
        }
    }
    __syncthreads();
    if (tid < CGB_NV) row[tid] = ((mask >> tid) & 1) ? ((sw[0][tid]+sw[1][tid])+sw[2][tid])+sw[3][tid] : 0.;
}

// tot[v] = sum of part[k][v] over the nb workgroups, v < 16: thread (j, v) adds the run k = j, j + 16, ... in ascending order, then
// the 16 runs are added in ascending j.  Ends with a barrier: every thread may read tot.
__device__ __forceinline__ void cgb_totals(const double *__restrict__ part, int nb, double *tot) {
    __shared__ double sp[CGB_NV][CGB_NV+1];
    const int tid = threadIdx.x, v = tid & 15, j = tid >> 4;
    double s = 0.;
    for (int k = j; k < nb; k += 16) s += part[k*CGB_NV+v];
    sp[j][v] = s;
    __syncthreads();
    if (tid < CGB_NV) {
        double t = sp[0][tid];
#pragma unroll
        for (int jj = 1; jj < 16; jj++) t += sp[jj][tid];
        tot[tid] = t;
    }
    __syncthreads();
}

// bit v: column v < nv is active; STRIDE doubles of state per column
template <int STRIDE>
__device__ __forceinline__ unsigned kb_active_mask(const double *__restrict__ state, int nv) {
    unsigned m = 0;
    for (int v = 0; v < nv; v++) m |= state[v*STRIDE+KB_ST_ACTIVE] != 0. ? 1u << v : 0u;
    return m;
}

// partial sums of U . V per column and workgroup -> part[wg][16].  ALL: every column v < nv (a start: there is no state yet); else the
// active ones
template <int STRIDE, bool ALL>
__global__ void __launch_bounds__(CGB_THREADS)
k_kb_dot(int n, int nv, const double *__restrict__ U, long long ldu, const double *__restrict__ V, long long ldv,
         const double *__restrict__ state, double *__restrict__ part) {
    const unsigned mask = ALL ? (1u << nv)-1u : kb_active_mask<STRIDE>(state, nv);
    double s[CGB_NV];
#pragma unroll
    for (int v = 0; v < CGB_NV; v++) s[v] = 0.;
    for (int i = blockIdx.x*CGB_THREADS+threadIdx.x; i < n; i += gridDim.x*CGB_THREADS) {
#pragma unroll
        for (int v = 0; v < CGB_NV; v++)
            if ((mask >> v) & 1) s[v] = __builtin_fma(U[v*ldu+i], V[v*ldv+i], s[v]);
    }
    cgb_block_sums(s, mask, part+(size_t)blockIdx.x*CGB_NV);
}

// the context's scratch for the partial sums, [5][CGB_MAXBLK][16]: a step entry point fills and reads it within its own launches
inline int kb_part(pnl_context *ctx, double **part) {
    if (int rc = ensure(ctx, ctx->b_kb_part, sizeof(double)*5*CGB_PART)) return rc;
    *part = (double*)ctx->b_kb_part.p;
    return PNL_OK;
}

// ---- the argument check of the step entry points ---------------------------------------------------------------------------------
enum { KB_READ = 0, KB_WRITTEN = 1, KB_APART = 2, KB_OPTIONAL = 4 };    // APART: compared with no other block; OPTIONAL: may be null
struct KbBlock { const void *p; int64_t ld; int use; };

// n or nvec out of range; a block that is null (unless optional) or has ld < n; a written block that is also another block of the list;
// with reads_differ, two blocks that are only read and are the same
inline bool kb_bad_args(int n, int nvec, std::initializer_list<KbBlock> blocks, bool reads_differ = false) {
    if (n < 1 || nvec < 1 || nvec > CGB_NV) return true;
    for (const KbBlock *a = blocks.begin(); a != blocks.end(); a++) {
        if (a->p ? a->ld < n : !(a->use & KB_OPTIONAL)) return true;
        for (const KbBlock *b = blocks.begin(); b != a; b++)
            if (a->p && a->p == b->p && !((a->use | b->use) & KB_APART) && (reads_differ || ((a->use | b->use) & KB_WRITTEN))) return true;
    }
    return false;
}

// ---- the drivers' work buffer: a head, k blocks [gmax][ld] with an even ld, the state of 16 columns ---------------------------------
inline int64_t kb_ld(int n) { return ((int64_t)n+1) & ~(int64_t)1; }
inline size_t kb_work_bytes(int64_t head, int k, int gmax, int64_t ld, int stride) { return sizeof(double)*(size_t)(head+k*gmax*ld+CGB_NV*stride); }
struct KbCarve {
    double *p;
    int64_t step;                                  // gmax * ld
    double *next() { double *q = p; p += step; return q; }      // behind the last block: the state
};

// ---- the columns of one group on the host --------------------------------------------------------------------------------------------
// iters / residuals: the caller's outputs at the group's first column, or null.  The host reads the group's state once per pass.
template <int STRIDE>
struct KbColumns {
    pnl_context *ctx;
    const double *state;
    int nv, *iters;
    double *residuals;
    int nactive = 0;
    bool active[CGB_NV];
    double hs[CGB_NV*STRIDE];
    // it < 0: after the start, every column reports and the active ones are counted; else after pass `it`: the columns that are active
    // here and no longer on the device have converged (or broken down) in that pass
    int read(int it) {
        HIPCHK(ctx, hipMemcpyAsync(hs, state, sizeof(double)*nv*STRIDE, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int v = 0; v < nv; v++) {
            if (it >= 0 && !active[v]) continue;
            if (residuals) residuals[v] = hs[v*STRIDE+KB_ST_RES];
            const bool on = hs[v*STRIDE+KB_ST_ACTIVE] != 0.;
            if (it < 0) { active[v] = on; nactive += on; if (iters) iters[v] = 0; }
            else if (!on) { active[v] = false; nactive--; if (iters) iters[v] = it; }
        }
        return PNL_OK;
    }
    // at the end: the columns that are still active have used every pass
    void end(int maxiter) {
        for (int v = 0; v < nv; v++)
            if (active[v] && iters) iters[v] = maxiter;
    }
};

}  // namespace
