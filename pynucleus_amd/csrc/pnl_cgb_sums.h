// The grid rule and the fixed-shape dot products of the block Krylov solvers (pnl_cg_block.hip, pnl_bicgstab_block.hip): kernels over
// [nvec][n] blocks run cgb_blocks(n) = min(CGB_MAXBLK, ceil(n / 256)) workgroups of 256 threads, element i of every column in thread
// (i mod 256) of workgroup (i / 256) mod blocks.  A dot product is summed in a shape that depends on n only: per thread in ascending
// i (fma), the 64 lanes in the DPP tree of wave_sum, the four waves in ascending order (cgb_block_sums), the workgroups in 16
// interleaved runs in ascending order and those 16 in ascending order (cgb_totals).  No floating-point atomics.
// Both helpers keep their LDS in a function-local array: a kernel that calls one of them twice puts a barrier between the calls.
#pragma once
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int CGB_NV = PNL_CGB_MAXVEC;     // columns per group = vectors per pass of the block products
constexpr int CGB_THREADS = 256;
constexpr int CGB_MAXBLK = 256;            // workgroups per launch at most (one per CU)
constexpr int CGB_PART = CGB_MAXBLK*CGB_NV;
static_assert(CGB_NV == 16 && CGB_THREADS == 16*CGB_NV, "cgb_totals: 16 runs of partial sums x 16 columns");

inline int cgb_blocks(int n) { return std::min(CGB_MAXBLK, (n+CGB_THREADS-1)/CGB_THREADS); }

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

inline bool cgb_bad_block(const void *p, int64_t ld, int n) { return !p || ld < n; }

}  // namespace
