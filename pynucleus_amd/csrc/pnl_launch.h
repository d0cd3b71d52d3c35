// Internal, host only: the launch sequences that pnl_hip.hip, pnl_sparse.hip and pnl_pwnear.hip share.  Include it behind
// pnl_context.h and pnl_kernels.h.  Every function is a static template that names template kernels only, so a unit gets exactly
// the instantiations it launches and none by including this file (the work-list sort, whose kernels are no templates, is the host
// function pnl_wl_sort of pnl_context.h).
#pragma once
#include "pnl_dispatch.h"

// grid of a persistent tile kernel: as many workgroups as the occupancy query says are resident on the 256 CUs (per_cu_fallback
// where it fails), at most one per item; sets the kernel's dynamic LDS limit on the way.  rc != 0: that failed (ctx->err is set)
struct PersistentGrid { int rc, grid, per_cu; };
template <class K>
static PersistentGrid persistent_grid(pnl_context *ctx, K kfun, int threads, size_t lds, int nitems, int per_cu_fallback) {
    const hipError_t e = hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return {fail(ctx, PNL_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e)), 0, 0};
    int per_cu = per_cu_fallback;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kfun, threads, lds);
    return {PNL_OK, pnl_grid_cap(std::min(nitems, 256*std::max(per_cu, 1))), per_cu};
}

// dynamic LDS of the work-list kernels: the rule copy (+ for P2 the column sums of the PNL_NTHREADS / 16 pairs of a chunk) of
// k_worklist_sorted; for P2 the per-lane column sums of k_worklist_lane (eval_distant_blocked)
template <int DPE>
static int wl_tab_max(int wl_kb) {
    // points of the largest rule that is staged; larger rules are read from global memory, point pair by point pair (slow: at 49,152
    // P2 cells of the 12-sector disc, s = 0.7, 100,000 near pairs take the rules of 240 and 256 points -- 6e9 of the 13e9 kernel values
    // of the work lists).  P2 (one workgroup per CU for its registers anyway): 320 ... 512 points, 80 + 128 bytes of LDS per point.
    const int t = (wl_kb*1024)/((4+DPE)*(int)sizeof(double));
    return wl_csum_lds(DPE) ? std::max(320, std::min(t, 512)) : t;
}
template <int DPE>
static size_t wl_sorted_lds(int tab_max) {
    return sizeof(double)*((size_t)tab_max*(4+DPE)+(wl_csum_lds(DPE) ? (size_t)(PNL_NTHREADS/16)*tab_max : 0));
}
template <typename F>
static size_t wl_lane_lds(F fun, int dpe, int kt) {
    const size_t b = wl_lane_blocked(dpe, kt) ? sizeof(double)*PNL_WL_LANE_MAXPTS*PNL_NTHREADS : 0;
    if (b) (void)hipFuncSetAttribute((const void*)fun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
    return b;
}

// sorted evaluation of a work list: the orders with at most PNL_WL_LANE_MAXPTS points one pair per lane (k_worklist_lane),
// the others 16 lanes per pair with the rule in LDS (k_worklist_sorted, up to bin last_bin); sym: dense output, both images of
// every entry (PNL_FLAG_SYMMETRIC_FLUSH, or behind the fold pass of the block-slot storage).  wl_kb: KB of LDS for the
// rule copy; rules with more points are read from global memory.  18 KB are 8 workgroups per CU
// (60 KB / 2 workgroups per CU was 0.6 ms slower at 98,304 cells in the dense path and 4 ms at C4 in the cluster path)
constexpr int WL_RULE_KB = 18;       // dense and cluster work lists
template <int DIM, int DPE, int KT, bool SPARSE>
static int worklist_eval(pnl_context *ctx, int wl_kb, const int4 *sorted, const WlBins &B, double *A, int64_t ldA,
                  double *D, const SparseOut &S, const ClusterTiles &CT, int last_bin, bool sym) {
    const int tab_max = wl_tab_max<DPE>(wl_kb);
    const int wl_grid = 256*std::max(1, std::min(8, 150/(wl_kb+(KT == 0 ? 3 : 0))));      // KT == 0: + 3 KB of power tables
    const size_t lds = wl_sorted_lds<DPE>(tab_max);
    auto wfun = k_worklist_sorted<DIM, DPE, KT, SPARSE>;
    HIPCHK(ctx, hipFuncSetAttribute((const void*)wfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_worklist_lane<DIM, DPE, KT, SPARSE>), dim3(256*4), dim3(PNL_NTHREADS), wl_lane_lds(k_worklist_lane<DIM, DPE, KT, SPARSE>, DPE, KT), ctx->stream, ctx->P,
                       sorted, (const unsigned*)B.offs, A, (long long)ldA, D, S, sym ? 8 : 0, CT);
    hipLaunchKernelGGL(wfun, dim3(wl_grid), dim3(PNL_NTHREADS), lds, ctx->stream, ctx->P, sorted, (const unsigned*)B.offs,
                       (const unsigned*)B.coff, A, (long long)ldA, D, tab_max, S, last_bin, (PNL_WL_LANE_MAXPTS+1) | (sym ? 1 << 16 : 0), CT);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// touching pairs (k_singular_pairs): the rule of the slot staged in LDS if it needs at most 150 KB, else read from global memory;
// at most 256 * min(workgroups per CU, 4) workgroups, fewer if `want` (the site's own count) is smaller; INT_MAX selects that
// fixed grid (the sparse path, whose pairs are counted on the device)
template <int DIM, int DPE, int SLOT, int KT, bool SPARSE>
static int launch_singular_pairs(pnl_context *ctx, int want, const int2 *pairs, int np, double *A, int64_t ldA, int cell_begin, int cell_end,
                          const SparseOut &S, const int4 *sorted, const unsigned *offs, const ClusterTiles &CT) {
    const int M = ctx->P.sM[SLOT], rows = ctx->P.sRows[SLOT];
    const size_t lds = sizeof(double)*(size_t)(2*(DIM+1)+1+rows)*M;
    const bool stage = lds <= 150*1024;
    const int per_cu = stage ? std::max(1, (int)((160*1024)/std::max<size_t>(lds, 1))) : 4;
    const int grid = std::min(want, 256*std::min(per_cu, 4));
    auto launch = [&](auto kfun, size_t bytes) {
        hipLaunchKernelGGL(kfun, dim3(grid), dim3(PNL_SING_THREADS), bytes, ctx->stream, ctx->P, pairs, np, A, (long long)ldA, cell_begin,
                           cell_end, S, sorted, offs, CT);
    };
    if (stage) {
        auto kfun = k_singular_pairs<DIM, DPE, SLOT, KT, true, SPARSE>;
        HIPCHK(ctx, hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        launch(kfun, lds);
    } else launch(k_singular_pairs<DIM, DPE, SLOT, KT, false, SPARSE>, 0);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}
