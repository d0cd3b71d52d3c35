// Internal, host only: the launch sequences that pnl_hip.hip and pnl_pwnear.hip share.  Include it behind pnl_kernels.h (the
// k_wl_* kernels) and pnl_context.h; every function is static, each translation unit launches its own copies of the kernels.
#pragma once
#include "pnl_dispatch.h"

// counting sort of a work list by order: histogram, offsets, cursors of the bins (PNL_WL_BINS + 1 words each, carved out of aux_base)
struct WlBins { unsigned *hist, *offs, *coff, *cursor; };
static int wl_sort(pnl_context *ctx, const int4 *wl, const unsigned *count, unsigned cap, unsigned *aux_base, int4 *sorted, WlBins &B) {
    B.hist = aux_base; B.offs = B.hist+(PNL_WL_BINS+1); B.coff = B.offs+(PNL_WL_BINS+1); B.cursor = B.coff+(PNL_WL_BINS+1);
    HIPCHK(ctx, hipMemsetAsync(B.hist, 0, sizeof(unsigned)*(PNL_WL_BINS+1), ctx->stream));
    hipLaunchKernelGGL(k_wl_hist, dim3(512), dim3(PNL_NTHREADS), 0, ctx->stream, wl, count, cap, B.hist);
    hipLaunchKernelGGL(k_wl_scan, dim3(1), dim3(64), 0, ctx->stream, (const unsigned*)B.hist, B.offs, B.coff, B.cursor);
    hipLaunchKernelGGL(k_wl_scatter, dim3(512), dim3(PNL_NTHREADS), 0, ctx->stream, wl, count, cap, (const unsigned*)B.offs, B.cursor, sorted);
    return PNL_OK;
}

// grid of a persistent tile kernel: as many workgroups as the occupancy query says are resident on the 256 CUs (per_cu_fallback
// where it fails), at most one per item; sets the kernel's dynamic LDS limit on the way.  rc != 0: that failed (ctx->err is set)
struct PersistentGrid { int rc, grid, per_cu; };
template <class K>
static PersistentGrid persistent_grid(pnl_context *ctx, K kfun, int threads, size_t lds, int nitems, int per_cu_fallback, int mult = 1) {
    const hipError_t e = hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return {fail(ctx, PNL_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e)), 0, 0};
    int per_cu = per_cu_fallback;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kfun, threads, lds);
    return {PNL_OK, pnl_grid_cap(std::min(nitems, 256*std::max(per_cu, 1)*std::max(mult, 1))), per_cu};
}
