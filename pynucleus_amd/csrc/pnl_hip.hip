// libpnl_hip.so -- the assemblies that share the SPARSE = false work-list, the touching-pair and the k_boundary_items
// instantiations of pnl_kernels.h / pnl_bndtile.h (gfx950 only): dense tiles with their work lists, touching pairs and boundary
// term (assemble_impl behind pnl_assemble_dense / pnl_assemble_dense_tiles), masked boundary items, cluster tiles of the near
// field; next to them the kernels that are no templates (k_mirror, the work-list sort) and the launch of k_tile_order_range
// for the tile plan.  Launches on the caller's stream and the side streams of the context.  Context, uploads, finalize() and the
// tile plan are host code of pnl_setup.hip; what the two units ask of each other is declared in pnl_context.h.
#include "pnl_context.h"
#include "pnl_kernels.h"
#include "pnl_bndtile.h"
#include "pnl_launch.h"

namespace {

// A <- A + A^T on the strict off-diagonal (cross contributions were written on one side only)
__global__ void __launch_bounds__(PNL_NTHREADS)
k_mirror(double *__restrict__ A, long long ldA, int N) {
    __shared__ double t1[32][33], t2[32][33];
    const int nb = (N+31)/32;
    // linear block id over the upper block triangle
    int bid = blockIdx.x;
    int bi = 0;
    {
        // solve bi from bid = bi*nb - bi(bi-1)/2 + (bj-bi)
        double fb = ((2.*nb+1.)-sqrt((2.*nb+1.)*(2.*nb+1.)-8.*bid))*0.5;
        bi = (int)fb;
        while (bi > 0 && (long long)bi*nb-(long long)bi*(bi-1)/2 > bid) bi--;
        while ((long long)(bi+1)*nb-(long long)(bi+1)*bi/2 <= bid) bi++;
    }
    const int bj = bi+(bid-(int)((long long)bi*nb-(long long)bi*(bi-1)/2));
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int I = bi*32+r, J = bj*32+tx;
        t1[r][tx] = (I < N && J < N) ? A[(long long)I*ldA+J] : 0.;
        const int I2 = bj*32+r, J2 = bi*32+tx;
        t2[r][tx] = (I2 < N && J2 < N) ? A[(long long)I2*ldA+J2] : 0.;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int I = bi*32+r, J = bj*32+tx;
        if (I < N && J < N) {
            if (bi != bj) A[(long long)I*ldA+J] = t1[r][tx]+t2[tx][r];
            else if (r != tx) A[(long long)I*ldA+J] = t1[r][tx]+t1[tx][r];
        }
        const int I2 = bj*32+r, J2 = bi*32+tx;
        if (bi != bj && I2 < N && J2 < N) A[(long long)I2*ldA+J2] = t2[r][tx]+t1[tx][r];
    }
}

// the per-cell diagonal blocks D (packed upper triangles, cells of P) into the dense matrix / into the sparse data
template <int DPE>
void scatter_diag(pnl_context *ctx, const DevProblem &P, const double *D, double *A, int64_t ldA) {
    const long long nt = (long long)ctx->nc*DPE*DPE;
    hipLaunchKernelGGL((k_scatter_diag<DPE>), dim3((unsigned)((nt+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0, ctx->stream, P, D,
                       A, (long long)ldA);
}

template <int DIM, int DPE, int KT>
int launch_pure(pnl_context *ctx, double *A, int64_t ldA, const SlotOut &SO) {
    if (ctx->run.n_pure == 0) return PNL_OK;
    constexpr int NP = DIM == 2 ? 3 : 2, ND = DPE*(DPE+1)/2;
    const int acc_stride = acc_stride_of(ctx->nU);
    const size_t lds = sizeof(double)*(64*NP*DIM+64+2*64*ND+NP*(4+DPE)+(KT == 0 ? PNL_POW_TAB_DOUBLES : 0))+sizeof(int)*(64*DPE+64)
                       +sizeof(double)*(size_t)(ctx->nU+1)*acc_stride;
    auto kfun = k_tile_pure<DIM, DPE, KT>;
    const PersistentGrid g = persistent_grid(ctx, kfun, PNL_NTHREADS, lds, ctx->run.n_pure, 2);
    if (g.rc) return g.rc;
    if (pnl_tune("PNL_VERBOSE")) fprintf(stderr, "[pnl] uniform tiles=%d of %d, lds=%zu bytes, occupancy API: %d blocks/CU\n", ctx->run.n_pure,
                                       ctx->run.n_pure+ctx->run.n_mixed, lds, g.per_cu);
    kt_begin(ctx, PNL_K_TILE_UNIFORM2);
    hipLaunchKernelGGL(kfun, dim3(g.grid), dim3(PNL_NTHREADS), lds, ctx->stream, tile_problem(ctx), (const int2*)ctx->b_tiles.p+ctx->run.tile_off+ctx->run.n_mixed,
                       ctx->run.n_pure, A, (long long)ldA, (double*)(ctx->have_tile_order ? ctx->b_Dt.p : ctx->b_D.p), acc_stride, 2,
                       ctx->run.symflush ? 1 : 0, SO);
    kt_end(ctx, PNL_K_TILE_UNIFORM2);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// The per-class passes of a variable order run on side streams (pnl_context::aux): fork from the caller's stream, class k on
// stream k mod NAUX (ctx->stream is redirected through `scope` while a class is being launched), join back.  One class: nothing happens.
struct ClassFork {
    pnl_context *ctx;
    StreamScope scope;                  // scope.prev: the stream the fork was made on
    bool on, used[pnl_context::NAUX] = {};
    hipEvent_t start;
    // from: an event recorded earlier on the caller's stream (the fold pass) -- the side streams start there instead of behind
    // everything the caller's stream holds, so consecutive forked phases run back to back on every side stream
    ClassFork(pnl_context *c, int nclasses, hipEvent_t from = nullptr)
        : ctx(c), scope(c, c->stream), on(nclasses > 1 && !pnl_tune("PNL_NO_FORK")), start(from ? from : c->ev_fork) {
        if (on && !from) (void)hipEventRecord(ctx->ev_fork, scope.prev);
    }
    // classes of very different weight (three layers: the pairs inside a layer against the few across an interface): heaviest first
    // onto the least loaded stream, so that two heavy classes do not queue behind each other while a stream of light ones runs dry
    std::vector<int> slot;
    void plan(const std::vector<int> &weight) {
        const int n = (int)weight.size();
        std::vector<int> order(n);
        for (int k = 0; k < n; k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight[a] > weight[b]; });
        long long load[pnl_context::NAUX] = {};
        slot.assign(n, 0);
        for (int k : order) {
            int best = 0;
            for (int j = 1; j < pnl_context::NAUX; j++) if (load[j] < load[best]) best = j;
            slot[k] = best; load[best] += std::max(1, weight[k]);
        }
    }
    void use(int k) {
        if (!on) return;
        const int j = k < (int)slot.size() ? slot[k] : k % pnl_context::NAUX;
        if (!used[j]) { (void)hipStreamWaitEvent(ctx->aux[j], start, 0); used[j] = true; }
        scope.to(ctx->aux[j]);
    }
    void join() {
        if (!on) return;
        scope.to(scope.prev);
        for (int j = 0; j < pnl_context::NAUX; j++)
            if (used[j]) {
                (void)hipEventRecord(ctx->ev_join[j], ctx->aux[j]);
                (void)hipStreamWaitEvent(scope.prev, ctx->ev_join[j], 0);
                used[j] = false;
            }
        on = false;
    }
    ~ClassFork() { join(); }
};

// counting sort of a work-list region by order, then the sorted evaluation;
// region: which copy of the sort buffers to use (passes that may run concurrently need their own)
template <int DIM, int DPE, int KT>
int run_worklist(pnl_context *ctx, const int4 *wl, const unsigned *wlc, unsigned cap, double *A, int64_t ldA, bool sym, int region = 0,
                 int nregions = 1) {
    int rc;
    if ((rc = ensure(ctx, ctx->b_wlsorted, (size_t)cap*nregions*sizeof(int4)))) return rc;
    if ((rc = ensure(ctx, ctx->b_wlaux, sizeof(unsigned)*(4*(PNL_WL_BINS+1))*nregions))) return rc;
    const int4 *wlsorted = (const int4*)ctx->b_wlsorted.p+(size_t)region*cap;
    WlBins B;
    if ((rc = pnl_wl_sort(ctx, wl, wlc, cap, (unsigned*)ctx->b_wlaux.p+(size_t)region*4*(PNL_WL_BINS+1), (int4*)wlsorted, B))) return rc;
    return worklist_eval<DIM, DPE, KT, false>(ctx, WL_RULE_KB, wlsorted, B, A, ldA, (double*)ctx->b_D.p, SparseOut{}, ClusterTiles{}, PNL_WL_BINS-1, sym);
}

// work list for the orders that are integrated one pair per wave: `regions` regions of equal capacity, sized generously;
// an overflow is detected (check_overflow)
int ensure_worklist(pnl_context *ctx, double pairs, int regions) {
    const double frac = pnl_tune("PNL_WL_FRAC") ? atof(pnl_tune("PNL_WL_FRAC")) : 0.05;
    const double floor_entries = pnl_tune("PNL_WL_FRAC") ? 64. : (double)(1 << 20);
    const size_t each = (size_t)std::min<double>(std::max<double>(pairs*frac, floor_entries), 400e6);
    int rc;
    if ((rc = ensure(ctx, ctx->b_wl, each*(size_t)regions*sizeof(int4)))) return rc;
    ctx->wl_cap = (unsigned)std::min<size_t>(ctx->b_wl.bytes/sizeof(int4), 0xffffffffu);
    ctx->wl_cap_each = (unsigned)each;
    if ((rc = ensure(ctx, ctx->b_tilectr, sizeof(unsigned)))) return rc;
    return PNL_OK;
}

// the mixed tiles of the current class (k_tile_distant): one region of the work list, reused by every class / orientation pass; the
// fill counter wlc of pass p stays in slot p (check_overflow).
// The plan lists the unsettled tiles first, then the settled ones with their pair codes in b_codes (pnl_setup.hip).  An assembly that
// writes the block-slot storage of the whole operator (one rank, symmetric, no PNL_FLAG_SYMMETRIC_FLUSH) runs the unsettled tiles
// -- they fill the work list --, then the settled ones through the SETTLED instantiation with a ticket counter of its own; every
// other assembly takes the whole list through the classifying kernel.  Where the plan also holds the pair lists of the settled tiles
// (b_lists; not with the option PNL_SETTLED_CODES) the settled launch is the LISTS instantiation, which reads the records instead of the codes.
template <int DIM, int DPE, int TILE, int KT, bool SETTLED = false>
int launch_mixed_tiles(pnl_context *ctx, unsigned *wlc, double *A, int64_t ldA, int cell_begin, int cell_end, const SlotOut &SO) {
    using S = TileSmem<DIM, DPE, TILE, KT == 0>;
    // the SETTLED instantiations: every KT the dense 2D P1 launcher dispatches
    constexpr bool can_settle = DIM == 2 && DPE == 3 && TILE == 64;
    int ntiles = ctx->run.n_mixed, first = 0, ns = 0;
    unsigned *ctr = (unsigned*)ctx->b_tilectr.p;
    if (can_settle && ctx->cls.size() == 1 && SO.A2 && !ctx->run.symflush && !ctx->nonsym && ctx->b_codes.p && cell_begin <= 0 && cell_end >= ctx->nc)
        ns = std::min(ctx->n_settled, ntiles);
    if (SETTLED) {
        first = ntiles-ns; ntiles = ns;
        // a ticket counter of the block the assembly zeroed at its start, like the uniform-tile launches (pnl_tile2.hip)
        ctr = (unsigned*)ctx->b_unictr.p+ctx->run.uni_ctr_next;
        ctx->run.uni_ctr_next = (ctx->run.uni_ctr_next+1)%pnl_context::UNI_CTRS;
        if (ctx->run.uni_ctr_fresh > 0) ctx->run.uni_ctr_fresh--;
        else HIPCHK(ctx, hipMemsetAsync(ctr, 0, sizeof(unsigned), ctx->stream));
    } else {
        ntiles -= ns;
        ctx->run.settled_run = ns;
        HIPCHK(ctx, hipMemsetAsync(ctr, 0, sizeof(unsigned), ctx->stream));
    }
    const int acc_stride = acc_stride_of(ctx->nU, S::fixed_bytes);
    const size_t lds = S::fixed_bytes+sizeof(double)*(size_t)(ctx->nU+1)*acc_stride;
    if (lds > 160*1024)
        return fail(ctx, PNL_ERR_UNSUPPORTED, "a block of %d cells touches %d DoFs: LDS sub-block of %zu bytes exceeds 160 KiB "
                    "(cells must be numbered with spatial locality)", TILE, ctx->nU, lds);
    auto kfun = k_tile_distant<DIM, DPE, TILE, KT, false, false, SETTLED>;
    const unsigned short *codes = SETTLED ? (const unsigned short*)ctx->b_codes.p : (const unsigned short*)nullptr;
    if constexpr (can_settle && SETTLED) {
        if (ctx->b_lists.p) {
            kfun = k_tile_distant<DIM, DPE, TILE, KT, false, false, true, true>;
            codes = (const unsigned short*)ctx->b_lists.p;
            ctx->run.lists_run = ns;
        }
    }
    const PersistentGrid g = persistent_grid(ctx, kfun, tile_threads(DPE), lds, ntiles, 2);
    if (g.rc) return g.rc;
    if (pnl_tune("PNL_VERBOSE"))
        fprintf(stderr, "[pnl] %stiles=%d nU=%d lds=%zu bytes, occupancy API: %d blocks/CU\n", SETTLED ? "settled " : "", ntiles, ctx->nU, lds, g.per_cu);
    SlotOut SOk = SO;
    SOk.nU = ctx->nU;                                       // rows of the LDS sub-block (also without the block-slot storage)
    // the time of the settled launch counts for the mixed-tile kernel and is reported on its own as well
    kt_begin(ctx, PNL_K_TILE_GENERAL);
    if (SETTLED) kt_begin(ctx, PNL_K_TILE_SETTLED);
    if (g.grid > 0)
        hipLaunchKernelGGL(kfun, dim3(g.grid), dim3(tile_threads(DPE)), lds, ctx->stream, with_mixed_rules(ctx, tile_problem(ctx)),
                           (const int2*)ctx->b_tiles.p+ctx->run.tile_off+first, A,
                           (long long)ldA, (double*)(ctx->have_tile_order ? ctx->b_Dt.p : ctx->b_D.p), cell_begin, cell_end, acc_stride, (int4*)ctx->b_wl.p,
                           wlc, ctx->wl_cap_each, ctx->run.symflush ? 256 : 0, ntiles, ClusterTiles{},
                           ctr, SOk, codes);
    if (SETTLED) kt_end(ctx, PNL_K_TILE_SETTLED);
    kt_end(ctx, PNL_K_TILE_GENERAL);
    HIPCHK(ctx, hipGetLastError());
    if constexpr (can_settle && !SETTLED) {
        if (ns > 0) return launch_mixed_tiles<DIM, DPE, TILE, KT, true>(ctx, wlc, A, ldA, cell_begin, cell_end, SO);
    }
    return PNL_OK;
}

template <int DIM, int DPE, int TILE, int KT>
int launch_tiles(pnl_context *ctx, int wl_slot, double *A, int64_t ldA, int cell_begin, int cell_end, const SlotOut &SO = SlotOut{}) {
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    ctx->run.pure_launched = false;              // of this class pass
    if (TILE == 64 && DPE <= 3) {
        int rc;
        // order-2 uniform tiles: 2D P1 the pipelined k_tile_uniform<3, 3> (with three or four workgroups per CU it beats k_tile_pure:
        // 41.3 against 45.5 ms at 98,304 cells, s = 1/2), where the order-2 rule has its three points; else and in 1D k_tile_pure
        if (DIM == 2 && DPE == 3 && ctx->uni_off[2] >= 0 && ctx->uni_np[2] == 3)
            rc = pnl2_launch_uniform(ctx, KT, tile_problem(ctx), (const int2*)ctx->b_tiles.p+ctx->run.tile_off+ctx->run.n_mixed, nullptr, ctx->run.n_pure, 2,
                                     A, ldA, (double*)(ctx->have_tile_order ? ctx->b_Dt.p : ctx->b_D.p), SO);
        else rc = launch_pure<DIM, (DPE <= 3 ? DPE : 3), KT>(ctx, A, ldA, SO);
        if (rc) return rc;
        ctx->run.pure_launched = ctx->run.n_pure > 0;
        if (DIM == 2 && DPE == 3) {
            // tiles whose pairs are all of order 3 / all of order 4 (6-point rules): pnl_tile2.h
            int off = ctx->run.tile_off+ctx->run.n_mixed+ctx->run.n_pure;
            for (int q = 3; q <= 4; q++) {
                const int n = ctx->cls_n_uni[q-2][ctx->cur];
                if ((rc = pnl2_launch_uniform(ctx, KT, tile_problem(ctx), (const int2*)ctx->b_tiles.p+off, nullptr, n, q, A, ldA,
                                              (double*)(ctx->have_tile_order ? ctx->b_Dt.p : ctx->b_D.p), SO))) return rc;
                ctx->run.pure_launched = ctx->run.pure_launched || n > 0;
                off += n;
            }
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    }
    unsigned *wlc = (unsigned*)ctx->b_wlcount.p+wl_slot;
    if (int rc = launch_mixed_tiles<DIM, DPE, TILE, KT>(ctx, wlc, A, ldA, cell_begin, cell_end, SO)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_DONE], ctx->stream));
    // block-slot storage: A = A' + A'^T is formed now (it overwrites A); the work-list kernels then write both images
    if (SO.A2) {
        if (int rc = pnl2_fold_mirror(ctx, SO, A, ldA)) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev_fold, ctx->stream));
        ctx->run.fold_event_set = true;
    }
    return run_worklist<DIM, DPE, KT>(ctx, (const int4*)ctx->b_wl.p, wlc, ctx->wl_cap_each, A, ldA, ctx->run.symflush || SO.A2 != nullptr);
}

template <int DIM, int DPE, int KT>
int launch_singular(pnl_context *ctx, double *A, int64_t ldA, int cell_begin, int cell_end) {
    for (int s = 0; s < DIM+1; s++) {
        const int np = ctx->orient ? ctx->C().n_spairs1[s] : ctx->C().n_spairs[s];
        if (!np) continue;
        if (!ctx->C().have_sing[0][s]) return fail(ctx, PNL_ERR_STATE, "singular rule for %d common vertices not uploaded", s+1);
        const int wpb = PNL_SING_THREADS/64;
        int rc = with_slot<DIM>(s, [&](auto slot) {
            constexpr int SLOT = decltype(slot)::value;
            const int2 *pairs = (const int2*)(ctx->orient ? ctx->C().b_spairs1[SLOT].p : ctx->C().b_spairs[SLOT].p);
            return launch_singular_pairs<DIM, DPE, SLOT, KT, false>(ctx, (np+wpb-1)/wpb, pairs, np, A, ldA, cell_begin, cell_end, SparseOut{},
                                                                    nullptr, nullptr, ClusterTiles{});
        });
        if (rc) return rc;
    }
    return PNL_OK;
}

// what: 1 distant pairs, 2 touching pairs, 3 both; bkcls / bfcls: class tables for the one-launch distant pass of a variable order
template <int DIM, int DPE, int KT>
int launch_boundary(pnl_context *ctx, int cell_begin, int cell_end, int what = 3, const DevKernel *bkcls = nullptr,
                    const DevFormula *bfcls = nullptr, bool all_fast = false) {
    if (ctx->nb == 0 || cell_end <= cell_begin) return PNL_OK;
    const int ncell = cell_end-cell_begin;
    const int gx = (ncell+PNL_NTHREADS-1)/PNL_NTHREADS;
    // small facet chunks: many waves in flight hide the latency of the per-facet dependent chain
    // a rank's share of the cells may be small: shrink the facet chunks until the grid has a few thousand workgroups
    // (measured at 98,304 cells x 768 facets: 16 per chunk 5.4 ms, 32 per chunk 4.5 ms, 64 the same; 8: 6.9 ms, 1: 33.6 ms)
    int per = 32;
    while (per > 1 && (long long)gx*((ctx->nb+per-1)/per) < 4096) per >>= 1;
    const int chunks = (ctx->nb+per-1)/per;
    if (what & 1) {
        // pairs with more than `defer` point pairs are integrated one per wave (k_boundary_items) instead of by one lane; the
        // list holds at least 64 items per facet -- pairs that do not fit are integrated in place
        constexpr int defer = 48;
        const unsigned cap = (unsigned)std::min<long long>(std::max<long long>(65536, 64ll*ctx->nb), 1ll << 24);
        if (int rc = ensure(ctx, ctx->b_bdefer, sizeof(int)*(size_t)cap*(3+DIM)+sizeof(unsigned))) return rc;
        int *dcells = (int*)ctx->b_bdefer.p, *dfacets = dcells+cap;
        unsigned *dslots = (unsigned*)(dfacets+(size_t)cap*DIM);
        int *dcls = (int*)(dslots+cap);
        unsigned *dcount = (unsigned*)(dcls+cap);
        HIPCHK(ctx, hipMemsetAsync(dcount, 0, sizeof(unsigned), ctx->stream));
        const bool fast = bkcls ? all_fast : (ctx->P.bkn.fast != 0);
        bool tiled = false;
        if constexpr (DIM == 2) {
            // tiled kernel (pnl_bndtile.h): 256 cells per workgroup, facets in LDS chunks of 64, rules up to order qi in LDS
            const int qi = std::min(PNL_BT_QI, ctx->qmax);
            if (!pnl_tune("PNL_BND_OLD") && qi >= 2 && (int)ctx->rule_off.size() > qi+1) {
                const int npts = ctx->rule_off[qi+1]-ctx->rule_off[2], nfp = ctx->frule_off[qi+1]-ctx->frule_off[2];
                const int ncls = bkcls ? (int)ctx->cls.size() : 0;
                const BndTileLds LY = bnd_tile_layout(npts, nfp, 4+DPE, ncls);
                const size_t lds = sizeof(double)*(size_t)LY.total;
                if (lds <= 64*1024) {
                    // facet blocks: enough workgroups to fill the chip (a rank's share of the cells may be small), whole chunks of 64
                    const int nfb = (ctx->nb+PNL_BT_FB-1)/PNL_BT_FB;
                    constexpr int want = 2048;
                    const int gy = std::max(1, std::min(nfb, (want+gx-1)/gx));
                    const int per_block = ((nfb+gy-1)/gy)*PNL_BT_FB;
                    const int gyy = (ctx->nb+per_block-1)/per_block;
                    auto launch = [&](auto kfun) {
                        (void)hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                        hipLaunchKernelGGL(kfun, dim3(gx, gyy), dim3(PNL_NTHREADS), lds, ctx->stream, ctx->P, (double*)ctx->b_D.p, cell_begin,
                                           cell_end, per_block, qi, bkcls, bfcls, ncls, defer, dcells, dfacets, dslots, dcount, cap, dcls);
                    };
                    if (fast) launch(k_boundary_tile<DIM, DPE, 1>); else launch(k_boundary_tile<DIM, DPE, 0>);
                    tiled = true;
                }
            }
        }
        // one dispatch per kernel: both instantiations of a kernel are named together, in the order the code object has them
        if (!tiled) with_kt(fast, [&](auto kt) {
            hipLaunchKernelGGL((k_boundary_distant<DIM, DPE, decltype(kt)::value>), dim3(gx, chunks), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P,
                               (double*)ctx->b_D.p, cell_begin, cell_end, per, bkcls, bfcls, defer, dcells, dfacets, dslots, dcount, cap, dcls);
            return PNL_OK;
        });
        with_kt(fast, [&](auto kt) {
            hipLaunchKernelGGL((k_boundary_items<DIM, DPE, decltype(kt)::value>), dim3(256*4), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P,
                               (const double*)ctx->b_vertices.p, (const int*)dcells, (const int*)dfacets, (const unsigned*)dslots, (int)cap, 1.,
                               SparseOut{}, (double*)ctx->b_D.p, (const unsigned*)dcount, bkcls ? (const int*)dcls : nullptr, bkcls, bfcls);
            return PNL_OK;
        });
        HIPCHK(ctx, hipGetLastError());
    }
    if (what & 2)
    for (int s = 0; s < DIM; s++) {
        const int np = ctx->C().n_bpairs[s];
        if (!np) continue;
        if (!ctx->C().have_sing[1][s]) return fail(ctx, PNL_ERR_STATE, "boundary singular rule for %d common vertices not uploaded", s+1);
        const int grid = (np+3)/4;
        const int2 *pairs = (const int2*)ctx->C().b_bpairs[s].p;
        auto launch = [&](auto kfun) {
            hipLaunchKernelGGL(kfun, dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, pairs, np, (double*)ctx->b_D.p, cell_begin, cell_end);
            return PNL_OK;
        };
        const bool fast = ctx->P.bkn.fast != 0;
        if (s == 0) with_kt(fast, [&](auto kt) { return launch(k_boundary_singular<DIM, DPE, 0, decltype(kt)::value>); });
        else with_kt(fast, [&](auto kt) { return launch(k_boundary_singular<DIM, DPE, (DIM == 2 ? 1 : 0), decltype(kt)::value>); });
        HIPCHK(ctx, hipGetLastError());
    }
    return PNL_OK;
}

// block-slot storage of the one-sided operator (pnl_tile2.h): allocated when the device has room for it next to the caller's matrix
bool slot_storage_ready(pnl_context *ctx) {
    if (ctx->nonsym) return false;
    size_t free_b = 0, total_b = 0;
    const size_t need = sizeof(double)*(size_t)ctx->slot_total;
    if (ctx->b_slotA.bytes >= need) return true;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b <= need+(size_t(2) << 30)) return false;
    return ensure(ctx, ctx->b_slotA, need) == PNL_OK;
}

// dim 2, dpe 6: ONE launch of the uniform-tile kernels per order and ONE of the general P2 tile kernel over the tiles of all
// order classes (every tile entry carries its class: kernel parameters and order formula come from per-class tables), then the
// sorted work-list evaluation per class on that class's region of the work list
template <int DIM, int DPE>
int launch_tiles_single(pnl_context *ctx, double *A, int64_t ldA, int cell_begin, int cell_end, bool slot_ok) {
    int rc;
    const int ncls = (int)ctx->cls.size();
    const bool var = ctx->nlab > 0;
    ctx->kcls_host.resize(ncls); ctx->fcls_host.resize(ncls);
    bool all_fast = true, all_half = true;
    ClassScope cls(ctx, 0);
    for (int k = 0; k < ncls; k++) {
        cls.select(k, 0);
        ctx->kcls_host[k] = ctx->P.k; ctx->fcls_host[k] = ctx->P.qo;
        all_fast = all_fast && ctx->P.k.fast;
        all_half = all_half && ctx->P.k.fast && ctx->P.k.qm == 6;
    }
    const int kt = all_half ? 2 : (all_fast ? 1 : 0);
    if (kt == 0)
        // three layers with s = 0.3 .. 0.7: the class s = 1/2 (half of the pairs) is a "fast" kernel without tables of its own
        for (int k = 0; k < ncls; k++)
            if (!ctx->kcls_host[k].ptab) ctx->kcls_host[k].ptab = pnl_pow_table(ctx, ctx->kcls_host[k], true);
    if ((rc = ensure(ctx, ctx->b_kcls, sizeof(DevKernel)*ncls))) return rc;
    if ((rc = ensure(ctx, ctx->b_fcls, sizeof(DevFormula)*ncls))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_kcls.p, ctx->kcls_host.data(), sizeof(DevKernel)*ncls, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_fcls.p, ctx->fcls_host.data(), sizeof(DevFormula)*ncls, hipMemcpyHostToDevice, ctx->stream));
    cls.select(0, 0);
    const int2 *tiles = (const int2*)ctx->b_tiles.p;
    const int *tcls = var ? (const int*)ctx->b_tilecls.p : nullptr;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_tilectr.p, 0, sizeof(unsigned), ctx->stream));
    // block-slot storage when the whole upper block triangle is assembled by this call and mirrored afterwards
    SlotOut SO{};
    if (slot_ok && slot_storage_ready(ctx)) {
        SO = slot_out(ctx);
        ctx->run.slot_used = true;
        if (var && (rc = pnl2_zero_slot_tiles(ctx, SO))) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    for (int q = 2; q <= 4; q++) {
        const int n = ctx->sl_n[q-1];
        if ((rc = pnl2_launch_uniform(ctx, kt, ctx->P, tiles+ctx->sl_off[q-1], tcls ? tcls+ctx->sl_off[q-1] : nullptr, n, q, A, ldA,
                                      (double*)ctx->b_D.p, SO))) return rc;
        ctx->run.pure_launched = ctx->run.pure_launched || n > 0;
    }
    if (ctx->run.pure_launched) HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    if ((rc = pnl2_launch_p2(ctx, kt, tiles+ctx->sl_off[0], tcls ? tcls+ctx->sl_off[0] : nullptr, ctx->sl_n[0], A, ldA, cell_begin, cell_end,
                             ctx->wl_cap_each, SO))) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_DONE], ctx->stream));
    // block-slot storage: A = A' + A'^T is formed now (it overwrites A); the work-list kernels then write both images
    if (ctx->run.slot_used) {
        if ((rc = pnl2_fold_mirror(ctx, SO, A, ldA))) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev_fold, ctx->stream));
        ctx->run.fold_event_set = true;
    }
    const bool sym = ctx->run.symflush || ctx->run.slot_used;
    {
        ClassFork fork(ctx, ncls);
        if (ncls > pnl_context::NAUX && (int)ctx->cls_n_mixed.size() == ncls) fork.plan(ctx->cls_n_mixed);     // the work lists come from the mixed tiles
        for (int k = 0; k < ncls; k++) {
            cls.select(k, 0);
            fork.use(k);
            const int4 *wl = (const int4*)ctx->b_wl.p+(size_t)k*ctx->wl_cap_each;
            const unsigned *wlc = (const unsigned*)ctx->b_wlcount.p+k;
            rc = with_kt(ctx->P.k.fast, [&](auto kt) {
                return run_worklist<DIM, DPE, decltype(kt)::value>(ctx, wl, wlc, ctx->wl_cap_each, A, ldA, sym, k, ncls);
            });
            if (rc) return rc;
        }
    }
    return PNL_OK;
}

// the whole upper block triangle is assembled by this call (full_list: the tile list is that of pnl_assemble_dense) and mirrored afterwards
bool slot_eligible(const pnl_context *ctx, bool full_list, int cell_begin, int cell_end, int flags) {
    // P2: every tile list (several order classes: multi-visit tiles accumulate); P1: one class, every tile visited by one kernel
    const bool elem = ctx->dpe == 6 || (ctx->dpe == 3 && ctx->cls.size() == 1 && !ctx->nonsym);
    return ctx->dim == 2 && elem && full_list && ctx->slab_rows == 0 && cell_begin == 0 && cell_end == ctx->nc &&
           !(flags & (PNL_FLAG_NO_MIRROR | PNL_FLAG_SYMMETRIC_FLUSH));
}

template <int DIM, int DPE, int TILE>
int assemble_impl(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int ntiles, int cell_begin, int cell_end, int flags) {
    int rc;
    const int ncls = (int)ctx->cls.size();
    ctx->run.symflush = (flags & PNL_FLAG_SYMMETRIC_FLUSH) != 0;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->b_D.p, 0, sizeof(double)*(size_t)ctx->ncp*(DPE*(DPE+1)/2), ctx->stream));
    if (ctx->have_tile_order) HIPCHK(ctx, hipMemsetAsync(ctx->b_Dt.p, 0, sizeof(double)*(size_t)ctx->ncp*(DPE*(DPE+1)/2), ctx->stream));
    if (DIM == 2 && DPE == 3) {
        // ticket counters of the uniform-tile launches (pnl_tile2.hip): one fill for all launches of this assembly
        if ((rc = ensure(ctx, ctx->b_unictr, sizeof(unsigned)*pnl_context::UNI_CTRS))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->b_unictr.p, 0, sizeof(unsigned)*pnl_context::UNI_CTRS, ctx->stream));
        ctx->run.uni_ctr_next = 0; ctx->run.uni_ctr_fresh = pnl_context::UNI_CTRS;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    ctx->run.tiles_launched = ntiles > 0;
    // variable order, zero exterior: the distant (cell, facet) pairs of ALL classes run in one launch with per-class kernel /
    // order-formula tables; the tables go up now, ahead of the tile kernels, so that the launch needs nothing from the
    // caller's stream later than the fold
    const bool bnd_one_pass = zero_exterior && ncls > 1 && ctx->nlab > 0;
    bool bnd_all_fast = true;
    if (bnd_one_pass) {
        std::vector<DevKernel> &bk = ctx->bkcls_host;
        std::vector<DevFormula> &bf = ctx->bfcls_host;
        bk.resize(ncls); bf.resize(ncls);
        ClassScope cls(ctx, 0);
        for (int k = 0; k < ncls; k++) {
            cls.select(k, 0);
            bk[k] = ctx->P.bkn; bf[k] = ctx->P.bqo;
            bnd_all_fast = bnd_all_fast && ctx->P.bkn.fast;
        }
        if ((rc = ensure(ctx, ctx->b_bkcls, sizeof(DevKernel)*ncls))) return rc;
        if ((rc = ensure(ctx, ctx->b_bfcls, sizeof(DevFormula)*ncls))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->b_bkcls.p, bk.data(), sizeof(DevKernel)*ncls, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->b_bfcls.p, bf.data(), sizeof(DevFormula)*ncls, hipMemcpyHostToDevice, ctx->stream));
    }
    // Omega x Omega^c.  Variable order: the distant (cell, facet) pairs of ALL classes in one launch with per-class kernel /
    // order-formula tables, the touching pairs per class (their rules are per class).  chain: fork over the side streams from that
    // event (the order classes' streams after a fold); nullptr: everything on ctx->stream
    auto boundary_term = [&](hipEvent_t chain) -> int {
        int rcb;
        ClassScope cls(ctx, 0);
        ClassFork fork(ctx, chain ? ncls : 1, chain);
        if (chain && ncls > pnl_context::NAUX && (int)ctx->cls_n_mixed.size() == ncls) fork.plan(ctx->cls_n_mixed);
        for (int k = 0; k < ncls; k++) {
            cls.select(k, 0);
            if (!ctx->have_boundary || !ctx->C().have_kernel[1] || !ctx->C().have_form[1])
                return fail(ctx, PNL_ERR_STATE, "zero_exterior needs boundary facets, boundary kernel and order formula");
            if (chain) fork.use(k);
            if (bnd_one_pass && k == 0 &&
                (rcb = launch_boundary<DIM, DPE, 0>(ctx, cell_begin, cell_end, 1, (const DevKernel*)ctx->b_bkcls.p, (const DevFormula*)ctx->b_bfcls.p,
                                                    bnd_all_fast))) return rcb;
            if (chain) fork.use(k);
            if ((rcb = launch_boundary<DIM, DPE, 0>(ctx, cell_begin, cell_end, bnd_one_pass ? 2 : 3))) return rcb;
        }
        return PNL_OK;
    };
    // The boundary term only adds to the per-cell diagonal blocks (b_D, scattered into A at the very end) and never touches A.  Behind a
    // fold pass it runs on side stream 1 behind the LAST TILE KERNEL, i.e. next to the fold: the fold is bound by HBM, the boundary kernels
    // by latency and arithmetic, and nothing else can run there (everything else adds into A, which the fold overwrites).  Not earlier:
    // boundary kernels that are ready while the tile kernels still have workgroups to place take CU slots in front of them, and the tile
    // phase loses more than the term costs (the placements that lost: docs/CHANGELOG_kernels.md, round 3).  Without a fold pass: on side
    // stream 1 behind ev_fold, next to the touching pairs (one class and orientation), else on the caller's stream
    bool bnd_side = false;
    auto boundary_side = [&](hipEvent_t after) -> int {
        hipStream_t const side = ctx->aux[1];
        HIPCHK(ctx, hipStreamWaitEvent(side, after, 0));
        const int rcb = [&] { StreamScope on(ctx, side); return boundary_term(nullptr); }();
        if (rcb) return rcb;
        HIPCHK(ctx, hipEventRecord(ctx->ev_join[1], side));
        bnd_side = true;
        return PNL_OK;
    };
    // a piecewise-constant variable order is assembled class by class: every pass sees the kernel, order formula and
    // singular rules of one order value and skips the pairs of the other classes in its classification
    const int norient = ctx->nonsym ? 2 : 1;
    if (ntiles > 0) {
        const bool single = DIM == 2 && DPE == 6;
        if (ncls*norient > PNL_WL_SLOTS) return fail(ctx, PNL_ERR_UNSUPPORTED, "more than %d order classes x orientations", PNL_WL_SLOTS);
        if ((rc = ensure(ctx, ctx->b_wlcount, sizeof(unsigned)*PNL_WL_SLOTS))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned)*PNL_WL_SLOTS, ctx->stream));
        if ((rc = ensure_worklist(ctx, (double)ntiles*TILE*TILE, single ? ncls : 1))) return rc;
        ctx->run.wl_slots = single ? ncls : ncls*norient;
        if constexpr (DIM == 2 && DPE == 6) {
            // the block-slot storage needs every tile of the upper block triangle written by this call, then the fold + mirror pass
            const bool slot_ok = slot_eligible(ctx, ctx->run.full_tile_list, cell_begin, cell_end, flags);
            if ((rc = launch_tiles_single<DIM, DPE>(ctx, A, ldA, ctx->run.tile_cell_filter ? cell_begin : 0, ctx->run.tile_cell_filter ? cell_end : ctx->nc, slot_ok)))
                return rc;
        } else {
        // 2D P1, one order class: block-slot storage like the P2 path (plain stores instead of 47 GB of fp64 atomics at 48,769
        // DoFs, fold + mirror instead of zero fill + mirror)
        SlotOut SO{};
        if (slot_eligible(ctx, ctx->run.full_tile_list, cell_begin, cell_end, flags) && slot_storage_ready(ctx)) { SO = slot_out(ctx); ctx->run.slot_used = true; }
        ClassScope cls(ctx, 0);
        for (int ko = 0; ko < ncls*norient; ko++) {
            const int k = ko/norient;
            cls.select(k, ko%norient);
            ctx->run.tile_off = ctx->cls_tile_off[k]; ctx->run.n_mixed = ctx->cls_n_mixed[k]; ctx->run.n_pure = ctx->cls_n_pure[k];
            if (ctx->run.n_mixed+ctx->run.n_pure+ctx->cls_n_uni[1][k]+ctx->cls_n_uni[2][k] == 0) continue;
            const int tb0 = ctx->run.tile_cell_filter ? cell_begin : 0, tb1 = ctx->run.tile_cell_filter ? cell_end : ctx->nc;
            // s = 1/2 in 2D (exponent -6/4) has its own instantiation: branch-free evaluations
            if (ctx->P.k.fast && ctx->P.k.qm == 6 && DPE == 3) rc = launch_tiles<DIM, DPE, TILE, (DPE == 3 ? 2 : 1)>(ctx, ko, A, ldA, tb0, tb1, SO);
            else rc = with_kt(ctx->P.k.fast, [&](auto kt) { return launch_tiles<DIM, DPE, TILE, decltype(kt)::value>(ctx, ko, A, ldA, tb0, tb1, SO); });
            if (rc) return rc;
        }
        }
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WORKLIST_DONE], ctx->stream));
    // mirror the cross part before the symmetric contributions are added on both sides (block-slot storage: folded and mirrored behind the tiles)
    if (!ctx->run.slot_used && !(flags & (PNL_FLAG_NO_MIRROR | PNL_FLAG_SYMMETRIC_FLUSH))) {
        const long long nb = (ctx->N+31)/32;
        hipLaunchKernelGGL(k_mirror, dim3((unsigned)(nb*(nb+1)/2)), dim3(PNL_NTHREADS), 0, ctx->stream, A, (long long)ldA, ctx->N);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_MIRROR_DONE], ctx->stream));
    // one order class behind a fold pass: the touching pairs (side stream 0) and the boundary term (side stream 1) start at the
    // fold, next to the work-list kernels on the caller's stream -- everything after the fold only adds with atomics.  The
    // phase timers then show what is left of them after the work list ("singular"), the boundary phase reads 0
    hipStream_t const main_stream = ctx->stream;
    // without a fold pass (row slabs of a rank, 1D, P0) the same holds from here on: the touching pairs and the boundary term add
    // with atomics and run side by side
    bool fold_like = ctx->run.fold_event_set;
    if (!fold_like && ncls*norient == 1 && zero_exterior && !pnl_tune("PNL_NO_OVERLAP")) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fold, ctx->stream));
        fold_like = true;
    }
    const bool overlap = fold_like && ncls*norient == 1 && !pnl_tune("PNL_NO_OVERLAP");
    // several classes behind a fold pass: the side streams of the touching pairs and of the boundary term start at the fold
    // too, class k follows the work list of class k on its stream, nothing waits for the other classes
    hipEvent_t const chain = (ctx->run.fold_event_set && !overlap && !pnl_tune("PNL_NO_OVERLAP")) ? ctx->ev_fold : nullptr;
    if (overlap) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[0], ctx->ev_fold, 0));
    {
        StreamScope on(ctx, overlap ? ctx->aux[0] : main_stream);
        ClassScope cls(ctx, 0);
        ClassFork fork(ctx, ncls*norient, chain);
        if (norient == 1 && ncls > pnl_context::NAUX && (int)ctx->cls_n_mixed.size() == ncls) fork.plan(ctx->cls_n_mixed);    // as the work lists
        for (int ko = 0; ko < ncls*norient; ko++) {
            cls.select(ko/norient, ko%norient);
            fork.use(ko);
            rc = with_kt(ctx->P.k.fast, [&](auto kt) { return launch_singular<DIM, DPE, decltype(kt)::value>(ctx, A, ldA, cell_begin, cell_end); });
            if (rc) return rc;
        }
    }
    if (overlap) HIPCHK(ctx, hipEventRecord(ctx->ev_join[0], ctx->aux[0]));
    else HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    if (zero_exterior) {
        if (ctx->run.fold_event_set) rc = boundary_side(ctx->ev[EV_TILES_DONE]);      // next to the fold pass
        else if (overlap) rc = boundary_side(ctx->ev_fold);
        else rc = boundary_term(chain);
        if (rc) return rc;
    }
    if (overlap) {
        HIPCHK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join[0], 0));
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    }
    if (bnd_side) HIPCHK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join[1], 0));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_BOUNDARY_DONE], ctx->stream));
    if (ctx->slab_rows == 0) {
        scatter_diag<DPE>(ctx, ctx->P, (const double*)ctx->b_D.p, A, ldA);
        if (ctx->have_tile_order) scatter_diag<DPE>(ctx, tile_problem(ctx), (const double*)ctx->b_Dt.p, A, ldA);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_END], ctx->stream));
    ctx->run.ev_valid = true;
    return PNL_OK;
}

template <int DIM, int DPE>
int boundary_masked_impl(pnl_context *ctx, int ni, double fac, const SparseOut &S) {
    const int grid = std::min((ni+3)/4, 256*8);
    const int *cells = (const int*)ctx->b_bi_cells.p, *facets = (const int*)ctx->b_bi_facets.p;
    const unsigned *masks = (const unsigned*)ctx->b_bi_masks.p;
    with_kt(ctx->P.bkn.fast, [&](auto kt) {
        hipLaunchKernelGGL((k_boundary_items<DIM, DPE, decltype(kt)::value>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P,
                           (const double*)ctx->b_vertices.p, cells, facets, masks, ni, fac, S, (double*)nullptr, (const unsigned*)nullptr,
                           (const int*)nullptr, (const DevKernel*)nullptr, (const DevFormula*)nullptr);
        return PNL_OK;
    });
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

// ---- tiled near-field assembly -------------------------------------------------------------------------------------------
template <int DIM, int DPE, int TILE, int KT>
int clusters_tiled_impl(pnl_context *ctx, const pnl_cluster_plan *pl, ClusterTiles CT, int cluster_boundary, const int *d_cell,
                        const int *d_pair, const int2 *sing_dev[3], const int *sing_pair_dev[3], const int *pair_foff, const int *fvid,
                        const double *fgeo, int maxf, const int *bt_cell, const int *bt_facet, const unsigned *bt_slot) {
    using S = TileSmem<DIM, DPE, TILE, KT == 0>;
    constexpr int ND = DPE*(DPE+1)/2;
    int rc;
    const int acc_stride = pl->chunk_stride+1;
    const size_t lds = S::fixed_bytes+sizeof(double)*(size_t)(pl->chunk_stride+1)*acc_stride;
    if (lds > 160*1024) return fail(ctx, PNL_ERR_UNSUPPORTED, "cluster chunk with %d DoFs: LDS sub-block of %zu bytes exceeds 160 KiB", pl->chunk_stride, lds);
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(CT.D, 0, sizeof(double)*(size_t)std::max(pl->num_dslots, 1)*ND, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    // work list of the orders the tiles do not integrate themselves
    {
        const double pairs = (double)pl->ntiles*TILE*TILE;
        const size_t want = (size_t)std::min<double>(std::max<double>(pairs*0.25, 1<<20), 400e6);
        if (ctx->wl_cap < want) {
            if ((rc = ensure(ctx, ctx->b_wl, want*sizeof(int4)))) return rc;
            ctx->wl_cap = (unsigned)want;
        }
        if ((rc = ensure(ctx, ctx->b_wlds, (size_t)ctx->wl_cap*sizeof(int2)))) return rc;
        if ((rc = ensure(ctx, ctx->b_wlpair, (size_t)ctx->wl_cap*sizeof(int)))) return rc;
        if ((rc = ensure(ctx, ctx->b_wlcount, sizeof(unsigned)*PNL_WL_SLOTS))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned), ctx->stream));
        ctx->run.wl_slots = 1; ctx->wl_cap_each = ctx->wl_cap;
        if ((rc = ensure(ctx, ctx->b_tilectr, sizeof(unsigned)))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->b_tilectr.p, 0, sizeof(unsigned), ctx->stream));
        CT.wl_ds = (int2*)ctx->b_wlds.p; CT.wl_pair = (int*)ctx->b_wlpair.p;
    }
    if (pl->ntiles > 0) {
        auto kfun = k_tile_distant<DIM, DPE, TILE, KT, true>;
        const PersistentGrid g = persistent_grid(ctx, kfun, tile_threads(DPE), lds, pl->ntiles, 2);
        if (g.rc) return g.rc;
        if (pnl_tune("PNL_VERBOSE")) fprintf(stderr, "[pnl] cluster tiles=%d nU=%d lds=%zu bytes, occupancy API: %d blocks/CU\n", pl->ntiles,
                                           pl->chunk_stride, lds, g.per_cu);
        hipLaunchKernelGGL(kfun, dim3(g.grid), dim3(tile_threads(DPE)), lds, ctx->stream, with_mixed_rules(ctx, ctx->P), (const int2*)nullptr, (double*)nullptr, 0ll,
                           (double*)nullptr, 0, ctx->nc, acc_stride, (int4*)ctx->b_wl.p, (unsigned*)ctx->b_wlcount.p, ctx->wl_cap, 0,
                           pl->ntiles, CT, (unsigned*)ctx->b_tilectr.p, SlotOut{}, (const unsigned short*)nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_DONE], ctx->stream));
    // behind the tile kernel everything only adds (sparse data, diagonal-block buffer) with atomics: the touching pairs run on side
    // stream 0 and the cluster-local boundary term on side stream 1 next to the work-list kernels; joined before the diagonal
    // blocks are scattered.  The phase timers then show what is left of them after the work list
    hipStream_t const main_stream = ctx->stream;
    const bool overlap = !pnl_tune("PNL_NO_OVERLAP");
    StreamScope side(ctx, main_stream);
    if (overlap) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fold, main_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[0], ctx->ev_fold, 0));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[1], ctx->ev_fold, 0));
    }
    {
        if ((rc = ensure(ctx, ctx->b_wlsorted, (size_t)ctx->wl_cap*sizeof(int4)))) return rc;
        if ((rc = ensure(ctx, ctx->b_wlaux, sizeof(unsigned)*(4*(PNL_WL_BINS+1))))) return rc;
        WlBins B;
        if ((rc = pnl_wl_sort(ctx, (const int4*)ctx->b_wl.p, (const unsigned*)ctx->b_wlcount.p, ctx->wl_cap, (unsigned*)ctx->b_wlaux.p,
                          (int4*)ctx->b_wlsorted.p, B))) return rc;
        if ((rc = worklist_eval<DIM, DPE, KT, false>(ctx, WL_RULE_KB, (const int4*)ctx->b_wlsorted.p, B, nullptr, 0, nullptr, SparseOut{},
                                                     CT, PNL_WL_BINS-1, false))) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WORKLIST_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_MIRROR_DONE], ctx->stream));
    // touching element pairs
    if (overlap) side.to(ctx->aux[0]);
    for (int s = 0; s < DIM+1; s++) {
        const int np = pl->n_sing[s];
        if (!np) continue;
        if (!ctx->C().have_sing[0][s]) return fail(ctx, PNL_ERR_STATE, "singular rule for %d common vertices not uploaded", s+1);
        ClusterTiles C2 = CT;
        C2.sing_pair = sing_pair_dev[s];
        const int wpb = PNL_SING_THREADS/64;
        if ((rc = with_slot<DIM>(s, [&](auto slot) {
                return launch_singular_pairs<DIM, DPE, decltype(slot)::value, KT, false>(ctx, (np+wpb-1)/wpb, sing_dev[s], np, nullptr, 0, 0, ctx->nc,
                                                                                         SparseOut{}, nullptr, nullptr, C2);
            }))) return rc;
    }
    if (overlap) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_join[0], ctx->aux[0]));
        side.to(ctx->aux[1]);
    } else HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    // cluster-local Gauss-theorem term into the diagonal-block buffer
    if (cluster_boundary && pl->num_dslots > 0 && pl->nfacets > 0) {
        if (!ctx->C().have_kernel[1] || !ctx->C().have_form[1]) return fail(ctx, PNL_ERR_STATE, "boundary kernel and order formula must be set");
        // few cells (those of cellsInter), many facets each: small facet chunks give the parallelism
        // (measured at C4, 9.9e6 pairs / 5.0e8 point pairs: all in place 9.0 ms; list for > 48 point pairs 4.7 ms, > 200: 4.1 ms,
        // > 200 with 4 facets per chunk 3.2 ms, > 1000: 5.4 ms)
        constexpr int per = 4;
        const dim3 grid((pl->num_dslots+PNL_NTHREADS-1)/PNL_NTHREADS, (maxf+per-1)/per);
        const double *verts = (const double*)ctx->b_vertices.p;
        // (cell, facet) pairs with more than `defer` point pairs: list of items for k_boundary_items (one per wave); pairs that do
        // not fit into the list are integrated in place
        constexpr int defer = 200;
        constexpr unsigned cap = 1u << 22;
        if ((rc = ensure(ctx, ctx->b_bdefer, sizeof(int)*(size_t)cap*(3+DIM)+sizeof(unsigned)))) return rc;
        int *dcells = (int*)ctx->b_bdefer.p, *dfacets = dcells+cap;
        unsigned *dslots = (unsigned*)(dfacets+(size_t)cap*DIM);
        unsigned *dcount = (unsigned*)((int*)(dslots+cap)+cap);
        HIPCHK(ctx, hipMemsetAsync(dcount, 0, sizeof(unsigned), ctx->stream));
        // items of k_boundary_items, one per wave: the deferred pairs (count on the device) and the touching (cell, facet) pairs
        auto items = [&](auto kt, int g, const int *cells, const int *facets, const unsigned *slots, int n, const unsigned *count) {
            hipLaunchKernelGGL((k_boundary_items<DIM, DPE, decltype(kt)::value>), dim3(g), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, verts, cells,
                               facets, slots, n, 1., SparseOut{}, CT.D, count, (const int*)nullptr, (const DevKernel*)nullptr, (const DevFormula*)nullptr);
        };
        with_kt(ctx->P.bkn.fast, [&](auto kt) {
            hipLaunchKernelGGL((k_cluster_boundary<DIM, DPE, decltype(kt)::value>), grid, dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, verts, d_cell,
                               d_pair, pl->num_dslots, pair_foff, fvid, fgeo, pl->nfacets, CT.D, per, defer, dcells, dfacets, dslots, dcount, cap);
            return PNL_OK;
        });
        HIPCHK(ctx, hipGetLastError());
        with_kt(ctx->P.bkn.fast, [&](auto kt) { items(kt, 256*8, dcells, dfacets, dslots, (int)cap, dcount); return PNL_OK; });
        HIPCHK(ctx, hipGetLastError());
        if (pl->n_btouch > 0) {
            for (int s = 0; s < DIM; s++)
                if (!ctx->C().have_sing[1][s]) return fail(ctx, PNL_ERR_STATE, "boundary singular rule for %d common vertices not uploaded", s+1);
            with_kt(ctx->P.bkn.fast, [&](auto kt) {
                items(kt, std::min((pl->n_btouch+3)/4, 256*8), bt_cell, bt_facet, bt_slot, pl->n_btouch, nullptr);
                return PNL_OK;
            });
            HIPCHK(ctx, hipGetLastError());
        }
    }
    if (overlap) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_join[1], ctx->aux[1]));
        side.to(main_stream);
        HIPCHK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join[0], 0));
        HIPCHK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join[1], 0));
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_BOUNDARY_DONE], ctx->stream));
    if (pl->num_dslots > 0) {
        const long long nt = (long long)pl->num_dslots*DPE*DPE;
        hipLaunchKernelGGL((k_cluster_scatter_diag<DPE>), dim3((unsigned)((nt+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0,
                           ctx->stream, ctx->P, CT, d_cell, d_pair, pl->num_dslots);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_END], ctx->stream));
    ctx->run.ev_valid = true;
    ctx->run.tiles_launched = true;
    return PNL_OK;
}

int dispatch(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int ntiles, int cell_begin, int cell_end, int flags) {
    for (auto *c : ctx->cls)
        if (!std::isinf(c->kern[0].horizon2))
            return fail(ctx, PNL_ERR_UNSUPPORTED, "finite-horizon kernels are assembled from an explicit pair list (pnl_assemble_pairs_masked, "
                        "nonlocalBuilder.getSparse): the all-pairs dense loop has no REMOTE / CUT handling");
    pnl_refresh_tables(ctx);
    return with_shape(ctx, [&](auto D, auto E) {
        constexpr int DIM = decltype(D)::value, DPE = decltype(E)::value;
        return assemble_impl<DIM, DPE, tile_cells<DIM, DPE>>(ctx, A, ldA, zero_exterior, ntiles, cell_begin, cell_end, flags);
    });
}

}  // namespace

void pnl_scatter_diag(pnl_context *ctx, const DevProblem &P, const double *D, double *A, int64_t ldA) {
    if (ctx->dpe == 2) scatter_diag<2>(ctx, P, D, A, ldA);
    else if (ctx->dpe == 3) scatter_diag<3>(ctx, P, D, A, ldA);
    else scatter_diag<6>(ctx, P, D, A, ldA);
}

// counting sort of a work list by order (WlBins: pnl_context.h)
__global__ void __launch_bounds__(PNL_NTHREADS)
k_wl_hist(const int4 *__restrict__ wl, const unsigned *__restrict__ wl_count, unsigned wl_cap, unsigned *__restrict__ hist) {
    __shared__ unsigned h[PNL_WL_BINS];
    if (threadIdx.x < PNL_WL_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned count = min(*wl_count, wl_cap);
    for (unsigned i = blockIdx.x*PNL_NTHREADS+threadIdx.x; i < count; i += gridDim.x*PNL_NTHREADS)
        atomicAdd(&h[(wl[i].w >> 16) & (PNL_WL_BINS-1)], 1u);
    __syncthreads();
    if (threadIdx.x < PNL_WL_BINS && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// offs[q] = first sorted position of order q, chunk_off[q] = first 16-pair chunk of order q; both have PNL_WL_BINS+1 entries
__global__ void k_wl_scan(const unsigned *__restrict__ hist, unsigned *__restrict__ offs, unsigned *__restrict__ chunk_off,
                          unsigned *__restrict__ cursor) {
    if (threadIdx.x == 0) {
        unsigned run = 0, crun = 0;
        for (int q = 0; q < PNL_WL_BINS; q++) {
            offs[q] = run; chunk_off[q] = crun; cursor[q] = 0;
            run += hist[q]; crun += (hist[q]+15)/16;
        }
        offs[PNL_WL_BINS] = run; chunk_off[PNL_WL_BINS] = crun;
    }
}

// Stable within a wave's slice: every wave owns a contiguous part of its workgroup's input range and hands out positions in
// input order (ballot ranks), so runs of consecutive entries with one key stay consecutive.  The producers append whole
// waves of neighbouring pairs (k_fh_pairs: 64 consecutive cells c1 against one c2), and the consumers run 64 consecutive
// sorted entries per wave: coalesced cell data, neighbouring pattern rows, shared cells that can be summed over the wave.
__global__ void __launch_bounds__(PNL_NTHREADS)
k_wl_scatter(const int4 *__restrict__ wl, const unsigned *__restrict__ wl_count, unsigned wl_cap, const unsigned *__restrict__ offs,
             unsigned *__restrict__ cursor, int4 *__restrict__ sorted) {
    constexpr int NW = PNL_NTHREADS/64;
    __shared__ unsigned h[NW][PNL_WL_BINS], base[NW][PNL_WL_BINS];
    const unsigned count = min(*wl_count, wl_cap);
    const unsigned per = (count+gridDim.x-1)/gridDim.x;
    const unsigned b0 = blockIdx.x*per, b1 = min(count, b0+per);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned perw = ((b1 > b0 ? b1-b0 : 0u)+NW-1)/NW;
    const unsigned i0 = min(b1, b0+wave*perw), i1 = min(b1, i0+perw);
    const unsigned long long lt = (1ull << lane)-1ull;
    for (int t = threadIdx.x; t < NW*PNL_WL_BINS; t += PNL_NTHREADS) (&h[0][0])[t] = 0;
    __syncthreads();
    // pass 1: keys per wave slice; pass 2 hands out positions with the same loop
    auto sweep = [&](bool place) {
        for (unsigned i = i0; i < i1; i += 64) {
            const bool act = i+lane < i1;
            int4 e = make_int4(0, 0, 0, 0);
            if (act) e = wl[i+lane];
            const int q = act ? ((e.w >> 16) & (PNL_WL_BINS-1)) : -1;
            unsigned long long todo = __ballot(act);
            while (todo) {
                const int leader = __ffsll((long long)todo)-1;
                const int qL = __builtin_amdgcn_readlane(q, leader);
                const unsigned long long same = __ballot(q == qL);
                if (place) {
                    const unsigned start = base[wave][qL]+h[wave][qL];          // the wave is the only writer of its row
                    if (q == qL) sorted[start+__popcll(same & lt)] = e;
                }
                __builtin_amdgcn_wave_barrier();
                if (lane == leader) h[wave][qL] += (unsigned)__popcll(same);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                todo &= ~same;
            }
        }
    };
    sweep(false);
    __syncthreads();
    if (threadIdx.x < PNL_WL_BINS) {
        unsigned tot = 0;
        for (int w = 0; w < NW; w++) tot += h[w][threadIdx.x];
        unsigned run = tot ? offs[threadIdx.x]+atomicAdd(&cursor[threadIdx.x], tot) : 0u;
        for (int w = 0; w < NW; w++) { base[w][threadIdx.x] = run; run += h[w][threadIdx.x]; h[w][threadIdx.x] = 0; }
    }
    __syncthreads();
    sweep(true);
}

int pnl_wl_sort(pnl_context *ctx, const int4 *wl, const unsigned *count, unsigned cap, unsigned *aux_base, int4 *sorted, WlBins &B) {
    B.hist = aux_base; B.offs = B.hist+(PNL_WL_BINS+1); B.coff = B.offs+(PNL_WL_BINS+1); B.cursor = B.coff+(PNL_WL_BINS+1);
    HIPCHK(ctx, hipMemsetAsync(B.hist, 0, sizeof(unsigned)*(PNL_WL_BINS+1), ctx->stream));
    hipLaunchKernelGGL(k_wl_hist, dim3(512), dim3(PNL_NTHREADS), 0, ctx->stream, wl, count, cap, B.hist);
    hipLaunchKernelGGL(k_wl_scan, dim3(1), dim3(64), 0, ctx->stream, (const unsigned*)B.hist, B.offs, B.coff, B.cursor);
    hipLaunchKernelGGL(k_wl_scatter, dim3(512), dim3(PNL_NTHREADS), 0, ctx->stream, wl, count, cap, (const unsigned*)B.offs, B.cursor, sorted);
    return PNL_OK;
}

// the tile plan (pnl_setup.hip): k_tile_pair_codes over n tiles (device pointer); codes: 512 words per tile or nullptr; host_stat: per tile
// -1 not settled, else its number of 6-point pairs, through b_candq, or nullptr.  Synchronises the stream.
int pnl_tile_pair_codes(pnl_context *ctx, const DevFormula &qo, const int2 *tiles, int n, unsigned short *codes, int *host_stat) {
    if (n <= 0) return PNL_OK;
    if (ctx->tile != 64) return fail(ctx, PNL_ERR_STATE, "pair codes: tiles of 64 cells");
    int rc;
    if (host_stat && (rc = ensure(ctx, ctx->b_candq, sizeof(int)*(size_t)n))) return rc;
    // the cell tables of finalize and the packed rules; the first plan of a context is made before pnl_refresh_tables has run
    DevProblem P = ctx->P;
    P.qmax = ctx->qmax;
    P.tt_n = (const int*)ctx->b_ttn.p;
    if (!P.tt_n || !P.cslot) return fail(ctx, PNL_ERR_STATE, "pair codes: rules and DoF map first");
    hipLaunchKernelGGL(k_tile_pair_codes<64>, dim3(std::min(n, 256*8)), dim3(512), 0, ctx->stream, P, qo, tiles, n, codes,
                       host_stat ? (int*)ctx->b_candq.p : (int*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    if (host_stat) HIPCHK(ctx, hipMemcpyAsync(host_stat, ctx->b_candq.p, sizeof(int)*(size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PNL_OK;
}

// the tile plan (pnl_setup.hip): k_tile_pair_lists, the records of n settled tiles (device, PNL_LIST_STRIDE words per tile) from their
// codes (device, 512 words per tile).  Synchronises the stream.
int pnl_tile_pair_lists(pnl_context *ctx, const unsigned short *codes, int n, unsigned short *lists) {
    if (n <= 0) return PNL_OK;
    if (ctx->tile != 64) return fail(ctx, PNL_ERR_STATE, "pair lists: tiles of 64 cells");
    HIPCHK(ctx, hipMemsetAsync(lists, 0, (size_t)n*PNL_LIST_STRIDE*sizeof(unsigned short), ctx->stream));
    hipLaunchKernelGGL(k_tile_pair_lists<64>, dim3(std::min(n, 256*8)), dim3(512), 0, ctx->stream, codes, n, lists);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PNL_OK;
}

// the tile plan (pnl_setup.hip): the exact order range of the cell pairs of the ncand tiles in b_candtiles, through b_candq to the host
int pnl_tile_order_range(pnl_context *ctx, const DevFormula &qo, int ncand, signed char *host_out) {
    const int grid = std::min(ncand, 256*8);
    if (ctx->tile == 64)
        hipLaunchKernelGGL(k_tile_order_range<64>, dim3(grid), dim3(256), 0, ctx->stream, ctx->P, qo, (const int2*)ctx->b_candtiles.p,
                           ncand, (signed char*)ctx->b_candq.p);
    else
        hipLaunchKernelGGL(k_tile_order_range<32>, dim3(grid), dim3(256), 0, ctx->stream, ctx->P, qo, (const int2*)ctx->b_candtiles.p,
                           ncand, (signed char*)ctx->b_candq.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(host_out, ctx->b_candq.p, ncand, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PNL_OK;
}

extern "C" {

// A row slab (pnl_set_row_slab) is written one-sided: no mirror pass, no scatter of the per-cell diagonal blocks (they stay
// in the per-cell buffer, pnl_get_diag_blocks), columns are counted from col0.  The rows of every cell of the caller's cell
// range must be in the slab.
static int slab_prepare(pnl_context *ctx, int &flags, int cell_begin, int cell_end) {
    if (ctx->slab_rows <= 0) return PNL_OK;
    if (flags & PNL_FLAG_SYMMETRIC_FLUSH) return fail(ctx, PNL_ERR_INVALID, "a row slab is one-sided: PNL_FLAG_SYMMETRIC_FLUSH does not apply");
    if (ctx->have_pw) return fail(ctx, PNL_ERR_UNSUPPORTED, "row slabs are not implemented for kernels with an order per quadrature point");
    const auto &rd = ctx->slab_rowdofs, &cd = ctx->slab_coldofs;
    for (int c = cell_begin; c < ctx->nc; c++)
        for (int k = 0; k < ctx->dpe; k++) {
            const int g = ctx->dofs[(size_t)c*ctx->dpe+k];
            if (g < 0) continue;
            if (c < cell_end && !std::binary_search(rd.begin(), rd.end(), g))
                return fail(ctx, PNL_ERR_INVALID, "DoF %d of cell %d is not a row of the slab", g, c);
            if (!std::binary_search(cd.begin(), cd.end(), g))
                return fail(ctx, PNL_ERR_INVALID, "DoF %d of cell %d is not a column of the slab", g, c);
        }
    flags |= PNL_FLAG_NO_MIRROR;
    return PNL_OK;
}

int pnl_assemble_dense(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int cell_begin, int cell_end, int flags) {
    if (!ctx) return PNL_ERR_INVALID;
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    if ((rc = pnl_tile_order_ready(ctx))) return rc;
    if (!A || ldA < (ctx->slab_rows ? ctx->slab_cols : ctx->N)) return fail(ctx, PNL_ERR_INVALID, "bad output matrix (ldA=%lld, num_dofs=%d)", (long long)ldA, ctx->N);
    if (cell_begin < 0 || cell_end > ctx->nc || cell_begin > cell_end) return fail(ctx, PNL_ERR_INVALID, "bad cell range");
    if ((rc = slab_prepare(ctx, flags, cell_begin, cell_end))) return rc;
    pnl_begin_assembly(ctx);
    ctx->run.full_tile_list = true;
    std::vector<int2> tiles;
    if (cell_end > cell_begin) pnl_make_tiles(ctx, tiles, cell_begin, cell_end);
    if ((rc = pnl_upload_tiles(ctx, tiles, cell_begin, cell_end))) return rc;
    // pairs visited by the reference loop: c1 in [begin,end), c2 in [c1, nc)
    for (long long c = cell_begin; c < cell_end; c++)
        if (ctx->real_from[c] != ctx->real_from[c+1]) ctx->run.visited_pairs += (unsigned long long)ctx->real_from[c];      // zero-volume padding cells do not count
    return dispatch(ctx, A, ldA, zero_exterior, (int)tiles.size(), cell_begin, cell_end, flags);
}

int pnl_dense_overwrites(pnl_context *ctx, int cell_begin, int cell_end, int flags) {
    if (!ctx) return PNL_ERR_INVALID;
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    return slot_eligible(ctx, true, cell_begin, cell_end, flags) && slot_storage_ready(ctx) ? 1 : 0;      // true: what pnl_assemble_dense sets
}

int pnl_assemble_dense_tiles(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int ntiles, const int32_t *tiles_host,
                             int cell_begin, int cell_end, int flags) {
    if (!ctx) return PNL_ERR_INVALID;
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    if ((rc = pnl_tile_order_ready(ctx))) return rc;
    if (!A || ldA < (ctx->slab_rows ? ctx->slab_cols : ctx->N) || ntiles < 0 || (ntiles && !tiles_host)) return fail(ctx, PNL_ERR_INVALID, "bad arguments");
    if (cell_begin < 0 || cell_end > ctx->nc || cell_begin > cell_end) return fail(ctx, PNL_ERR_INVALID, "bad cell range");
    if ((rc = slab_prepare(ctx, flags, cell_begin, cell_end))) return rc;
    std::vector<int2> tiles(ntiles);
    for (int i = 0; i < ntiles; i++) {
        tiles[i] = make_int2(tiles_host[2*i], tiles_host[2*i+1]);
        if (tiles[i].x < 0 || tiles[i].y >= ctx->nblocks || tiles[i].x > tiles[i].y) return fail(ctx, PNL_ERR_INVALID, "bad tile %d", i);
    }
    pnl_begin_assembly(ctx);
    ctx->run.tile_cell_filter = false;          // the caller's tiles, whole
    if ((rc = pnl_upload_tiles(ctx, tiles, cell_begin, cell_end))) return rc;
    return dispatch(ctx, A, ldA, zero_exterior, ntiles, cell_begin, cell_end, flags);
}

int pnl_assemble_boundary_masked(pnl_context *ctx, int ni, const int32_t *cells, const int32_t *facets, const uint32_t *masks,
                                 double fac, double *data, double *diag) {
    if (!ctx) return PNL_ERR_INVALID;
    if (ni < 0 || (ni && (!cells || !facets || !masks))) return fail(ctx, PNL_ERR_INVALID, "bad item list");
    if (!ctx->C().have_kernel[1] || !ctx->C().have_form[1]) return fail(ctx, PNL_ERR_STATE, "boundary kernel and order formula must be set");
    for (int i = 0; i < ni; i++) {
        if (cells[i] < 0 || cells[i] >= ctx->nc) return fail(ctx, PNL_ERR_INVALID, "item %d: bad cell %d", i, cells[i]);
        for (int k = 0; k < ctx->dim; k++)
            if (facets[(size_t)i*ctx->dim+k] < 0 || facets[(size_t)i*ctx->dim+k] >= ctx->nv)
                return fail(ctx, PNL_ERR_INVALID, "item %d: bad facet vertex", i);
    }
    for (int s = 0; s < ctx->dim; s++)
        if (!ctx->C().have_sing[1][s]) return fail(ctx, PNL_ERR_STATE, "boundary singular rule for %d common vertices not uploaded", s+1);
    int rc;
    if ((rc = upload(ctx, ctx->b_bi_cells, cells, (size_t)ni))) return rc;
    if ((rc = upload(ctx, ctx->b_bi_facets, facets, (size_t)ni*ctx->dim))) return rc;
    if ((rc = upload(ctx, ctx->b_bi_masks, masks, (size_t)ni))) return rc;
    SparseOut S;
    if ((rc = pnl_sparse_ready(ctx, data, diag, S))) return rc;
    if (ni == 0) return PNL_OK;
    return with_shape(ctx, [&](auto D, auto E) { return boundary_masked_impl<decltype(D)::value, decltype(E)::value>(ctx, ni, fac, S); });
}

int pnl_assemble_clusters_tiled(pnl_context *ctx, const pnl_cluster_plan *pl, int cluster_boundary, double *data, double *diag) {
    if (!ctx || !pl) return PNL_ERR_INVALID;
    if (ctx->nlab > 0) return fail(ctx, PNL_ERR_UNSUPPORTED, "cluster assembly with a variable order needs the jump terms (NA:1966-2156)");
    if (!std::isinf(ctx->C().kern[0].horizon2)) return fail(ctx, PNL_ERR_UNSUPPORTED, "tiled cluster assembly: infinite horizon only");
    int rc;
    SparseOut S;
    if ((rc = pnl_sparse_ready(ctx, data, diag, S))) return rc;
    if (pl->tile != ctx->tile) return fail(ctx, PNL_ERR_INVALID, "plan built for tiles of %d cells, the kernels use %d", pl->tile, ctx->tile);
    if (pl->npairs < 0 || pl->ntiles < 0 || pl->num_dslots < 0 || pl->chunk_stride < 1) return fail(ctx, PNL_ERR_INVALID, "bad plan sizes");
    const int T = pl->tile, dim = ctx->dim, dpe = ctx->dpe;
    // light validation of the index arrays (a wrong index here would be an out-of-bounds access on the device)
    for (int t = 0; t < pl->ntiles; t++) {
        if (pl->tile_chunkA[t] < 0 || pl->tile_chunkA[t] >= pl->nchunks || pl->tile_chunkB[t] < 0 || pl->tile_chunkB[t] >= pl->nchunks ||
            pl->tile_pair[t] < 0 || pl->tile_pair[t] >= pl->npairs)
            return fail(ctx, PNL_ERR_INVALID, "tile %d out of range", t);
        for (int l = 0; l < T; l++)
            if (pl->tile_dslotA[(size_t)t*T+l] >= pl->num_dslots || pl->tile_dslotB[(size_t)t*T+l] >= pl->num_dslots)
                return fail(ctx, PNL_ERR_INVALID, "tile %d: diagonal-block slot out of range", t);
    }
    for (size_t i = 0; i < (size_t)pl->nchunks*T; i++)
        if (pl->chunk_cells[i] >= ctx->nc) return fail(ctx, PNL_ERR_INVALID, "chunk cell out of range");
    for (int c = 0; c < pl->nchunks; c++)
        if (pl->chunk_ndof[c] < 0 || pl->chunk_ndof[c] > pl->chunk_stride) return fail(ctx, PNL_ERR_INVALID, "chunk %d: bad DoF count", c);
    for (size_t i = 0; i < (size_t)pl->nchunks*dpe*T; i++)
        if (pl->chunk_slot[i] >= pl->chunk_stride) return fail(ctx, PNL_ERR_INVALID, "chunk slot out of range");
    for (int k = 0; k < 2*pl->npairs; k++)
        if (pl->pair_nodes[k] < 0 || pl->pair_nodes[k] >= pl->nnodes) return fail(ctx, PNL_ERR_INVALID, "pair node out of range");
    for (int d = 0; d < pl->num_dslots; d++)
        if (pl->d_cell[d] < 0 || pl->d_cell[d] >= ctx->nc || pl->d_pair[d] < 0 || pl->d_pair[d] >= pl->npairs)
            return fail(ctx, PNL_ERR_INVALID, "diagonal-block slot %d out of range", d);
    for (size_t i = 0; i < (size_t)pl->nfacets*dim; i++)
        if (pl->fvid[i] < 0 || pl->fvid[i] >= ctx->nv) return fail(ctx, PNL_ERR_INVALID, "facet vertex out of range");
    DevBuf *B = ctx->b_cp;
    int nb = 0;
#define UP(ptr, n) ((rc = upload(ctx, B[nb], ptr, (size_t)(n))) ? nullptr : B[nb++].p)
    ClusterTiles CT;
    std::memset(&CT, 0, sizeof(CT));
    CT.npairs = pl->npairs; CT.chunk_stride = pl->chunk_stride; CT.S = S;
    if (!(CT.pair_nodes = (const int*)UP(pl->pair_nodes, 2*pl->npairs))) return rc;
    if (!(CT.node_off = (const int*)UP(pl->node_off, pl->nnodes+1))) return rc;
    if (!(CT.node_dofs = (const int*)UP(pl->node_dofs, pl->node_off[pl->nnodes]))) return rc;
    if (!(CT.chunk_cells = (const int*)UP(pl->chunk_cells, (size_t)pl->nchunks*T))) return rc;
    if (!(CT.chunk_ndof = (const int*)UP(pl->chunk_ndof, pl->nchunks))) return rc;
    if (!(CT.chunk_dofs = (const int*)UP(pl->chunk_dofs, (size_t)pl->nchunks*pl->chunk_stride))) return rc;
    if (!(CT.chunk_slot = (const short*)UP(pl->chunk_slot, (size_t)pl->nchunks*dpe*T))) return rc;
    if (!(CT.chunkA = (const int*)UP(pl->tile_chunkA, pl->ntiles))) return rc;
    if (!(CT.chunkB = (const int*)UP(pl->tile_chunkB, pl->ntiles))) return rc;
    if (!(CT.pair = (const int*)UP(pl->tile_pair, pl->ntiles))) return rc;
    if (!(CT.flags = (const int*)UP(pl->tile_flags, pl->ntiles))) return rc;
    if (!(CT.dslotA = (const int*)UP(pl->tile_dslotA, (size_t)pl->ntiles*T))) return rc;
    if (!(CT.dslotB = (const int*)UP(pl->tile_dslotB, (size_t)pl->ntiles*T))) return rc;
    const int *d_cell, *d_pair, *pair_foff, *fvid, *bt_cell, *bt_facet;
    const unsigned *bt_slot;
    if (!(d_cell = (const int*)UP(pl->d_cell, pl->num_dslots))) return rc;
    if (!(d_pair = (const int*)UP(pl->d_pair, pl->num_dslots))) return rc;
    if (!(pair_foff = (const int*)UP(pl->pair_foff, pl->npairs+1))) return rc;
    if (!(fvid = (const int*)UP(pl->fvid, (size_t)pl->nfacets*dim))) return rc;
    if (!(bt_cell = (const int*)UP(pl->bt_cell, pl->n_btouch))) return rc;
    if (!(bt_facet = (const int*)UP(pl->bt_facet, (size_t)pl->n_btouch*dim))) return rc;
    if (!(bt_slot = (const unsigned*)UP((const unsigned*)pl->bt_slot, pl->n_btouch))) return rc;
    const int2 *sing_dev[3] = {nullptr, nullptr, nullptr};
    const int *sing_pair_dev[3] = {nullptr, nullptr, nullptr};
    for (int s = 0; s < 3; s++) {
        const int n = pl->n_sing[s];
        std::vector<int2> pr(n);
        std::vector<int> pk(n);
        for (int i = 0; i < n; i++) {
            const int32_t *it = pl->sing_items[s]+3*(size_t)i;
            if (it[0] < 0 || it[0] >= pl->npairs || it[1] < 0 || it[1] > it[2] || it[2] >= ctx->nc)
                return fail(ctx, PNL_ERR_INVALID, "touching item %d of slot %d out of range", i, s);
            pk[i] = it[0]; pr[i] = make_int2(it[1], it[2]);
        }
        if (!(sing_dev[s] = (const int2*)UP(pr.data(), n))) return rc;
        if (!(sing_pair_dev[s] = (const int*)UP(pk.data(), n))) return rc;
    }
    // facet geometry (centre, unit normal, length, |ln(len/H0)|, ln(len)) like DevProblem::bgeo
    int maxf = 0;
    std::vector<double> geo((size_t)(2*dim+3)*std::max(pl->nfacets, 1), 0.);
    for (int k = 0; k < pl->npairs; k++) maxf = std::max(maxf, pl->pair_foff[k+1]-pl->pair_foff[k]);
    for (int f = 0; f < pl->nfacets; f++) {
        const size_t nf = pl->nfacets;
        double len = 1.;
        const double *v0 = &ctx->vertices[(size_t)pl->fvid[(size_t)f*dim]*dim];
        const double *v1 = &ctx->vertices[(size_t)pl->fvid[(size_t)f*dim+(dim-1)]*dim];
        for (int d = 0; d < dim; d++) geo[(size_t)d*nf+f] = dim == 2 ? 0.5*(v0[d]+v1[d]) : v0[d];
        if (dim == 2) {
            const double n0 = v1[1]-v0[1], n1 = v0[0]-v1[0];
            const double inv = 1./std::sqrt(n0*n0+n1*n1);
            geo[(size_t)(dim+0)*nf+f] = n0*inv; geo[(size_t)(dim+1)*nf+f] = n1*inv;
            const double dx = v1[0]-v0[0], dy = v1[1]-v0[1];
            len = std::sqrt(dx*dx+dy*dy);
        }
        geo[(size_t)(2*dim)*nf+f] = len;
        geo[(size_t)(2*dim+1)*nf+f] = std::fabs(std::log(len/ctx->H0));
        geo[(size_t)(2*dim+2)*nf+f] = std::log(len);
    }
    const double *fgeo;
    if (!(fgeo = (const double*)UP(geo.data(), geo.size()))) return rc;
#undef UP
    if ((rc = ensure(ctx, ctx->b_cpD, sizeof(double)*(size_t)std::max(pl->num_dslots, 1)*(dpe*(dpe+1)/2)))) return rc;
    CT.D = (double*)ctx->b_cpD.p;
    pnl_begin_assembly(ctx);
    return with_shape(ctx, [&](auto D, auto E) {
        constexpr int DIM = decltype(D)::value, DPE = decltype(E)::value;
        return with_kt(ctx->P.k.fast, [&](auto kt) {
            return clusters_tiled_impl<DIM, DPE, tile_cells<DIM, DPE>, decltype(kt)::value>(ctx, pl, CT, cluster_boundary, d_cell, d_pair, sing_dev,
                                                                                          sing_pair_dev, pair_foff, fvid, fgeo, maxf, bt_cell, bt_facet, bt_slot);
        });
    });
}

}  // extern "C"
