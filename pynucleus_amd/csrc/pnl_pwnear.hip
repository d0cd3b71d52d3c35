// Every assembly of the non-symmetric kernels with an order per quadrature point (gfx950 only).  Dense: fractionalLaplacian{1,2}D_nonsym
// over all pairs (pnl_assemble_dense_pointwise).  Near field and far field: the part of assembleClusters / getH2
// (nonlocalAssembly_{SCALAR}.pxi:1663-2156, 3094-3219) these kernels take -- ordered element pairs with masks over the (2 dpe)^2 local
// entries, the cluster exterior with the pointwise boundary kernel, the kernel interpolants of the admissible pairs with the order at
// the nodes of the row cluster.  Kernels: pnl_pointwise.h; the state setters and pnl_pw_prepare launch nothing and are in pnl_setup.hip.
#include "pnl_context.h"
// the kernel templates this unit instantiates stay in an unnamed namespace: nothing collides with pnl_hip.o or pnl_sparse.o at link time
namespace {
#include "pnl_pointwise.h"
}
#include "pnl_launch.h"

namespace {

// statistics from the histogram of the sorted list: pairs per order, both orientations' kernel evaluations
__global__ void k_pw_stats(const DevProblem P, const unsigned *__restrict__ hist) {
    const int q = threadIdx.x;
    if (q < 2 || q > P.qmax || q > PNL_MAXQ) return;
    const unsigned long long c = hist[q];
    if (!c) return;
    const unsigned long long n = (unsigned long long)(P.off[q+1]-P.off[q]);
    atomicAdd(&P.counters[8+q], c);
    atomicAdd(&P.counters[1], c);
    atomicAdd(&P.counters[2], 2ull*c*n*n);
}

// statistics of the near-field work list: pairs per order, kernel evaluations of ONE orientation per item
__global__ void k_pw_stats_near(const DevProblem P, const unsigned *__restrict__ hist) {
    const int q = threadIdx.x;
    if (q < 2 || q > P.qmax || q > PNL_MAXQ) return;
    const unsigned long long c = hist[q];
    if (!c) return;
    const unsigned long long n = (unsigned long long)(P.off[q+1]-P.off[q]);
    atomicAdd(&P.counters[8+q], c);
    atomicAdd(&P.counters[1], c);
    atomicAdd(&P.counters[2], c*n*n);
}

// the single-region work list of both paths: at least `want` entries (it never shrinks), the buffers of its sort, an empty list
int reserve_worklist(pnl_context *ctx, size_t want) {
    int rc;
    if (ctx->wl_cap < want) {
        if ((rc = ensure(ctx, ctx->b_wl, want*sizeof(int4)))) return rc;
        ctx->wl_cap = (unsigned)want;
    }
    if ((rc = ensure(ctx, ctx->b_wlsorted, (size_t)ctx->wl_cap*sizeof(int4)))) return rc;
    if ((rc = ensure(ctx, ctx->b_wlcount, sizeof(unsigned)*PNL_WL_SLOTS))) return rc;
    if ((rc = ensure(ctx, ctx->b_wlaux, sizeof(unsigned)*(4*(PNL_WL_BINS+1))))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned), ctx->stream));
    ctx->run.wl_slots = 1; ctx->wl_cap_each = ctx->wl_cap;
    return PNL_OK;
}

bool tile_is_uniform(const pnl_context *ctx, const pnl_order_formula &F, int ta, int tb) { return pnl_tile_uniform_order(ctx, F, ta, tb, 2) == 2; }

template <int DIM, int DPE>
int pointwise_impl(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int cell_begin, int cell_end, int npairs,
                   int nbpairs) {
    // P1: tile kernels with LDS sub-blocks (k_pw_tile, k_pw_mixed, k_pw_lane).  P2 (FL2:894-1184 is element-agnostic): every
    // distant pair through classification, the sorted work list and k_pw_distant (16 lanes per pair, global atomics)
    constexpr int NV = DIM+1, ND = DPE*(DPE+1)/2, ST = 4+DPE;
    constexpr bool P1el = DPE == NV;
    const bool P1 = P1el && ctx->pw.type != 5;           // a P1 order function (type 5) is known per cell: the generic kernels
    int rc;
    const DevProblem &P = ctx->P;                        // distant rules, no order class: pnl_pw_prepare
    const PwDev &W = ctx->pw;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->b_D.p, 0, sizeof(double)*(size_t)ctx->ncp*ND, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    ctx->run.tiles_launched = true;
    const int nbk = (ctx->nc+63)/64;
    // the mixed tiles evaluate the rules with at most 16 points themselves (LDS sub-blocks); every other configuration classifies only
    const bool in_tile = P1 && ctx->tile == 64;
    {
        // work list: only the pairs whose rule has more than 16 points arrive there when the tiles evaluate the others
        // themselves (overflow is detected by pnl_get_counters); the tile-less variant lists every pair of the cell range
        double pairs = 0.;
        for (long long c = cell_begin; c < cell_end; c++) pairs += (double)(ctx->nc-c);
        const size_t want = in_tile ? (size_t)std::min<double>(std::max<double>(pairs*0.1, 1 << 20), 400e6)
                                           : (size_t)std::max<double>(pairs, 1024.);
        if (want > 1500000000ull) return fail(ctx, PNL_ERR_UNSUPPORTED, "%zu pairs exceed the work list of the pointwise path", want);
        if ((rc = reserve_worklist(ctx, want))) return rc;
    }
    // block tiles of the upper triangle: uniform ones (every pair provably of order 2 for every pair order in the range of
    // the two blocks) go to k_pw_tile, the others through classification and the sorted work list
    std::vector<int2> mixed, uniform;
    {
        const int T = 64;
        std::vector<double> smin(nbk, 1e300), smax(nbk, -1e300);
        for (int c = 0; c < ctx->nc; c++) {
            const int b = c/T;
            smin[b] = std::min(smin[b], ctx->pw_cell_smax[c]); smax[b] = std::max(smax[b], ctx->pw_cell_smax[c]);
        }
        auto formula = [&](double sv) {
            pnl_order_formula F;
            std::memset(&F, 0, sizeof(F));
            F.c0 = W.c0;
            if (DIM == 2) { F.a = sv-1.; F.b = 1.; F.e = sv; F.den0 = 0.4; } else { F.a = 2.*sv-1.; F.b = 0.; F.e = 2.*sv; F.den0 = 0.8; }
            return F;
        };
        const bool allow = P1 && ctx->tile == T && ctx->qmax >= 2;
        const int a0 = cell_begin/T, a1 = (cell_end+T-1)/T;
        for (int d = 0; d < nbk; d++)
            for (int a = a0; a < a1 && a+d < nbk; a++) {
                const int b = a+d;
                // the pair order max(m_c1, m_c2) lies between the larger of the block minima and the larger of the maxima; the
                // formula is linear in it, so the two end points bound it
                const double lo = std::max(smin[a], smin[b]), hi = std::max(smax[a], smax[b]);
                bool u = allow && a*T >= cell_begin && (a+1)*T <= cell_end && tile_is_uniform(ctx, formula(lo), a, b) &&
                         tile_is_uniform(ctx, formula(hi), a, b);
                (u ? uniform : mixed).push_back(make_int2(a, b));
            }
        std::vector<int2> all(mixed);
        all.insert(all.end(), uniform.begin(), uniform.end());
        if ((rc = upload(ctx, ctx->b_tiles, all.data(), all.size()))) return rc;
        ctx->tiles_cached.clear(); ctx->tiles_cb = -1;            // b_tiles no longer holds the dense tile list
    }
    if constexpr (P1el) if (P1 && !uniform.empty()) {
        const int acc_stride = ctx->nU+1;
        constexpr int NP = DIM == 2 ? 3 : 2;
        const size_t lds = sizeof(double)*(64*NP*DIM+2*64*NP+64+2*64*ND)+sizeof(int)*(64*DPE+64)
                           +2*sizeof(double)*(size_t)(ctx->nU+1)*acc_stride;
        auto tfun = k_pw_tile<DIM>;
        const PersistentGrid g = persistent_grid(ctx, tfun, PNL_NTHREADS, lds, (int)uniform.size(), 1);
        if (g.rc) return g.rc;
        hipLaunchKernelGGL(tfun, dim3(g.grid), dim3(PNL_NTHREADS), lds, ctx->stream, P, W, (const int2*)ctx->b_tiles.p+mixed.size(),
                           (int)uniform.size(), A, (long long)ldA, (double*)ctx->b_D.p, acc_stride);
        HIPCHK(ctx, hipGetLastError());
        ctx->run.pure_launched = true;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_UNIFORM_DONE], ctx->stream));
    // the other tiles: classification, in-tile evaluation of the rules with at most 16 points (LDS sub-blocks), work list for the rest
    if constexpr (P1el) if (!mixed.empty() && in_tile) {
        const int acc_stride = ctx->nU+1;
        const size_t lds = sizeof(double)*(PNL_PW_LANE_MAXPTS*ST+64*PNL_PW_LANE_MAXPTS*2+2*64*ND)+sizeof(unsigned short)*64*64
                           +sizeof(int)*(3*PNL_PW_NBUCK+2*64*DPE)+2*sizeof(double)*(size_t)(ctx->nU+1)*acc_stride;
        if (lds > 160*1024) return fail(ctx, PNL_ERR_UNSUPPORTED, "a block of 64 cells touches %d DoFs: LDS sub-blocks of %zu bytes exceed 160 KiB", ctx->nU, lds);
        auto mfun = k_pw_mixed<DIM>;
        const PersistentGrid g = persistent_grid(ctx, mfun, PNL_NTHREADS, lds, (int)mixed.size(), 1);
        if (g.rc) return g.rc;
        if ((rc = ensure(ctx, ctx->b_tilectr, sizeof(unsigned)))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->b_tilectr.p, 0, sizeof(unsigned), ctx->stream));
        hipLaunchKernelGGL(mfun, dim3(g.grid), dim3(PNL_NTHREADS), lds, ctx->stream, P, W, (const int2*)ctx->b_tiles.p, (int)mixed.size(), A,
                           (long long)ldA, (double*)ctx->b_D.p, acc_stride, (int4*)ctx->b_wl.p, (unsigned*)ctx->b_wlcount.p, ctx->wl_cap,
                           cell_begin, cell_end, (unsigned*)ctx->b_tilectr.p);
    }
    if (!mixed.empty() && !in_tile)
        hipLaunchKernelGGL((k_pw_classify<DIM, DPE>), dim3((unsigned)mixed.size()), dim3(PNL_NTHREADS), 0, ctx->stream, P, W,
                           (const int2*)ctx->b_tiles.p, (int4*)ctx->b_wl.p, (unsigned*)ctx->b_wlcount.p, ctx->wl_cap, cell_begin, cell_end);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_DONE], ctx->stream));
    {
        WlBins B;
        if ((rc = pnl_wl_sort(ctx, (const int4*)ctx->b_wl.p, (const unsigned*)ctx->b_wlcount.p, ctx->wl_cap, (unsigned*)ctx->b_wlaux.p,
                          (int4*)ctx->b_wlsorted.p, B))) return rc;
        hipLaunchKernelGGL(k_pw_stats, dim3(1), dim3(PNL_WL_BINS), 0, ctx->stream, P, (const unsigned*)B.hist);
        // LDS: rule table + order / scaling of the second cell's points for the 16 pairs of a chunk
        const int tab_max = 256;
        const size_t lds = sizeof(double)*((size_t)tab_max*ST+(size_t)(PNL_NTHREADS/16)*tab_max*2);
        auto kfun = k_pw_distant<DIM, DPE>;
        HIPCHK(ctx, hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const bool lane_kernel = P1;      // (with the in-tile evaluation only the rules of more than 16 points arrive here)
        if constexpr (P1el) if (lane_kernel)
            hipLaunchKernelGGL((k_pw_lane<DIM>), dim3(256*2), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, (const int4*)ctx->b_wlsorted.p,
                               (const unsigned*)B.offs, A, (long long)ldA, (double*)ctx->b_D.p);
        hipLaunchKernelGGL(kfun, dim3(256*4), dim3(PNL_NTHREADS), lds, ctx->stream, P, W, (const int4*)ctx->b_wlsorted.p,
                           (const unsigned*)B.offs, A, (long long)ldA, (double*)ctx->b_D.p, tab_max, lane_kernel ? PNL_PW_LANE_MAXPTS+1 : 0, PwNear{});
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WORKLIST_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_MIRROR_DONE], ctx->stream));
    if (npairs > 0) {
        const unsigned grid = (unsigned)((2ll*npairs*64+PNL_NTHREADS-1)/PNL_NTHREADS);
        const int4 *pp = (const int4*)ctx->b_pw_pairs.p;
        hipLaunchKernelGGL((k_pw_singular<DIM, DPE, 0>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, npairs, A, (long long)ldA, cell_begin, cell_end, PwNear{}, (const int*)nullptr);
        hipLaunchKernelGGL((k_pw_singular<DIM, DPE, 1>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, npairs, A, (long long)ldA, cell_begin, cell_end, PwNear{}, (const int*)nullptr);
        if (DIM == 2)
            hipLaunchKernelGGL((k_pw_singular<DIM, DPE, (DIM == 2 ? 2 : 1)>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, npairs, A, (long long)ldA, cell_begin, cell_end, PwNear{}, (const int*)nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    if (zero_exterior && cell_end > cell_begin) {
        const int ncell = cell_end-cell_begin, gx = (ncell+PNL_NTHREADS-1)/PNL_NTHREADS;
        int per = 16;
        while (per > 1 && (long long)gx*((ctx->nb+per-1)/per) < 4096) per >>= 1;
        hipLaunchKernelGGL((k_pw_boundary_distant<DIM, DPE>), dim3(gx, (ctx->nb+per-1)/per), dim3(PNL_NTHREADS), 0, ctx->stream, P, W,
                           (double*)ctx->b_D.p, cell_begin, cell_end, per);
        if (nbpairs > 0) {
            const unsigned grid = (unsigned)(((long long)nbpairs*64+PNL_NTHREADS-1)/PNL_NTHREADS);
            const int4 *bp = (const int4*)ctx->b_pw_bpairs.p;
            hipLaunchKernelGGL((k_pw_boundary_singular<DIM, DPE, 0>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, bp, nbpairs, (double*)ctx->b_D.p, cell_begin, cell_end);
            if (DIM == 2)
                hipLaunchKernelGGL((k_pw_boundary_singular<DIM, DPE, (DIM == 2 ? 1 : 0)>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, bp, nbpairs, (double*)ctx->b_D.p, cell_begin, cell_end);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_BOUNDARY_DONE], ctx->stream));
    pnl_scatter_diag(ctx, P, (const double*)ctx->b_D.p, A, ldA);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_END], ctx->stream));
    ctx->run.ev_valid = true;
    return PNL_OK;
}

int near_pattern(pnl_context *ctx, double *data, PwNear &NR) {
    if (ctx->sp_nnz < 0) return fail(ctx, PNL_ERR_STATE, "upload the sparsity pattern first");
    if (!data && ctx->sp_nnz > 0) return fail(ctx, PNL_ERR_INVALID, "null output");
    NR.indptr = (const int*)ctx->b_sp_indptr.p; NR.indices = (const int*)ctx->b_sp_indices.p;
    NR.data = data; NR.masks = (const unsigned long long*)ctx->b_mp_masks.p;
    return PNL_OK;
}

// items: touching[nt] / distant[nd] index the pair list; the touching ones come as (c1, c2, common, key) in b_pw_pairs
template <int DIM, int DPE>
int pairs_near_impl(pnl_context *ctx, int np, int nt, int nd, const PwNear &NR) {
    constexpr int ST = 4+DPE;
    int rc;
    const DevProblem &P = ctx->P;
    const PwDev &W = ctx->pw;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    for (int e : {EV_TILES_UNIFORM_DONE, EV_TILES_DONE}) HIPCHK(ctx, hipEventRecord(ctx->ev[e], ctx->stream));
    if ((rc = ensure(ctx, ctx->b_wlcount, sizeof(unsigned)*PNL_WL_SLOTS))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned), ctx->stream));
    ctx->run.wl_slots = 1;
    if (nd > 0) {
        // classification -> work list sorted by order -> 16 lanes per pair (k_pw_distant, this orientation alone)
        const size_t want = std::max<size_t>((size_t)nd, 1024);
        if ((rc = reserve_worklist(ctx, want))) return rc;
        hipLaunchKernelGGL((k_pw_classify_near<DIM, DPE>), dim3((nd+PNL_NTHREADS-1)/PNL_NTHREADS), dim3(PNL_NTHREADS), 0, ctx->stream, P, W,
                           (const int*)ctx->b_mp_pairs.p, (const int*)ctx->b_mp_sorted.p, nd, (int4*)ctx->b_wl.p,
                           (unsigned*)ctx->b_wlcount.p, ctx->wl_cap);
        WlBins B;
        if ((rc = pnl_wl_sort(ctx, (const int4*)ctx->b_wl.p, (const unsigned*)ctx->b_wlcount.p, ctx->wl_cap, (unsigned*)ctx->b_wlaux.p,
                          (int4*)ctx->b_wlsorted.p, B))) return rc;
        hipLaunchKernelGGL(k_pw_stats_near, dim3(1), dim3(PNL_WL_BINS), 0, ctx->stream, P, (const unsigned*)B.hist);
        const int tab_max = 256;
        const size_t lds = sizeof(double)*((size_t)tab_max*ST+(size_t)(PNL_NTHREADS/16)*tab_max*2);
        auto kfun = k_pw_distant<DIM, DPE, true>;
        HIPCHK(ctx, hipFuncSetAttribute((const void*)kfun, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kfun, dim3(256*4), dim3(PNL_NTHREADS), lds, ctx->stream, P, W, (const int4*)ctx->b_wlsorted.p, (const unsigned*)B.offs,
                           (double*)nullptr, 0ll, (double*)nullptr, tab_max, 0, NR);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WORKLIST_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_MIRROR_DONE], ctx->stream));
    if (nt > 0) {
        const unsigned grid = (unsigned)(((long long)nt*64+PNL_NTHREADS-1)/PNL_NTHREADS);
        const int4 *pp = (const int4*)ctx->b_pw_pairs.p;
        const int *item = (const int*)ctx->b_mp_wl.p;
        hipLaunchKernelGGL((k_pw_singular<DIM, DPE, 0, true>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, nt, (double*)nullptr, 0ll, 0, 0, NR, item);
        hipLaunchKernelGGL((k_pw_singular<DIM, DPE, 1, true>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, nt, (double*)nullptr, 0ll, 0, 0, NR, item);
        if (DIM == 2)
            hipLaunchKernelGGL((k_pw_singular<DIM, DPE, (DIM == 2 ? 2 : 1), true>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, P, W, pp, nt, (double*)nullptr, 0ll, 0, 0, NR, item);
        HIPCHK(ctx, hipGetLastError());
    }
    for (int e : {EV_SINGULAR_DONE, EV_BOUNDARY_DONE, EV_END}) HIPCHK(ctx, hipEventRecord(ctx->ev[e], ctx->stream));
    ctx->run.ev_valid = true;
    ctx->run.visited_pairs = (unsigned long long)np;
    return PNL_OK;
}

template <int DIM, int DPE>
int boundary_near_impl(pnl_context *ctx, int ni, double fac, const SparseOut &S) {
    const int grid = std::min((ni+3)/4, 256*8);
    hipLaunchKernelGGL((k_pw_boundary_items<DIM, DPE>), dim3(grid), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, ctx->pw,
                       (const double*)ctx->b_vertices.p, (const int*)ctx->b_bi_cells.p, (const int*)ctx->b_bi_facets.p,
                       (const unsigned*)ctx->b_bi_masks.p, (const int*)ctx->b_mp_aux.p, (const double*)ctx->b_mp_sorted.p, ni, fac, S);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // namespace

int pnl_pw_h2_interp(pnl_context *ctx) {
    const H2Dev &H = ctx->h2;
    if (H.nfar <= 0) return PNL_OK;
    if (ctx->dim == 2) hipLaunchKernelGGL((k_h2_kernel_interp_pw<2>), dim3(H.nfar), dim3(PNL_NTHREADS), 0, ctx->stream, H, ctx->pw);
    else hipLaunchKernelGGL((k_h2_kernel_interp_pw<1>), dim3(H.nfar), dim3(PNL_NTHREADS), 0, ctx->stream, H, ctx->pw);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

extern "C" {

int pnl_assemble_dense_pointwise(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int cell_begin, int cell_end,
                                 int npairs, const int32_t *pairs, int nbpairs, const int32_t *bpairs) {
    if (!ctx) return PNL_ERR_INVALID;
    int rc;
    if ((rc = pnl_pw_prepare(ctx, zero_exterior))) return rc;
    if (!A || ldA < ctx->N) return fail(ctx, PNL_ERR_INVALID, "bad output matrix (ldA=%lld, num_dofs=%d)", (long long)ldA, ctx->N);
    if (cell_begin < 0 || cell_end > ctx->nc || cell_begin > cell_end) return fail(ctx, PNL_ERR_INVALID, "bad cell range");
    if (npairs < 0 || nbpairs < 0 || (npairs && !pairs) || (nbpairs && !bpairs)) return fail(ctx, PNL_ERR_INVALID, "bad pair lists");
    for (int t = 0; t < npairs; t++) {
        const int32_t *q = pairs+4*(size_t)t;
        if (q[0] < 0 || q[1] < q[0] || q[1] >= ctx->nc || q[2] < 1 || q[2] > ctx->dim+1 || q[3] < 0 || q[3] >= ctx->pw_nkeys[0])
            return fail(ctx, PNL_ERR_INVALID, "bad touching pair %d", t);
    }
    for (int t = 0; t < nbpairs; t++) {
        const int32_t *q = bpairs+4*(size_t)t;
        if (q[0] < 0 || q[0] >= ctx->nc || q[1] < 0 || q[1] >= ctx->nb || q[2] < 1 || q[2] > ctx->dim || q[3] < 0 || q[3] >= ctx->pw_nkeys[1])
            return fail(ctx, PNL_ERR_INVALID, "bad touching cell/facet pair %d", t);
    }
    if ((rc = upload(ctx, ctx->b_pw_pairs, pairs, (size_t)4*npairs))) return rc;
    if ((rc = upload(ctx, ctx->b_pw_bpairs, bpairs, (size_t)4*nbpairs))) return rc;
    pnl_begin_assembly(ctx);
    for (long long c = cell_begin; c < cell_end; c++) ctx->run.visited_pairs += (unsigned long long)(ctx->nc-c);
    if (ctx->dim == 2)
        return ctx->dpe == 6 ? pointwise_impl<2, 6>(ctx, A, ldA, zero_exterior, cell_begin, cell_end, npairs, nbpairs)
                             : pointwise_impl<2, 3>(ctx, A, ldA, zero_exterior, cell_begin, cell_end, npairs, nbpairs);
    return ctx->dpe == 3 ? pointwise_impl<1, 3>(ctx, A, ldA, zero_exterior, cell_begin, cell_end, npairs, nbpairs)
                         : pointwise_impl<1, 2>(ctx, A, ldA, zero_exterior, cell_begin, cell_end, npairs, nbpairs);
}

int pnl_assemble_pairs_masked_pointwise(pnl_context *ctx, int np, const int32_t *pairs, const uint64_t *masks, const int32_t *rule,
                                        double *data) {
    if (!ctx) return PNL_ERR_INVALID;
    if (np < 0 || (np && (!pairs || !masks || !rule))) return fail(ctx, PNL_ERR_INVALID, "bad pair list");
    int rc;
    if ((rc = pnl_pw_prepare(ctx, 0))) return rc;
    const int nV = ctx->dim+1;
    // split by kind on the host: touching items with the key of their near rule, the others for the device classification; every
    // index is checked here (a wrong one would be an out-of-bounds access on the device)
    std::vector<int32_t> touching, distant, titems;
    for (int t = 0; t < np; t++) {
        const int c1 = pairs[2*(size_t)t], c2 = pairs[2*(size_t)t+1];
        if (c1 < 0 || c1 >= ctx->nc || c2 < 0 || c2 >= ctx->nc) return fail(ctx, PNL_ERR_INVALID, "pair %d = (%d, %d): not cells", t, c1, c2);
        int common = 0;
        for (int a = 0; a < nV; a++)
            for (int b = 0; b < nV; b++) common += ctx->cells[(size_t)c1*nV+a] == ctx->cells[(size_t)c2*nV+b];
        if (common > 0) {
            if (rule[t] < 0 || rule[t] >= ctx->pw_nkeys[0]) return fail(ctx, PNL_ERR_INVALID, "touching pair %d: rule key %d out of range", t, rule[t]);
            touching.push_back(c1); touching.push_back(c2); touching.push_back(common); touching.push_back(rule[t]);
            titems.push_back(t);
        } else {
            if (rule[t] >= 0) return fail(ctx, PNL_ERR_INVALID, "pair %d has no common vertex but names a near rule", t);
            distant.push_back(t);
        }
    }
    if ((rc = upload(ctx, ctx->b_mp_pairs, pairs, (size_t)2*np))) return rc;
    if ((rc = upload(ctx, ctx->b_mp_masks, masks, (size_t)4*np))) return rc;
    if ((rc = upload(ctx, ctx->b_pw_pairs, touching.data(), touching.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_mp_wl, titems.data(), titems.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_mp_sorted, distant.data(), distant.size()))) return rc;
    PwNear NR;
    if ((rc = near_pattern(ctx, data, NR))) return rc;
    const int nt = (int)titems.size(), nd = (int)distant.size();
    pnl_begin_assembly(ctx);
    if (ctx->dim == 2) return ctx->dpe == 6 ? pairs_near_impl<2, 6>(ctx, np, nt, nd, NR) : pairs_near_impl<2, 3>(ctx, np, nt, nd, NR);
    return ctx->dpe == 3 ? pairs_near_impl<1, 3>(ctx, np, nt, nd, NR) : pairs_near_impl<1, 2>(ctx, np, nt, nd, NR);
}

int pnl_assemble_boundary_masked_pointwise(pnl_context *ctx, int ni, const int32_t *cells, const int32_t *facets, const uint32_t *masks,
                                           const int32_t *rule, const double *sv, double fac, double *data, double *diag) {
    if (!ctx) return PNL_ERR_INVALID;
    if (ni < 0 || (ni && (!cells || !facets || !masks || !rule || !sv))) return fail(ctx, PNL_ERR_INVALID, "bad item list");
    int rc;
    if ((rc = pnl_pw_prepare(ctx, 0))) return rc;
    for (int s = 0; s < ctx->dim; s++)
        if (!ctx->have_pw_rules[1][s]) return fail(ctx, PNL_ERR_STATE, "pointwise boundary rule for %d common vertices not uploaded", s+1);
    const int dim = ctx->dim, nV = dim+1;
    for (int t = 0; t < ni; t++) {
        if (cells[t] < 0 || cells[t] >= ctx->nc) return fail(ctx, PNL_ERR_INVALID, "item %d: bad cell", t);
        int common = 0;
        for (int k = 0; k < dim; k++) {
            const int v = facets[(size_t)t*dim+k];
            if (v < 0 || v >= ctx->nv) return fail(ctx, PNL_ERR_INVALID, "item %d: bad facet vertex", t);
            for (int a = 0; a < nV; a++) common += ctx->cells[(size_t)cells[t]*nV+a] == v;
        }
        if (common > 0 ? (rule[t] < 0 || rule[t] >= ctx->pw_nkeys[1]) : rule[t] >= 0)
            return fail(ctx, PNL_ERR_INVALID, "item %d: %d common vertices but rule key %d", t, common, rule[t]);
        if (!(sv[t] > 0.) || !(sv[t] < 1.)) return fail(ctx, PNL_ERR_INVALID, "item %d: order %g outside (0, 1)", t, sv[t]);
    }
    if ((rc = upload(ctx, ctx->b_vertices, ctx->vertices.data(), ctx->vertices.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_bi_cells, cells, (size_t)ni))) return rc;
    if ((rc = upload(ctx, ctx->b_bi_facets, facets, (size_t)ni*dim))) return rc;
    if ((rc = upload(ctx, ctx->b_bi_masks, masks, (size_t)ni))) return rc;
    if ((rc = upload(ctx, ctx->b_mp_aux, rule, (size_t)ni))) return rc;
    if ((rc = upload(ctx, ctx->b_mp_sorted, sv, (size_t)ni))) return rc;
    if (ctx->sp_nnz < 0) return fail(ctx, PNL_ERR_STATE, "upload the sparsity pattern first");
    if (!data && ctx->sp_nnz > 0) return fail(ctx, PNL_ERR_INVALID, "null output");
    SparseOut S;
    S.indptr = (const int*)ctx->b_sp_indptr.p; S.indices = (const int*)ctx->b_sp_indices.p;
    S.data = data; S.diag = diag; S.pairs = nullptr; S.masks = nullptr;
    if (ni == 0) return PNL_OK;
    if (dim == 2) return ctx->dpe == 6 ? boundary_near_impl<2, 6>(ctx, ni, fac, S) : boundary_near_impl<2, 3>(ctx, ni, fac, S);
    return ctx->dpe == 3 ? boundary_near_impl<1, 3>(ctx, ni, fac, S) : boundary_near_impl<1, 2>(ctx, ni, fac, S);
}

}  // extern "C"
