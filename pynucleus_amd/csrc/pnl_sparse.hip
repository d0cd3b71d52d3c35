// The pair assemblies into a CSR / SSS pattern (gfx950 only): explicit pair lists with entry masks (assembleClusters,
// nonlocalAssembly_{SCALAR}.pxi:1663-1964) and getSparse for a finite horizon without a host pair list -- block tiles the horizon can
// reach, k_tile_distant<.., FH> for the pairs inside it, the sorted sparse pipeline (classification, work list, touching pairs) for the
// rest.  Kernels: the SPARSE instantiations of pnl_kernels.h, which nothing else launches; they stay in an unnamed namespace, so
// nothing collides with pnl_hip.o at link time.  What this unit needs from pnl_hip.hip and pnl_setup.hip are host functions of pnl_context.h.
#include <climits>
#include "pnl_context.h"
namespace {
#include "pnl_kernels.h"
}
#include "pnl_launch.h"

namespace {

// ---- masked pair assembly (assembleClusters, NA:1663-1964): statistics of the sorted pair list ---------------------
// hist[q] pairs of order q: numAssembledCellPairs, kernel evaluations n(q)^2 each and the order histogram (the touching
// pairs in bins 121.. are counted by k_singular_pairs itself)
__global__ void k_mp_stats(const DevProblem P, const unsigned *__restrict__ hist) {
    const int q = threadIdx.x;
    if (q < 2 || q > P.qmax || q > PNL_MAXQ) return;
    const unsigned long long c = hist[q];
    // pairs cut by a finite horizon sit in bin q + PNL_CUT_SHIFT; their kernel evaluations are counted by the kernel
    const unsigned long long ccut = (P.k.horizon2 < 1e300 && q+PNL_CUT_SHIFT < PNL_WL_BINS && q <= PNL_CUT_SHIFT) ? hist[q+PNL_CUT_SHIFT] : 0ull;
    if (!c && !ccut) return;
    const unsigned long long n = (unsigned long long)(P.off[q+1]-P.off[q]);
    atomicAdd(&P.counters[8+q], c+ccut);
    atomicAdd(&P.counters[1], c+ccut);
    if (c) atomicAdd(&P.counters[2], c*n*n);
}

template <int DPE>
void scatter_diag_sparse(pnl_context *ctx, const double *D, const SparseOut &S) {
    const long long n = (long long)ctx->nc*(DPE*(DPE+1)/2);
    hipLaunchKernelGGL((k_scatter_diag_sparse<DPE>), dim3((unsigned)((n+PNL_NTHREADS-1)/PNL_NTHREADS)), dim3(PNL_NTHREADS), 0, ctx->stream,
                       ctx->P, D, ctx->nc, S);
}

// end of an assembly path that skips its later phases: every event but EV_START, so that the phase timers read zero
int finish_events(pnl_context *ctx) {
    for (int e = EV_START+1; e < EV_COUNT; e++) HIPCHK(ctx, hipEventRecord(ctx->ev[e], ctx->stream));
    ctx->run.ev_valid = true; ctx->run.tiles_launched = true;
    return PNL_OK;
}

// ---- masked pair assembly into CSR / SSS (assembleClusters) --------------------------------------------------------
// classify == false: the work list b_mp_wl[0..np) has been filled on the device (k_fh_pairs)
template <int DIM, int DPE, int KT>
int pairs_masked_impl(pnl_context *ctx, int np, const SparseOut &S, bool classify = true, bool first = true, bool keepD = false) {
    int rc;
    if ((rc = ensure(ctx, ctx->b_mp_wl, (size_t)np*sizeof(int4)))) return rc;
    if ((rc = ensure(ctx, ctx->b_mp_sorted, (size_t)np*sizeof(int4)))) return rc;
    if ((rc = ensure(ctx, ctx->b_mp_aux, sizeof(unsigned)*(4*(PNL_WL_BINS+1)+1)))) return rc;
    unsigned *count = (unsigned*)ctx->b_mp_aux.p+4*(PNL_WL_BINS+1);      // behind the four bin arrays of pnl_wl_sort
    int4 *wl = (int4*)ctx->b_mp_wl.p, *sorted = (int4*)ctx->b_mp_sorted.p;
    const unsigned unp = (unsigned)np;
    HIPCHK(ctx, hipMemcpyAsync(count, &unp, sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // unp lives on this stack frame
    if (first) HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    if (classify)
        hipLaunchKernelGGL((k_mp_classify<DIM, DPE>), dim3((np+PNL_NTHREADS-1)/PNL_NTHREADS), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P,
                           S.pairs, np, wl);
    WlBins B;
    if ((rc = pnl_wl_sort(ctx, wl, count, unp, (unsigned*)ctx->b_mp_aux.p, sorted, B))) return rc;
    hipLaunchKernelGGL(k_mp_stats, dim3(1), dim3(PNL_WL_BINS), 0, ctx->stream, ctx->P, (const unsigned*)B.hist);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_TILES_DONE], ctx->stream));
    {
        // no masks (getSparse): diagonal blocks through the per-cell buffer, one scatter per cell at the end
        constexpr int ND = DPE*(DPE+1)/2;
        double *Dbuf = S.masks ? nullptr : (double*)ctx->b_D.p;
        if (Dbuf && !keepD) HIPCHK(ctx, hipMemsetAsync(Dbuf, 0, sizeof(double)*(size_t)ctx->ncp*ND, ctx->stream));      // keepD: the tiles of a finite horizon have been there
        // 60 KB of rule copy and the bins up to PNL_MAXQ: differences from the dense path that are kept, not decided
        constexpr int wl_mp_kb = 60;
        if ((rc = worklist_eval<DIM, DPE, KT, true>(ctx, wl_mp_kb, sorted, B, nullptr, 0, Dbuf, S, ClusterTiles{}, PNL_MAXQ, false))) return rc;
        if (Dbuf) scatter_diag_sparse<DPE>(ctx, Dbuf, S);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WORKLIST_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_MIRROR_DONE], ctx->stream));
    // touching pairs: bins 121 (common vertex), 122 (common edge / identical in 1D), 123 (identical in 2D)
    unsigned hh[PNL_WL_BINS+1];
    HIPCHK(ctx, hipMemcpyAsync(hh, B.hist, sizeof(hh), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < DIM+1; s++)
        if (hh[121+s] && !ctx->C().have_sing[0][s]) return fail(ctx, PNL_ERR_STATE, "singular rule for %d common vertices not uploaded", s+1);
    for (int s = 0; s < DIM+1; s++)
        if (hh[121+s] && (rc = with_slot<DIM>(s, [&](auto slot) {
                // the pairs come from the sorted list: the fixed grid of the sparse path, whatever their number
                return launch_singular_pairs<DIM, DPE, decltype(slot)::value, KT, true>(ctx, INT_MAX, nullptr, 0, nullptr, 0, 0, 0, S, sorted, B.offs,
                                                                                        ClusterTiles{});
            }))) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SINGULAR_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_BOUNDARY_DONE], ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_END], ctx->stream));
    ctx->run.ev_valid = true;
    ctx->run.tiles_launched = true;
    return PNL_OK;
}

// getSparse without a host pair list: block tiles the horizon can reach -> k_fh_pairs -> the sorted pipeline of the masked path
template <int DIM, int DPE, int KT>
int horizon_impl(pnl_context *ctx, SparseOut S, int cell_begin, int cell_end) {
    int rc;
    const int T = ctx->tile, nbk = ctx->nblocks;
    const double delta = std::sqrt(ctx->C().kern[0].horizon2);
    const bool whole = cell_begin <= 0 && cell_end >= ctx->nc;
    std::vector<int2> tiles;
    for (int a = 0; a < nbk; a++)
        for (int b = a; b < nbk; b++) {
            // a range of first cells (the reference's cellNo1 split, NA:1280-1285): only block rows that hold one
            if ((a+1)*T <= cell_begin || a*T >= cell_end) continue;
            const auto &A = ctx->blocks[a], &B = ctx->blocks[b];
            const double dx = A.tcx-B.tcx, dy = A.tcy-B.tcy;
            // every vertex of a block lies within trad of (tcx, tcy) (vertices within h of their cell's centre)
            if (std::sqrt(dx*dx+dy*dy)-A.trad-B.trad <= delta) tiles.push_back(make_int2(a, b));
        }
    if ((rc = upload(ctx, ctx->b_tiles, tiles.data(), tiles.size()))) return rc;
    ctx->tiles_cached.clear(); ctx->tiles_cb = -1;            // b_tiles no longer holds the dense tile list
    const size_t per_tile = (size_t)T*T, chunk_tiles = std::max<size_t>(1, (size_t)(48u << 20)/per_tile);
    const size_t cap = std::min(tiles.size(), chunk_tiles)*per_tile;
    if ((rc = ensure(ctx, ctx->b_mp_pairs, cap*sizeof(int2)))) return rc;
    if ((rc = ensure(ctx, ctx->b_mp_wl, cap*sizeof(int4)))) return rc;
    if ((rc = ensure(ctx, ctx->b_wlcount, sizeof(unsigned)*PNL_WL_SLOTS))) return rc;
    ctx->run.wl_slots = 1; ctx->wl_cap_each = (unsigned)cap;
    S.pairs = (const int*)ctx->b_mp_pairs.p;
    S.masks = nullptr;
    unsigned long long total = 0;
    bool first = true;
    // The pairs inside the horizon are integrated by the tile kernel (LDS sub-block, one pattern search per sub-block entry
    // instead of one per pair and entry); what it cannot do itself -- pairs cut by the horizon, touching pairs, orders
    // without a packed rule -- it hands to the sorted sparse pipeline through the far list.  PNL_FH_NOTILES=1 keeps the
    // pair generator k_fh_pairs, which sends every pair down that pipeline.
    constexpr int TILE = (DPE == 6 || (DIM == 1 && DPE == 3)) ? 32 : 64, ND = DPE*(DPE+1)/2;
    using TS = TileSmem<DIM, DPE, TILE, KT == 0>;
    const int acc_stride = acc_stride_of(ctx->nU, TS::fixed_bytes);
    const size_t lds = TS::fixed_bytes+sizeof(double)*(size_t)(ctx->nU+1)*acc_stride;
    // piecewise-constant order: the candidate pairs of a chunk once (k_fh_pairs), then the sorted pipeline once per order class and
    // orientation, whose classification keeps the pairs of the class (like pnl_assemble_pairs_masked)
    const bool var = ctx->nlab > 0;
    const bool use_tiles = T == TILE && lds <= 160*1024 && !pnl_tune("PNL_FH_NOTILES") && !var;
    if (!use_tiles && !whole) return fail(ctx, PNL_ERR_UNSUPPORTED, "a range of first cells needs the tile route of the finite-horizon assembly");
    ctx->run.visited_is_assembled = use_tiles;
    for (size_t t0 = 0; t0 < tiles.size(); t0 += chunk_tiles) {
        const int nt = (int)std::min(chunk_tiles, tiles.size()-t0);
        HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned), ctx->stream));
        if (first) HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
        if (use_tiles) {
            auto kfun = k_tile_distant<DIM, DPE, TILE, KT, false, true>;
            const PersistentGrid g = persistent_grid(ctx, kfun, tile_threads(DPE, true), lds, nt, 2);
            if (g.rc) return g.rc;
            if ((rc = ensure(ctx, ctx->b_tilectr, sizeof(unsigned)))) return rc;
            HIPCHK(ctx, hipMemsetAsync(ctx->b_tilectr.p, 0, sizeof(unsigned), ctx->stream));
            HIPCHK(ctx, hipMemsetAsync(ctx->b_D.p, 0, sizeof(double)*(size_t)ctx->ncp*ND, ctx->stream));
            ClusterTiles CT{};
            CT.S = S;
            CT.wl_ds = (int2*)ctx->b_mp_pairs.p;                   // the pairs of the far-list entries
            SlotOut SOk{};
            SOk.nU = ctx->nU;                                      // rows of the LDS sub-block
            hipLaunchKernelGGL(kfun, dim3(g.grid), dim3(tile_threads(DPE, true)), lds, ctx->stream, ctx->P, (const int2*)ctx->b_tiles.p+t0,
                               (double*)nullptr, 0ll, (double*)ctx->b_D.p, std::max(cell_begin, 0), std::min(cell_end, ctx->nc), acc_stride, (int4*)ctx->b_mp_wl.p,
                               (unsigned*)ctx->b_wlcount.p, (unsigned)cap, 0, nt, CT, (unsigned*)ctx->b_tilectr.p, SOk, (const unsigned short*)nullptr);
        } else
            hipLaunchKernelGGL((k_fh_pairs<DIM, DPE>), dim3(nt), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, (const int2*)ctx->b_tiles.p+t0, T,
                               (int2*)ctx->b_mp_pairs.p, (int4*)ctx->b_mp_wl.p, (unsigned*)ctx->b_wlcount.p, (unsigned)cap);
        HIPCHK(ctx, hipGetLastError());
        unsigned np = 0;
        HIPCHK(ctx, hipMemcpyAsync(&np, ctx->b_wlcount.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (np > cap) return fail(ctx, PNL_ERR_STATE, "far list of the finite-horizon tiles overflowed (%u > %zu)", np, cap);
        total += np;
        if (np && var) {
            const int ncls = (int)ctx->cls.size(), norient = ctx->nonsym ? 2 : 1;
            ClassScope cls(ctx, ctx->cur, true);
            for (int ko = 0; ko < ncls*norient; ko++) {
                cls.select(ko/norient, ko%norient);
                if ((rc = pairs_masked_impl<DIM, DPE, 0>(ctx, (int)np, S, true, false, false))) return rc;
            }
        } else
        if (np && (rc = pairs_masked_impl<DIM, DPE, KT>(ctx, (int)np, S, false, false, use_tiles))) return rc;
        if (!np && use_tiles) {
            // no far entries in this chunk: the diagonal blocks of its tiles still have to reach the matrix
            scatter_diag_sparse<DPE>(ctx, (const double*)ctx->b_D.p, S);
            if ((rc = finish_events(ctx))) return rc;
        }
        first = false;
    }
    ctx->run.visited_pairs = total;
    if (total == 0 && (rc = finish_events(ctx))) return rc;
    // slot 0 of b_wlcount holds the far-list fill of the last chunk, which check_overflow holds against its capacity (wl_slots = 1); it is
    // no length of a work list of the tile kernels, and pnl_get_counters sums the slots in use as workListLength
    HIPCHK(ctx, hipMemsetAsync(ctx->b_wlcount.p, 0, sizeof(unsigned), ctx->stream));
    return PNL_OK;
}

}  // namespace

// pnl_hip.hip (pnl_assemble_boundary_masked, pnl_assemble_clusters_tiled) too: see pnl_context.h
int pnl_sparse_ready(pnl_context *ctx, double *data, double *diag, SparseOut &S) {
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    if (ctx->sp_nnz < 0) return fail(ctx, PNL_ERR_STATE, "upload the sparsity pattern first");
    if (!data && ctx->sp_nnz > 0) return fail(ctx, PNL_ERR_INVALID, "null output");
    pnl_refresh_tables(ctx);
    S.indptr = (const int*)ctx->b_sp_indptr.p; S.indices = (const int*)ctx->b_sp_indices.p;
    S.data = data; S.diag = diag;
    S.pairs = (const int*)ctx->b_mp_pairs.p; S.masks = (const unsigned long long*)ctx->b_mp_masks.p;
    return PNL_OK;
}

extern "C" {

int pnl_upload_sparsity(pnl_context *ctx, int nnz, const int32_t *indptr, const int32_t *indices) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "upload the DoF map first");
    if (nnz < 0 || !indptr || (nnz && !indices) || indptr[0] != 0 || indptr[ctx->N] != nnz)
        return fail(ctx, PNL_ERR_INVALID, "bad sparsity pattern (nnz=%d)", nnz);
    for (int i = 0; i < ctx->N; i++) {
        if (indptr[i+1] < indptr[i]) return fail(ctx, PNL_ERR_INVALID, "indptr is not monotone at row %d", i);
        for (int t = indptr[i]; t < indptr[i+1]; t++)
            if (indices[t] < 0 || indices[t] >= ctx->N || (t > indptr[i] && indices[t] <= indices[t-1]))
                return fail(ctx, PNL_ERR_INVALID, "row %d of the pattern is not sorted / in range", i);
    }
    int rc;
    if ((rc = upload(ctx, ctx->b_sp_indptr, indptr, (size_t)ctx->N+1))) return rc;
    if ((rc = upload(ctx, ctx->b_sp_indices, indices, (size_t)nnz))) return rc;
    ctx->sp_nnz = nnz;
    return PNL_OK;
}

int pnl_upload_sparsity_device(pnl_context *ctx, int nnz, const int32_t *indptr_dev, const int32_t *indices_dev) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "upload the DoF map first");
    if (nnz < 0 || !indptr_dev || (nnz && !indices_dev)) return fail(ctx, PNL_ERR_INVALID, "bad sparsity pattern (nnz=%d)", nnz);
    int rc;
    if ((rc = ensure(ctx, ctx->b_sp_indptr, sizeof(int32_t)*((size_t)ctx->N+1)))) return rc;
    if ((rc = ensure(ctx, ctx->b_sp_indices, sizeof(int32_t)*(size_t)std::max(nnz, 1)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_sp_indptr.p, indptr_dev, sizeof(int32_t)*((size_t)ctx->N+1), hipMemcpyDeviceToDevice, ctx->stream));
    if (nnz) HIPCHK(ctx, hipMemcpyAsync(ctx->b_sp_indices.p, indices_dev, sizeof(int32_t)*(size_t)nnz, hipMemcpyDeviceToDevice, ctx->stream));
    int32_t ends[2] = {-1, -1};
    HIPCHK(ctx, hipMemcpyAsync(&ends[0], ctx->b_sp_indptr.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&ends[1], (const int32_t*)ctx->b_sp_indptr.p+ctx->N, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ends[0] != 0 || ends[1] != nnz) { ctx->sp_nnz = -1; return fail(ctx, PNL_ERR_INVALID, "bad sparsity pattern: indptr runs from %d to %d, nnz=%d", ends[0], ends[1], nnz); }
    ctx->sp_nnz = nnz;
    return PNL_OK;
}

int pnl_assemble_pairs_masked(pnl_context *ctx, int np, const int32_t *pairs, const uint64_t *masks, double *data, double *diag) {
    if (!ctx) return PNL_ERR_INVALID;
    if (np < 0 || (np && !pairs)) return fail(ctx, PNL_ERR_INVALID, "bad pair list");
    for (int i = 0; i < np; i++)
        if (pairs[2*i] < 0 || pairs[2*i] > pairs[2*i+1] || pairs[2*i+1] >= ctx->nc)
            return fail(ctx, PNL_ERR_INVALID, "pair %d = (%d, %d) is not an ordered pair of cells", i, pairs[2*i], pairs[2*i+1]);
    int rc;
    if ((rc = upload(ctx, ctx->b_mp_pairs, pairs, (size_t)2*np))) return rc;
    if (masks && (rc = upload(ctx, ctx->b_mp_masks, masks, (size_t)4*np))) return rc;
    if (!std::isinf(ctx->C().kern[0].horizon2) && ctx->qmax > PNL_CUT_SHIFT)
        return fail(ctx, PNL_ERR_UNSUPPORTED, "finite horizon: upload distant rules up to order %d at most", PNL_CUT_SHIFT);
    SparseOut S;
    if ((rc = pnl_sparse_ready(ctx, data, diag, S))) return rc;
    if (!masks) S.masks = nullptr;               // every entry of every pair is requested
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    pnl_begin_assembly(ctx);
    ctx->run.visited_pairs = (unsigned long long)np;
    if (np == 0) HIPCHK(ctx, hipEventRecord(ctx->ev[EV_START], ctx->stream));
    if (np == 0) return finish_events(ctx);                  // an empty assembly: every timer reads zero
    // variable order (piecewise constant, symmetric table): the pair list once per class, k_mp_classify keeps the pairs of the
    // class (the interface terms of NA:1966-2156 are boundary items, pnl_assemble_boundary_masked after pnl_select_class)
    // non-symmetric class table (NA:1776-1840 with symmetricCells == False): the listed pairs (c1 <= c2) once per orientation, each
    // with the class of its orientation and half the kernel (the machinery applies the factor 2 of the symmetric case); the masks
    // of (c1, c2) and (c2, c1) request the same DoF pairs, so the list of the symmetric case serves both
    const int ncls = ctx->nlab > 0 ? (int)ctx->cls.size() : 1;
    const int norient = (ctx->nlab > 0 && ctx->nonsym) ? 2 : 1;
    ClassScope cls(ctx, ctx->cur, norient > 1);
    for (int ko = 0; ko < ncls*norient; ko++) {
        if (ctx->nlab > 0) cls.select(ko/norient, ko%norient);      // a constant order: the class of pnl_select_class
        const bool fast = ctx->P.k.fast != 0, first = ko == 0;
        rc = with_shape(ctx, [&](auto D, auto E) {
            constexpr int DIM = decltype(D)::value, DPE = decltype(E)::value;
            return with_kt_2d<DIM>(fast, [&](auto kt) { return pairs_masked_impl<DIM, DPE, decltype(kt)::value>(ctx, np, S, true, first); });
        });
        if (rc) return rc;
    }
    return PNL_OK;
}

int pnl_assemble_pairs_in_horizon(pnl_context *ctx, double *data, double *diag) {
    return pnl_assemble_pairs_in_horizon_range(ctx, data, diag, 0, ctx ? ctx->nc : 0);
}

int pnl_assemble_pairs_in_horizon_range(pnl_context *ctx, double *data, double *diag, int cell_begin, int cell_end) {
    if (!ctx) return PNL_ERR_INVALID;
    if (cell_begin < 0 || cell_end > ctx->nc || cell_begin > cell_end) return fail(ctx, PNL_ERR_INVALID, "bad cell range");
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    // (a non-symmetric order table would need the pairs the horizon cuts re-triangulated with the roles of the two cells swapped in the
    // second orientation, NA:1418 swapCells: the cut evaluation of the sorted pipeline takes the listed order)
    if (ctx->nlab > 0 && ctx->nonsym) return fail(ctx, PNL_ERR_UNSUPPORTED, "finite horizon with a non-symmetric order table");
    if (std::isinf(ctx->C().kern[0].horizon2)) return fail(ctx, PNL_ERR_STATE, "pnl_assemble_pairs_in_horizon needs a finite horizon");
    if (ctx->qmax > PNL_CUT_SHIFT) return fail(ctx, PNL_ERR_UNSUPPORTED, "finite horizon: upload distant rules up to order %d at most", PNL_CUT_SHIFT);
    SparseOut S;
    if ((rc = pnl_sparse_ready(ctx, data, diag, S))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS, ctx->stream));
    pnl_begin_assembly(ctx);
    const bool fast = ctx->P.k.fast != 0;
    return with_shape(ctx, [&](auto D, auto E) {
        constexpr int DIM = decltype(D)::value, DPE = decltype(E)::value;
        return with_kt_2d<DIM>(fast, [&](auto kt) { return horizon_impl<DIM, DPE, decltype(kt)::value>(ctx, S, cell_begin, cell_end); });
    });
}

}  // extern "C"
